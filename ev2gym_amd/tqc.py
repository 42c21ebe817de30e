"""TQC on the device: sb3_contrib's `TQC.train()` (Truncated Quantile Critics; MlpPolicy, Box actions, `use_sde=False`) behind a device replay
ring (`csrc/ev2g_tqc.h` over `csrc/ev2g_sac.h`, `ev2g_tqc_*`).

The actor is SAC's squashed Gaussian, bit for bit: `TQCCollector` is `SACCollector` whose episodes run through `ev2g_tqc_collect`, and
`TQCLearner(collector)` creates the device object (learner and collection actor are one object) and binds it to the collector, as `SACLearner`
does.  The critics are `n_critics` networks (s, a) -> h1 -> h2 -> `n_quantiles`.  With nq = n_quantiles, nc = n_critics, d =
top_quantiles_to_drop_per_net, M = nc nq pooled atoms, K = M - d nc kept ones and tau_i = (i + 0.5) / nq, one update on (s, a~, r, s', done) of B
rows, alpha = exp(log_ent_coef) as it stands before the update:

    a_pi, log pi on s;  a', log pi' on s'                                                          (SAC's head and draws)
    per row: the M atoms critic_target_j(s', a')[i], pooled j-major, sorted ascending, the first K kept
    z_k = r + (1 - done) gamma (sorted_k - alpha log pi')                                           (no gradient through z)
    delta = z_k - critic_j(s, a~)[i];  huber = |delta| - 0.5 where |delta| > 1, else 0.5 delta^2
    critic_loss = mean over (b, j, i, k) of |tau_i - 1[delta < 0]| huber(delta)                      -> Adam on all critics
    actor_loss = mean_b(alpha log pi_b - mean_{j,i} critic_j(s, a_pi)[i]), the critics after their step -> Adam on the actor
    ent_coef_loss = -mean(log_ent_coef (log pi + target_entropy))                                   -> Adam on log_ent_coef ("auto" only)
    every target_update_interval-th update: target <- (1 - tau) target + tau param (critics only)

The ring stores the env's action in [lo, 1]; the critics take the scaled action in [-1, 1].  `done` is used as stored.

`tqc_update_numpy` (with `tqc_critic_numpy` / `tqc_actor_numpy`) is the float64 restatement with analytic backprop, no torch: the numerics
reference the tests hold the kernels to.  Limits: n_critics 1 .. 5, n_quantiles 1 .. 64, at most 128 pooled atoms, at least one kept.  Refused
with a message: `use_sde`, `action_noise`, a `learning_starts` warm-up, schedule objects (drive one with `set_rate()`),
`optimize_memory_usage`, `ent_coef` strings other than `auto` / `auto_<float>`.
"""
from __future__ import annotations

import math
import types

import numpy as np

from . import _abi
from .ppo import adam_numpy
from .sac import ACTOR_KEYS, EPS, LOG_STD_MAX, LOG_STD_MIN, SACCollector, SACLearner, init_sac_actor_weights, sac_actor_forward, sac_state
from .td3 import CRITIC_KEYS, _backward, _f64, _forward, scale_action


def init_tqc_critic_weights(D, P, n_quantiles=25, seed=0, h1=256, h2=256):
    """torch.nn.Linear-style uniform(-1/sqrt(in), 1/sqrt(in)) weights of one quantile critic (D + P -> h1 -> h2 -> n_quantiles) as numpy float32."""
    rng = np.random.default_rng(seed)
    out = []
    for n_in, n_out in ((D + P, h1), (h1, h2), (h2, int(n_quantiles))):
        k = 1.0 / np.sqrt(n_in)
        out += [rng.uniform(-k, k, (n_out, n_in)).astype(np.float32), rng.uniform(-k, k, n_out).astype(np.float32)]
    return out


def kept_atoms(n_critics, n_quantiles, drop):
    """K = n_critics (n_quantiles - top_quantiles_to_drop_per_net)."""
    return int(n_critics) * (int(n_quantiles) - int(drop))


def quantile_huber_terms(current, target):
    """The pairwise terms |tau_i - 1[delta < 0]| huber(delta) [B, nc, nq, K] and delta = target_k - current_{j,i} of the same shape, float64, from
    current quantiles [B, nc, nq] and target atoms [B, K]."""
    q, z = np.asarray(current, np.float64), np.asarray(target, np.float64)
    nq = q.shape[2]
    tau = (np.arange(nq, dtype=np.float64) + 0.5) / nq
    delta = z[:, None, None, :] - q[:, :, :, None]
    ad = np.abs(delta)
    huber = np.where(ad > 1.0, ad - 0.5, 0.5 * delta * delta)
    w = np.abs(tau[None, None, :, None] - (delta < 0.0))
    return w * huber, delta


def quantile_huber_loss_numpy(current, target):
    """sb3_contrib's quantile_huber_loss(current_quantiles [B, nc, nq], target_quantiles [B, K], sum_over_quantiles=False) in float64: the plain
    mean over all B nc nq K pairwise terms."""
    return float(quantile_huber_terms(current, target)[0].mean())


def tqc_critic_numpy(actor, critics, critics_target, obs, actions, reward, next_obs, done, eps_next, log_ent_coef=0.0, lo=-1.0, gamma=0.99,
                     top_quantiles_to_drop_per_net=2):
    """The critics' half of one update in float64.  eps_next [B, P]: the standard normals of a'.  Returns (grads: one list of six per critic,
    critic_loss, aux) with aux.z [B, K], aux.q / aux.tq [n_critics, B, n_quantiles], aux.sorted [B, M], aux.order [B, M] (pool indices, stable),
    aux.delta [B, nc, nq, K], aux.logp_next, aux.a_next and the forwards aux.f."""
    s, s2 = np.asarray(obs, np.float64), np.asarray(next_obs, np.float64)
    a = scale_action(np.asarray(actions, np.float64), lo)
    r, d = np.asarray(reward, np.float64).reshape(-1), np.asarray(done, np.float64).reshape(-1)
    B, nc = s.shape[0], len(critics)
    alpha = math.exp(float(log_ent_coef))
    fn = sac_actor_forward(actor, s2, eps_next)
    tq = np.stack([_forward(_f64(c), np.concatenate([s2, fn.a], 1), False).out for c in critics_target])   # [nc, B, nq]
    nq = tq.shape[2]
    K = kept_atoms(nc, nq, top_quantiles_to_drop_per_net)
    pool = tq.transpose(1, 0, 2).reshape(B, nc * nq)
    order = np.argsort(pool, axis=1, kind="stable")
    srt = np.take_along_axis(pool, order, 1)
    z = r[:, None] + ((1.0 - d) * gamma)[:, None] * (srt[:, :K] - alpha * fn.logp[:, None])
    xa = np.concatenate([s, a], 1)
    fs = [_forward(_f64(c), xa, False) for c in critics]
    q = np.stack([f.out for f in fs])
    terms, delta = quantile_huber_terms(q.transpose(1, 0, 2), z)
    w = np.abs(((np.arange(nq) + 0.5) / nq)[None, None, :, None] - (delta < 0.0))
    dq = -(w * np.clip(delta, -1.0, 1.0)).sum(3) / float(B * nc * nq * K)   # [B, nc, nq]
    grads = [_backward(_f64(c), f, dq[:, j, :])[0] for j, (c, f) in enumerate(zip(critics, fs))]
    return grads, float(terms.mean()), types.SimpleNamespace(z=z, q=q, tq=tq, sorted=srt, order=order, delta=delta, dq=dq, logp_next=fn.logp, a_next=fn.a, f=fs)


def tqc_actor_numpy(actor, critics, obs, eps, log_ent_coef=0.0, target_entropy=None, ent_coef_auto=True):
    """The actor's half in float64 with the standard normals eps [B, P]: (the actor's eight gradients, actor_loss, the gradient of
    log_ent_coef, ent_coef_loss, aux) with aux.fa the actor's forward, aux.fc the critics' forwards on (s, a_pi), aux.q [n_critics, B,
    n_quantiles], aux.d_mu and aux.d_log_std [B, P].  target_entropy None: -P.  A fixed coefficient has gradient and loss 0."""
    wa = _f64(actor)
    fa = sac_actor_forward(wa, obs, eps)
    B, D = fa.x.shape
    P = fa.a.shape[1]
    alpha, la = math.exp(float(log_ent_coef)), float(log_ent_coef)
    te = -float(P) if target_entropy is None else float(target_entropy)
    xa = np.concatenate([fa.x, fa.a], 1)
    fcs = [_forward(_f64(c), xa, False) for c in critics]
    q = np.stack([f.out for f in fcs])
    nc, nq = q.shape[0], q.shape[2]
    g = sum(_backward(_f64(c), f, np.full((B, nq), 1.0 / (nc * nq)))[1][:, D:] for c, f in zip(critics, fcs))   # d mean_{j,i} q / da
    omt = 1.0 - fa.a * fa.a
    du = (alpha * 2.0 * fa.a * omt / (omt + EPS) - g * omt) / B
    inside = (fa.raw > LOG_STD_MIN) & (fa.raw < LOG_STD_MAX)
    dls = np.where(inside, du * np.exp(fa.log_std) * fa.eps - alpha / B, 0.0)
    d2 = (du @ wa[4] + dls @ wa[6]) * (fa.z2 > 0.0)
    d1 = (d2 @ wa[2]) * (fa.z1 > 0.0)
    grads = [d1.T @ fa.x, d1.sum(0), d2.T @ fa.h1, d2.sum(0), du.T @ fa.h2, du.sum(0), dls.T @ fa.h2, dls.sum(0)]
    aloss = float((alpha * fa.logp - q.mean(axis=(0, 2))).mean())
    g_alpha = -float((fa.logp + te).mean()) if ent_coef_auto else 0.0
    return grads, aloss, g_alpha, (la * g_alpha if ent_coef_auto else 0.0), types.SimpleNamespace(fa=fa, fc=fcs, q=q, d_mu=du, d_log_std=dls)


tqc_state = sac_state   # a float64 learner state from initial weights: SAC's (masters, target critics, Adam's moments, log_ent_coef, n)


def tqc_update_numpy(st, obs, actions, reward, next_obs, done, eps, eps_next, lo=-1.0, lr=3e-4, tau=0.005, gamma=0.99, target_update_interval=1,
                     target_entropy=None, ent_coef_auto=True, top_quantiles_to_drop_per_net=2, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """One update of TQC on the float64 state `st` (tqc_state), in place.  eps / eps_next [B, P]: the standard normals of a_pi on s / a' on s'.
    Returns a namespace: critic_loss, actor_loss, ent_coef_loss, ent_coef (alpha of this update), z, log_pi, log_pi_next, critic_grads,
    actor_grads, ent_coef_grad."""
    la = float(st.log_ent_coef)
    cg, closs, aux = tqc_critic_numpy(st.actor, st.critics, st.critics_target, obs, actions, reward, next_obs, done, eps_next, la, lo, gamma,
                                      top_quantiles_to_drop_per_net)
    st.n += 1
    for j, g in enumerate(cg):
        for i in range(6):
            st.critics[j][i], st.m_critics[j][i], st.v_critics[j][i] = adam_numpy(st.critics[j][i], st.m_critics[j][i], st.v_critics[j][i], g[i], st.n, lr, beta1,
                                                                                   beta2, adam_eps)
    ag, aloss, ga, eloss, aaux = tqc_actor_numpy(st.actor, st.critics, obs, eps, la, target_entropy, ent_coef_auto)
    for i in range(8):
        st.actor[i], st.m_actor[i], st.v_actor[i] = adam_numpy(st.actor[i], st.m_actor[i], st.v_actor[i], ag[i], st.n, lr, beta1, beta2, adam_eps)
    if ent_coef_auto:
        st.log_ent_coef, st.m_alpha, st.v_alpha = adam_numpy(st.log_ent_coef, st.m_alpha, st.v_alpha, np.float64(ga), st.n, lr, beta1, beta2, adam_eps)
    if st.n % int(target_update_interval) == 0:
        for tgt, src in zip(st.critics_target, st.critics):
            for i in range(6):
                tgt[i] = (1.0 - tau) * tgt[i] + tau * src[i]
    return types.SimpleNamespace(critic_loss=closs, actor_loss=aloss, ent_coef_loss=eloss, ent_coef=math.exp(la), z=aux.z, log_pi=aaux.fa.logp,
                                 log_pi_next=aux.logp_next, critic_grads=cg, actor_grads=ag, ent_coef_grad=ga, aux=aux, actor_aux=aaux)


class TQCCollector(SACCollector):
    """`SACCollector` for a `TQCLearner`: the same ring and the same stochastic actor, the episodes through `ev2g_tqc_collect`."""

    tqc = property(lambda self: getattr(self.learner, "learner", None))   # the device object

    @property
    def sac(self):   # (hasattr(collector, "sac") is how SACLearner tells its collector: this one is not)
        raise AttributeError("a TQCCollector holds no SAC object (its device object is `tqc`)")

    def collect_episode(self, deterministic=False):
        if not self.tqc:
            raise RuntimeError("collect_episode: no TQCLearner is bound to this collector (the device object holds the collection actor)")
        b, eng = self.head, self.eng
        eng.tqc_collect(self.tqc, self.T - eng.current_step, self.obs[b], self.actions[b], self.reward[b], self.done[b], self.mask[b], deterministic)
        return self._advance()


class TQCLearner(SACLearner):
    """sb3_contrib's TQC.train() on the device behind a TQCCollector: `SACLearner`'s methods (`train()`, `learn()`, `get_weights()`,
    `get_grads()`, `state_dict()`, `set_rate()`, `counters()`, `close()`) over the `ev2g_tqc_*` entries, with `n_quantiles` and
    `top_quantiles_to_drop_per_net`."""

    PRESET = dict(SACLearner.PRESET, n_quantiles=25, top_quantiles_to_drop_per_net=2)
    ABI, COLLECTOR = "tqc", "TQCCollector"
    QUANTILE_KEYS = ()              # (the two quantile keys are this learner's own: not refused)
    OUT_OF_SCOPE = "state-dependent exploration, exploration noise, a random warm-up and the replay buffer's memory options are out of scope"

    def _check_quantiles(self, cfg):
        nc, nq, d = int(cfg["n_critics"]), int(cfg["n_quantiles"]), int(cfg["top_quantiles_to_drop_per_net"])
        name = type(self).__name__
        if not 1 <= nc <= _abi.TQC_MAX_CRITICS:
            raise ValueError(f"{name}: n_critics {nc} is outside 1 .. {_abi.TQC_MAX_CRITICS}")
        if not 1 <= nq <= _abi.TQC_MAX_QUANTILES:
            raise ValueError(f"{name}: n_quantiles {nq} is outside 1 .. {_abi.TQC_MAX_QUANTILES}")
        if nc * nq > _abi.TQC_MAX_ATOMS:
            raise ValueError(f"{name}: n_critics * n_quantiles {nc * nq} is outside 1 .. {_abi.TQC_MAX_ATOMS}")
        if not 0 <= d <= nq - 1:
            raise ValueError(f"{name}: top_quantiles_to_drop_per_net {d} is outside 0 .. {nq - 1}")

    def _init_critics(self, D, P, h1, h2, seed, cfg):
        self._check_quantiles(cfg)
        return [init_tqc_critic_weights(D, P, int(cfg["n_quantiles"]), seed=int(seed) + 1 + j, h1=h1, h2=h2) for j in range(int(cfg["n_critics"]))]

    def _shape(self, D, h1, h2, P, cfg):
        self._check_quantiles(cfg)
        return (D, h1, h2, P, int(cfg["n_critics"]), int(cfg["n_quantiles"]))

    tqc = property(lambda self: self.learner)   # the device object

    @property
    def sac(self):   # (as on TQCCollector: the device object is no SAC object, and ev2g_sac_* entries refuse it)
        raise AttributeError("a TQCLearner holds no SAC object (its device object is `tqc`)")
    kept_atoms = property(lambda self: kept_atoms(self.shape[4], self.shape[5], self.cfg["top_quantiles_to_drop_per_net"]))


def make_learner(algo, collector, **kw):
    """The learner of sb3_contrib's "TQC" behind a TQCCollector.  SAC is ev2gym_amd.sac.make_learner's, TD3 and DDPG ev2gym_amd.td3.make_learner's."""
    if str(algo).lower() != "tqc":
        raise ValueError(f"make_learner: {algo} is not supported here (TQC is; SAC is ev2gym_amd.sac.make_learner's, TD3 and DDPG are "
                         "ev2gym_amd.td3.make_learner's)")
    return TQCLearner(collector, **kw)


__all__ = ["TQCCollector", "TQCLearner", "make_learner", "tqc_update_numpy", "tqc_critic_numpy", "tqc_actor_numpy", "tqc_state", "quantile_huber_loss_numpy",
           "quantile_huber_terms", "init_tqc_critic_weights", "init_sac_actor_weights", "kept_atoms", "ACTOR_KEYS", "CRITIC_KEYS"]
