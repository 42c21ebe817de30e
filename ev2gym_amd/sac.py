"""SAC on the device: SB3's `SAC.train()` for `SACPolicy` (MlpPolicy, Box actions, `use_sde=False`) behind a device replay ring
(`csrc/ev2g_sac.h`, `ev2g_sac_*`).

`SACCollector(engine, actor_weights, lo)` is the replay ring of `DeviceReplayCollector` filled by the STOCHASTIC actor: `ev2g_sac_collect` runs
squashed-Gaussian actor launch -> env step per vector step, straight into the ring's blocks.  `SACLearner(collector)` creates the device object
(learner and collection actor are one object: the learner rewrites the actor's packed weights after every update) and binds it to the collector.
`train(gradient_steps, batch_size)` runs sample -> update on the device with one synchronisation at the end; `learn(total_timesteps)` alternates
`collector.collect_episode()` and `train()`.

Per update on (s, a~, r, s', done) of B rows, alpha = exp(log_ent_coef) as it stands before the update (SB3's arithmetic):

    h = ReLU(W2 ReLU(W1 s + b1) + b2);  mu = Wmu h + bmu;  log_std = clamp(Wls h + bls, -20, 2);  a = tanh(mu + exp(log_std) eps)
    log pi = sum_p [-eps^2 / 2 - log_std - log(2 pi) / 2] - sum_p log(1 - a^2 + 1e-6)
    ent_coef_loss = -mean(log_ent_coef (log pi + target_entropy))                                  -> Adam on log_ent_coef ("auto" only), LAST
    y = r + (1 - done) gamma (min_j critic_target_j(s', a') - alpha log pi');  critic_loss = 0.5 sum_j mean((critic_j(s, a~) - y)^2) -> Adam
    actor_loss = mean(alpha log pi - min_j critic_j(s, a_pi)), the critics after their step       -> Adam on the actor
    every target_update_interval-th update: target <- (1 - tau) target + tau param (critics only)

The Gaussian term is the reduced form of `Normal(mu, sigma).log_prob(mu + sigma eps)`: identical in exact arithmetic, but the literal form cancels
`(mu + sigma eps) - mu`, which loses every digit once sigma = e^-20 (tests/test_sac_cpu.py shows both).  The ring stores the env's action in
[lo, 1]; the critics take SB3's scaled action in [-1, 1].  `done` is used as stored (the reference registers no time limit).

`sac_update_numpy` (with `sac_critic_numpy` / `sac_actor_numpy`) is the float64 restatement with analytic backprop, no torch: the numerics
reference the tests hold the kernels to.  Refused with a message: `use_sde`, `action_noise`, a `learning_starts` warm-up, schedule objects (drive
one with `set_rate()`), `optimize_memory_usage`, TQC's arguments (TQC is `ev2gym_amd.tqc`, over this module's actor and learner class), `ent_coef`
strings other than `auto` / `auto_<float>`.
"""
from __future__ import annotations

import math
import types

import numpy as np

from . import _abi
from .ppo import adam_numpy
from .sb3_vec_env import ReplayRing
from .td3 import CRITIC_KEYS, MAX_BLOCKS, _backward, _f64, _forward, init_critic_weights, scale_action

ACTOR_KEYS = tuple(f"{n}.{k}" for n in ("latent_pi.0", "latent_pi.2", "mu", "log_std") for k in ("weight", "bias"))
LOG_STD_MIN, LOG_STD_MAX, EPS = -20.0, 2.0, 1e-6


def init_sac_actor_weights(D, P, seed=0, h1=256, h2=256):
    """torch.nn.Linear-style uniform(-1/sqrt(in), 1/sqrt(in)) weights of a SAC actor (D -> h1 -> h2 -> mu [P], log_std [P]) as the eight numpy
    float32 arrays of SB3's parameter order."""
    rng = np.random.default_rng(seed)
    out = []
    for n_in, n_out in ((D, h1), (h1, h2), (h2, P), (h2, P)):
        k = 1.0 / np.sqrt(n_in)
        out += [rng.uniform(-k, k, (n_out, n_in)).astype(np.float32), rng.uniform(-k, k, n_out).astype(np.float32)]
    return out


def unscale_action(a, lo):
    """The tanh action in [-1, 1] as the env takes it, in [lo, 1] (SB3's unscale_action)."""
    return 0.5 * (a + 1.0) if float(lo) == 0.0 else a


def parse_ent_coef(ent_coef):
    """SB3's `ent_coef` argument -> (initial or fixed coefficient, auto?).  "auto" starts at 1.0, "auto_0.1" at 0.1; a number is fixed."""
    if isinstance(ent_coef, str):
        if ent_coef == "auto":
            return 1.0, True
        if ent_coef.startswith("auto_"):
            try:
                v = float(ent_coef[5:])
            except ValueError:
                v = float("nan")
            if v > 0.0 and math.isfinite(v):
                return v, True
        raise ValueError(f"SAC: ent_coef {ent_coef!r} is not supported ('auto', 'auto_<positive float>' or a positive number are)")
    v = float(ent_coef)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"SAC: ent_coef {ent_coef!r} must be a positive finite number")
    return v, False


def sac_actor_forward(actor, obs, eps):
    """The actor in float64 on obs [B, D] with the standard normals eps [B, P]: a namespace of the trunk's forward values (z1, h1, z2, h2), mu,
    the raw and the clamped log_std, a = tanh(u) and log pi [B]."""
    w = _f64(actor)
    s, eps = np.asarray(obs, np.float64), np.asarray(eps, np.float64)
    z1 = s @ w[0].T + w[1]; h1 = np.maximum(z1, 0.0)
    z2 = h1 @ w[2].T + w[3]; h2 = np.maximum(z2, 0.0)
    mu, raw = h2 @ w[4].T + w[5], h2 @ w[6].T + w[7]
    ls = np.clip(raw, LOG_STD_MIN, LOG_STD_MAX)
    a = np.tanh(mu + np.exp(ls) * eps)
    logp = (-0.5 * eps * eps - ls - 0.5 * math.log(2.0 * math.pi)).sum(1) - np.log(1.0 - a * a + EPS).sum(1)
    return types.SimpleNamespace(x=s, z1=z1, h1=h1, z2=z2, h2=h2, mu=mu, raw=raw, log_std=ls, eps=eps, a=a, logp=logp)


def sac_critic_numpy(actor, critics, critics_target, obs, actions, reward, next_obs, done, eps_next, log_ent_coef=0.0, lo=-1.0, gamma=0.99):
    """The critics' half of one update in float64.  eps_next [B, P]: the standard normals of a'.  Returns (grads: one list of six per critic,
    critic_loss, aux) with aux.y, aux.q / aux.tq [n_critics, B], aux.logp_next, aux.a_next and the forwards aux.f."""
    s, s2 = np.asarray(obs, np.float64), np.asarray(next_obs, np.float64)
    a = scale_action(np.asarray(actions, np.float64), lo)
    r, d = np.asarray(reward, np.float64).reshape(-1), np.asarray(done, np.float64).reshape(-1)
    B = s.shape[0]
    alpha = math.exp(float(log_ent_coef))
    fn = sac_actor_forward(actor, s2, eps_next)
    tq = np.stack([_forward(_f64(c), np.concatenate([s2, fn.a], 1), False).out[:, 0] for c in critics_target])
    y = r + (1.0 - d) * gamma * (tq.min(axis=0) - alpha * fn.logp)
    xa = np.concatenate([s, a], 1)
    grads, q, fs, loss = [], [], [], 0.0
    for c in critics:
        c = _f64(c)
        f = _forward(c, xa, False)
        qj = f.out[:, 0]
        loss += 0.5 * float(((qj - y) ** 2).mean())
        grads.append(_backward(c, f, ((qj - y) / B)[:, None])[0])
        q.append(qj); fs.append(f)
    return grads, loss, types.SimpleNamespace(y=y, q=np.stack(q), tq=tq, logp_next=fn.logp, a_next=fn.a, f=fs)


def sac_actor_numpy(actor, critics, obs, eps, log_ent_coef=0.0, target_entropy=None, ent_coef_auto=True):
    """The actor's half in float64 with the standard normals eps [B, P]: (the actor's eight gradients, actor_loss, the gradient of
    log_ent_coef, ent_coef_loss, aux) with aux.fa the actor's forward, aux.q [n_critics, B] on (s, a_pi), aux.argmin [B], aux.d_mu and
    aux.d_log_std [B, P].  target_entropy None: -P.  A fixed coefficient has gradient and loss 0."""
    wa = _f64(actor)
    fa = sac_actor_forward(wa, obs, eps)
    B, D = fa.x.shape
    P = fa.a.shape[1]
    alpha, la = math.exp(float(log_ent_coef)), float(log_ent_coef)
    te = -float(P) if target_entropy is None else float(target_entropy)
    xa = np.concatenate([fa.x, fa.a], 1)
    q, dA, fcs = [], [], []
    for c in critics:
        c = _f64(c)
        f = _forward(c, xa, False)
        q.append(f.out[:, 0]); fcs.append(f)
        dA.append(_backward(c, f, np.ones((B, 1)))[1][:, D:])
    q = np.stack(q)
    j = q.argmin(axis=0)
    g = np.choose(j[:, None], dA) if len(dA) > 1 else dA[0]
    omt = 1.0 - fa.a * fa.a
    du = (alpha * 2.0 * fa.a * omt / (omt + EPS) - g * omt) / B
    inside = (fa.raw > LOG_STD_MIN) & (fa.raw < LOG_STD_MAX)
    dls = np.where(inside, du * np.exp(fa.log_std) * fa.eps - alpha / B, 0.0)
    d2 = (du @ wa[4] + dls @ wa[6]) * (fa.z2 > 0.0)
    d1 = (d2 @ wa[2]) * (fa.z1 > 0.0)
    grads = [d1.T @ fa.x, d1.sum(0), d2.T @ fa.h1, d2.sum(0), du.T @ fa.h2, du.sum(0), dls.T @ fa.h2, dls.sum(0)]
    aloss = float((alpha * fa.logp - q.min(axis=0)).mean())
    g_alpha = -float((fa.logp + te).mean()) if ent_coef_auto else 0.0
    return grads, aloss, g_alpha, (la * g_alpha if ent_coef_auto else 0.0), types.SimpleNamespace(fa=fa, fc=fcs, q=q, argmin=j, d_mu=du, d_log_std=dls)


def sac_state(actor, critics, ent_coef=1.0):
    """A float64 learner state from initial weights: masters, target critics (copies), Adam's moments at zero, log_ent_coef, the counters."""
    actor, critics = _f64(actor), [_f64(c) for c in critics]
    zeros = lambda ws: [np.zeros_like(a) for a in ws]  # noqa: E731
    return types.SimpleNamespace(actor=actor, critics=critics, critics_target=[[a.copy() for a in c] for c in critics], m_actor=zeros(actor), v_actor=zeros(actor),
                                 m_critics=[zeros(c) for c in critics], v_critics=[zeros(c) for c in critics], log_ent_coef=np.float64(math.log(ent_coef)),
                                 m_alpha=np.float64(0.0), v_alpha=np.float64(0.0), n=0)


def sac_update_numpy(st, obs, actions, reward, next_obs, done, eps, eps_next, lo=-1.0, lr=3e-4, tau=0.005, gamma=0.99, target_update_interval=1,
                     target_entropy=None, ent_coef_auto=True, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """One update of SAC on the float64 state `st` (sac_state), in place.  eps / eps_next [B, P]: the standard normals of a_pi on s / a' on s'.
    Returns a namespace: critic_loss, actor_loss, ent_coef_loss, ent_coef (alpha of this update), y, log_pi, critic_grads, actor_grads,
    ent_coef_grad."""
    la = float(st.log_ent_coef)
    cg, closs, aux = sac_critic_numpy(st.actor, st.critics, st.critics_target, obs, actions, reward, next_obs, done, eps_next, la, lo, gamma)
    st.n += 1
    for j, g in enumerate(cg):
        for i in range(6):
            st.critics[j][i], st.m_critics[j][i], st.v_critics[j][i] = adam_numpy(st.critics[j][i], st.m_critics[j][i], st.v_critics[j][i], g[i], st.n, lr, beta1,
                                                                                   beta2, adam_eps)
    ag, aloss, ga, eloss, aaux = sac_actor_numpy(st.actor, st.critics, obs, eps, la, target_entropy, ent_coef_auto)
    for i in range(8):
        st.actor[i], st.m_actor[i], st.v_actor[i] = adam_numpy(st.actor[i], st.m_actor[i], st.v_actor[i], ag[i], st.n, lr, beta1, beta2, adam_eps)
    if ent_coef_auto:
        st.log_ent_coef, st.m_alpha, st.v_alpha = adam_numpy(st.log_ent_coef, st.m_alpha, st.v_alpha, np.float64(ga), st.n, lr, beta1, beta2, adam_eps)
    if st.n % int(target_update_interval) == 0:
        for tgt, src in zip(st.critics_target, st.critics):
            for i in range(6):
                tgt[i] = (1.0 - tau) * tgt[i] + tau * src[i]
    return types.SimpleNamespace(critic_loss=closs, actor_loss=aloss, ent_coef_loss=eloss, ent_coef=math.exp(la), y=aux.y, log_pi=aaux.fa.logp,
                                 log_pi_next=aux.logp_next, critic_grads=cg, actor_grads=ag, ent_coef_grad=ga, aux=aux, actor_aux=aaux)


class SACCollector(ReplayRing):
    """The device replay ring of `DeviceReplayCollector` filled by SAC's stochastic actor (`ev2g_sac_collect`): blocks, `head`, `filled`, `cap`,
    `collect_episode(deterministic=False)`, `terminal_observation`, `sample`.

    `weights` are the actor's eight float32 arrays (SB3's order); they seed the `SACLearner` that is bound next.  The device object is the
    learner's -- learner and collection actor are one object -- so `collect_episode()` needs a bound `SACLearner`."""

    def __init__(self, engine, weights, lo: float, capacity_episodes: int = 2, offset_stride=None, use_torch=None):
        weights = [np.ascontiguousarray(w, np.float32) for w in weights]
        if len(weights) != 8:
            raise ValueError("SACCollector: the actor's eight arrays are needed (latent_pi.0, latent_pi.2, mu, log_std: weight and bias each)")
        self.lo = float(lo)
        self.weights = weights
        self.learner = None      # the SACLearner bound to the ring (it registers itself)
        self._init_ring(engine, capacity_episodes, offset_stride, use_torch)

    sac = property(lambda self: getattr(self.learner, "learner", None))   # the device object

    def collect_episode(self, deterministic=False):
        """One whole episode of every env into the head block with the stochastic actor (deterministic: a = tanh(mu), nothing drawn); statistics
        of the finished episode; reset onto the next pool window.  Returns the index of the block that was filled."""
        if not self.sac:
            raise RuntimeError("collect_episode: no SACLearner is bound to this collector (the device object holds the collection actor)")
        b, eng = self.head, self.eng
        eng.sac_collect(self.sac, self.T - eng.current_step, self.obs[b], self.actions[b], self.reward[b], self.done[b], self.mask[b], deterministic)
        return self._advance()

    def close(self):
        if self.learner is not None:
            self.learner.close()


class SACLearner:
    """SB3's SAC.train() on the device behind a SACCollector.

    The learner takes `actor` (default: the collector's weights) and `critics` (default: torch.nn.Linear-style draws from `seed`) as float32
    masters on the device; the collection actor's packed weights are rewritten from the masters after every update.  `state_dict()` reads the
    parameters back under SB3's keys; `close()` (or closing the collector or the engine, in any order) frees the device object."""

    PRESET = dict(n_critics=2, lr=3e-4, tau=0.005, gamma=0.99, batch_size=256, target_update_interval=1, ent_coef="auto", target_entropy="auto")
    # what ev2gym_amd.tqc.TQCLearner overrides: the entries' prefix (engine.<ABI>_create, ...; the collector's attribute of that name), the collector's name, the keys refused as TQC's
    ABI, COLLECTOR = "sac", "SACCollector"
    QUANTILE_KEYS = ("top_quantiles_to_drop_per_net", "n_quantiles")
    OUT_OF_SCOPE = ("state-dependent exploration, exploration noise, a random warm-up, the replay buffer's memory options and TQC's quantile critics are "
                    "out of scope")

    def _eng(self, entry):
        return getattr(self.eng, f"{self.ABI}_{entry}")

    def _init_critics(self, D, P, h1, h2, seed, cfg):
        return [init_critic_weights(D, P, seed=int(seed) + 1 + j, h1=h1, h2=h2) for j in range(int(cfg["n_critics"]))]

    def _shape(self, D, h1, h2, P, cfg):
        return (D, h1, h2, P, int(cfg["n_critics"]))

    def __init__(self, collector, actor=None, critics=None, seed=0, sample_seed=None, **kw):
        name = type(self).__name__
        for k, bad in (("use_sde", lambda v: bool(v)), ("use_sde_at_warmup", lambda v: bool(v)), ("action_noise", lambda v: v is not None),
                       ("learning_starts", lambda v: int(v) != 0), ("optimize_memory_usage", lambda v: bool(v)), ("handle_timeout_termination", lambda v: bool(v)),
                       *((k, lambda v: True) for k in self.QUANTILE_KEYS)):
            if k in kw and bad(kw.pop(k)):
                raise ValueError(f"{name}: {k} is not supported ({self.OUT_OF_SCOPE}; see the module docstring)")
        cfg = dict(self.PRESET, **{k: kw.pop(k) for k in list(kw) if k in self.PRESET or k in ("beta1", "beta2", "adam_eps")})
        if kw:
            raise ValueError(f"{name}: {sorted(kw)[0]} is not supported (see the module docstring)")
        if any(callable(cfg[k]) for k in ("lr", "tau", "gamma")):
            raise ValueError(f"{name}: lr, tau and gamma are numbers; drive a schedule with set_rate() between train() calls")
        self.learner, self._bufs = None, None   # (close() works on a learner whose creation failed)
        ent0, self.ent_coef_auto = parse_ent_coef(cfg.pop("ent_coef"))
        te = cfg.pop("target_entropy")
        if isinstance(te, str) and te != "auto":
            raise ValueError(f"{name}: target_entropy {te!r} is not supported ('auto' or a number are)")
        self.batch_size = int(cfg.pop("batch_size"))
        if not 1 <= self.batch_size <= _abi.TD3_MAX_BATCH:
            raise ValueError(f"{name}: batch_size {self.batch_size} is outside 1 .. {_abi.TD3_MAX_BATCH}")
        self.collector, self.eng = collector, collector.eng
        if getattr(getattr(collector, "learner", None), "learner", None):
            raise ValueError(f"{name}: the collector already has a learner")
        if not hasattr(collector, self.ABI):
            raise ValueError(f"{name}: the collector is not a {self.COLLECTOR} (a DeviceReplayCollector owns a deterministic policy object)")
        if collector.cap - 1 > MAX_BLOCKS:
            raise ValueError(f"{name}: the collector's ring holds up to {collector.cap - 1} complete episodes, the sampler's table {MAX_BLOCKS}: "
                             f"capacity_episodes must be at most {MAX_BLOCKS + 1}")
        actor = [np.ascontiguousarray(a, np.float32) for a in (actor if actor is not None else collector.weights)]
        (h1, D), h2, P = actor[0].shape, actor[2].shape[0], actor[4].shape[0]
        self.shape = self._shape(D, h1, h2, P, cfg)
        if critics is None:
            critics = self._init_critics(D, P, h1, h2, seed, cfg)
        self.cfg, self.lr = cfg, float(cfg["lr"])
        self.sample_seed = int(seed if sample_seed is None else sample_seed)
        self.sample_counter = 0     # the draw counter of the next sampled batch (ev2g_replay_sample)
        self.num_timesteps = 0
        self.last_losses = None
        self.learner = self._eng("create")(actor, critics, collector.lo, seed=seed, ent_coef=ent0, ent_coef_auto=int(self.ent_coef_auto),
                                           target_entropy_auto=int(te == "auto"), target_entropy=0.0 if te == "auto" else float(te), **cfg)
        collector.learner = self

    sac = property(lambda self: self.learner)   # the device object

    def set_rate(self, lr):
        """The learning rate of the following updates, of all three optimisers (how a schedule is driven from Python)."""
        self.lr = float(lr)
        self._eng("set_rate")(self.learner, self.lr)

    def counters(self):
        """(updates, Polyak steps among them, the learner's next draw base, the collection actor's sampling launches)."""
        return self._eng("counters")(self.learner)

    def complete_blocks(self):
        """The ring's complete blocks, newest first: the list the sampler draws from."""
        c = self.collector
        return [(c.head - 1 - i) % c.cap for i in range(c.filled)]

    def _batch_buffers(self, B, steps):
        key = (B, steps)
        if self._bufs is None or self._bufs[0] != key:
            if self._bufs is not None:
                for b in self._bufs[1]:
                    b.free()
            c, e = self.collector, self.eng
            self._bufs = (key, [e.empty((B, c.D), np.float32), e.empty((B, c.P), np.float32), e.empty((B,), np.float32), e.empty((B, c.D), np.float32),
                                e.empty((B,), np.uint8), e.empty((steps, 4), np.float32)])
        return self._bufs[1]

    def train(self, gradient_steps, batch_size=None):
        """gradient_steps x (sample a batch from the complete blocks -> one update), all enqueued on the engine's stream, one synchronisation at
        the end.  Returns the means of critic_loss, actor_loss, ent_coef_loss and ent_coef, and n_updates."""
        B, steps = int(batch_size or self.batch_size), int(gradient_steps)
        if steps < 1:
            raise ValueError("train: gradient_steps must be at least 1")
        blocks = self.complete_blocks()
        if not blocks:
            raise RuntimeError("train: the replay ring holds no complete episode (collector.collect_episode() first)")
        c, eng, update = self.collector, self.eng, self._eng("update")
        obs, act, rew, nxt, done, losses = self._batch_buffers(B, steps)
        ring = [(c.obs[b], c.actions[b], c.reward[b], c.done[b]) for b in blocks]
        for k in range(steps):
            eng.replay_sample(ring, c.T, c.E, c.D, c.P, B, self.sample_seed, self.sample_counter, obs, act, rew, nxt, done)
            self.sample_counter += 1
            update(self.learner, obs, act, rew, nxt, done, B, losses.at(4 * k))
        self.last_losses = losses.to_host()   # (synchronises)
        mean = self.last_losses.astype(np.float64).mean(axis=0)
        return dict(critic_loss=float(mean[0]), actor_loss=float(mean[1]), ent_coef_loss=float(mean[2]), ent_coef=float(mean[3]), n_updates=self.counters()[0])

    def learn(self, total_timesteps, gradient_steps=None, batch_size=None):
        """collector.collect_episode() and train() in turn until total_timesteps env steps were collected; returns what every train() returned.
        gradient_steps defaults to T: one update per collected vector step.  As with TD3Learner the policy changes PER EPISODE here."""
        out = []
        target = self.num_timesteps + int(total_timesteps)
        while self.num_timesteps < target:
            self.collector.collect_episode()
            self.num_timesteps += self.collector.T * self.collector.E
            out.append(self.train(self.collector.T if gradient_steps is None else gradient_steps, batch_size))
        return out

    def ent_coef(self):
        """alpha = exp(log_ent_coef) as it stands."""
        return float(np.exp(np.float64(self._eng("get_ent_coef")(self.learner)[0])))

    def get_weights(self, target=False):
        """(actor eight arrays, [critic six arrays, ...]) read back from the device, or (target) (None, the target critics)."""
        flat = self._eng("get_weights")(self.learner, self.shape, target)
        if target:
            return None, [flat[6 * j:6 + 6 * j] for j in range(self.shape[4])]
        return flat[:8], [flat[8 + 6 * j:14 + 6 * j] for j in range(self.shape[4])]

    def get_grads(self):
        """(actor eight arrays, [critic six arrays, ...], the gradient of log_ent_coef) of the last gradient of each half."""
        flat, g = self._eng("get_grads")(self.learner, self.shape)
        return flat[:8], [flat[8 + 6 * j:14 + 6 * j] for j in range(self.shape[4])], g

    def state_dict(self):
        """The parameters under SB3's keys: actor.{latent_pi.0,latent_pi.2,mu,log_std}.*, critic.qf{j}.{0,2,4}.*, critic_target.qf{j}.*, and
        log_ent_coef [1] (also for a fixed coefficient: its logarithm)."""
        actor, critics = self.get_weights()
        out = {f"actor.{k}": a for k, a in zip(ACTOR_KEYS, actor)}
        for prefix, cs in (("critic", critics), ("critic_target", self.get_weights(True)[1])):
            for j, c in enumerate(cs):
                out.update({f"{prefix}.qf{j}.{k}": a for k, a in zip(CRITIC_KEYS, c)})
        out["log_ent_coef"] = self._eng("get_ent_coef")(self.learner)[:1].copy()
        return out

    def close(self):
        if self.learner:
            self._eng("destroy")(self.learner)   # (nothing happens if the engine already took it along)
        self.learner = None
        if getattr(self.collector, "learner", None) is self:
            self.collector.learner = None
        if self._bufs is not None and self.eng._h:
            for b in self._bufs[1]:
                b.free()
        self._bufs = None


def make_learner(algo, collector, **kw):
    """The learner of SB3's "SAC" behind a SACCollector.  TD3 and DDPG are ev2gym_amd.td3.make_learner's; TQC is refused."""
    if str(algo).lower() != "sac":
        raise ValueError(f"make_learner: {algo} is not supported here (SAC is; TD3 and DDPG are ev2gym_amd.td3.make_learner's, TQC is out of scope)")
    return SACLearner(collector, **kw)


__all__ = ["SACCollector", "SACLearner", "make_learner", "sac_update_numpy", "sac_critic_numpy", "sac_actor_numpy", "sac_actor_forward", "sac_state",
           "init_sac_actor_weights", "unscale_action", "parse_ent_coef", "ACTOR_KEYS"]
