"""The third learner of the on-policy collector: sb3_contrib's `TRPO.train()` with default settings, on the device (`csrc/ev2g_trpo.h`,
`ev2g_trpo_*`).

`TRPOLearner(collector)` binds a device learner to the collector's `GaussianActorCritic`; `train(batch)` makes ONE natural-gradient policy step
over the `RolloutBatch` -- the objective's gradient, conjugate gradient on Fisher-vector products, the backtracking line search, all queued on
the engine's stream without a host round trip -- then `n_critic_updates` passes of Adam minibatches on the value function alone, without the
batch or the weights leaving the device; `learn(total_timesteps)` alternates `collector.collect()` and `train()`.

`trpo_step_numpy` is the float64 statement of the policy step (analytic gradient and analytic Fisher product, no torch): the numerics reference
the tests hold the kernels to.  sb3_contrib is not a dependency; the formulas follow `TRPO.train()` for `ActorCriticPolicy` on a Box action
space, theta being the parameters without "value" in their name, flat in `named_parameters()` order (`ACTOR_ORDER`):

    A^ = (A - mean(A)) / (std(A) + 1e-8), unbiased std, if normalize_advantage and there is more than one row
    J(theta) = mean(A^ exp(lp - old_lp)),  g = grad J
    KL(theta) = mean_i sum_p [ls0 - ls + (e^{2 ls} + (mu - mu0)^2) / (2 e^{2 ls0}) - 1/2]      (new || old; mu0, ls0 at theta0)
    H v = grad(grad KL . v) + cg_damping v = J_mu^T diag(e^{-2 ls0}) J_mu v / B + 2 v_log_std + cg_damping v   (exact at theta0)
    conjugate gradient on H x = g (at most cg_max_steps updates of x, exits at r . r < 1e-10),  beta = sqrt(2 target_kl / (x . Hx))
    theta = theta0 + c beta x for c = 1, s, s^2, ...: accepted when KL < target_kl and J > J(theta0); theta0 when no try is

DEVIATION: a non-finite or non-positive x . Hx (x = 0 from a vanishing gradient included) fails the step and leaves theta0 in place, on the
device and here; sb3_contrib would write NaN parameters.  The critic is `value_loss = mean((R - v)^2)`, `torch.optim.Adam(lr, eps=1e-5)`, no
gradient clipping, the actor's parameters untouched.  Out of scope, refused where a caller could ask for them: `use_sde`, shared trunks,
learning-rate schedules as objects (`set_rate` between calls drives one), action masks.
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from .onpolicy import SB3_KEYS, SB3_LOG_STD
from .ppo import _Learner, check_batch

ACTOR_ORDER = tuple(_abi.AC_PARAMS[i] for i in _abi.TRPO_ACTOR)   # log_std, pi_W1, pi_b1, pi_W2, pi_b2, action_W, action_b
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
RHO_MIN = 1e-10


def actor_arrays(weights, log_std):
    """The actor's seven arrays (float64) of a network's twelve arrays and log_std, in ACTOR_ORDER."""
    every = [np.asarray(a, np.float64) for a in weights] + [np.asarray(log_std, np.float64)]
    return [every[i] for i in _abi.TRPO_ACTOR]


def flatten(arrays):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in arrays])


def unflatten(v, like):
    out, o = [], 0
    for a in like:
        out.append(np.asarray(v[o:o + a.size], np.float64).reshape(a.shape))
        o += a.size
    return out


class _Actor:
    """The float64 policy trunk on fixed rows: objective, gradient, KL and Fisher product as functions of the actor's seven arrays."""

    def __init__(self, obs, actions, old_log_prob, advantages, idx, activation, normalize_advantage):
        idx = np.asarray(idx, np.int64)
        self.x, self.a = np.asarray(obs, np.float64)[idx], np.asarray(actions, np.float64)[idx]
        self.old, A = np.asarray(old_log_prob, np.float64)[idx], np.asarray(advantages, np.float64)[idx]
        self.B = len(idx)
        if normalize_advantage and self.B > 1:
            A = (A - A.mean()) / (A.std(ddof=1) + 1e-8)
        self.A = A
        tanh = activation == "tanh"
        self.act = np.tanh if tanh else (lambda z: np.maximum(z, 0.0))
        self.dact = (lambda h: 1.0 - h * h) if tanh else (lambda h: (h > 0.0).astype(np.float64))

    def forward(self, th):
        ls, W1, b1, W2, b2, W3, b3 = th
        h1 = self.act(self.x @ W1.T + b1)
        h2 = self.act(h1 @ W2.T + b2)
        return h1, h2, h2 @ W3.T + b3

    def _back(self, th, h1, h2, d_mu):
        _, W1, b1, W2, b2, W3, b3 = th
        d2 = (d_mu @ W3) * self.dact(h2)
        d1 = (d2 @ W2) * self.dact(h1)
        return [d1.T @ self.x, d1.sum(0), d2.T @ h1, d2.sum(0), d_mu.T @ h2, d_mu.sum(0)]

    def objective(self, th, with_grad=False):
        ls = th[0]
        h1, h2, mu = self.forward(th)
        iv, d = np.exp(-2.0 * ls), self.a - mu
        lp = (-(d * d) * (0.5 * iv) - ls - _HALF_LOG_2PI).sum(axis=1)
        r = np.exp(lp - self.old)
        J = float((self.A * r).mean())
        if not with_grad:
            return J, mu
        g_lp = self.A * r / self.B
        d_mu = g_lp[:, None] * d * iv
        d_ls = (g_lp[:, None] * (d * d * iv - 1.0)).sum(axis=0)
        return J, mu, [d_ls] + self._back(th, h1, h2, d_mu)

    def kl(self, th, mu0, ls0):
        ls = th[0]
        _, _, mu = self.forward(th)
        return float((ls0 - ls + (np.exp(2.0 * ls) + (mu - mu0) ** 2) / (2.0 * np.exp(2.0 * ls0)) - 0.5).sum(axis=1).mean())

    def fvp(self, th, v, damping):
        """H v at th (the Fisher matrix of the Gaussian policy there, plus damping): v and the result are lists in ACTOR_ORDER."""
        ls, W1, b1, W2, b2, W3, b3 = th
        v_ls, V1, vb1, V2, vb2, V3, vb3 = v
        h1, h2, _ = self.forward(th)
        t1 = (self.x @ V1.T + vb1) * self.dact(h1)
        t2 = (t1 @ W2.T + h1 @ V2.T + vb2) * self.dact(h2)
        t_mu = t2 @ W3.T + h2 @ V3.T + vb3
        d_mu = t_mu * np.exp(-2.0 * ls) / self.B
        out = [2.0 * v_ls] + self._back(th, h1, h2, d_mu)
        return [o + damping * vi for o, vi in zip(out, v)]


def trpo_fvp_numpy(weights, log_std, obs, idx, v, activation="tanh", cg_damping=0.1):
    """H v (flat, ACTOR_ORDER) at the given parameters over rows idx of obs, in float64."""
    th = actor_arrays(weights, log_std)
    n = np.asarray(obs).shape[0]
    actor = _Actor(obs, np.zeros((n, th[6].size)), np.zeros(n), np.zeros(n), idx, activation, False)   # (the product reads observations only)
    return flatten(actor.fvp(th, unflatten(np.asarray(v, np.float64), th), cg_damping))


def cg_numpy(fvp, g, cg_max_steps=15, history=None):
    """The conjugate-gradient solve of H x = g as sb3_contrib writes it: (x, iterations), iterations = the updates of x.  history: a list that
    receives every r . r the 1e-10 exit was tested on."""
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rho = float(r @ r)
    if history is not None:
        history.append(rho)
    if rho < RHO_MIN:
        return x, 0
    for i in range(cg_max_steps):
        Hp = fvp(p)
        alpha = rho / float(p @ Hp)
        x = x + alpha * p
        if i == cg_max_steps - 1:
            return x, i + 1
        r = r - alpha * Hp
        rho_new = float(r @ r)
        if history is not None:
            history.append(rho_new)
        if rho_new < RHO_MIN:
            return x, i + 1
        p = r + (rho_new / rho) * p
        rho = rho_new
    return x, cg_max_steps


def trpo_step_numpy(weights, log_std, obs, actions, old_log_prob, advantages, idx, activation="tanh", target_kl=0.01, cg_damping=0.1,
                    cg_max_steps=15, line_search_shrinking_factor=0.8, line_search_max_iter=10, normalize_advantage=True):
    """One TRPO policy step in float64 (module docstring).  weights: the twelve arrays of GaussianActorCritic's order; idx: the rows of the
    flattened rollout.  Returns a dict: g and x (flat, ACTOR_ORDER), rho_history (cg_numpy's), objective_before, mu0, xHx, beta, cg_iterations, tries (the (KL, J) of
    every try evaluated), line_search_tries, accepted, failed, c (the last coefficient tried), kl and objective_after (of the last try, 0 when
    none was made), params (the actor's seven arrays after the step)."""
    th0 = actor_arrays(weights, log_std)
    actor = _Actor(obs, actions, old_log_prob, advantages, idx, activation, normalize_advantage)
    J0, mu0, grads = actor.objective(th0, with_grad=True)
    g = flatten(grads)
    fvp = lambda v: flatten(actor.fvp(th0, unflatten(v, th0), cg_damping))  # noqa: E731
    rhos = []
    x, iters = cg_numpy(fvp, g, cg_max_steps, rhos)
    xHx = float(x @ fvp(x))
    out = dict(g=g, x=x, rho_history=rhos, objective_before=J0, mu0=mu0, xHx=xHx, cg_iterations=iters, tries=[], accepted=False, c=1.0, kl=0.0, objective_after=0.0,
               failed=not (math.isfinite(xHx) and xHx > 0.0), beta=0.0, params=[a.copy() for a in th0])
    if not out["failed"]:
        beta = out["beta"] = math.sqrt(2.0 * target_kl / xHx)
        theta0, c = flatten(th0), 1.0
        for k in range(line_search_max_iter):
            out["c"] = c
            th = unflatten(theta0 + c * beta * x, th0)
            J, _ = actor.objective(th)
            KL = actor.kl(th, mu0, th0[0])
            out["tries"].append((KL, J))
            out["kl"], out["objective_after"] = KL, J
            if KL < target_kl and J > J0:
                out["accepted"], out["params"] = True, th
                break
            c *= line_search_shrinking_factor
    out["line_search_tries"] = len(out["tries"])
    return out


def value_grad_numpy(weights, obs, returns, idx, activation="tanh"):
    """value_loss = mean((R - v)^2) over rows idx and its gradient for the six value arrays (vf_W1, vf_b1, vf_W2, vf_b2, value_W, value_b), float64."""
    w = [np.asarray(a, np.float64) for a in weights]
    idx = np.asarray(idx, np.int64)
    x, R = np.asarray(obs, np.float64)[idx], np.asarray(returns, np.float64)[idx]
    tanh = activation == "tanh"
    act = np.tanh if tanh else (lambda z: np.maximum(z, 0.0))
    dact = (lambda h: 1.0 - h * h) if tanh else (lambda h: (h > 0.0).astype(np.float64))
    v1 = act(x @ w[4].T + w[5])
    v2 = act(v1 @ w[6].T + w[7])
    v = (v2 @ w[10].T + w[11])[:, 0]
    g_v = 2.0 * (v - R) / len(idx)
    e2 = (g_v[:, None] * w[10]) * dact(v2)
    e1 = (e2 @ w[6]) * dact(v1)
    return float(((R - v) ** 2).mean()), [e1.T @ x, e1.sum(0), e2.T @ v1, e2.sum(0), (g_v[:, None] * v2).sum(0)[None, :], np.array([g_v.sum()])]


class TRPOLearner(_Learner):
    """sb3_contrib's TRPO.train() on the device for an OnPolicyCollector's GaussianActorCritic.

    The learner takes the policy's current weights as float32 masters on the device.  While it lives, `policy.set_weights` / `set_log_std`
    also reset the masters (the critic's Adam state is kept); `state_dict()` reads them back.  `close()` (or closing the policy or the engine)
    frees it."""

    trpo = property(lambda self: self.learner)   # the device learner

    def __init__(self, collector, learning_rate=1e-3, batch_size=128, cg_max_steps=15, cg_damping=0.1, line_search_shrinking_factor=0.8,
                 line_search_max_iter=10, n_critic_updates=10, target_kl=0.01, normalize_advantage=True, sub_sampling_factor=1, seed=0,
                 use_sde=False, **unsupported):
        for k in unsupported:
            raise ValueError(f"TRPOLearner: {k} is not supported (use_sde, shared trunks and other policy_kwargs, schedules as objects and action "
                             "masks are out of scope; n_steps, gamma and gae_lambda belong to the collector; see the module docstring)")
        if use_sde:
            raise ValueError("TRPOLearner: use_sde is not supported (out of scope; see the module docstring)")
        self._numbers("TRPOLearner: learning_rate is a number; drive a schedule with set_rate() between train() calls", learning_rate)
        for name, v in (("batch_size", batch_size), ("n_critic_updates", n_critic_updates), ("sub_sampling_factor", sub_sampling_factor),
                        ("cg_max_steps", cg_max_steps), ("line_search_max_iter", line_search_max_iter)):
            if int(v) < (0 if name == "n_critic_updates" else 1):
                raise ValueError(f"TRPOLearner: {name} {v} must be at least {0 if name == 'n_critic_updates' else 1}")
        self._bind(collector)
        self.lr, self.batch_size, self.n_critic_updates = float(learning_rate), int(batch_size), int(n_critic_updates)
        self.sub_sampling_factor, self.normalize_advantage = int(sub_sampling_factor), bool(normalize_advantage)
        self.generator = self.torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self.learner = self.eng.trpo_create(self.policy.ac, lr=learning_rate, target_kl=target_kl, cg_damping=cg_damping,
                                            line_search_shrinking_factor=line_search_shrinking_factor, cg_max_steps=cg_max_steps,
                                            line_search_max_iter=line_search_max_iter, normalize_advantage=normalize_advantage)
        self._arange = None

    def set_rate(self, lr):
        """The value function's learning rate of the following critic minibatches (how a schedule is driven from Python)."""
        self._numbers("TRPOLearner.set_rate: lr is a number", lr)
        self.lr = float(lr)
        self.eng.trpo_set_rate(self.trpo, self.lr)

    def _indices(self, ix, N, what):
        t = self.torch
        ix = t.as_tensor(ix).to(device=self.device, dtype=t.int32).contiguous()
        if ix.ndim != 1 or ix.numel() < 1:
            raise ValueError(f"TRPOLearner.train: {what} must be a non-empty 1-d index array")
        if int(ix.min()) < 0 or int(ix.max()) >= N:
            raise ValueError(f"TRPOLearner.train: an index of {what} is outside the batch's {N} rows")
        return ix

    def train(self, batch, policy_rows=None, minibatches=None):
        """One policy step over the RolloutBatch `batch` -- every row, or with sub_sampling_factor f > 1 the rows randperm(N)[::f] of the seeded
        generator, or exactly `policy_rows` -- then the critic's minibatches: n_critic_updates passes of fresh device permutations cut into
        batch_size pieces (the shorter last piece included), or exactly the iterable `minibatches`.  Returns policy_objective (J at the old
        parameters, as sb3_contrib logs it), kl_divergence_loss (0 when the line search failed), value_loss (the mean over the minibatches),
        is_line_search_success, line_search_tries and cg_iterations."""
        t, eng = self.torch, self.eng
        N = check_batch(self.policy, batch, "TRPOLearner.train")
        obs, actions, old_lp, adv, ret = self._flat(batch, N, "log_probs", "advantages", "returns")
        if policy_rows is not None:
            rows = self._indices(policy_rows, N, "policy_rows")
        elif self.sub_sampling_factor > 1:
            rows = t.randperm(N, generator=self.generator, device=self.device)[::self.sub_sampling_factor].to(t.int32).contiguous()
        else:
            if self._arange is None or self._arange.numel() != N:
                self._arange = t.arange(N, dtype=t.int32, device=self.device)
            rows = self._arange
        if minibatches is None:
            pieces = []
            for _ in range(self.n_critic_updates):
                perm = t.randperm(N, generator=self.generator, device=self.device).to(t.int32)
                pieces += [perm[i:i + self.batch_size] for i in range(0, N, self.batch_size)]
        else:
            pieces = [t.as_tensor(ix).to(device=self.device, dtype=t.int32).contiguous() for ix in minibatches]
            if any(ix.ndim != 1 or ix.numel() < 1 for ix in pieces):
                raise ValueError("TRPOLearner.train: every minibatch must be a non-empty 1-d index array")
            if pieces:   # (one check over all of them: a check per minibatch would synchronise twice per minibatch)
                self._indices(t.cat(pieces), N, "a minibatch")
        losses = t.zeros(max(len(pieces), 1), dtype=t.float32, device=self.device)
        t.cuda.synchronize(self.device)   # the engine works on its own stream
        eng.trpo_policy_step(self.trpo, obs, actions, old_lp, adv, rows, rows.numel())
        for k, ix in enumerate(pieces):
            eng.trpo_critic_minibatch(self.trpo, obs, ret, ix, ix.numel(), losses[k:k + 1])
        eng.ppo_sync(self.trpo)           # (synchronises; the policy samples from the new log_std afterwards)
        rep = self.last_report = eng.trpo_get_report(self.trpo)
        self.last_value_losses = losses.cpu().numpy()[:len(pieces)]
        ok = bool(rep["accepted"])
        return dict(policy_objective=float(rep["objective_before"]), kl_divergence_loss=float(rep["kl"]) if ok else 0.0,
                    value_loss=float(self.last_value_losses.astype(np.float64).mean()) if len(pieces) else float("nan"), is_line_search_success=ok,
                    line_search_tries=int(rep["line_search_tries"]), cg_iterations=int(rep["cg_iterations"]))


__all__ = ["TRPOLearner", "trpo_step_numpy", "trpo_fvp_numpy", "cg_numpy", "value_grad_numpy", "actor_arrays", "flatten", "unflatten", "ACTOR_ORDER",
           "check_batch", "SB3_KEYS", "SB3_LOG_STD"]
