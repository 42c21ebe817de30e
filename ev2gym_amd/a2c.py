"""The second learner of the on-policy collector: SB3's `A2C.train()` with default settings, on the device (`csrc/ev2g_ppo.h`, `ev2g_a2c_*`).

`A2CLearner(collector)` binds a device learner to the collector's `GaussianActorCritic`; `train(batch)` makes ONE update over the whole
`RolloutBatch` -- forward, policy-gradient / value / entropy loss, backprop, `clip_grad_norm_`, `torch.optim.RMSprop`, and the rewrite of the
packed weights the collector's launches read -- without the batch or the weights leaving the device; `learn(total_timesteps)` alternates
`collector.collect()` and `train()`.  SB3's collector-side defaults for A2C are `OnPolicyCollector(n_steps=5, gae_lambda=1.0)`.

`a2c_update_numpy` and `rmsprop_numpy` (with `ppo.clip_grad_norm_numpy`) are float64 restatements of the arithmetic (analytic backprop, no
torch): the numerics references the tests hold the kernels to.  SB3 is not a dependency; the formulas follow `A2C.train()` for
`ActorCriticPolicy` on a Box action space:

    lp = sum_p [-(a - mu)^2 / (2 sigma^2) - log_std - log(2 pi) / 2] on the unclipped action
    A^ = (A - mean(A)) / (std(A) + 1e-8), unbiased std, if normalize_advantage (default off), else A
    loss = -mean(A^ lp) + ent_coef * (-entropy) + vf_coef * mean((R - v)^2)
    g <- g * min(1, max_grad_norm / (|g| + 1e-6))
    torch.optim.RMSprop(lr, alpha=0.99, eps=1e-5): sq <- alpha sq + (1 - alpha) g g;  theta <- theta - lr g / (sqrt(sq) + eps)

`use_rms_prop=False` selects `torch.optim.Adam(eps=1e-5)`, which is what SB3's policy builds then.  Out of scope, refused where a caller could
ask for them: `RMSpropTFLike` (and any other `policy_kwargs`), learning-rate schedules as objects (the rate is settable between calls:
`set_rate`), action masks, orthogonal initialisation (weights arrive from the caller).
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .onpolicy import SB3_KEYS, SB3_LOG_STD
from .ppo import _backward, _forward, _Learner, check_batch, clip_grad_norm_numpy

STAT_NAMES = _abi.PPO_STATS[:4]   # ev2g_a2c_grad writes six statistics in ev2g_ppo_grad's order; the two ratio ones are exact zeros


def a2c_update_numpy(weights, log_std, obs, actions, advantages, returns, idx, activation="tanh", vf_coef=0.5, ent_coef=0.0,
                     normalize_advantage=False):
    """One update of A2C's loss in float64 with analytic backprop.  weights: the twelve arrays of GaussianActorCritic's order; idx: the rows of
    the flattened rollout.  Returns (grads, stats, aux): the thirteen gradients (the twelve arrays' order, then log_std), the six statistics
    (ev2g_ppo_grad's order, the last two 0) and a dict of intermediates (lp, adv, mean, value, the pre-activations z)."""
    idx = np.asarray(idx, np.int64)
    n = _forward(weights, log_std, obs, actions, idx, activation)
    A, R = (np.asarray(v, np.float64)[idx] for v in (advantages, returns))
    B, lp, v = len(idx), n.lp, n.v
    if normalize_advantage:
        if B < 2:
            raise ValueError("a2c_update_numpy: normalize_advantage needs at least two rows (the unbiased std of one advantage is undefined)")
        A = (A - A.mean()) / (A.std(ddof=1) + 1e-8)
    pl, vl, el = -(A * lp).mean(), ((R - v) ** 2).mean(), -n.entropy
    stats = np.array([pl, vl, el, pl + ent_coef * el + vf_coef * vl, 0.0, 0.0])
    g_lp = -A / B
    g_v = 2.0 * vf_coef * (v - R) / B
    grads, d_mu = _backward(n, g_lp, g_v, ent_coef)
    aux = dict(lp=lp, adv=A, mean=n.mu, value=v, z=n.z, d_mean=d_mu, d_value=g_v)
    return grads, stats, aux


def rmsprop_numpy(theta, sq, g, lr=7e-4, alpha=0.99, eps=1e-5):
    """One step of torch.optim.RMSprop (no weight decay, no momentum, not centered) in float64: (theta, sq) as new arrays."""
    theta, sq, g = (np.asarray(a, np.float64) for a in (theta, sq, g))
    sq = alpha * sq + (1.0 - alpha) * g * g
    return theta - lr * g / (np.sqrt(sq) + eps), sq


class A2CLearner(_Learner):
    """SB3's A2C.train() on the device for an OnPolicyCollector's GaussianActorCritic.

    The learner takes the policy's current weights as float32 masters on the device.  While it lives, `policy.set_weights` / `set_log_std`
    also reset the masters (the optimiser's state is kept); `state_dict()` reads them back.  `close()` (or closing the policy or the engine)
    frees it."""

    a2c = property(lambda self: self.learner)   # the device learner

    def __init__(self, collector, lr=7e-4, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, rms_prop_eps=1e-5, use_rms_prop=True,
                 normalize_advantage=False, **unsupported):
        for k in unsupported:
            raise ValueError(f"A2CLearner: {k} is not supported (RMSpropTFLike and other policy_kwargs, schedules as objects, action masks and "
                             "orthogonal initialisation are out of scope; n_steps, gamma and gae_lambda belong to the collector; see the module "
                             "docstring)")
        self._numbers("A2CLearner: lr is a number; drive a schedule with set_rate() between train() calls", lr)
        self._bind(collector)
        self.lr, self.normalize_advantage = float(lr), bool(normalize_advantage)
        self.learner = self.eng.a2c_create(self.policy.ac, lr=lr, rms_eps=rms_prop_eps, vf_coef=vf_coef, ent_coef=ent_coef, max_grad_norm=max_grad_norm,
                                           normalize_advantage=normalize_advantage, use_rms_prop=use_rms_prop)
        self._arange = None   # the one device arange: an update takes every row of the batch, in order
        self._stats = self.torch.zeros(6, dtype=self.torch.float32, device=self.device)

    def set_rate(self, lr):
        """The learning rate of the following updates (how a schedule is driven from Python)."""
        self._numbers("A2CLearner.set_rate: lr is a number", lr)
        self.lr = float(lr)
        self.eng.a2c_set_rate(self.a2c, self.lr)

    def train(self, batch):
        """One update over every row of the RolloutBatch `batch`.  Returns policy_loss, value_loss, entropy_loss, loss and explained_variance
        (of the batch's stored values against its returns, as SB3 logs it: 1 - var(returns - values) / var(returns), nan when var(returns) is 0)."""
        t, eng = self.torch, self.eng
        N = check_batch(self.policy, batch, "A2CLearner.train")
        if batch["values"].numel() != N:
            raise ValueError(f"A2CLearner.train: the batch's arrays do not all have {N} rows")
        if self.normalize_advantage and N < 2:
            raise ValueError("A2CLearner.train: normalize_advantage needs a batch of at least two rows")
        obs, actions, adv, ret, values = self._flat(batch, N, "advantages", "returns", "values")
        if self._arange is None or self._arange.numel() != N:
            self._arange = t.arange(N, dtype=t.int32, device=self.device)
        # (float64: returns far from zero with a small spread lose digits in a float32 variance, and the two casts cost nothing next to an update)
        ret64, val64 = ret.to(t.float64), values.to(t.float64)
        var_y = t.var(ret64, unbiased=False)
        ev = t.where(var_y == 0, t.full_like(var_y, float("nan")), 1.0 - t.var(ret64 - val64, unbiased=False) / var_y)
        t.cuda.synchronize(self.device)   # the engine works on its own stream
        eng.a2c_update(self.a2c, obs, actions, adv, ret, self._arange, N, self._stats)
        eng.ppo_sync(self.a2c)            # (synchronises; the policy samples from the new log_std afterwards)
        self.last_stats = self._stats.cpu().numpy()
        out = dict(zip(STAT_NAMES, (float(v) for v in self.last_stats[:4])))
        out["explained_variance"] = float(ev)
        return out


__all__ = ["A2CLearner", "a2c_update_numpy", "rmsprop_numpy", "clip_grad_norm_numpy", "check_batch", "STAT_NAMES", "SB3_KEYS", "SB3_LOG_STD"]
