"""ARS (Augmented Random Search, `sb3_contrib.ARS`) on the device: the eighth algorithm of the reference's training script
(`train_stable_baselines.py:89-123`).  An iteration evaluates 2 n_delta perturbed copies of a deterministic policy for whole episodes and steps
theta from the episode returns; there is no backprop and no replay.  The engine's envs are split into 2 n_delta groups of E / (2 n_delta)
consecutive envs, every group runs under its own candidate's weights in ONE actor launch per step (`ev2g_ars_act_kernel`), and perturbation,
returns and the update stay on the device (`csrc/ev2g_ars.h`).

    candidates   k: theta + delta_std delta_k,   n_delta + k: theta - delta_std delta_k,   delta ~ N(0, 1) [n_delta, n_params]
    return_c     the SUM of the candidate's deterministic episode rewards + alive_bonus_offset x the summed episode lengths
    score_k      max(r+_k, r-_k); the n_top best directions are kept, in descending score (ties to the lower k)
    sigma_R      the unbiased standard deviation of the 2 n_top kept returns;   step = learning_rate / (n_top sigma_R + 1e-6)
    theta        <- theta + step sum_j (r+_j - r-_j) delta_j

`ARSPolicy` ("MlpPolicy": obs -> ReLU -> ReLU -> linear -> tanh, unscaled into the env's box [lo, 1]) and `ARSLinearPolicy` ("LinearPolicy":
obs -> linear without bias, clipped to [lo, 1]) hold the parameters as numpy arrays under sb3_contrib's state-dict names (`action_net.0.weight`,
`.0.bias`, `.2.*`, `.4.*`; the linear policy `action_net.0.weight` alone).  sb3_contrib is not a dependency and is not installed where this was
written: the names and the formulas above follow its source and are checked against the names only, not against a live sb3_contrib.
Not reproduced: VecNormalize-style observation statistics, callbacks, asynchronous evaluation (`async_eval`).

`ars_forward_numpy` and `ars_update_numpy` are the float64 numerics references; `ars_iteration_host` is the twin loop the tests hold
`ARSLearner.train()` to, bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .engine import EngineError, ars_query, host_ars_perturb, host_ars_returns, host_ars_update  # noqa: F401

MLP_KEYS = ("action_net.0.weight", "action_net.0.bias", "action_net.2.weight", "action_net.2.bias", "action_net.4.weight", "action_net.4.bias")
LINEAR_KEYS = ("action_net.0.weight",)


def _host(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


class _Policy:
    KIND, KEYS = "", ()

    def __init__(self, arrays, lo=-1.0):
        if float(lo) not in (-1.0, 0.0):
            raise ValueError(f"{type(self).__name__}: lo {lo} must be -1 or 0")
        w = [np.ascontiguousarray(_host(a), np.float32) for a in arrays]
        if len(w) != len(self.KEYS) or w[0].ndim != 2:
            raise ValueError(f"{type(self).__name__}: {len(self.KEYS)} arrays expected ({', '.join(self.KEYS)}), the first an [out, in] matrix")
        self.d_in = w[0].shape[1]
        if self.KIND == "MlpPolicy":
            self.h1, self.h2, self.d_out = w[0].shape[0], w[2].shape[0] if w[2].ndim == 2 else -1, w[4].shape[0] if w[4].ndim == 2 else -1
        else:
            self.h1, self.h2, self.d_out = 0, 0, w[0].shape[0]
        for name, a, s in zip(self.KEYS, w, _abi.ars_param_shapes(self.KIND, self.d_in, self.h1, self.h2, self.d_out)):
            if a.shape != s:
                raise ValueError(f"{type(self).__name__}: {name} has shape {a.shape}, expected {s}")
        try:
            ars_query(self.KIND, self.d_in, self.h1, self.h2, self.d_out)   # the kernel's limits, with the library's own message
        except EngineError as e:
            raise ValueError(f"{type(self).__name__}: {e}") from None
        self.arrays, self.lo = w, float(lo)

    @classmethod
    def zeros(cls, d_in, d_out, net_arch=(64, 64), lo=-1.0):
        """sb3_contrib's zero_policy: every parameter 0."""
        h1, h2 = (net_arch if cls.KIND == "MlpPolicy" else (0, 0))
        return cls([np.zeros(s, np.float32) for s in _abi.ars_param_shapes(cls.KIND, d_in, h1, h2, d_out)], lo=lo)

    @classmethod
    def from_state_dict(cls, state_dict, lo=-1.0):
        missing = [k for k in cls.KEYS if k not in state_dict]
        if missing:
            raise KeyError(f"{cls.__name__}.from_state_dict: missing {missing}")
        extra = [k for k in state_dict if k.startswith("action_net.") and k not in cls.KEYS]
        if extra:
            raise ValueError(f"{cls.__name__}.from_state_dict: parameters this policy does not have ({extra})")
        return cls([state_dict[k] for k in cls.KEYS], lo=lo)

    def state_dict(self):
        return dict(zip(self.KEYS, self.arrays))

    @property
    def n_params(self):
        return int(sum(a.size for a in self.arrays))

    def theta(self):
        """parameters_to_vector: the arrays flattened one behind the other, float32"""
        return np.concatenate([a.ravel() for a in self.arrays]).astype(np.float32)

    def set_theta(self, theta):
        theta = np.ascontiguousarray(theta, np.float32)
        if theta.shape != (self.n_params,):
            raise ValueError(f"{type(self).__name__}: theta has shape {theta.shape}, expected {(self.n_params,)}")
        o = 0
        for i, a in enumerate(self.arrays):
            self.arrays[i] = theta[o:o + a.size].reshape(a.shape).copy()
            o += a.size

    def forward_numpy(self, x):
        return ars_forward_numpy(x, self.arrays, self.KIND, self.lo)


class ARSPolicy(_Policy):
    """sb3_contrib's ARSPolicy with two hidden ReLU layers, biases and squash_output=True, as host arrays.  Limits of the device kernel:
    D <= 192, hidden widths <= 256, P <= 64."""
    KIND, KEYS = "MlpPolicy", MLP_KEYS


class ARSLinearPolicy(_Policy):
    """sb3_contrib's ARSLinearPolicy: one linear layer without bias, no squash; the action is clipped to the env's box."""
    KIND, KEYS = "LinearPolicy", LINEAR_KEYS


POLICIES = {"MlpPolicy": ARSPolicy, "LinearPolicy": ARSLinearPolicy}


def split_theta(theta, kind, d_in, h1, h2, d_out):
    """The arrays of a flat parameter vector (views of `theta`)."""
    out, o = [], 0
    for s in _abi.ars_param_shapes(kind, d_in, h1, h2, d_out):
        n = int(np.prod(s))
        out.append(np.asarray(theta)[o:o + n].reshape(s))
        o += n
    return out


def ars_forward_numpy(x, arrays, kind="MlpPolicy", lo=-1.0):
    """Float64 forward of a policy's arrays on rows x [n, D]: the env's action [n, P] in [lo, 1].  The numerics reference of ev2g_ars_act."""
    w = [np.asarray(a, np.float64) for a in arrays]
    x = np.asarray(x, np.float64)
    if kind == "LinearPolicy":
        return np.clip(x @ w[0].T, lo, 1.0)
    h = np.maximum(np.maximum(x @ w[0].T + w[1], 0.0) @ w[2].T + w[3], 0.0)
    a = np.tanh(h @ w[4].T + w[5])
    return 0.5 * (a + 1.0) if lo == 0.0 else a


def ars_update_numpy(theta, delta, returns, n_top, learning_rate):
    """One ARS step in float64: (new theta, dict(order, sigma_r, step)).  returns [2 n_delta]: r+ of the directions, then r-."""
    theta, delta, r = np.asarray(theta, np.float64), np.asarray(delta, np.float64), np.asarray(returns, np.float64)
    n_delta = delta.shape[0]
    plus, minus = r[:n_delta], r[n_delta:]
    score = np.maximum(plus, minus)
    order = np.argsort(-score, kind="stable")[:n_top]   # descending, ties to the lower index
    kept = np.concatenate([plus[order], minus[order]])
    sigma = kept.std(ddof=1)
    step = learning_rate / (n_top * sigma + 1e-6)
    return theta + step * ((plus[order] - minus[order]) @ delta[order]), dict(order=order, sigma_r=float(sigma), step=float(step))


def _rounds(E, n_delta, n_eval_episodes):
    per = E // (2 * n_delta) if E % (2 * n_delta) == 0 else 0
    if per < 1:
        raise ValueError(f"ARSLearner: the engine's {E} envs are not a positive multiple of 2 n_delta ({2 * n_delta})")
    n_eval = per if n_eval_episodes is None else int(n_eval_episodes)
    if n_eval < 1 or n_eval % per:
        raise ValueError(f"ARSLearner: n_eval_episodes {n_eval} must be a positive multiple of E / (2 n_delta) = {per}")
    return n_eval // per


class ARSLearner:
    """sb3_contrib's ARS over an Engine: `train()` is one iteration (perturb, the episodes of every candidate, the update) without the weights,
    the directions or the returns leaving the device; `learn(total_timesteps)` repeats it.

    Every candidate is evaluated on E / (2 n_delta) envs at once; n_eval_episodes (default: that figure) must be a multiple of it, and the
    multiple is the number of reset -> whole-episode rounds per iteration, each on the next E scenarios of the pool.  On shapes whose steps go
    through the registered float32 hand-over buffers (`Engine.set_extras`, observation stride 0) those must be registered first."""

    def __init__(self, engine, policy="MlpPolicy", n_delta=8, n_top=None, learning_rate=0.02, delta_std=0.05, zero_policy=True, alive_bonus_offset=0,
                 n_eval_episodes=None, seed=0, net_arch=(64, 64), lo=-1.0):
        if isinstance(policy, str):
            if policy not in POLICIES:
                raise ValueError(f"ARSLearner: policy {policy!r} is not one of {sorted(POLICIES)}")
            if not zero_policy:
                raise ValueError("ARSLearner: zero_policy=False needs the initial parameters: pass an ARSPolicy / ARSLinearPolicy as `policy`")
            policy = POLICIES[policy].zeros(engine.D, engine.P, net_arch=tuple(net_arch), lo=lo)
        elif zero_policy:
            policy.set_theta(np.zeros(policy.n_params, np.float32))
        if callable(learning_rate) or callable(delta_std):
            raise ValueError("ARSLearner: schedule objects are not reproduced; call set_rates between iterations")
        n_delta = int(n_delta)
        n_top = n_delta if n_top is None else int(n_top)
        if not 1 <= n_top <= n_delta:
            raise ValueError(f"ARSLearner: n_top {n_top} is outside 1 .. n_delta ({n_delta})")
        if (policy.d_in, policy.d_out) != (engine.D, engine.P):
            raise ValueError(f"ARSLearner: the policy maps {policy.d_in} -> {policy.d_out}, the engine's envs {engine.D} -> {engine.P}")
        self.rounds = _rounds(engine.E, n_delta, n_eval_episodes)
        self.eng, self.policy, self.n_delta, self.n_top, self.seed = engine, policy, n_delta, n_top, int(seed)
        self.learning_rate, self.delta_std, self.alive_bonus_offset = float(learning_rate), float(delta_std), float(alive_bonus_offset)
        self.ars = engine.ars_create(policy.KIND, policy.d_in, policy.h1, policy.h2, policy.d_out, policy.lo, policy.theta(), seed=seed, n_delta=n_delta,
                                     n_top=n_top, learning_rate=self.learning_rate, delta_std=self.delta_std, alive_bonus_offset=self.alive_bonus_offset)
        self.obs32 = engine.ars_obs_f32(self.ars)
        self.num_timesteps, self.iterations = 0, 0

    def _next_offset(self):
        return (self.eng.scenario_offset + self.eng.E) % self.eng.M

    def _episode(self, population, offset):
        eng = self.eng
        eng.reset_f32(self.obs32, offset)
        eng.ars_rollout(self.ars, eng.T, population=population)

    def train(self, first_offset=None):
        """One iteration; returns the report (returns per candidate, ranks, sigma_r, step, refused, first_bad, iteration)."""
        eng = self.eng
        eng.ars_perturb(self.ars)
        for r in range(self.rounds):
            self._episode(True, first_offset if (r == 0 and first_offset is not None) else self._next_offset())
        eng.ars_update(self.ars)
        self.num_timesteps += self.rounds * eng.T * eng.E
        self.iterations += 1
        return eng.ars_get_report(self.ars, self.n_delta)

    def learn(self, total_timesteps):
        """train() until total_timesteps env steps were taken; returns every iteration's report."""
        out = []
        target = self.num_timesteps + int(total_timesteps)
        while self.num_timesteps < target:
            out.append(self.train())
        return out

    def predict(self, obs):
        """The centre policy's actions [n, P] (host float32) for host observation rows [n, D]."""
        eng = self.eng
        x = np.ascontiguousarray(np.atleast_2d(obs), np.float32)
        dx, da = eng.empty(x.shape, np.float32).upload(x), eng.empty((x.shape[0], self.policy.d_out), np.float32)
        try:
            eng.ars_act(self.ars, dx, x.shape[0], da)
            eng.synchronize()
            return da.to_host()
        finally:
            dx.free()
            da.free()

    def evaluate(self, n_rounds=1):
        """n_rounds whole episodes of all E envs under the centre policy; the mean episode return (float64 sums per env)."""
        eng, total = self.eng, 0.0
        rew = eng.empty((eng.T, eng.E))
        try:
            for _ in range(int(n_rounds)):
                eng.reset_f32(self.obs32, self._next_offset())
                eng.ars_rollout(self.ars, eng.T, population=False, reward=rew, r_stride=eng.E)
                eng.synchronize()
                total += float(rew.to_host().sum(axis=0).mean())
        finally:
            rew.free()
        return total / int(n_rounds)

    def set_rates(self, learning_rate, delta_std):
        self.eng.ars_set_rates(self.ars, learning_rate, delta_std)
        self.learning_rate, self.delta_std = float(learning_rate), float(delta_std)

    def get_weights(self):
        """theta read back from the device (the policy holder is refreshed)"""
        th = self.eng.ars_get_weights(self.ars, self.policy.n_params)
        self.policy.set_theta(th)
        return th

    def set_weights(self, theta):
        self.policy.set_theta(theta)
        self.eng.ars_set_weights(self.ars, self.policy.theta())

    def state_dict(self):
        self.get_weights()
        return self.policy.state_dict()

    def close(self):
        if self.ars:
            self.eng.ars_destroy(self.ars)
        self.ars = None


def ars_iteration_host(twin, twin_ars, theta, iteration, offsets, n_delta, n_top, learning_rate, delta_std, alive_bonus_offset=0.0, seed=0):
    """The twin of one ARSLearner.train(): the directions, the returns and the update through the host twins; only the candidates' actions come from
    a device -- ev2g_ars_act on `twin` (an Engine on the same pool) with `twin_ars` (an ARS object of the same shape there), whose steps go
    through a registered float32 hand-over pair.  `offsets`: the pool window of every round.  Returns (new theta, report, delta)."""
    E, D, P, T = twin.E, twin.D, twin.P, twin.T
    theta = np.ascontiguousarray(theta, np.float32)
    delta, _ = host_ars_perturb(theta, n_delta, delta_std, seed, iteration)
    twin.ars_set_weights(twin_ars, theta)
    twin.ars_set_rates(twin_ars, learning_rate, delta_std)
    twin.ars_seed(twin_ars, seed, iteration)
    twin.ars_perturb(twin_ars)
    x_obs, x_act = twin.empty((E, D), np.float32), twin.empty((E, P), np.float32)
    rew, done, mask = twin.empty((T, E)), twin.empty((E,), np.uint8), twin.empty((E, P), np.uint8)
    env_return = np.zeros(E, np.float64)
    try:
        twin.set_extras(obs_f32=x_obs, actions_f32=x_act)
        for off in offsets:
            twin.reset_f32(x_obs, off)
            for t in range(T):
                twin.ars_act(twin_ars, x_obs, E, x_act, population=True)
                twin.step_n(1, None, 0, None, 0, rew.at(t * E), 0, done, 0, mask, 0, auto_reset=False, persistent=False)
            twin.synchronize()
            host_ars_returns(env_return, rew.to_host())
        returns = host_ars_returns(env_return, None, 2 * n_delta, alive_bonus_offset, len(offsets) * T)
        new_theta, report = host_ars_update(theta, delta, returns, n_top, learning_rate)
        report["env_return"] = env_return
        return new_theta, report, delta
    finally:
        twin.set_extras()
        for b in (x_obs, x_act, rew, done, mask):
            b.free()
