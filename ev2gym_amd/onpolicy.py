"""On-policy rollout collection on the device: the collect_rollouts() half of the reference's default training run
(`train_stable_baselines.py:24`: PPO; A2C and TRPO fill the same buffer).

`GaussianActorCritic` holds SB3's default `ActorCriticPolicy` for a Box action space -- a policy trunk with a linear action head, a separate
value trunk with a linear value head, one activation, a state-independent log_std -- as numpy arrays; `attach(engine)` puts it on the device
(`ev2g_ac_create`), where one launch per step evaluates both trunks, samples the action, and returns its log-probability and the value.
`OnPolicyCollector.collect()` runs n_steps x (that launch -> env step) with every row landing in device tensors shaped like SB3's
`RolloutBuffer`, bootstraps the last value and computes GAE advantages and returns on the device (`ev2g_gae`).

`ac_forward_numpy` (float64) and `gae_numpy` (float32, SB3's loop restated) are the numerics twins the tests hold the kernels to.

Stable-Baselines3 itself is not a dependency and is not installed where this was written: the state-dict key mapping below follows the parameter
names SB3 gives `ActorCriticPolicy(net_arch=dict(pi=[h1, h2], vf=[v1, v2]))` and is checked against those names only, not against a live SB3
policy.  Out of scope: action masks, recurrent policies (SAC's squashed Gaussian is `ev2gym_amd.sac`, behind the replay ring).  The learner is `ev2gym_amd.ppo.PPOLearner`.
"""
from __future__ import annotations

import numpy as np

from . import _abi

# SB3 parameter name -> position in the twelve-array order of ev2g_ac_create (policy trunk, value trunk, action head, value head)
SB3_KEYS = (
    "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
    "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
    "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias",
)
SB3_LOG_STD = "log_std"
_FIELDS = _abi.AC_PARAMS[:12]   # the weight and bias arrays; log_std is held apart


def _host(a):
    """numpy view of a numpy array or a (CPU or device) torch tensor"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def init_ac_weights(D, P, seed=0, h=(64, 64), v=(64, 64)):
    """torch.nn.Linear-style uniform(-1/sqrt(in), 1/sqrt(in)) weights, in the twelve-array order, as numpy float32."""
    rng = np.random.default_rng(seed)
    shapes = _abi.ac_param_shapes(D, h[0], h[1], v[0], v[1], P)[:12]
    out = []
    for w_shape, b_shape in zip(shapes[0::2], shapes[1::2]):   # (a layer's weight, then its bias, drawn in that order)
        k = 1.0 / np.sqrt(w_shape[1])
        out += [rng.uniform(-k, k, w_shape).astype(np.float32), rng.uniform(-k, k, b_shape[0]).astype(np.float32)]
    return out


def ac_forward_numpy(x, weights, activation="tanh"):
    """Float64 forward of the twelve arrays on rows x [n, D]: (mean [n, P], value [n]).  The numerics reference of ev2g_ac_forward."""
    w = [np.asarray(a, np.float64) for a in weights]
    act = np.tanh if activation == "tanh" else (lambda z: np.maximum(z, 0.0))
    x = np.asarray(x, np.float64)
    hp = act(act(x @ w[0].T + w[1]) @ w[2].T + w[3])
    hv = act(act(x @ w[4].T + w[5]) @ w[6].T + w[7])
    return hp @ w[8].T + w[9], (hv @ w[10].T + w[11])[:, 0]


def log_prob_numpy(actions, mean, log_std):
    """Float64 diagonal-Gaussian log-probability, summed over the action dimensions (SB3's DiagGaussianDistribution.log_prob)."""
    a, m, ls = (np.asarray(v, np.float64) for v in (actions, mean, log_std))
    return (-((a - m) ** 2) / (2.0 * np.exp(ls) ** 2) - ls - 0.5 * np.log(2.0 * np.pi)).sum(axis=-1)


def gae_numpy(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """SB3's RolloutBuffer.compute_returns_and_advantage restated in float32 numpy: (advantages, returns) [k, E].  gamma and gamma * gae_lambda
    meet the float32 arrays as numpy scalars of that width, which is what SB3's python floats do under numpy's casting rules."""
    r = np.asarray(rewards).astype(np.float32)
    v = np.asarray(values, np.float32)
    starts = np.asarray(episode_starts).astype(np.float32)
    g, c = np.float32(gamma), np.float32(float(gamma) * float(gae_lambda))
    k = r.shape[0]
    adv = np.zeros_like(v)
    last = np.zeros(v.shape[1], np.float32)
    for t in reversed(range(k)):
        if t == k - 1:
            nnt, next_v = np.float32(1.0) - np.asarray(last_dones).astype(np.float32), np.asarray(last_values, np.float32)
        else:
            nnt, next_v = np.float32(1.0) - starts[t + 1], v[t + 1]
        delta = (r[t] + (g * next_v) * nnt) - v[t]
        last = delta + (c * nnt) * last
        adv[t] = last
    return adv, adv + v


class GaussianActorCritic:
    """SB3's default ActorCriticPolicy for a Box action space as host arrays.  Limits of the device kernel (ev2g_ac_create): D <= 192, hidden
    widths <= 256, P <= 64; lo is the lower edge of the env's action box, -1 (V2G) or 0."""

    def __init__(self, weights, log_std, activation="tanh", lo=-1.0, seed=0):
        if len(weights) != 12:
            raise ValueError(f"GaussianActorCritic: twelve weight / bias arrays expected ({', '.join(_FIELDS)}), got {len(weights)}")
        w = [np.ascontiguousarray(_host(a), np.float32) for a in weights]
        if w[0].ndim != 2 or w[4].ndim != 2:
            raise ValueError("GaussianActorCritic: pi_W1 and vf_W1 must be [out, in] matrices")
        D, h1, h2, v1, v2, P = _abi.ac_widths(w)
        for name, a, s in zip(_FIELDS, w, _abi.ac_param_shapes(D, h1, h2, v1, v2, P)):
            if a.shape != s:
                raise ValueError(f"GaussianActorCritic: {name} has shape {a.shape}, expected {s}")
        if not 1 <= D <= _abi.AC_MAX_IN:
            raise ValueError(f"GaussianActorCritic: d_in {D} is outside 1 .. {_abi.AC_MAX_IN}")
        for name, n in (("h1", h1), ("h2", h2), ("v1", v1), ("v2", v2)):
            if not 1 <= n <= _abi.AC_MAX_HIDDEN:
                raise ValueError(f"GaussianActorCritic: {name} {n} is outside 1 .. {_abi.AC_MAX_HIDDEN}")
        if not 1 <= P <= _abi.AC_MAX_OUT:
            raise ValueError(f"GaussianActorCritic: d_out {P} is outside 1 .. {_abi.AC_MAX_OUT}")
        if activation not in _abi.AC_ACTIVATIONS:
            raise ValueError(f"GaussianActorCritic: activation {activation!r} is not one of {sorted(_abi.AC_ACTIVATIONS)}")
        if float(lo) not in (-1.0, 0.0):
            raise ValueError(f"GaussianActorCritic: lo {lo} must be -1 or 0")
        self.weights, self.activation, self.lo, self.seed = w, activation, float(lo), int(seed)
        self.d_in, self.h1, self.h2, self.v1, self.v2, self.d_out = D, h1, h2, v1, v2, P
        self.log_std = self._check_log_std(log_std)
        self.engine, self.ac = None, None

    def _check_log_std(self, log_std):
        ls = np.ascontiguousarray(_host(log_std), np.float32)
        if ls.shape != (self.d_out,):
            raise ValueError(f"GaussianActorCritic: log_std has shape {ls.shape}, expected {(self.d_out,)}")
        if not np.isfinite(ls).all():
            raise ValueError("GaussianActorCritic: log_std is not finite")
        return ls

    @classmethod
    def from_state_dict(cls, state_dict, activation="tanh", lo=-1.0, seed=0):
        """From `policy.state_dict()` of an SB3 ActorCriticPolicy with two hidden layers per trunk (torch tensors or numpy arrays)."""
        missing = [k for k in SB3_KEYS + (SB3_LOG_STD,) if k not in state_dict]
        if missing:
            raise KeyError(f"GaussianActorCritic.from_state_dict: missing {missing}")
        deeper = [k for k in state_dict if k.startswith("mlp_extractor.") and k not in SB3_KEYS]
        if deeper:
            raise ValueError(f"GaussianActorCritic.from_state_dict: the trunks have more than two hidden layers ({deeper}); net_arch must be "
                             "dict(pi=[h1, h2], vf=[v1, v2])")
        return cls([state_dict[k] for k in SB3_KEYS], state_dict[SB3_LOG_STD], activation=activation, lo=lo, seed=seed)

    def state_dict(self):
        d = dict(zip(SB3_KEYS, self.weights))
        d[SB3_LOG_STD] = self.log_std
        return d

    def forward_numpy(self, x):
        return ac_forward_numpy(x, self.weights, self.activation)

    # ---- device side ----
    def attach(self, engine):
        """Create the device object on `engine` (ev2gym_amd.engine.Engine); returns self."""
        self.engine = engine
        self.ac = engine.ac_create(self.weights, self.log_std, activation=self.activation, lo=self.lo, seed=self.seed)
        return self

    def set_log_std(self, log_std):
        self.log_std = self._check_log_std(log_std)
        if self.ac:
            self.engine.ac_set_log_std(self.ac, self.log_std)

    def set_weights(self, weights):
        fresh = GaussianActorCritic(weights, self.log_std, self.activation, self.lo, self.seed)
        if [a.shape for a in fresh.weights] != [a.shape for a in self.weights]:
            raise ValueError("GaussianActorCritic.set_weights: the shapes differ from the ones the policy was created with")
        self.weights = fresh.weights
        if self.ac:
            self.engine.ac_set_weights(self.ac, self.weights)

    def get_weights(self):
        """Refresh `weights` / `log_std` from the device (ev2g_ac_get_weights: a bound learner's masters, else the packed images) and return
        them; without a device object, the host arrays as they are."""
        if self.ac:
            self.weights, self.log_std = self.engine.ac_get_weights(self.ac, (self.d_in, self.h1, self.h2, self.v1, self.v2, self.d_out))
        return self.weights, self.log_std

    def load_state_dict(self, state_dict):
        self.set_weights([state_dict[k] for k in SB3_KEYS])
        self.set_log_std(state_dict[SB3_LOG_STD])

    def reseed(self, seed, first_draw=0):
        self.seed = int(seed)
        if self.ac:
            self.engine.ac_seed(self.ac, seed, first_draw)

    def close(self):
        if self.ac and self.engine is not None:
            self.engine.ac_destroy(self.ac)
        self.ac = None


class RolloutBatch:
    """What OnPolicyCollector.collect() returns: SB3 RolloutBuffer's arrays as device tensors [n_steps, E, ...] (observations / actions /
    values / log_probs / advantages / returns / rewards / episode_starts float32), plus action_masks (uint8) and the [n_steps + 1, E, D] block
    whose last row is the observation the next collect() starts from.

    The tensors are VIEWS of the collector's own buffers: the next collect() overwrites them in place.  A learner that keeps a batch across
    updates takes `batch.clone()`."""
    FIELDS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getitem__(self, k):
        return self.__dict__[k]

    def clone(self):
        """A batch of tensors of its own, which later collect() calls leave alone."""
        return RolloutBatch(**{k: v.clone() for k, v in self.__dict__.items()})


class OnPolicyCollector:
    """n_steps x (Gaussian actor-critic -> env step) into RolloutBuffer-shaped device tensors, then GAE, without a host round trip per step.

    vec_or_engine: an EV2GymVec (its engine and its scenario-window order are used) or an Engine.  An episode that ends inside the n_steps is
    closed as an auto-resetting VecEnv closes it: statistics and reset in one launch (`last_episode_stats`, [E, 17] device tensor), the reset
    observation takes the terminal observation's place in the next row, and `episode_starts` is 1 there.  As in SB3's buffer the value behind an
    episode end is not bootstrapped (the reference's episodes end by time limit; SB3's optional terminal-value bootstrap is not reproduced).

    With an EV2GymVec the collector drives the vec's ENGINE: it takes the episode the vec's last reset() armed, draws every later scenario window
    from the vec's own order (and tells the vec which window runs), and leaves the vec's gym surface behind -- `vec.step()` results, its observation
    buffer and `vec.stats` are stale until the next `vec.reset()`.  What the chain of `ev2g_ac_collect` does not apply is refused here rather than
    skipped: a vec with a grid (`grid=`, and V2G_grid_state with it), with a cost function (its cost buffer is a registered step extra), or with
    `device_refill` / `resample_every` (the vec re-draws the pool inside its own reset())."""

    def __init__(self, vec_or_engine, policy, n_steps, gamma=0.99, gae_lambda=0.95, deterministic=False):
        import torch
        self.torch = torch
        self.vec = vec_or_engine if hasattr(vec_or_engine, "engine") else None
        self.eng = eng = vec_or_engine.engine if self.vec is not None else vec_or_engine
        if self.vec is not None:
            v = self.vec
            for what, on in (("a grid (grid=): the collector's chain holds no power-flow stage", getattr(v, "_grid", None) is not None),
                             ("a cost function: its cost buffer is a registered step extra", bool(getattr(v, "cost_kind", 0))),
                             ("device_refill / resample_every: the pool is re-drawn inside the vec's own reset()",
                              bool(getattr(v, "device_refill", False) or getattr(v, "resample_every", None)))):
                if on:
                    raise ValueError(f"OnPolicyCollector: the EV2GymVec has {what}")
        if policy.ac is None:
            policy.attach(eng)
        if (policy.d_in, policy.d_out) != (eng.D, eng.P):
            raise ValueError(f"OnPolicyCollector: the policy maps {policy.d_in} -> {policy.d_out}, the engine's envs {eng.D} -> {eng.P}")
        self.policy, self.n_steps, self.gamma, self.gae_lambda, self.deterministic = policy, int(n_steps), float(gamma), float(gae_lambda), deterministic
        n, E, D, P = self.n_steps, eng.E, eng.D, eng.P
        dev = torch.device("cuda", eng.device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.obs = z((n + 1, E, D), torch.float32)
        self.actions, self.values, self.log_probs = z((n, E, P), torch.float32), z((n, E), torch.float32), z((n, E), torch.float32)
        self.reward, self.done, self.mask = z((n, E), torch.float64), z((n, E), torch.uint8), z((n, E, P), torch.uint8)
        self.starts = z((n, E), torch.uint8)
        self.advantages, self.returns = z((n, E), torch.float32), z((n, E), torch.float32)
        self.last_values, self.last_dones = z((E,), torch.float32), z((E,), torch.uint8)
        self.last_episode_stats = z((E, _abi.N_STATS), torch.float64)
        self.episodes = 0
        self._next_start = True          # the next row is the first of an episode
        self._have_obs = False           # obs[0] holds the observation of the engine's current step
        torch.cuda.synchronize(dev)      # the engine works on its own stream

    def _next_offset(self):
        if self.vec is not None:   # the vec's windows without replacement; it is told which one runs, as its own reset() notes it
            off = self.vec._next_window(self.eng.M)
            self.vec._last_offset = off
            self.vec._episodes += 1
            return off
        return (self.eng.scenario_offset + self.eng.E) % self.eng.M

    def reset(self, offset=None):
        """Start a fresh episode on the pool window `offset` (None: the engine's current one); its observation becomes row 0."""
        self.eng.reset_f32(self.obs[0], self.eng.scenario_offset if offset is None else offset)
        self._next_start, self._have_obs = True, True

    def collect(self) -> RolloutBatch:
        torch, eng, n, T = self.torch, self.eng, self.n_steps, self.eng.T
        dev = self.obs.device
        if not self._have_obs:
            self.reset()
        else:
            self.obs[0].copy_(self.obs[n])
        # the rows at which an episode starts follow from the step counter alone: written up front, so that nothing but engine calls follows
        t, flags = eng.current_step, np.zeros(n, np.uint8)
        flags[0] = 1 if self._next_start else 0
        plan = []   # (first row, steps) of every segment; a reset precedes every segment but the first
        i = 0
        while i < n:
            if t >= T:
                t, flags[i] = 0, 1
            seg = min(n - i, T - t)
            plan.append((i, seg))
            i, t = i + seg, t + seg
        ended = t >= T   # the buffer's last row closes an episode
        self.starts.copy_(torch.from_numpy(flags).to(dev)[:, None].expand(n, eng.E))
        self.last_dones.fill_(1 if ended else 0)
        torch.cuda.synchronize(dev)
        for j, (i, seg) in enumerate(plan):
            if j > 0 or eng.current_step >= T:
                self._episode_end(self.obs[i])
            eng.ac_collect(self.policy.ac, seg, self.obs[i:], self.actions[i:], self.values[i:], self.log_probs[i:], self.reward[i:], self.done[i:],
                           self.mask[i:], deterministic=self.deterministic)
        if ended:   # the successor of the last row is a reset observation, whose value GAE does not read
            self._episode_end(self.obs[n])
        self._next_start = ended
        eng.ac_forward(self.policy.ac, self.obs[n], eng.E, value=self.last_values)
        eng.gae(self.reward, self.values, self.starts, self.last_values, self.last_dones, n, eng.E, self.gamma, self.gae_lambda, self.advantages,
                self.returns)
        eng.synchronize()
        return RolloutBatch(observations=self.obs[:n], actions=self.actions, rewards=self.reward.to(torch.float32),
                            episode_starts=self.starts.to(torch.float32), values=self.values, log_probs=self.log_probs, advantages=self.advantages,
                            returns=self.returns, action_masks=self.mask, dones=self.done, all_observations=self.obs)

    def _episode_end(self, obs_row):
        self.eng.stats_reset_f32(self.last_episode_stats, obs32=obs_row, offset=self._next_offset())
        self.episodes += 1

    def close(self):
        self.policy.close()
