"""The reference's two communication-fault models (ev2gym/rl_agent/noise_wrappers.py) for the device engine.

  FailedActionCommunication(env, p_fail)   a charger that misses a command keeps executing the one it was sent last
  DelayedObservation(env, p_delay)         a PublicPST observation whose per-EV energy column arrives one step late, the aggregate power
                                           reading corrected for what was not communicated

Both wrap an `EV2GymVec` (the device kernels of csrc/ev2g_link.h run on its own action / observation buffers; `reset` / `step` keep their
shape) or the single-env `EV2Gym` facade, and stack in either order.  They need an engine with the `link_*` entry points: there is no host
fallback.  Loops that never surface an action or an observation (`Engine.link_run`, `Engine.link_rollout`, `evaluate(p_fail=...)`) use the
engine's link directly.  A wrapper owns its link: `close()` destroys it and closes the env, `destroy_link()` destroys it alone, for the
caller who wraps one env anew for every run (or keep the wrapper and call `reset_state()`).

`LinkModel` is a vectorised numpy statement of both wrappers, operation for operation what the reference computes per env: the tests hold the
device to it bit for bit, and it to the reference's own objects.

Two differences to the reference, as in include/ev2g.h: the terminal observation (current_step == T), where the reference indexes its
[P, T] matrix out of range, passes through with no slot delayed; and its `assert obs[2] >= -5` is not reproduced, only the clamp at 0.
"""
from __future__ import annotations

import numpy as np


class LinkModel:
    """Both wrappers for E envs at once, in numpy.  `rand_act` / `rand_obs`: uniforms [E, P, T] (env e's [P, T] block is the reference
    wrapper's `random`).  State (held commands, the two remembered energy columns) carries over episodes until `reset_state()`."""

    def __init__(self, E, P, T, timescale, p_fail=0.0, p_delay=0.0, rand_act=None, rand_obs=None):
        self.E, self.P, self.T, self.timescale = int(E), int(P), int(T), timescale
        self.p_fail, self.p_delay = p_fail, p_delay
        self.rand_act = None if rand_act is None else np.asarray(rand_act, np.float64).reshape(self.E, self.P, self.T)
        self.rand_obs = None if rand_obs is None else np.asarray(rand_obs, np.float64).reshape(self.E, self.P, self.T)
        self.reset_state()

    def reset_state(self):
        self.held = np.zeros((self.E, self.P))             # previous_actions_list
        self.prev = np.zeros((self.E, self.P))             # previous_obs_list[4 + 3 i]
        self.actual = np.zeros((self.E, self.P))           # actual_previous_obs_list[4 + 3 i]

    def action(self, actions, t):
        """noise_wrappers.py:37-60 at current_step t: the delivered commands [E, P]."""
        a = np.asarray(actions, np.float64).reshape(self.E, self.P)
        if self.p_fail > 0:
            a = np.where(self.rand_act[:, :, t] < self.p_fail, self.held, a)
        self.held = a.copy()
        return a.copy()

    def observation(self, obs, t):
        """noise_wrappers.py:165-175,193-194 at current_step t (0: the reset observation; T: passes through): the delivered rows [E, D]."""
        o = np.array(obs, np.float64).reshape(self.E, 3 + 3 * self.P)
        raw = o[:, 4::3].copy()
        nc = np.zeros(self.E)
        if t < self.T and self.p_delay > 0:
            hit = (o[:, 3::3] != 0) & (self.rand_obs[:, :, t] < self.p_delay)
            for i in range(self.P):   # the reference's slot loop: a left-to-right sum per env
                nc = np.where(hit[:, i], nc + (raw[:, i] - self.actual[:, i]), nc)
            o[:, 4::3] = np.where(hit, self.prev, raw)
        o[:, 2] = o[:, 2] - nc * 60 / self.timescale
        self.prev = o[:, 4::3].copy()
        self.actual = raw
        o[:, 2] = np.where(o[:, 2] > 0, o[:, 2], 0.0)   # max(0, x)
        return o


def _base(env):
    while isinstance(env, _LinkWrapper):
        env = env.env
    return env


class _LinkWrapper:
    """What both wrappers share: the wrapped env, its engine's link, pass-through of everything else."""

    def __init__(self, env, p_fail, p_delay, seed, random):
        assert 0 <= max(p_fail, p_delay) <= 1 and min(p_fail, p_delay) >= 0, "the probability must be between 0 and 1"
        self.env = env
        base = _base(env)
        eng = getattr(base, "engine", None)
        if eng is None or not hasattr(eng, "link_create"):
            raise NotImplementedError(f"{type(self).__name__}: the wrapped env's engine has no link_* entry points (the fault models run on "
                                      "the device; there is no host fallback)")
        self._eng, self._vec = eng, hasattr(base, "num_envs")
        self.seed = int(seed)
        if random is not None:
            random = np.ascontiguousarray(random, np.float64).reshape(eng.E, eng.P, eng.T)
        self._random = random
        self._link = eng.link_create(p_fail, p_delay, seed_act=seed, seed_obs=seed, rand_act=random if p_fail > 0 else None,
                                     rand_obs=random if p_delay > 0 else None)
        self._buf = None

    @property
    def unwrapped(self):
        return _base(self.env)

    @property
    def random(self):
        """The uniforms, [E, P, T] ([P, T] for the single-env facade), as the reference's wrapper holds them."""
        r = self._random
        if r is None:
            from ..engine import host_uniform
            r = host_uniform(self._eng.E * self._eng.P * self._eng.T, self.seed, 0.0, 1.0).reshape(self._eng.E, self._eng.P, self._eng.T)
        return r if self._vec else r[0]

    def reset_state(self):
        """Forget the held commands / remembered rows: what constructing a fresh wrapper does in the reference."""
        self._eng.link_reset_state(self._link)

    def __getattr__(self, name):
        if name.startswith("_") or name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)

    def step(self, actions):
        return self.env.step(actions)

    def destroy_link(self):
        """Free this wrapper's link on the engine (its uniforms and state); the wrapped env stays open.  For the caller who wraps one env
        anew for every run, the reference's evaluator style: otherwise the links pile up on the engine until it is closed."""
        link, self._link = self._link, None
        if link is not None:
            self._eng.link_destroy(link)
        if self._buf is not None:
            self._buf.free()
            self._buf = None

    def close(self):
        self.destroy_link()
        return self.env.close()


class FailedActionCommunication(_LinkWrapper):
    """noise_wrappers.py:12-60.  `random`: the reference's uniforms ([P, T]; [E, P, T] for an EV2GymVec), or None: generated on the device from
    `seed` (engine.host_uniform(E * P * T, seed, 0, 1) gives the same matrix)."""

    def __init__(self, env, p_fail: float = 0.1, seed: int = 0, random=None):
        super().__init__(env, p_fail, 0.0, seed, random)
        self.p_fail = p_fail

    def step(self, actions):
        base, eng = self.unwrapped, self._eng
        if self._vec:
            a = base._as_device_actions(actions)
            eng.link_actions(self._link, a, out=base._act)   # the env's own action buffer: env.step takes it as it is
            return self.env.step(base._act)
        if self._buf is None:
            self._buf = eng.empty((1, eng.P))
        self._buf.upload(np.asarray(actions, np.float64).reshape(1, -1))
        eng.link_actions(self._link, self._buf, out=self._buf)
        return self.env.step(self._buf.to_host()[0])   # (the env zeroes empty ports in this copy, not in what is held)


class DelayedObservation(_LinkWrapper):
    """noise_wrappers.py:62-198, the PublicPST branch; applied to the reset observation and to every step's."""

    def __init__(self, env, p_delay: float = 0.1, seed: int = 0, random=None):
        super().__init__(env, 0.0, p_delay, seed, random)
        self.p_delay = p_delay

    def _deliver(self, obs):
        base, eng = self.unwrapped, self._eng
        if self._vec:
            eng.link_observe(self._link, base._obs)   # at the env's current step (0 right after an auto-reset: its reset observation)
            return base._out(base._obs)
        if self._buf is None:
            self._buf = eng.empty((1, eng.D))
        self._buf.upload(np.asarray(obs, np.float64).reshape(1, -1))
        eng.link_observe(self._link, self._buf)
        return self._buf.to_host()[0]

    def reset(self, **kwargs):
        obs, info = self.env.reset(**kwargs)
        return self._deliver(obs), info

    def step(self, actions):
        obs, *rest = self.env.step(actions)
        return (self._deliver(obs), *rest)
