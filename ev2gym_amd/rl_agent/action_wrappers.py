"""The reference's gym action wrappers (ev2gym/rl_agent/action_wrappers.py) for the device engine.

  BinaryAction(env)                            action > 0.5 ? 1 : min_action
  ThreeStep_Action(env)                        0 -> 0, 1 -> min_action, anything else -> 1
  ThreeStep_Action_DiscreteActionSpace(env)    the same action(); the reference also swaps the action space for MultiDiscrete([3] * P)
  Rescale_RepairLayer(env)                     rescales (0, 1) actions to (min_action, 1) and repairs them towards the step's power setpoint
  MinMax_RepairLayer(env)                      raises NotImplementedError, as the reference's constructor does

All wrap an `EV2GymVec` (the device kernels of csrc/ev2g_wrap.h write the env's own action buffer; `reset` / `step` keep their shape) or the
single-env `EV2Gym` facade.  They need an engine with the `wrap_*` entry points: there is no host fallback.  Loops that never surface an
action (`Engine.wrap_run`, `Engine.wrap_rollout`) use the engine's wrapper directly.  A wrapper owns its device object: `close()` destroys it
and closes the env, `destroy_wrap()` destroys it alone.  The repair layer's queue lives across `reset()`, as the reference's object does;
`reset_state()` empties it (a freshly built wrapper).  `mask_fn` is left out.

`WrapModel` is a vectorised numpy statement of the three kinds for E envs, operation for operation what the reference computes per env: the
tests hold the device to it bit for bit, and it to the reference's own objects.  Every sum is the plain left-to-right float64 sum in queue order
(Python's sum() before CPython 3.12; later interpreters compensate float sums).

Two quirks of the reference's repair layer are reproduced, as in include/ev2g.h: a queue entry keeps the min_power / max_power it was inserted
with (a port whose next EV arrives the step after the last one left keeps the old EV's), and new_action[i] divides by the charger power at
the queue POSITION i, not by the entry's own port.
"""
from __future__ import annotations

import numpy as np

from .. import _abi

BINARY, THREE_STEP, RESCALE_REPAIR = 0, 1, 2
# WrapModel.branch of a repair call, per env
PASS, RAISE, RAISE_NO_RANGE, REDUCE, REDUCE_TOPUP = 0, 1, 2, 3, 4


def charger_tables(arrays):
    """Per-port (min_action, max_cs_power, min_cs_power) of a scenario's chargers (`ScenarioBatch.arrays` or anything with the cs_* arrays of
    one scenario), each in the reference's operation order: action_wrappers.py:31-32, EV_Charger.get_max_power / get_min_charge_power."""
    lo, hi = np.asarray(arrays["cs_min_charge_current"], np.float64), np.asarray(arrays["cs_max_charge_current"], np.float64)
    volt, ph = np.asarray(arrays["cs_voltage"], np.float64), np.asarray(arrays["cs_phases"])
    n = np.asarray(arrays["cs_n_ports"]) if "cs_n_ports" in arrays else np.ones(len(lo), np.int64)
    sq = np.array([np.sqrt(float(p)) for p in ph])
    return (np.repeat(lo / hi + 1e-4, n), np.repeat(hi * volt * sq / 1000, n), np.repeat(lo * volt * sq / 1000, n))


class WrapModel:
    """One wrapper kind for E envs at once, in numpy.  `min_action`, `cs_kw`, `cs_min_kw`: per port [P] (charger_tables).  The repair layer's
    queue (port ids, min_power, max_power per entry) carries over episodes until `reset_state()`.  After a repair call `branch` [E] says which
    branch each env took and `mismatch` [E] whether some queue position's charger power differed from its port's."""

    def __init__(self, kind, E, P, min_action, cs_kw=None, cs_min_kw=None):
        self.kind = _abi.WRAP_KINDS[kind] if isinstance(kind, str) else int(kind)
        self.E, self.P = int(E), int(P)
        self.min_action = np.asarray(min_action, np.float64).reshape(self.P)
        self.cs_kw = None if cs_kw is None else np.asarray(cs_kw, np.float64).reshape(self.P)
        self.cs_min_kw = None if cs_min_kw is None else np.asarray(cs_min_kw, np.float64).reshape(self.P)
        self.reset_state()

    def reset_state(self):
        self.queue = np.full((self.E, self.P), -1, np.int64)   # ev_buffer, padded
        self.qmin = np.zeros((self.E, self.P))                  # min_power
        self.qmax = np.zeros((self.E, self.P))                  # max_power
        self.qlen = np.zeros(self.E, np.int64)
        self.branch = np.zeros(self.E, np.int64)
        self.mismatch = np.zeros(self.E, bool)

    def _update_ev_buffer(self, wants, pac_min, pac_max):
        """action_wrappers.py:205-243 per env: new wanting ports to the front (inserted at index 0 in ascending port order), queued ports
        that no longer want removed, the others in their order with the powers they were inserted with."""
        for e in range(self.E):
            n = int(self.qlen[e])
            old = self.queue[e, :n]
            queued = np.zeros(self.P, bool)
            queued[old] = True
            new = np.nonzero(wants[e] & ~queued)[0][::-1]
            keep = wants[e][old]
            lo = np.maximum(self.cs_min_kw[new], pac_min[e, new])   # max(cs.get_min_charge_power(), ev.min_ac_charge_power)
            hi = np.minimum(self.cs_kw[new], pac_max[e, new])       # min(cs.get_max_power(), ev.max_ac_charge_power)
            q = np.concatenate([new, old[keep]])
            m = len(q)
            self.qmin[e, :m] = np.concatenate([lo, self.qmin[e, :n][keep]])
            self.qmax[e, :m] = np.concatenate([hi, self.qmax[e, :n][keep]])
            self.queue[e, :m], self.queue[e, m:] = q, -1
            self.qlen[e] = m

    def _sum(self, x, valid):
        """Left-to-right float64 sum over the queue positions, from 0, per env."""
        total = np.zeros(self.E)
        for i in range(int(self.qlen.max(initial=0))):
            total = np.where(valid[:, i], total + x[:, i], total)
        return total

    def action(self, actions, connected=None, cap=None, B=None, pac_min=None, pac_max=None, setpoint=None):
        """The wrapped actions [E, P] for raw `actions`.  The repair layer also takes the step's per-port state [E, P] -- `connected` (an EV is
        plugged in), its current capacity `cap`, battery capacity `B`, min / max AC charge power -- and the step's power `setpoint` [E]."""
        a = np.asarray(actions, np.float64).reshape(self.E, self.P)
        if self.kind == BINARY:
            return np.where(a > 0.5, 1, self.min_action)
        if self.kind == THREE_STEP:
            return np.where(a == 0, 0, np.where(a == 1, self.min_action, 1))
        E, P = self.E, self.P
        act = a * (1 - self.min_action) + self.min_action
        conn = np.asarray(connected, bool).reshape(E, P)
        with np.errstate(all="ignore"):
            wants = conn & (np.asarray(cap, np.float64).reshape(E, P) / np.asarray(B, np.float64).reshape(E, P) < 1)
        self._update_ev_buffer(wants, np.asarray(pac_min, np.float64).reshape(E, P), np.asarray(pac_max, np.float64).reshape(E, P))
        n = int(self.qlen.max(initial=0))
        pos = np.arange(P)
        valid = pos[None, :] < self.qlen[:, None]
        q = np.where(valid, self.queue, 0)
        rows = np.arange(E)[:, None]
        lo, hi = self.qmin, self.qmax
        with np.errstate(all="ignore"):
            prop = np.minimum(np.maximum(act[rows, q] * self.cs_kw[q], lo), hi)   # np.clip(action[i] * max_cs_power[i], min_power, max_power)
            sp = np.asarray(setpoint, np.float64).reshape(E)
            current = self._sum(prop, valid)
            raise_ = current < sp
            reduce_ = ~raise_ & (current > sp)
            # :312-371
            rng_up = hi - prop
            tot_up = self._sum(rng_up, valid)
            x = (sp - current) / tot_up
            f_up = np.where(x < 1, x, 1.0)                                    # min(1, x)
            v = prop + rng_up * f_up[:, None]
            up = np.where(hi < v, hi, v)                                      # min(new_power, max_power)
            grow = raise_ & (tot_up > 0)
            # :373-411
            rng_dn = prop - lo
            tot_dn = self._sum(rng_dn, valid)
            x = (current - sp) / tot_dn
            f_dn = np.where(x < 1, x, 1.0)
            v = prop - rng_dn * f_dn[:, None]
            dn = np.where(lo > v, lo, v)                                      # max(new_power, min_power)
            shrink = reduce_ & (tot_dn > 0)
            prop = np.where(grow[:, None], up, np.where(shrink[:, None], dn, prop))
            # :413-421: the greedy top-up in queue order, a dependent loop that breaks at remaining <= 0
            rem = sp - self._sum(prop, valid)
            took = reduce_ & (rem > 0)
            live = took.copy()
            for i in range(n):
                go = live & valid[:, i] & (rem > 0)
                room = hi[:, i] - prop[:, i]
                inc = np.where(room < rem, room, rem)                         # min(remaining_deficit, increaseable_amount)
                prop[:, i] = np.where(go, prop[:, i] + inc, prop[:, i])
                rem = np.where(go, rem - inc, rem)
                live = live & (go | ~valid[:, i])                             # (the break ends the loop for good)
            new = prop / self.cs_kw[pos][None, :]                             # new_actions[i] = proposed_power[i] / max_cs_power[i], i the POSITION
        adjust = raise_ | reduce_
        out = act.copy()
        for e in np.nonzero(adjust)[0]:
            m = int(self.qlen[e])
            out[e, self.queue[e, :m]] = new[e, :m]
        self.branch = np.where(raise_, np.where(tot_up > 0, RAISE, RAISE_NO_RANGE), np.where(took, REDUCE_TOPUP, np.where(reduce_, REDUCE, PASS)))
        self.mismatch = adjust & (valid & (self.cs_kw[pos][None, :] != self.cs_kw[q])).any(axis=1)
        return out * wants   # action * occupied_ports: occupied is "queued after the update"


def _base(env):
    while isinstance(env, _ActionWrapper):
        env = env.env
    return env


class _ActionWrapper:
    """What the wrappers share: the wrapped env, its engine's wrapper object, pass-through of everything else."""

    def __init__(self, env):
        self.env = env
        base = _base(env)
        eng = getattr(base, "engine", None)
        if eng is None or not hasattr(eng, "wrap_create"):
            raise NotImplementedError(f"{type(self).__name__}: the wrapped env's engine has no wrap_* entry points (the action wrappers run on "
                                      "the device; there is no host fallback)")
        self._eng, self._vec = eng, hasattr(base, "num_envs")
        self._check(eng)
        self._wrap = eng.wrap_create(type(self).__name__)
        self._buf = None

    def _check(self, eng):
        pass

    @property
    def unwrapped(self):
        return _base(self.env)

    def reset_state(self):
        """Empty the repair layer's queue: what constructing a fresh wrapper does in the reference.  Nothing to do for the discretisers."""
        self._eng.wrap_reset_state(self._wrap)

    def __getattr__(self, name):
        if name.startswith("_") or name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)

    def _host_action(self, actions):
        eng = self._eng
        if self._buf is None:
            self._buf = eng.empty((1, eng.P))
        self._buf.upload(np.asarray(actions, np.float64).reshape(1, -1))
        eng.wrap_actions(self._wrap, self._buf, self._buf)
        return self._buf.to_host()[0]

    def action(self, actions):
        """The wrapped actions for the env's current step; no step is taken (the repair layer's queue advances, as the reference's does on
        every action() call).  On an EV2GymVec the result is the env's own action buffer."""
        base = self.unwrapped
        if self._vec:
            a = base._as_device_actions(actions)
            self._eng.wrap_actions(self._wrap, a, base._act)   # the env's own action buffer: env.step takes it as it is
            return base._act
        return self._host_action(actions)

    def step(self, actions):
        return self.env.step(self.action(actions))

    def destroy_wrap(self):
        """Free this wrapper's device object (the repair layer's queue); the wrapped env stays open."""
        wrap, self._wrap = self._wrap, None
        if wrap is not None:
            self._eng.wrap_destroy(wrap)
        if self._buf is not None:
            self._buf.free()
            self._buf = None

    def close(self):
        self.destroy_wrap()
        return self.env.close()


class BinaryAction(_ActionWrapper):
    """action_wrappers.py:8-47."""


class ThreeStep_Action(_ActionWrapper):
    """action_wrappers.py:50-90: raw actions 0 / 1 / 2."""


class ThreeStep_Action_DiscreteActionSpace(_ActionWrapper):
    """action_wrappers.py:93-138: ThreeStep_Action's action(); the reference also sets env.action_space to MultiDiscrete([3] * P), which is
    left to the caller here (the engine's envs carry no gymnasium spaces of their own to replace)."""


class Rescale_RepairLayer(_ActionWrapper):
    """action_wrappers.py:159-451; one port per charger only (:186)."""

    def _check(self, eng):
        if int(eng.P) != int(eng.C):
            raise ValueError("Rescale_RepairLayer: this class is only implemented for one port per charging station (action_wrappers.py:186)")


class MinMax_RepairLayer:
    """action_wrappers.py:454-605: the reference's constructor raises before it does anything."""

    def __init__(self, env, verbose=False, **kwargs):
        raise NotImplementedError("MinMax_RepairLayer is not implemented yet!!!!")
