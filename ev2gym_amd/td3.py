"""The learner of the off-policy collector: SB3's `TD3.train()` for `TD3Policy` on a Box action space, on the device (`csrc/ev2g_td3.h`,
`ev2g_td3_*`), with DDPG as the preset SB3 itself makes of it (one critic, no delay, no target noise).

`TD3Learner(collector)` / `DDPGLearner(collector)` bind a device learner to a `DeviceReplayCollector`'s policy object.  `train(gradient_steps,
batch_size)` runs sample -> update on the device -- the uniform draw from the replay ring's complete blocks (`ev2g_replay_sample`), the target
with its smoothing noise, the critics' step, every policy_delay-th update the actor's step, the Polyak step and the rewrite of the packed weights
the collector's launches read -- with one synchronisation at the end; neither the batch nor the weights leave the device, and
`collector.set_weights` is not needed in the loop.  `learn(total_timesteps)` alternates `collector.collect_episode()` and `train()`.

Per gradient step on (s, a, r, s', done), the update counter n incremented first (SB3's arithmetic):

    eps = clamp(N(0, target_policy_noise), -target_noise_clip, +target_noise_clip);  a' = clamp(actor_target(s') + eps, -1, 1)
    y = r + (1 - done) * gamma * min_j critic_target_j(s', a');   critic_loss = sum_j mean((critic_j(s, a~) - y)^2)   -> Adam on all critics
    n % policy_delay == 0: actor_loss = -mean(critic_0(s, actor(s))) with critic_0 after its step -> Adam on the actor, then
                           target <- (1 - tau) * target + tau * param
    torch.optim.Adam(eps=1e-8), no gradient clipping

The ring stores the env's action in [lo, 1]; the critics take SB3's scaled action a~ in [-1, 1]: 2 a - 1 for lo = 0, a itself for lo = -1.
`done` is used as stored: the reference registers no time limit, so SB3 treats its episode ends as terminal.

`td3_update_numpy` (with `td3_critic_numpy` / `td3_actor_numpy`) is the float64 restatement with analytic backprop, no torch: the numerics
reference the tests hold the kernels to.  Refused with a message: `action_noise`, a `learning_starts` warm-up, schedule objects (drive one with
`set_rate()`), `optimize_memory_usage` options, SAC / TQC (`make_learner`: SAC is `ev2gym_amd.sac.SACLearner`, behind its own collector).  SB3's default for both algorithms is `action_noise=None`, which
is what the reference script runs.
"""
from __future__ import annotations

import types

import numpy as np

from . import _abi
from .ppo import adam_numpy

ACTOR_KEYS = tuple(f"mu.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias"))
CRITIC_KEYS = tuple(f"{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias"))


def init_critic_weights(D, P, seed=0, h1=400, h2=300):
    """torch.nn.Linear-style uniform(-1/sqrt(in), 1/sqrt(in)) weights of one critic (D + P -> h1 -> h2 -> 1) as numpy float32."""
    rng = np.random.default_rng(seed)
    out = []
    for n_in, n_out in ((D + P, h1), (h1, h2), (h2, 1)):
        k = 1.0 / np.sqrt(n_in)
        out += [rng.uniform(-k, k, (n_out, n_in)).astype(np.float32), rng.uniform(-k, k, n_out).astype(np.float32)]
    return out


def scale_action(a, lo):
    """The stored env action in [lo, 1] as the critic reads it (SB3's scale_action)."""
    return 2.0 * a - 1.0 if float(lo) == 0.0 else a


def _forward(w, x, tanh):
    W1, b1, W2, b2, W3, b3 = w
    z1 = x @ W1.T + b1; h1 = np.maximum(z1, 0.0)
    z2 = h1 @ W2.T + b2; h2 = np.maximum(z2, 0.0)
    z3 = h2 @ W3.T + b3
    return types.SimpleNamespace(x=x, z1=z1, h1=h1, z2=z2, h2=h2, out=np.tanh(z3) if tanh else z3)


def _backward(w, f, d3):
    """From the delta at the output layer's pre-activation: (the six gradients, the delta of the input)."""
    d2 = (d3 @ w[4]) * (f.z2 > 0.0)
    d1 = (d2 @ w[2]) * (f.z1 > 0.0)
    return [d1.T @ f.x, d1.sum(0), d2.T @ f.h1, d2.sum(0), d3.T @ f.h2, d3.sum(0)], d1 @ w[0]


def _f64(ws):
    return [np.asarray(a, np.float64) for a in ws]


def td3_critic_numpy(actor_target, critics, critics_target, obs, actions, reward, next_obs, done, normals=None, lo=-1.0, gamma=0.99,
                     target_policy_noise=0.2, target_noise_clip=0.5):
    """The critics' half of one step in float64.  normals [B, P]: the standard normals of the smoothing noise (None or noise 0: none).
    Returns (grads: one list of six per critic, critic_loss, aux) with aux.y, aux.q [n_critics, B], aux.a_next and the forwards aux.f."""
    s, s2 = np.asarray(obs, np.float64), np.asarray(next_obs, np.float64)
    a = scale_action(np.asarray(actions, np.float64), lo)
    r, d = np.asarray(reward, np.float64).reshape(-1), np.asarray(done, np.float64).reshape(-1)
    B = s.shape[0]
    at = _forward(_f64(actor_target), s2, True).out
    eps = 0.0
    if normals is not None and target_policy_noise > 0.0:
        eps = np.clip(target_policy_noise * np.asarray(normals, np.float64).reshape(at.shape), -target_noise_clip, target_noise_clip)
    a_next = np.clip(at + eps, -1.0, 1.0)
    tq = np.stack([_forward(_f64(c), np.concatenate([s2, a_next], 1), False).out[:, 0] for c in critics_target])
    y = r + (1.0 - d) * gamma * tq.min(axis=0)
    xa = np.concatenate([s, a], 1)
    grads, q, fs, loss = [], [], [], 0.0
    for c in critics:
        c = _f64(c)
        f = _forward(c, xa, False)
        qj = f.out[:, 0]
        loss += float(((qj - y) ** 2).mean())
        grads.append(_backward(c, f, (2.0 * (qj - y) / B)[:, None])[0])
        q.append(qj); fs.append(f)
    return grads, loss, types.SimpleNamespace(y=y, q=np.stack(q), tq=tq, a_next=a_next, a_target=at, f=fs)


def td3_actor_numpy(actor, critic0, obs):
    """The actor's half in float64: (the actor's six gradients, actor_loss, aux) with aux.fa / aux.fc the actor's and critic_0's forwards."""
    s = np.asarray(obs, np.float64)
    B, D = s.shape
    wa, wc = _f64(actor), _f64(critic0)
    fa = _forward(wa, s, True)
    fc = _forward(wc, np.concatenate([s, fa.out], 1), False)
    _, dxa = _backward(wc, fc, np.full((B, 1), -1.0 / B))
    grads, _ = _backward(wa, fa, dxa[:, D:] * (1.0 - fa.out * fa.out))
    return grads, float(-fc.out[:, 0].mean()), types.SimpleNamespace(fa=fa, fc=fc)


def td3_state(actor, critics):
    """A float64 learner state from initial weights: masters, targets (copies), Adam's moments at zero, the counters."""
    actor, critics = _f64(actor), [_f64(c) for c in critics]
    zeros = lambda ws: [np.zeros_like(a) for a in ws]  # noqa: E731
    return types.SimpleNamespace(actor=actor, critics=critics, actor_target=[a.copy() for a in actor], critics_target=[[a.copy() for a in c] for c in critics],
                                 m_actor=zeros(actor), v_actor=zeros(actor), m_critics=[zeros(c) for c in critics], v_critics=[zeros(c) for c in critics],
                                 n=0, t_critic=0, t_actor=0)


def td3_update_numpy(st, obs, actions, reward, next_obs, done, normals=None, lo=-1.0, lr=1e-3, tau=0.005, gamma=0.99, policy_delay=2,
                     target_policy_noise=0.2, target_noise_clip=0.5, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """One gradient step of TD3 on the float64 state `st` (td3_state), in place.  Returns a namespace: critic_loss, actor_loss (None when the
    actor did not step), y, critic_grads, actor_grads (None likewise)."""
    cg, closs, aux = td3_critic_numpy(st.actor_target, st.critics, st.critics_target, obs, actions, reward, next_obs, done, normals, lo, gamma,
                                      target_policy_noise, target_noise_clip)
    st.n += 1; st.t_critic += 1
    for j, g in enumerate(cg):
        for i in range(6):
            st.critics[j][i], st.m_critics[j][i], st.v_critics[j][i] = adam_numpy(st.critics[j][i], st.m_critics[j][i], st.v_critics[j][i], g[i], st.t_critic,
                                                                                   lr, beta1, beta2, adam_eps)
    out = types.SimpleNamespace(critic_loss=closs, actor_loss=None, y=aux.y, critic_grads=cg, actor_grads=None, aux=aux)
    if st.n % int(policy_delay) == 0:
        ag, aloss, _ = td3_actor_numpy(st.actor, st.critics[0], obs)
        st.t_actor += 1
        for i in range(6):
            st.actor[i], st.m_actor[i], st.v_actor[i] = adam_numpy(st.actor[i], st.m_actor[i], st.v_actor[i], ag[i], st.t_actor, lr, beta1, beta2, adam_eps)
        for tgt, src in zip(st.critics_target + [st.actor_target], st.critics + [st.actor]):
            for i in range(6):
                tgt[i] = (1.0 - tau) * tgt[i] + tau * src[i]
        out.actor_loss, out.actor_grads = aloss, ag
    return out


MAX_BLOCKS = 32   # EV2G_REPLAY_MAX_BLOCKS: complete blocks a draw's table holds


class TD3Learner:
    """SB3's TD3.train() on the device behind a DeviceReplayCollector.

    The learner takes `actor` (default: the weights the collector was created with) and `critics` (default: torch.nn.Linear-style draws from
    `seed`) as float32 masters on the device and rewrites the collector's policy object from the actor's masters at creation and after every
    actor step.  `state_dict()` reads masters and targets back; `close()` (or closing the collector or the engine, in any order) frees it."""

    PRESET = dict(n_critics=2, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5, lr=1e-3, tau=0.005, gamma=0.99, batch_size=256)
    DDPG = False

    def __init__(self, collector, actor=None, critics=None, seed=0, sample_seed=None, **kw):
        name = type(self).__name__
        for k, bad in (("action_noise", lambda v: v is not None), ("learning_starts", lambda v: int(v) != 0),
                       ("optimize_memory_usage", lambda v: bool(v)), ("handle_timeout_termination", lambda v: bool(v))):
            if k in kw and bad(kw.pop(k)):
                raise ValueError(f"{name}: {k} is not supported (exploration noise, a random warm-up and the replay buffer's memory options are out "
                                 "of scope; see the module docstring)")
        cfg = dict(self.PRESET, **{k: kw.pop(k) for k in list(kw) if k in self.PRESET or k in ("beta1", "beta2", "adam_eps")})
        if kw:
            raise ValueError(f"{name}: {sorted(kw)[0]} is not supported (see the module docstring)")
        if any(callable(cfg[k]) for k in ("lr", "tau", "gamma")):
            raise ValueError(f"{name}: lr, tau and gamma are numbers; drive a schedule with set_rate() between train() calls")
        self.learner, self._bufs = None, None   # (close() works on a learner whose creation failed)
        self.batch_size = int(cfg.pop("batch_size"))
        if not 1 <= self.batch_size <= _abi.TD3_MAX_BATCH:
            raise ValueError(f"{name}: batch_size {self.batch_size} is outside 1 .. {_abi.TD3_MAX_BATCH}")
        self.collector, self.eng = collector, collector.eng
        if getattr(getattr(collector, "learner", None), "learner", None):
            raise ValueError(f"{name}: the collector's policy already has a learner")
        if getattr(collector, "cap", 2) - 1 > MAX_BLOCKS:
            raise ValueError(f"{name}: the collector's ring holds up to {collector.cap - 1} complete episodes, the sampler's table {MAX_BLOCKS}: "
                             f"capacity_episodes must be at most {MAX_BLOCKS + 1}")
        actor = actor if actor is not None else getattr(collector, "weights", None)
        if actor is None:
            raise ValueError(f"{name}: the collector does not keep its weights; pass actor=")
        actor = [np.ascontiguousarray(a, np.float32) for a in actor]
        (h1, D), h2, P = actor[0].shape, actor[2].shape[0], actor[4].shape[0]
        n_critics = int(cfg["n_critics"])
        if critics is None:
            critics = [init_critic_weights(D, P, seed=int(seed) + 1 + j, h1=h1, h2=h2) for j in range(n_critics)]
        self.shape = (D, h1, h2, P, n_critics)
        self.cfg, self.lr = cfg, float(cfg["lr"])
        self.sample_seed = int(seed if sample_seed is None else sample_seed)
        self.sample_counter = 0     # the draw counter of the next sampled batch (ev2g_replay_sample)
        self.num_timesteps = 0
        self.last_losses = None
        self.learner = self.eng.td3_create(collector.mlp, actor, critics, seed=seed, ddpg=self.DDPG, **cfg)
        collector.learner = self

    td3 = property(lambda self: self.learner)   # the device learner

    def set_rate(self, lr):
        """The learning rate of the following updates (how a schedule is driven from Python)."""
        self.lr = float(lr)
        self.eng.td3_set_rate(self.learner, self.lr)

    def counters(self):
        """(updates, actor steps -- each one a refresh of the collector's policy --, the next noise draw index)."""
        return self.eng.td3_counters(self.learner)

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
                                e.empty((B,), np.uint8), e.empty((steps, 2), np.float32)])
        return self._bufs[1]

    def train(self, gradient_steps, batch_size=None):
        """gradient_steps x (sample a batch from the complete blocks -> one update), all enqueued on the engine's stream, one synchronisation
        at the end.  Returns critic_loss (mean), actor_loss (mean over the updates that stepped the actor; NaN if none did) and n_updates."""
        B, steps = int(batch_size or self.batch_size), int(gradient_steps)
        if steps < 1:
            raise ValueError("train: gradient_steps must be at least 1")
        blocks = self.complete_blocks()
        if not blocks:
            raise RuntimeError("train: the replay ring holds no complete episode (collector.collect_episode() first)")
        c, eng = self.collector, self.eng
        obs, act, rew, nxt, done, losses = self._batch_buffers(B, steps)
        losses.upload(np.full((steps, 2), np.nan, np.float32))
        ring = [(c.obs[b], c.actions[b], c.reward[b], c.done[b]) for b in blocks]
        for k in range(steps):
            eng.replay_sample(ring, c.T, c.E, c.D, c.P, B, self.sample_seed, self.sample_counter, obs, act, rew, nxt, done)
            self.sample_counter += 1
            eng.td3_update(self.learner, obs, act, rew, nxt, done, B, losses.at(2 * k))
        self.last_losses = losses.to_host()   # (synchronises)
        al = self.last_losses[:, 1]
        return dict(critic_loss=float(self.last_losses[:, 0].astype(np.float64).mean()),
                    actor_loss=float(al[~np.isnan(al)].astype(np.float64).mean()) if (~np.isnan(al)).any() else float("nan"), n_updates=self.counters()[0])

    def learn(self, total_timesteps, gradient_steps=None, batch_size=None):
        """collector.collect_episode() and train() in turn until total_timesteps env steps were collected; returns what every train() returned.
        gradient_steps defaults to T: one update per collected vector step, the cadence of SB3's train_freq=1, gradient_steps=1 on a VecEnv.
        Unlike SB3's loop the policy changes PER EPISODE here, not per step: a whole episode is collected with the actor as it stood at its
        start, then the episode's updates run."""
        out = []
        target = self.num_timesteps + int(total_timesteps)
        while self.num_timesteps < target:
            self.collector.collect_episode()
            self.num_timesteps += self.collector.T * self.collector.E
            out.append(self.train(self.collector.T if gradient_steps is None else gradient_steps, batch_size))
        return out

    def get_weights(self, target=False):
        """(actor six arrays, [critic six arrays, ...]) read back from the device: the masters, or the target networks."""
        flat = self.eng.td3_get_weights(self.learner, self.shape, target)
        return flat[:6], [flat[6 + 6 * j:12 + 6 * j] for j in range(self.shape[4])]

    def get_grads(self):
        flat = self.eng.td3_get_grads(self.learner, self.shape)
        return flat[:6], [flat[6 + 6 * j:12 + 6 * j] for j in range(self.shape[4])]

    def state_dict(self):
        """The parameters under SB3's TD3Policy keys: actor.mu.{0,2,4}.*, critic.qf{j}.{0,2,4}.* and the *_target twins."""
        out = {}
        for suffix, target in (("", False), ("_target", True)):
            actor, critics = self.get_weights(target)
            out.update({f"actor{suffix}.{k}": a for k, a in zip(ACTOR_KEYS, actor)})
            for j, c in enumerate(critics):
                out.update({f"critic{suffix}.qf{j}.{k}": a for k, a in zip(CRITIC_KEYS, c)})
        return out

    def close(self):
        if self.learner:
            self.eng.td3_destroy(self.learner)   # (nothing happens if the collector's policy or the engine already took it along)
        self.learner = None
        if getattr(self.collector, "learner", None) is self:
            self.collector.learner = None
        if self._bufs is not None and self.eng._h:
            for b in self._bufs[1]:
                b.free()
        self._bufs = None


class DDPGLearner(TD3Learner):
    """SB3's DDPG: TD3 with one critic, no delay and no target noise, and the reference script's lr 1e-3, batch_size 100, tau 0.005, gamma 0.99."""

    PRESET = dict(n_critics=1, policy_delay=1, target_policy_noise=0.0, target_noise_clip=0.5, lr=1e-3, tau=0.005, gamma=0.99, batch_size=100)
    DDPG = True


def make_learner(algo, collector, **kw):
    """The learner of an off-policy algorithm by SB3's name: "TD3" or "DDPG".  SAC is refused here -- this module's collector owns a deterministic
    policy object; ev2gym_amd.sac.SACLearner trains SAC behind a SACCollector -- and so is TQC."""
    kinds = {"td3": TD3Learner, "ddpg": DDPGLearner}
    if str(algo).lower() not in kinds:
        raise ValueError(f"make_learner: {algo} is not supported (TD3 and DDPG are; SAC / TQC are not this module's: SAC is "
                         "ev2gym_amd.sac.SACLearner behind a SACCollector, TQC is out of scope)")
    return kinds[str(algo).lower()](collector, **kw)


__all__ = ["TD3Learner", "DDPGLearner", "make_learner", "td3_update_numpy", "td3_critic_numpy", "td3_actor_numpy", "td3_state", "init_critic_weights",
           "scale_action", "ACTOR_KEYS", "CRITIC_KEYS"]
