"""The TQC learner and its collection actor on the device (csrc/ev2g_tqc.h over csrc/ev2g_sac.h, ev2gym_amd/tqc.py).

Tolerance idiom (tests/test_sac_gpu.py): the reference is float64 (torch autograd, torch.sort and torch.optim.Adam in float64, which
tests/test_tqc_cpu.py ties to tqc_update_numpy at 1e-9); d32 is the largest deviation of the same computation in torch-CPU float32; the device
gets 4 d32 + 4 * 2^-23 * s, s = max(1, |value|) for values and the array's largest reference magnitude for gradients.  Every d32 and device
deviation is printed before it is asserted.  Everything else is bit for bit: the sort-and-truncate kernel against its host twin, Adam and Polyak
against theirs, two fresh learners against each other, and the collection actor against SAC's.

The case builder (tests/tqc_cases.py) redraws any row with a backpropagated ReLU pre-activation below 1e-5, centres the rewards, and asserts that
all four regions of the Huber loss are met and that the truncation drops atoms of more than one critic."""
import math

import numpy as np
import pytest

from tests import tqc_cases as tc
from tests.learner_cases import engines  # noqa: F401  (the fixture)
from tests.test_onpolicy_gpu import E_GEN, T_SHORT, _bits, _gen_engine, _up

pytestmark = pytest.mark.gpu


class _Dev:
    """A case's rows on an engine and a TQC object."""

    def __init__(self, eng, case, rows=None, **cfg):
        self.eng, self.case = eng, case
        self.shape = (case["D"], case["h"][0], case["h"][1], case["P"], case["n_critics"], case["n_quantiles"])
        self.K = tc.kept(case)
        self.t = eng.tqc_create(case["actor"], case["critics"], case["lo"], seed=case["noise_seed"], n_critics=case["n_critics"], n_quantiles=case["n_quantiles"],
                                top_quantiles_to_drop_per_net=case["drop"], ent_coef=math.exp(case["log_ent_coef"]), ent_coef_auto=int(case["auto"]),
                                gamma=case["gamma"], **cfg)
        eng.tqc_seed(self.t, case["noise_seed"], case["first_draw"])
        self.losses = eng.empty((4,), np.float32)
        self.bufs = None
        self.load(slice(None) if rows is None else rows)

    def load(self, rows):
        if self.bufs:
            for b in self.bufs:
                b.free()
        c = self.case
        self.bufs = [_up(self.eng, c[k][rows]) for k in ("obs", "actions", "reward", "next_obs", "done")]
        self.B = self.bufs[0].shape[0]

    def split(self, flat):
        return flat[:8], [flat[8 + 6 * j:14 + 6 * j] for j in range(self.shape[4])]

    def grads(self):
        flat, g = self.eng.tqc_get_grads(self.t, self.shape)
        return (*self.split(flat), g)

    def weights(self):
        return self.split(self.eng.tqc_get_weights(self.t, self.shape))

    def targets(self):
        flat = self.eng.tqc_get_weights(self.t, self.shape, True)
        return [flat[6 * j:6 + 6 * j] for j in range(self.shape[4])]

    def update(self):
        self.eng.tqc_update(self.t, *self.bufs, self.B, self.losses)
        return self.losses.to_host()

    def act(self, x, deterministic=False, t=None, fn=None):
        eng, n, P = self.eng, len(x), self.case["P"]
        xb = _up(eng, np.ascontiguousarray(x, np.float32))
        outs = [eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n,), np.float32)]
        (fn or eng.tqc_act)(t or self.t, xb, n, outs[0], deterministic, *outs[1:])
        got = [o.to_host() for o in outs]
        for b in [xb] + outs:
            b.free()
        return got

    def close(self):
        self.eng.tqc_destroy(self.t)
        for b in self.bufs + [self.losses]:
            b.free()


def _flat(actor, critics):
    return list(actor) + [a for c in critics for a in c]


# ---- 1. one staged step against the float64 reference ----
def _staged_step(eng, case, ref, ref32, tag):
    """The critics' stage, then the actor's, on `case`: z, both log pi, the losses, every gradient and that of log_ent_coef under the idiom."""
    nc, B, auto = case["n_critics"], case["B"], case["auto"]
    d = _Dev(eng, case)
    try:
        eng.tqc_critic_grad(d.t, *d.bufs, B, d.losses)
        z, lp2 = eng.tqc_get_z(d.t, B, d.K)
        _, cg, _ = d.grads()
        closs = d.losses.to_host()[0]
        assert eng.tqc_counters(d.t) == (0, 0, 1000, 0)
        assert (np.diff(z, axis=1) >= 0.0).all() or case["done"].all()   # a row's kept atoms ascend (gamma (1 - done) >= 0)
        eng.tqc_actor_grad(d.t, d.bufs[0], B, d.losses)
        ag, cg_after, ga = d.grads()
        lp = eng.tqc_get_log_pi(d.t, B)
        _, aloss, eloss, alpha = d.losses.to_host()
        for a, b in zip(_flat([], cg), _flat([], cg_after)):   # the actor's stage leaves the critics' gradient alone
            assert np.array_equal(_bits(a), _bits(b))
        assert abs(float(alpha) - math.exp(case["log_ent_coef"])) <= 2.0 ** -23
        tc.check_arrays(tag + " z, log pi', log pi", [z, lp2, lp], [ref["z"], ref["log_pi_next"], ref["log_pi"]], [ref32["z"], ref32["log_pi_next"], ref32["log_pi"]],
                        values=True)
        tc.check_arrays(tag + " losses", [[closs], [aloss]], [[ref["critic_loss"]], [ref["actor_loss"]]], [[ref32["critic_loss"]], [ref32["actor_loss"]]], values=True)
        if auto:
            tc.check_arrays(tag + " ent_coef loss, grad", [[eloss], [ga]], [[ref["ent_coef_loss"]], [ref["ent_coef_grad"]]],
                            [[ref32["ent_coef_loss"]], [ref32["ent_coef_grad"]]], values=True)
        else:
            assert eloss == 0.0 and ga == 0.0
        for j in range(nc):
            tc.check_arrays(tag + f" critic {j} grad", cg[j], ref["critic_grads"][j], ref32["critic_grads"][j])
        tc.check_arrays(tag + " actor grad", ag, ref["actor_grads"], ref32["actor_grads"])
    finally:
        d.close()


# tests/tqc_cases.grad_cases(): every network with every (nc, nq, d) and every (D, P); tests/test_tqc_cpu.py asserts that coverage.
@pytest.mark.parametrize("net,dp,qs,lo,auto,B", tc.grad_cases())
def test_gradients_z_log_pi_and_losses_against_float64(engines, net, dp, qs, lo, auto, B):  # noqa: F811
    import torch
    (D, P), (nc, nq, drop) = dp, qs
    case = tc.grad_case(net, dp, qs, lo, auto, B)
    ref, ref32 = tc.torch_grads(case, torch.float64), tc.torch_grads(case, torch.float32)
    tag = (f"tqc {net} D{D} P{P} {nc}x{nq} d{drop} lo{lo:g} auto{int(auto)} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}, regions "
           f"{np.round(case['regions'], 3).tolist()}, mixed drop {case['mixed_drop']})")
    _staged_step(engines["pst"], case, ref, ref32, tag)


# The plan's limits and the sort's lane edges (tests/tqc_cases.EDGE_GRAD_CASES; tests/test_tqc_cpu.py pins the cases' conditions).
@pytest.mark.parametrize("tag,nc,nq,drop,lo,auto,B", tc.EDGE_GRAD_CASES)
def test_gradients_at_the_plans_limits_and_lane_edges(engines, tag, nc, nq, drop, lo, auto, B):  # noqa: F811
    import torch
    case = tc.edge_grad_case(tag, nc, nq, drop, lo, auto, B)
    name = f"tqc edge {tag} {nc}x{nq} d{drop} lo{lo:g} auto{int(auto)} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']})"
    _staged_step(engines["pst"], case, case["ref64"], tc.torch_grads(case, torch.float32), name)


# ---- 2. the sort-and-truncate kernel alone against its host twin, bit for bit ----
@pytest.mark.parametrize("nc,nq,drop", tc.SORT_SHAPES)
def test_truncate_equals_the_host_twin_bit_for_bit(engines, nc, nq, drop):  # noqa: F811
    from ev2gym_amd.engine import host_tqc_target
    eng = engines["pst"]
    la = np.array([math.log(0.3)], np.float32)
    la_dev = _up(eng, la)
    try:
        for B in (1, 33):
            for kind in tc.SORT_KINDS:
                tq, lp, r, done = tc.sort_rows(kind, nc, nq, B)
                bufs = [_up(eng, a) for a in (tq, lp, r, done)]
                out = eng.empty((B, nc * (nq - drop)), np.float32)
                try:
                    eng.tqc_truncate(*bufs, B, nc, nq, drop, 0.99, la_dev, out)
                    got = out.to_host()
                finally:
                    for b in bufs + [out]:
                        b.free()
                want = host_tqc_target(tq, lp, r, done, drop, 0.99, la[0])
                assert np.array_equal(_bits(got), _bits(want)), (kind, B)
                if kind == "done":
                    assert np.array_equal(got, np.broadcast_to(r[:, None], got.shape))
    finally:
        la_dev.free()


# ---- 3. the same update on two fresh learners gives the same bits ----
@pytest.mark.parametrize("net,qs,B", [("256-256", (2, 25, 2), 37), ("33-17", (5, 25, 2), 257), ("limits", (2, 64, 0), 1024)])
def test_an_update_is_reproducible_bit_for_bit(engines, net, qs, B):  # noqa: F811
    D, P = tc.EDGE_NETS[net][0::3] if net in tc.EDGE_NETS else (63, 20)
    nc = qs[0]
    case = tc.make_case(D, P, net, *qs, B, 0.0, 0.7, True, seed=21)
    got = []
    for _ in range(2):
        d = _Dev(engines["pst"], case)
        try:
            losses = d.update()
            ag, cg, ga = d.grads()
            got.append([losses, np.float32(ga), d.eng.tqc_get_ent_coef(d.t)] + _flat(ag, cg) + _flat(*d.weights()) + _flat([], d.targets()) + d.act(case["obs"][:33]))
        finally:
            d.close()
    assert len(got[0]) == len(got[1]) == 3 + 2 * (8 + 6 * nc) + 6 * nc + 4
    assert np.isfinite(got[0][0]).all()
    for a, b in zip(*got):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 4. three updates: Adam and Polyak bit for bit by the host twins, the loop under the idiom; the repacked images ----
@pytest.mark.parametrize("net,qs,B,tui,auto", [("64-64", (2, 25, 2), 37, 1, True), ("256-256", (3, 7, 1), 17, 3, True), ("33-17", (1, 25, 2), 37, 3, False)])
def test_three_updates_adam_polyak_counters_and_repacked_images(engines, net, qs, B, tui, auto):  # noqa: F811
    import torch
    from ev2gym_amd.engine import host_adam, host_polyak
    eng = engines["pst"]
    D, P, nc = 63, 20, qs[0]
    case = tc.make_case(D, P, net, *qs, 3 * B, 0.0, 0.7, auto, seed=5)
    batches = tc.loop_batches(case, 3, B)
    ref, ref32 = tc.torch_loop(case, batches, torch.float64, tui), tc.torch_loop(case, batches, torch.float32, tui)
    d = _Dev(eng, case, rows=batches[0][0], target_update_interval=tui)
    fresh = None
    try:
        masters, targets = _flat(*d.weights()), _flat([], d.targets())
        for a, b in zip(masters[8:], targets):
            assert np.array_equal(_bits(a), _bits(b))
        m, v = [np.zeros_like(a) for a in masters], [np.zeros_like(a) for a in masters]
        ent = eng.tqc_get_ent_coef(d.t)
        assert ent[0] == np.float32(case["log_ent_coef"]) and not ent[1:].any()
        x_probe = case["obs"][:8]
        a_probe = d.act(x_probe, deterministic=True)[0]
        for k in range(3):
            d.load(batches[k][0])
            losses = d.update()
            ag, cg, ga = d.grads()
            grads, new, new_t, new_ent = _flat(ag, cg), _flat(*d.weights()), _flat([], d.targets()), eng.tqc_get_ent_coef(d.t)
            want = [a.copy() for a in masters]
            for i in range(len(want)):   # every array steps on every update, its Adam count is the update's
                host_adam(want[i], m[i], v[i], grads[i], k + 1, lr=3e-4, eps=1e-8)
            for i, (a, b) in enumerate(zip(new, want)):
                assert np.array_equal(_bits(a), _bits(b)), (k, i)
            e_want = [ent[i:i + 1].copy() for i in range(3)]
            if auto:
                host_adam(*e_want, np.array([ga], np.float32), k + 1, lr=3e-4, eps=1e-8)
                assert ga != 0.0
            assert np.array_equal(_bits(new_ent), _bits(np.concatenate(e_want))), k
            if (k + 1) % tui == 0:
                for i, (t_new, t_old, p) in enumerate(zip(new_t, targets, new[8:])):
                    moved = t_old.copy()
                    host_polyak(moved, p, 0.005)
                    assert np.array_equal(_bits(t_new), _bits(moved)), i
                    assert not np.array_equal(t_new, t_old)
            else:
                for a, b in zip(new_t, targets):
                    assert np.array_equal(_bits(a), _bits(b))
            assert eng.tqc_counters(d.t) == (k + 1, (k + 1) // tui, 2 * (k + 1) * B * P, 0)   # (deterministic launches draw nothing)
            tag = f"tqc loop {net} {qs[0]}x{qs[1]} d{qs[2]} B{B} tui{tui} step {k}"
            r, r32 = ref[k], ref32[k]
            names = ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")
            tc.check_arrays(tag + " losses", [[x] for x in losses], [[r[n]] for n in names], [[r32[n]] for n in names], values=True)
            tc.check_arrays(tag + " log_ent_coef", [new_ent[:1]], [[r["log_ent_coef"]]], [[r32["log_ent_coef"]]], values=True)
            tc.check_arrays(tag + " actor", new[:8], r["actor"], r32["actor"], values=True)
            for j in range(nc):
                tc.check_arrays(tag + f" critic {j}", new[8 + 6 * j:14 + 6 * j], r["critics"][j], r32["critics"][j], values=True)
                tc.check_arrays(tag + f" critic_target {j}", new_t[6 * j:6 + 6 * j], r["critics_target"][j], r32["critics_target"][j], values=True)
            masters, targets, ent = new, new_t, new_ent
        # the collection actor reads the trained masters: it equals, bit for bit, a fresh object created from them (the repack, and its padding)
        assert not np.array_equal(d.act(x_probe, deterministic=True)[0], a_probe)
        actor, critics = d.weights()
        fresh = eng.tqc_create(actor, critics, case["lo"], seed=case["noise_seed"], n_critics=nc, n_quantiles=qs[1], top_quantiles_to_drop_per_net=qs[2])
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:40]])
        for det in (True, False):
            eng.tqc_act_seed(d.t, 77, 3); eng.tqc_act_seed(fresh, 77, 3)
            for a, b in zip(d.act(x, det), d.act(x, det, t=fresh)):
                assert np.array_equal(_bits(a), _bits(b)), det
    finally:
        if fresh:
            eng.tqc_destroy(fresh)
        d.close()


# ---- 5. the actor is SAC's, bit for bit ----
@pytest.mark.parametrize("net,dp,lo", [("256-256", (162, 50), 0.0), ("33-17", (11, 5), -1.0), ("limits", (192, 64), 0.0)])
def test_act_rows_equal_sacs(engines, net, dp, lo):  # noqa: F811
    from ev2gym_amd.td3 import init_critic_weights
    eng = engines["ppl"]
    D, P = dp
    case = tc.make_case(D, P, net, 2, 25, 2, 37, lo, 0.7, True, seed=3)
    h1, h2 = case["h"]
    x = np.random.default_rng(8).uniform(0.0, 1.0, (70, D)).astype(np.float32)
    d = _Dev(eng, case)
    s = eng.sac_create(case["actor"], [init_critic_weights(D, P, 1, h1, h2)], lo, seed=case["noise_seed"], n_critics=1)
    try:
        for rows in (1, 33, 70):
            for det in (True, False):
                eng.tqc_act_seed(d.t, 19, 4); eng.sac_act_seed(s, 19, 4)
                for a, b in zip(d.act(x[:rows], det), d.act(x[:rows], det, t=s, fn=eng.sac_act)):
                    assert np.array_equal(_bits(a), _bits(b)), (rows, det)
                assert eng.tqc_counters(d.t)[3] == eng.sac_counters(s)[3] == 4 + (0 if det else 1)
    finally:
        eng.sac_destroy(s)
        d.close()


@pytest.mark.parametrize("kind,lo", [("pst", 0.0), ("ppl", -1.0)])
def test_collect_equals_a_twin_engine_driven_by_sac_collect(kind, lo):
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.td3 import init_critic_weights
    from ev2gym_amd.tqc import init_tqc_critic_weights
    eng, twin = _gen_engine(kind), _gen_engine(kind)
    E, D, P, k = eng.E, eng.D, eng.P, 4
    assert E == E_GEN
    actor = init_sac_actor_weights(D, P, 2, 64, 64)
    t = eng.tqc_create(actor, [init_tqc_critic_weights(D, P, 25, 5 + j, 64, 64) for j in range(2)], lo, seed=9)
    s = twin.sac_create(actor, [init_critic_weights(D, P, 5, 64, 64)], lo, seed=9, n_critics=1)
    mk = lambda e: [e.empty((k + 1, E, D), np.float32), e.empty((k, E, P), np.float32), e.empty((k, E), np.float64), e.empty((k, E), np.uint8),  # noqa: E731
                    e.empty((k, E, P), np.uint8)]
    a_bufs, b_bufs = mk(eng), mk(twin)
    try:
        for det in (False, True):
            eng.reset_f32(a_bufs[0], 0); twin.reset_f32(b_bufs[0], 0)
            eng.tqc_act_seed(t, 41, 5); twin.sac_act_seed(s, 41, 5)
            eng.tqc_collect(t, k, *a_bufs, deterministic=det)
            twin.sac_collect(s, k, *b_bufs, deterministic=det)
            assert eng.current_step == twin.current_step == k
            assert eng.tqc_counters(t)[3] == twin.sac_counters(s)[3] == 5 + (0 if det else k)
            for i, (a, b) in enumerate(zip(a_bufs, b_bufs)):
                assert np.array_equal(_bits(a.to_host()), _bits(b.to_host())), (det, i)
            act = a_bufs[1].to_host()
            assert act.min() >= lo and act.max() <= 1.0
            assert det or np.unique(act).size > k * E * P // 2   # (sampled: the draws tell the envs apart; tanh(mu) of like observations does not)
    finally:
        eng.close()
        twin.close()


# ---- 6. end to end, lifetimes and refusals ----
def _collector(eng, cap=3, seed=0, net=(64, 64)):
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.tqc import TQCCollector
    return TQCCollector(eng, init_sac_actor_weights(eng.D, eng.P, seed, *net), lo=0.0, capacity_episodes=cap, use_torch=False)


@pytest.mark.parametrize("ent_coef,qs", [("auto", (2, 25, 2)), (0.2, (3, 7, 1))])
def test_learn_end_to_end(ent_coef, qs):
    from ev2gym_amd.sac import SACLearner
    from ev2gym_amd.tqc import TQCLearner, make_learner
    eng = _gen_engine("pst")
    col = _collector(eng, seed=4)
    with pytest.raises(RuntimeError, match="no TQCLearner is bound"):
        col.collect_episode()
    with pytest.raises(ValueError, match="not a SACCollector"):
        SACLearner(col)
    nc, nq, drop = qs
    learner = make_learner("TQC", col, seed=3, batch_size=64, ent_coef=ent_coef, n_critics=nc, n_quantiles=nq, top_quantiles_to_drop_per_net=drop)
    try:
        assert isinstance(learner, TQCLearner) and col.tqc == learner.tqc
        T, E, D, P, B = col.T, col.E, col.D, col.P, 64
        assert (T, E) == (T_SHORT, E_GEN) and learner.shape == (D, 64, 64, P, nc, nq) and learner.kept_atoms == nc * (nq - drop)
        a0 = {"auto": 1.0, 0.2: 0.2}[ent_coef]
        assert abs(learner.ent_coef() - a0) < 1e-6 * a0
        out = learner.learn(2 * T * E, gradient_steps=3)
        assert len(out) == 2 and learner.num_timesteps == 2 * T * E and col.episodes == 2 and (col.head, col.filled) == (2, 2)
        assert learner.counters() == (6, 6, 6 * 2 * B * P, 2 * T) and learner.sample_counter == 6
        assert [o["n_updates"] for o in out] == [3, 6]
        assert all(np.isfinite(o[k]) for o in out for k in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef"))
        assert all(o["critic_loss"] > 0.0 for o in out)
        if isinstance(ent_coef, str):
            assert learner.ent_coef() != a0 and out[1]["ent_coef"] != out[0]["ent_coef"] and out[0]["ent_coef_loss"] != 0.0
        else:
            assert abs(learner.ent_coef() - a0) < 1e-6 * a0 and out[0]["ent_coef"] == out[1]["ent_coef"] and out[0]["ent_coef_loss"] == 0.0
        sd = learner.state_dict()
        assert len(sd) == 8 + 6 * nc + 6 * nc + 1
        assert sd["actor.latent_pi.0.weight"].shape == (64, D) and sd["actor.mu.weight"].shape == (P, 64) and sd["actor.log_std.bias"].shape == (P,)
        assert sd[f"critic.qf{nc - 1}.0.weight"].shape == (64, D + P) and sd["critic_target.qf0.4.weight"].shape == (nq, 64)
        assert sd["critic.qf0.4.bias"].shape == (nq,) and sd["log_ent_coef"].shape == (1,)
        assert not np.array_equal(sd["critic.qf0.4.weight"], sd["critic_target.qf0.4.weight"])
        ag, cg, _ = learner.get_grads()
        assert len(ag) == 8 and len(cg) == nc and cg[0][4].shape == (nq, 64) and all(np.isfinite(g).all() for g in ag + [a for c in cg for a in c])
        learner.set_rate(1e-4)
        acts = col.actions[1].to_host()
        assert acts.min() >= 0.0 and acts.max() <= 1.0 and np.unique(acts).size > acts.size // 2   # the ring holds sampled env actions
        assert col.collect_episode(deterministic=True) == 2 and learner.counters()[3] == 2 * T
    finally:
        if ent_coef == "auto":      # close() in any order frees everything once
            learner.close(); col.close(); eng.close(); learner.close()
        else:
            eng.close(); learner.close(); col.close()


def test_refusals_through_the_abi(engines):  # noqa: F811
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.tqc import init_tqc_critic_weights
    eng, other = engines["pst"], engines["ppl"]
    D, P = 63, 20
    case = tc.make_case(D, P, "64-64", 2, 25, 2, 8, -1.0, 0.7, True)
    d = _Dev(eng, case)

    def refused(code, word, fn, *a, **kw):
        with pytest.raises(EngineError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    s = None
    try:
        actor, critics = case["actor"], case["critics"]
        wide = init_sac_actor_weights(D, P, 0, 257, 64), [init_tqc_critic_weights(D, P, 25, 1 + j, 257, 64) for j in range(2)]
        refused(_abi.ERR_ARG, "ev2g_tqc: h1 257 is outside 1 .. 256", eng.tqc_create, *wide, -1.0)
        for (dd, hh1, hh2, pp), word in (((193, 64, 64, P), "d_in 193 is outside 1 .. 192"), ((D, 64, 257, P), "h2 257 is outside 1 .. 256"),
                                         ((D, 64, 64, 65), "d_out 65 is outside 1 .. 64")):
            refused(_abi.ERR_ARG, "ev2g_tqc: " + word, eng.tqc_create, init_sac_actor_weights(dd, pp, 0, hh1, hh2),
                    [init_tqc_critic_weights(dd, pp, 25, 1 + j, hh1, hh2) for j in range(2)], -1.0)
        refused(_abi.ERR_ARG, "tau must be in [0, 1]", eng.tqc_create, actor, critics, -1.0, tau=1.5)
        refused(_abi.ERR_ARG, "ent_coef must be finite and > 0", eng.tqc_create, actor, critics, -1.0, ent_coef=0.0)
        refused(_abi.ERR_ARG, "target_update_interval must be finite and >= 1", eng.tqc_create, actor, critics, -1.0, target_update_interval=0)
        refused(_abi.ERR_ARG, "n_critics 6 is outside 1 .. 5", eng.tqc_create, actor, critics * 3, -1.0, n_critics=6)
        q65 = [init_tqc_critic_weights(D, P, 65, 1 + j, 64, 64) for j in range(2)]
        refused(_abi.ERR_ARG, "n_quantiles 65 is outside 1 .. 64", eng.tqc_create, actor, q65, -1.0, n_quantiles=65)
        q43 = [init_tqc_critic_weights(D, P, 43, 1 + j, 64, 64) for j in range(3)]
        refused(_abi.ERR_ARG, "n_critics * n_quantiles 129 is outside 1 .. 128", eng.tqc_create, actor, q43, -1.0, n_critics=3, n_quantiles=43)
        refused(_abi.ERR_ARG, "top_quantiles_to_drop_per_net 25 is outside 0 .. 24", eng.tqc_create, actor, critics, -1.0, top_quantiles_to_drop_per_net=25)
        refused(_abi.ERR_ARG, "top_quantiles_to_drop_per_net -1 is outside 0 .. 24", eng.tqc_create, actor, critics, -1.0, top_quantiles_to_drop_per_net=-1)
        refused(_abi.ERR_ARG, "lo must be -1 or 0", eng.tqc_create, actor, critics, 0.5)
        for B in (0, 1025):
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.tqc_update, d.t, *d.bufs, B)
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.tqc_actor_grad, d.t, d.bufs[0], B)
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.tqc_truncate, d.bufs[0], d.bufs[2], d.bufs[2], d.bufs[4], B, 1, 4, 0, 0.99, d.bufs[2], d.bufs[1])
        refused(_abi.ERR_ARG, "n_quantiles 65 is outside 1 .. 64", eng.tqc_truncate, d.bufs[0], d.bufs[2], d.bufs[2], d.bufs[4], 8, 1, 65, 0, 0.99, d.bufs[2], d.bufs[1])
        refused(_abi.ERR_ARG, "null argument", eng.tqc_truncate, None, d.bufs[2], d.bufs[2], d.bufs[4], 8, 1, 4, 0, 0.99, d.bufs[2], d.bufs[1])
        # an object of another handle, and of another kind on this one
        refused(_abi.ERR_ARG, "the TQC learner was not created on this handle", other.tqc_update, d.t, *d.bufs, 8)
        s = eng.sac_create(actor, [c[:4] + [c[4][:1], c[5][:1]] for c in critics], -1.0)
        refused(_abi.ERR_ARG, "the TQC learner was not created on this handle", eng.tqc_apply, s)
        refused(_abi.ERR_ARG, "the SAC learner was not created on this handle", eng.sac_apply, d.t)
        refused(_abi.ERR_STATE, "no gradient to apply (ev2g_tqc_critic_grad or ev2g_tqc_actor_grad first)", eng.tqc_apply, d.t)
        refused(_abi.ERR_STATE, "no gradient to apply (ev2g_sac_critic_grad or ev2g_sac_actor_grad first)", eng.sac_apply, s)
        eng.tqc_critic_grad(d.t, *d.bufs, 8)
        eng.tqc_apply(d.t)
        assert eng.tqc_counters(d.t)[:3] == (0, 0, 0)   # a critics-only apply is no update: nothing counted, no draws consumed
        refused(_abi.ERR_STATE, "no gradient to apply", eng.tqc_apply, d.t)
        for lr in (float("nan"), -1.0, float("inf")):
            refused(_abi.ERR_ARG, "lr must be finite and >= 0", eng.tqc_set_rate, d.t, lr)
        eng.tqc_set_rate(d.t, 0.0)   # a zero rate is a rate: the masters and log_ent_coef stay
        before, ent = _flat(*d.weights()), eng.tqc_get_ent_coef(d.t)
        d.update()
        for a, b in zip(before, _flat(*d.weights())):
            assert np.array_equal(_bits(a), _bits(b))
        assert eng.tqc_get_ent_coef(d.t)[0] == ent[0]
        refused(_abi.ERR_ARG, "null argument", eng.tqc_update, d.t, None, *d.bufs[1:], 8)
        refused(_abi.ERR_ARG, "not the batch size", eng.tqc_get_z, d.t, 9, d.K)
        refused(_abi.ERR_ARG, "not the batch size", eng.tqc_get_log_pi, d.t, 9)
        refused(_abi.ERR_ARG, "n_rows is not positive", eng.tqc_act, d.t, d.bufs[0], 0, d.bufs[1])
        t2 = other.tqc_create(actor, critics, -1.0)
        E, k = other.E, 1
        bufs = [other.empty((k + 1, E, other.D), np.float32), other.empty((k, E, other.P), np.float32), other.empty((k, E), np.float64), other.empty((k, E), np.uint8),
                other.empty((k, E, other.P), np.uint8)]
        try:
            if (other.D, other.P) != (D, P):
                refused(_abi.ERR_ARG, "actor shape != (obs dim, ports)", other.tqc_collect, t2, 1, *bufs)
            refused(_abi.ERR_ARG, "not created on this handle", other.tqc_collect, d.t, 1, *bufs)
        finally:
            other.tqc_destroy(t2)
            for b in bufs:
                b.free()
        eng.tqc_destroy(d.t)
        refused(_abi.ERR_ARG, "not created on this handle", eng.tqc_apply, d.t)
    finally:
        if s:
            eng.sac_destroy(s)
        d.close()
