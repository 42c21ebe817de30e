"""The SAC learner and its collection actor on the device (csrc/ev2g_sac.h, ev2gym_amd/sac.py).

Tolerance idiom (tests/test_ppo_gpu.py): the reference is float64 (torch autograd and torch.optim.Adam in float64, which tests/test_sac_cpu.py
ties to sac_update_numpy at 1e-9); d32 is the largest deviation of the same computation in torch-CPU float32; the device gets 4 d32 + 4 * 2^-23 * s,
s = max(1, |y|) for values and the array's largest reference magnitude for gradients.  Every d32 and device deviation is printed before it is
asserted.  Everything else is bit for bit.

The case builder (tests/sac_cases.py) redraws any row with a backpropagated ReLU pre-activation, or the two critics' gap on (s, a_pi), below
1e-5, and asserts that fewer than a quarter of the rows needed it.

Off NETS (tests/sac_cases.EDGE_NETS): the plan's limits and the head's lane edges (one port per lane, a second and an eighth port on lane 0
alone, seven idle lanes) at batches up to 1024; a saturated actor under the mixed-precision yardstick, and the collection actor against its host
twin to one float32 ulp; the config's edges; the ring once it has wrapped.  tests/test_sac_cpu.py proves those cases' conditions without a GPU."""
import math

import numpy as np
import pytest

from tests import sac_cases as sc
from tests.learner_cases import engines  # noqa: F401  (the fixture)
from tests.test_onpolicy_gpu import E_GEN, T_SHORT, _bits, _gen_engine, _up

pytestmark = pytest.mark.gpu

BATCHES = (1, 17, 37, 257)
DP = ((11, 5), (63, 20), (162, 50))


def _grad_cases():
    """Every B with every network ((D, P), n_critics, lo and auto cycling so that each value meets each network and several B), the full cross of
    (n_critics, lo, auto) at 256-256, B 37, and the clamp case on two networks."""
    out, k = [], 0
    for B in BATCHES:
        for net in sc.NETS:
            out.append((net, DP[k % 3], 1 + (k // 2) % 2, (-1.0, 0.0)[(k // 3) % 2], bool((k // 5) % 2 == 0), False, B))
            k += 1
    for nc in (1, 2):
        for lo in (-1.0, 0.0):
            for auto in (True, False):
                out.append(("256-256", (63, 20), nc, lo, auto, False, 37))
    out += [("33-17", (11, 5), 2, -1.0, True, True, 37), ("256-256", (162, 50), 2, 0.0, True, True, 17)]
    return out


class _Dev:
    """A case's rows on an engine and a SAC object."""

    def __init__(self, eng, case, rows=None, **cfg):
        self.eng, self.case = eng, case
        self.shape = (case["D"], case["h"][0], case["h"][1], case["P"], case["n_critics"])
        self.s = eng.sac_create(case["actor"], case["critics"], case["lo"], seed=case["noise_seed"], n_critics=case["n_critics"],
                                ent_coef=math.exp(case["log_ent_coef"]), ent_coef_auto=int(case["auto"]), gamma=case["gamma"], **cfg)
        eng.sac_seed(self.s, case["noise_seed"], case["first_draw"])
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
        flat, g = self.eng.sac_get_grads(self.s, self.shape)
        return (*self.split(flat), g)

    def weights(self):
        return self.split(self.eng.sac_get_weights(self.s, self.shape))

    def targets(self):
        flat = self.eng.sac_get_weights(self.s, self.shape, True)
        return [flat[6 * j:6 + 6 * j] for j in range(self.shape[4])]

    def update(self):
        self.eng.sac_update(self.s, *self.bufs, self.B, self.losses)
        return self.losses.to_host()

    def act(self, x, deterministic=False, s=None, eng=None):
        eng = eng or self.eng
        n, P = len(x), self.case["P"]
        xb = _up(eng, np.ascontiguousarray(x, np.float32))
        outs = [eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n,), np.float32)]
        eng.sac_act(s or self.s, xb, n, outs[0], deterministic, *outs[1:])
        got = [o.to_host() for o in outs]
        for b in [xb] + outs:
            b.free()
        return got

    def close(self):
        self.eng.sac_destroy(self.s)
        for b in self.bufs + [self.losses]:
            b.free()


def _flat(actor, critics):
    return list(actor) + [a for c in critics for a in c]


# ---- 1. one staged step against the float64 reference ----
def _staged_step(eng, case, ref, ref32, tag, plain32=None):
    """The critics' stage, then the actor's, on `case`: y, both log pi, the losses and every gradient under the idiom, d32 taken from ref32
    (plain32: a second float32 computation whose d32 is printed next to it).  Returns the actor's gradient."""
    n_critics, B, auto, clamp = case["n_critics"], case["B"], case["auto"], case["clamp"]
    also = lambda *names: None if plain32 is None else [plain32[n] for n in names]   # noqa: E731
    d = _Dev(eng, case)
    try:
        d.eng.sac_critic_grad(d.s, *d.bufs, B, d.losses)
        y, lp2 = d.eng.sac_get_y(d.s, B)
        _, cg, _ = d.grads()
        closs = d.losses.to_host()[0]
        assert d.eng.sac_counters(d.s) == (0, 0, 1000, 0)
        d.eng.sac_actor_grad(d.s, d.bufs[0], B, d.losses)
        ag, cg_after, ga = d.grads()
        lp = d.eng.sac_get_log_pi(d.s, B)
        _, aloss, eloss, alpha = d.losses.to_host()
        for a, b in zip(_flat([], cg), _flat([], cg_after)):   # the actor's stage leaves the critics' gradient alone
            assert np.array_equal(_bits(a), _bits(b))
        assert abs(float(alpha) - math.exp(case["log_ent_coef"])) <= 2.0 ** -23   # (exp of the float32 log_ent_coef, rounded once; alpha 0.7)
        sc.check_arrays(tag + " y, log pi', log pi", [y, lp2, lp], [ref["y"], ref["log_pi_next"], ref["log_pi"]], [ref32["y"], ref32["log_pi_next"], ref32["log_pi"]],
                        values=True, plain32=also("y", "log_pi_next", "log_pi"))
        sc.check_arrays(tag + " losses", [[closs], [aloss]], [[ref["critic_loss"]], [ref["actor_loss"]]], [[ref32["critic_loss"]], [ref32["actor_loss"]]], values=True,
                        plain32=also("critic_loss", "actor_loss"))
        if auto:
            sc.check_arrays(tag + " ent_coef loss, grad", [[eloss], [ga]], [[ref["ent_coef_loss"]], [ref["ent_coef_grad"]]],
                            [[ref32["ent_coef_loss"]], [ref32["ent_coef_grad"]]], values=True, plain32=also("ent_coef_loss", "ent_coef_grad"))
        else:
            assert eloss == 0.0 and ga == 0.0
        for j in range(n_critics):
            sc.check_arrays(tag + f" critic {j} grad", cg[j], ref["critic_grads"][j], ref32["critic_grads"][j], plain32=plain32 and plain32["critic_grads"][j])
        sc.check_arrays(tag + " actor grad", ag, ref["actor_grads"], ref32["actor_grads"], plain32=plain32 and plain32["actor_grads"])
        if clamp:   # the two columns clamped for every row: exactly 0.0, not small
            assert np.array_equal(_bits(ag[6][:2]), _bits(np.zeros_like(ag[6][:2]))) and np.array_equal(_bits(ag[7][:2]), _bits(np.zeros(2, np.float32)))
            assert np.abs(ag[7][2:]).min() > 0.0
        return ag
    finally:
        d.close()


@pytest.mark.parametrize("net,dp,n_critics,lo,auto,clamp,B", _grad_cases())
def test_gradients_y_log_pi_and_losses_against_float64(engines, net, dp, n_critics, lo, auto, clamp, B):  # noqa: F811
    import torch
    D, P = dp
    case = sc.make_case(D, P, net, n_critics, B, lo, 0.7, auto, clamp, seed=7 + B, first_draw=1000)
    ref, ref32 = sc.torch_grads(case, torch.float64), sc.torch_grads(case, torch.float32)
    tag = f"sac {net} D{D} P{P} nc{n_critics} lo{lo:g} auto{int(auto)} clamp{int(clamp)} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']})"
    _staged_step(engines["pst"], case, ref, ref32, tag)


# The plan's limits and the head's lane edges (tests/sac_cases.EDGE_NETS; tests/test_sac_cpu.py pins the cases' conditions).
@pytest.mark.parametrize("tag,n_critics,lo,auto,B", sc.EDGE_GRAD_CASES)
def test_gradients_at_the_plans_limits_and_lane_edges(engines, tag, n_critics, lo, auto, B):  # noqa: F811
    import torch
    case = sc.edge_grad_case(tag, n_critics, lo, auto, B)
    name = f"sac edge {tag} nc{n_critics} lo{lo:g} auto{int(auto)} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']})"
    _staged_step(engines["pst"], case, case["ref64"], sc.torch_grads(case, torch.float32), name)


# A saturated actor: mu of every second port beyond +-10 for every row, so a = +-1 to float32 and log(1 - a^2 + 1e-6) sits at its floor.  The device
# computes the head in float64 from float32 mu / log_std (csrc/ev2g_sac.h), plain float32 torch forms 1 - a^2 in float32: its own error (1e-2 of
# log pi, 1 % of the actor's gradients) would make 4 d32 accept a device that returned zeros.  d32 is therefore taken from the MIXED reference --
# float32 networks, float64 head, the header's own split (sc.torch_actor) -- and the plain d32 is printed next to it.
@pytest.mark.parametrize("net,dp,n_critics,lo,auto,B", sc.SATURATED_GRAD_CASES)
def test_gradients_with_a_saturated_actor_against_the_mixed_reference(engines, net, dp, n_critics, lo, auto, B):  # noqa: F811
    import torch
    case = sc.saturated_grad_case(net, dp, n_critics, lo, auto, B)
    name = (f"sac saturated {net} nc{n_critics} lo{lo:g} auto{int(auto)} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}, "
            f"a at +-1 {case['share_at_1']:.4f})")
    mixed, plain = sc.torch_grads(case, torch.float32, mixed=True), sc.torch_grads(case, torch.float32)
    ag = _staged_step(engines["pst"], case, case["ref64"], mixed, name, plain32=plain)
    assert all(np.isfinite(g).all() and np.any(g) for g in ag)


# ---- 2. the same update on two fresh learners gives the same bits ----
@pytest.mark.parametrize("net,B", [("256-256", 37), ("33-17", 257), ("limits", 1024)])
def test_an_update_is_reproducible_bit_for_bit(engines, net, B):  # noqa: F811
    D, P = sc.EDGE_NETS[net][0::3] if net in sc.EDGE_NETS else (63, 20)
    case = sc.make_case(D, P, net, 2, B, 0.0, 0.7, True, seed=21)
    got = []
    for _ in range(2):
        d = _Dev(engines["pst"], case)
        try:
            losses = d.update()
            ag, cg, ga = d.grads()
            got.append([losses, np.float32(ga), d.eng.sac_get_ent_coef(d.s)] + _flat(ag, cg) + _flat(*d.weights()) + _flat([], d.targets()) + d.act(case["obs"][:33]))
        finally:
            d.close()
    assert len(got[0]) == len(got[1]) == 3 + 20 + 20 + 12 + 4
    assert np.isfinite(got[0][0]).all()
    for a, b in zip(*got):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 3. three updates: Adam and Polyak bit for bit by the host twins, the loop under the idiom; 5. the repacked images ----
@pytest.mark.parametrize("net,n_critics,B,tui,auto", [("64-64", 2, 37, 1, True), ("256-256", 2, 17, 2, True), ("33-17", 1, 37, 2, False)])
def test_three_updates_adam_polyak_counters_and_repacked_images(engines, net, n_critics, B, tui, auto):  # noqa: F811
    import torch
    from ev2gym_amd.engine import host_adam, host_polyak
    eng = engines["pst"]
    D, P = 63, 20
    case = sc.make_case(D, P, net, n_critics, 3 * B, 0.0, 0.7, auto, seed=5)
    batches = sc.loop_batches(case, 3, B)
    ref, ref32 = sc.torch_loop(case, batches, torch.float64, tui), sc.torch_loop(case, batches, torch.float32, tui)
    d = _Dev(eng, case, rows=batches[0][0], target_update_interval=tui)
    fresh = None
    try:
        masters, targets = _flat(*d.weights()), _flat([], d.targets())
        for a, b in zip(masters[8:], targets):
            assert np.array_equal(_bits(a), _bits(b))
        m, v = [np.zeros_like(a) for a in masters], [np.zeros_like(a) for a in masters]
        ent = d.eng.sac_get_ent_coef(d.s)
        assert ent[0] == np.float32(case["log_ent_coef"]) and not ent[1:].any()
        x_probe = case["obs"][:8]
        a_probe = d.act(x_probe, deterministic=True)[0]
        for k in range(3):
            d.load(batches[k][0])
            losses = d.update()
            ag, cg, ga = d.grads()
            grads, new, new_t, new_ent = _flat(ag, cg), _flat(*d.weights()), _flat([], d.targets()), d.eng.sac_get_ent_coef(d.s)
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
            assert d.eng.sac_counters(d.s) == (k + 1, (k + 1) // tui, 2 * (k + 1) * B * P, 0)   # (deterministic launches draw nothing)
            tag = f"sac loop {net} nc{n_critics} B{B} tui{tui} step {k}"
            r, r32 = ref[k], ref32[k]
            sc.check_arrays(tag + " losses", [[x] for x in losses], [[r[n]] for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")],
                            [[r32[n]] for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")], values=True)
            sc.check_arrays(tag + " log_ent_coef", [new_ent[:1]], [[r["log_ent_coef"]]], [[r32["log_ent_coef"]]], values=True)
            sc.check_arrays(tag + " actor", new[:8], r["actor"], r32["actor"], values=True)
            for j in range(n_critics):
                sc.check_arrays(tag + f" critic {j}", new[8 + 6 * j:14 + 6 * j], r["critics"][j], r32["critics"][j], values=True)
                sc.check_arrays(tag + f" critic_target {j}", new_t[6 * j:6 + 6 * j], r["critics_target"][j], r32["critics_target"][j], values=True)
            masters, targets, ent = new, new_t, new_ent
        # the collection actor reads the trained masters: it equals, bit for bit, a fresh object created from them (the repack, and its padding)
        assert not np.array_equal(d.act(x_probe, deterministic=True)[0], a_probe)
        actor, critics = d.weights()
        fresh = eng.sac_create(actor, critics, case["lo"], seed=case["noise_seed"], n_critics=n_critics)
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:40]])
        for det in (True, False):
            eng.sac_act_seed(d.s, 77, 3); eng.sac_act_seed(fresh, 77, 3)
            for a, b in zip(d.act(x, det), d.act(x, det, s=fresh)):
                assert np.array_equal(_bits(a), _bits(b)), det
    finally:
        if fresh:
            eng.sac_destroy(fresh)
        d.close()


# ---- 4. the collection actor ----
@pytest.mark.parametrize("net,dp,lo", [("256-256", (162, 50), 0.0), ("64-64", (63, 20), -1.0), ("33-17", (11, 5), 0.0)] +
                         [(tag, sc.EDGE_NETS[tag][0::3], lo) for tag, lo in sc.ACT_EDGE_CASES])
def test_act_against_float64_draw_indices_and_row_independence(engines, net, dp, lo):  # noqa: F811
    import torch
    from ev2gym_amd.engine import host_normal
    D, P = dp
    case = sc.make_case(D, P, net, 1, 70, lo, 0.7, True, clamp=P >= 3, seed=3)
    x = np.random.default_rng(8).uniform(0.0, 1.0, (70, D)).astype(np.float32)
    d = _Dev(engines["ppl"], case)
    try:
        n = 0
        for rows in (1, 31, 33, 70):
            for det in (True, False):
                d.eng.sac_act_seed(d.s, 19, n)
                got = d.act(x[:rows], det)
                eps = np.zeros((rows, P), np.float32) if det else host_normal(rows * P, 19, n * rows * P).reshape(rows, P)
                ref, ref32 = sc.torch_act(case["actor"], x[:rows], eps, torch.float64, lo), sc.torch_act(case["actor"], x[:rows], eps, torch.float32, lo)
                sc.check_arrays(f"sac act {net} D{D} P{P} lo{lo:g} rows{rows} det{int(det)} action, mu, log_std, log pi", got, ref, ref32, values=True)
                assert d.eng.sac_counters(d.s)[3] == n + (0 if det else 1)
                assert got[0].min() >= lo and got[0].max() <= 1.0
                n += 0 if det else 1
        # a row's outputs do not depend on the rows it is launched with: subset launches at the same draws (n n_rows = the first row's index)
        d.eng.sac_act_seed(d.s, 19, 0)
        full = d.act(x, False)
        for a, b in ((35, 70), (33, 66), (7, 14), (0, 1)):
            d.eng.sac_act_seed(d.s, 19, 1 if a else 0)
            assert (1 if a else 0) * (b - a) == a
            for f, s in zip(full, d.act(x[a:b], False)):
                assert np.array_equal(_bits(f[a:b]), _bits(s)), (a, b)
        det_full = d.act(x, True)
        for f, s in zip(det_full, d.act(x[33:66], True)):
            assert np.array_equal(_bits(f[33:66]), _bits(s))
        assert not np.array_equal(det_full[0], full[0])
    finally:
        d.close()


# The collection actor against its host twin on a saturated actor (every second port's mu beyond +-10; log_std column 0 at the upper clamp, column 1
# at the lower).  host_sac_head is applied to THE DEVICE'S OWN mu / log_std and host_normal's eps: both sides evaluate one float64 expression on
# identical float32 inputs and round once, and differ only by the double tanh / exp / log of two libraries.  1 - t^2 against 1e-6 amplifies that to
# about 4e-10 relative, so a result can only move across a float32 rounding boundary: 1 float32 ulp of the twin's value (np.spacing), for the tanh
# action -- the env action of lo 0 is held to the unscaled neighbours of the twin's tanh action -- and for log pi.  The butterfly's join order is
# part of the twin.  Where |u| >= 10 in float64 the action is exactly lo or 1: on every saturated port of the deterministic launch.  In the
# sampling launch the noise pulls some elements back, and those are left to the ulp bound: port 0 carries the upper clamp's sigma e^2 and is
# set aside; on the others sigma is about 1, u stays beyond 10 unless eps points inwards by more than about 2 (one draw in forty), and the
# float64 forward of these very inputs gives 0.976 -- at least 0.95 of them must be that deep.
@pytest.mark.parametrize("lo", [0.0, -1.0])
def test_act_on_a_saturated_actor_against_the_host_twin(engines, lo):  # noqa: F811
    from ev2gym_amd.engine import host_normal, host_sac_head
    from ev2gym_amd.sac import unscale_action
    from tests.test_ppo_cpu import _record
    D, P, rows = 63, 20, 70
    case = sc.act_case("64-64", (D, P), lo, saturate=True)
    x = np.random.default_rng(8).uniform(0.0, 1.0, (rows, D)).astype(np.float32)
    ports, sign = sc.saturated_ports(P)
    d = _Dev(engines["ppl"], case)
    try:
        for det in (True, False):
            d.eng.sac_act_seed(d.s, 19, 0)
            act, mu, ls, lp = d.act(x, det)
            eps = np.zeros((rows, P), np.float32) if det else host_normal(rows * P, 19, 0).reshape(rows, P)
            a, a_env, lp_twin = host_sac_head(mu, ls, eps, lo=lo)
            assert all(np.isfinite(o).all() for o in (act, mu, ls, lp))
            below, above = (unscale_action(np.nextafter(a, np.float32(s)), lo).astype(np.float32) for s in (-2.0, 2.0))
            off_a, off_lp = float((act != a_env).mean()), float((lp != lp_twin).mean())
            dev_lp = np.abs(lp.astype(np.float64) - lp_twin)
            _record(f"sac act twin lo{lo:g} det{int(det)}: actions off the twin's {off_a:.4f} of {act.size}, log pi off {off_lp:.4f} of {lp.size}, "
                    f"largest log pi deviation {dev_lp.max():.3e} against an ulp of {np.spacing(np.abs(lp_twin)).min():.3e} .. {np.spacing(np.abs(lp_twin)).max():.3e}")
            assert ((act >= below) & (act <= above)).all()
            assert (dev_lp <= np.spacing(np.abs(lp_twin))).all()
            u = mu.astype(np.float64) + np.exp(np.clip(ls.astype(np.float64), -20.0, 2.0)) * eps
            assert np.abs(mu[:, ports]).min() >= 10.0
            deep = np.abs(u[:, ports]) >= 10.0
            assert deep.all() if det else deep[:, 1:].mean() >= 0.95
            want = np.where(np.sign(u[:, ports]) > 0, np.float32(1.0), np.float32(lo))
            assert np.array_equal(act[:, ports][deep], want[deep])
            assert act.min() >= lo and act.max() <= 1.0
    finally:
        d.close()


# ---- 5b. config edges the checks accept: target_update_interval 3 with tau 1, a fixed target entropy ----
def test_config_edges_interval_3_tau_1(engines):  # noqa: F811
    """Three updates on 33-17: the targets stay through updates 1 and 2 and EQUAL the critics' masters bit for bit after the third
    (target * 0 + 1 * param with finite weights); the loop under the idiom."""
    import torch
    D, P, B = 63, 20, 37
    case = sc.make_case(D, P, "33-17", 2, 3 * B, -1.0, 0.7, True, seed=5)
    batches = sc.loop_batches(case, 3, B)
    ref, ref32 = sc.torch_loop(case, batches, torch.float64, 3, tau=1.0), sc.torch_loop(case, batches, torch.float32, 3, tau=1.0)
    d = _Dev(engines["pst"], case, rows=batches[0][0], target_update_interval=3, tau=1.0)
    try:
        targets = _flat([], d.targets())
        for k in range(3):
            d.load(batches[k][0])
            losses = d.update()
            new, new_t = _flat(*d.weights()), _flat([], d.targets())
            if k == 2:
                for i, (t_new, t_old, p) in enumerate(zip(new_t, targets, new[8:])):
                    assert np.array_equal(_bits(t_new), _bits(p)) and not np.array_equal(t_new, t_old), i
            else:
                for a, b in zip(new_t, targets):
                    assert np.array_equal(_bits(a), _bits(b))
            assert d.eng.sac_counters(d.s) == (k + 1, (k + 1) // 3, 2 * (k + 1) * B * P, 0)
            tag = f"sac config edges tui3 tau1 step {k}"
            r, r32 = ref[k], ref32[k]
            sc.check_arrays(tag + " losses", [[x] for x in losses], [[r[n]] for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")],
                            [[r32[n]] for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")], values=True)
            sc.check_arrays(tag + " actor", new[:8], r["actor"], r32["actor"], values=True)
            for j in range(2):
                sc.check_arrays(tag + f" critic {j}", new[8 + 6 * j:14 + 6 * j], r["critics"][j], r32["critics"][j], values=True)
                sc.check_arrays(tag + f" critic_target {j}", new_t[6 * j:6 + 6 * j], r["critics_target"][j], r32["critics_target"][j], values=True)
    finally:
        d.close()


def test_config_edges_a_fixed_target_entropy(engines):  # noqa: F811
    """target_entropy_auto 0 with target_entropy -3.5 (auto would be -P = -20): two updates against the loop given that entropy."""
    import torch
    D, P, B = 63, 20, 37
    case = sc.make_case(D, P, "33-17", 2, 2 * B, 0.0, 0.7, True, seed=6)
    case["target_entropy"] = -3.5
    batches = sc.loop_batches(case, 2, B)
    ref, ref32 = sc.torch_loop(case, batches, torch.float64), sc.torch_loop(case, batches, torch.float32)
    auto_ref = sc.torch_loop(dict(case, target_entropy=-float(P)), batches, torch.float64)
    d = _Dev(engines["pst"], case, rows=batches[0][0], target_entropy_auto=0, target_entropy=-3.5)
    try:
        for k in range(2):
            d.load(batches[k][0])
            losses = d.update()
            ent = d.eng.sac_get_ent_coef(d.s)
            tag = f"sac config edges target_entropy -3.5 step {k}"
            r, r32 = ref[k], ref32[k]
            assert abs(r["ent_coef_loss"] - auto_ref[k]["ent_coef_loss"]) > 1.0   # (the entropy in use is visible in the loss)
            sc.check_arrays(tag + " losses", [[x] for x in losses], [[r[n]] for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")],
                            [[r32[n]] for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")], values=True)
            sc.check_arrays(tag + " log_ent_coef", [ent[:1]], [[r["log_ent_coef"]]], [[r32["log_ent_coef"]]], values=True)
            sc.check_arrays(tag + " actor", _flat(*d.weights())[:8], r["actor"], r32["actor"], values=True)
    finally:
        d.close()


# ---- 6. ev2g_sac_collect ----
@pytest.mark.parametrize("kind,lo", [("pst", 0.0), ("ppl", -1.0)])
def test_collect_rows_equal_act_and_a_twin_engine(kind, lo):
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.td3 import init_critic_weights
    eng, twin = _gen_engine(kind), _gen_engine(kind)
    E, D, P, k = eng.E, eng.D, eng.P, 4
    assert E == E_GEN and E % 32 != 0
    actor, critics = init_sac_actor_weights(D, P, 2, 64, 64), [init_critic_weights(D, P, 5, 64, 64)]
    s = eng.sac_create(actor, critics, lo, seed=9, n_critics=1)
    bufs = [eng.empty((k + 1, E, D), np.float32), eng.empty((k, E, P), np.float32), eng.empty((k, E), np.float64), eng.empty((k, E), np.uint8),
            eng.empty((k, E, P), np.uint8)]
    try:
        eng.reset_f32(bufs[0], 0)
        eng.sac_act_seed(s, 41, 5)
        eng.sac_collect(s, k, *bufs)
        obs, act, rew, done, mask = [b.to_host() for b in bufs]
        assert eng.current_step == k and eng.sac_counters(s)[3] == 5 + k
        # action row t is ev2g_sac_act on observation row t at the draw base n E
        xb, ab = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
        for t in range(k):
            eng.sac_act_seed(s, 41, 5 + t)
            xb.upload(obs[t])
            eng.sac_act(s, xb, E, ab)
            assert np.array_equal(_bits(ab.to_host()), _bits(act[t])), t
        assert act.min() >= lo and act.max() <= 1.0 and np.unique(act).size > k * E * P // 2
        # the twin: the same scenarios stepped on the stored action rows through the registered float32 hand-over
        x_obs, x_act = twin.empty((E, D), np.float32), twin.empty((E, P), np.float32)
        t_rew, t_done, t_mask = twin.empty((E,)), twin.empty((E,), np.uint8), twin.empty((E, P), np.uint8)
        twin.reset_f32(x_obs, 0)
        assert np.array_equal(_bits(x_obs.to_host()), _bits(obs[0]))
        twin.set_extras(obs_f32=x_obs, actions_f32=x_act)
        for t in range(k):
            x_act.upload(act[t])
            twin.step_n(1, None, 0, None, 0, t_rew, 0, t_done, 0, t_mask, 0, auto_reset=False, persistent=False)
            twin.synchronize()
            assert np.array_equal(_bits(x_obs.to_host()), _bits(obs[t + 1])), t
            assert np.array_equal(_bits(t_rew.to_host()), _bits(rew[t])) and np.array_equal(t_done.to_host(), done[t]) and np.array_equal(t_mask.to_host(), mask[t]), t
        twin.set_extras()
        # the deterministic flag draws nothing: the counter does not move, and the actions are tanh(mu) unscaled
        eng.sac_collect(s, 2, *bufs, deterministic=True)
        assert eng.sac_counters(s)[3] == 5 + k and eng.current_step == k + 2
        obs2, act2 = bufs[0].to_host(), bufs[1].to_host()
        xb.upload(obs2[1])
        eng.sac_act(s, xb, E, ab, deterministic=True)
        assert np.array_equal(_bits(ab.to_host()), _bits(act2[1]))
    finally:
        eng.close()
        twin.close()


# ---- 7. end to end, lifetimes and refusals ----
def _collector(eng, cap=3, seed=0, net=(64, 64)):
    from ev2gym_amd.sac import SACCollector, init_sac_actor_weights
    return SACCollector(eng, init_sac_actor_weights(eng.D, eng.P, seed, *net), lo=0.0, capacity_episodes=cap, use_torch=False)


@pytest.mark.parametrize("ent_coef", ["auto", "auto_0.1", 0.2])
def test_learn_end_to_end(ent_coef):
    from ev2gym_amd.sac import SACLearner, make_learner
    eng = _gen_engine("pst")
    col = _collector(eng, seed=4)
    with pytest.raises(RuntimeError, match="no SACLearner is bound"):
        col.collect_episode()
    learner = make_learner("SAC", col, seed=3, batch_size=64, ent_coef=ent_coef)
    try:
        assert isinstance(learner, SACLearner)
        T, E, D, P, B = col.T, col.E, col.D, col.P, 64
        assert (T, E) == (T_SHORT, E_GEN) and learner.shape == (D, 64, 64, P, 2)
        a0 = {"auto": 1.0, "auto_0.1": 0.1, 0.2: 0.2}[ent_coef]
        assert abs(learner.ent_coef() - a0) < 1e-6 * a0
        out = learner.learn(2 * T * E, gradient_steps=3)
        assert len(out) == 2 and learner.num_timesteps == 2 * T * E and col.episodes == 2 and (col.head, col.filled) == (2, 2)
        assert learner.counters() == (6, 6, 6 * 2 * B * P, 2 * T) and learner.sample_counter == 6
        assert [o["n_updates"] for o in out] == [3, 6]
        assert all(np.isfinite(o[k]) for o in out for k in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef"))
        if isinstance(ent_coef, str):   # log_ent_coef is trained: it moved, and the reported mean is of the coefficients the updates used
            assert learner.ent_coef() != a0 and out[1]["ent_coef"] != out[0]["ent_coef"] and out[0]["ent_coef_loss"] != 0.0
        else:
            assert abs(learner.ent_coef() - a0) < 1e-6 * a0 and out[0]["ent_coef"] == out[1]["ent_coef"] and out[0]["ent_coef_loss"] == 0.0
        sd = learner.state_dict()
        assert len(sd) == 8 + 12 + 12 + 1
        assert sd["actor.latent_pi.0.weight"].shape == (64, D) and sd["actor.mu.weight"].shape == (P, 64) and sd["actor.log_std.bias"].shape == (P,)
        assert sd["critic.qf1.0.weight"].shape == (64, D + P) and sd["critic_target.qf0.4.weight"].shape == (1, 64) and sd["log_ent_coef"].shape == (1,)
        assert abs(float(np.exp(sd["log_ent_coef"][0])) - learner.ent_coef()) < 1e-6
        acts = col.actions[1].to_host()
        assert acts.min() >= 0.0 and acts.max() <= 1.0 and np.unique(acts).size > acts.size // 2   # the ring holds sampled env actions
        assert col.terminal_observation(1).shape == (E, D)
        assert col.collect_episode(deterministic=True) == 2 and learner.counters()[3] == 2 * T
    finally:
        if ent_coef == "auto":      # close() in any order frees everything once
            learner.close(); col.close(); eng.close(); learner.close()
        elif ent_coef == 0.2:
            col.close(); learner.close(); eng.close(); col.close()
        else:
            eng.close(); learner.close(); col.close()


def test_the_ring_wraps_and_the_sampler_reads_the_modular_block_list():
    from ev2gym_amd.sac import SACLearner
    eng = _gen_engine("pst", pool=4)
    col = _collector(eng, seed=4)
    learner = SACLearner(col, seed=3, batch_size=64)
    try:
        sc.check_ring_wrap(col, learner)
        out = learner.train(2)
        assert all(np.isfinite(out[k]) for k in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")) and out["n_updates"] == 2
        assert learner.counters() == (2, 2, 2 * 2 * 64 * col.P, 4 * col.T) and learner.sample_counter == 2 and col.episodes == 4
    finally:
        learner.close(); col.close(); eng.close()


def test_refusals_through_the_abi(engines):  # noqa: F811
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.td3 import init_critic_weights
    eng, other = engines["pst"], engines["ppl"]
    D, P = 63, 20
    case = sc.make_case(D, P, "64-64", 2, 8, -1.0, 0.7, True)
    d = _Dev(eng, case)

    def refused(code, word, fn, *a, **kw):
        with pytest.raises(EngineError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    bufs = None
    try:
        wide = init_sac_actor_weights(D, P, 0, 257, 64), [init_critic_weights(D, P, 1 + j, 257, 64) for j in range(2)]
        refused(_abi.ERR_ARG, "h1 257 is outside 1 .. 256", eng.sac_create, *wide, -1.0)
        refused(_abi.ERR_ARG, "tau must be in [0, 1]", eng.sac_create, case["actor"], case["critics"], -1.0, tau=1.5)
        refused(_abi.ERR_ARG, "ent_coef must be finite and > 0", eng.sac_create, case["actor"], case["critics"], -1.0, ent_coef=0.0)
        refused(_abi.ERR_ARG, "target_update_interval must be finite and >= 1", eng.sac_create, case["actor"], case["critics"], -1.0, target_update_interval=0)
        refused(_abi.ERR_ARG, "n_critics 3 is outside 1 .. 2", eng.sac_create, case["actor"], case["critics"] + case["critics"][:1], -1.0, n_critics=3)
        refused(_abi.ERR_ARG, "lo must be -1 or 0", eng.sac_create, case["actor"], case["critics"], 0.5)
        for B in (0, 1025):
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.sac_update, d.s, *d.bufs, B)
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.sac_actor_grad, d.s, d.bufs[0], B)
        refused(_abi.ERR_ARG, "not created on this handle", other.sac_update, d.s, *d.bufs, 8)
        refused(_abi.ERR_STATE, "no gradient to apply", eng.sac_apply, d.s)
        eng.sac_critic_grad(d.s, *d.bufs, 8)
        eng.sac_apply(d.s)
        assert eng.sac_counters(d.s)[:3] == (0, 0, 0)   # a critics-only apply is no update: nothing counted, no draws consumed
        refused(_abi.ERR_STATE, "no gradient to apply", eng.sac_apply, d.s)
        for lr in (float("nan"), -1.0, float("inf")):
            refused(_abi.ERR_ARG, "lr must be finite and >= 0", eng.sac_set_rate, d.s, lr)
        eng.sac_set_rate(d.s, 0.0)   # a zero rate is a rate: the masters and log_ent_coef stay
        before, ent = _flat(*d.weights()), eng.sac_get_ent_coef(d.s)
        d.update()
        for a, b in zip(before, _flat(*d.weights())):
            assert np.array_equal(_bits(a), _bits(b))
        assert eng.sac_get_ent_coef(d.s)[0] == ent[0]
        refused(_abi.ERR_ARG, "null argument", eng.sac_update, d.s, None, *d.bufs[1:], 8)
        refused(_abi.ERR_ARG, "not the batch size", eng.sac_get_y, d.s, 9)
        refused(_abi.ERR_ARG, "not the batch size", eng.sac_get_log_pi, d.s, 9)
        refused(_abi.ERR_ARG, "n_rows is not positive", eng.sac_act, d.s, d.bufs[0], 0, d.bufs[1])
        refused(_abi.ERR_ARG, "null", eng.sac_act, d.s, None, 8, d.bufs[1])
        # collect: the learner's shape is not the other engine's; a segment past the episode end; null rows
        E, k = eng.E, 2
        bufs = [eng.empty((k + 1, E, D), np.float32), eng.empty((k, E, P), np.float32), eng.empty((k, E), np.float64), eng.empty((k, E), np.uint8),
                eng.empty((k, E, P), np.uint8)]
        s2 = other.sac_create(case["actor"], case["critics"], -1.0)
        refused(_abi.ERR_ARG, "actor shape != (obs dim, ports)", other.sac_collect, s2, 1, *bufs)
        other.sac_destroy(s2)
        refused(_abi.ERR_ARG, "not created on this handle", other.sac_collect, d.s, 1, *bufs)
        refused(_abi.ERR_ARG, "null argument", eng.sac_collect, d.s, k, bufs[0], None, *bufs[2:])
        eng.reset_f32(bufs[0], 0)
        refused(_abi.ERR_DONE, "past the episode end", eng.sac_collect, d.s, eng.T + 1, *bufs)
        eng.sac_destroy(d.s)
        refused(_abi.ERR_ARG, "not created on this handle", eng.sac_apply, d.s)
    finally:
        for b in (bufs or []):
            b.free()
        d.close()
