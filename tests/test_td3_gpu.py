"""The TD3 / DDPG learner on the device (csrc/ev2g_td3.h, ev2gym_amd/td3.py) and the replay ring's sampler.

Tolerance idiom (tests/test_ppo_gpu.py): the reference is float64 (torch autograd / torch.optim.Adam in float64, which tests/test_td3_cpu.py
ties to td3_update_numpy at 1e-10); d32 is the largest deviation of the same computation in torch-CPU float32; the device gets 4 d32 + 4 * 2^-23 * s,
s = max(1, |y|) for values and the array's largest reference magnitude for gradients.  Every d32 and device deviation is printed before it is
asserted and appended to the file EV2G_PPO_RECORD names.  Everything else is bit for bit.

ReLU's derivative is discontinuous, so the case builder (tests/td3_cases.py) redraws any row whose smallest float64 |pre-activation| over the
backpropagated ReLU layers is below 1e-5, and asserts that fewer than a quarter of the rows needed it.

Off the handles' shapes (tests/td3_cases.EDGE_NETS): the plan's limits, one exact 16-wide tile, every dimension ragged by one, layers narrower
than a tile, at batches up to the workspace's 1024 rows; a saturated actor; the config's edges; the ring once it has wrapped, a sampler wider
than its 64 threads and its full 32-entry table.  tests/test_td3_cpu.py proves those cases' conditions without a GPU."""
import numpy as np
import pytest

from tests import td3_cases as tc
from tests.learner_cases import SHAPES, engines  # noqa: F401  (the fixture)
from tests.test_onpolicy_gpu import _bits, _gen_engine, _up

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 32, 33, 100, 256, 257)


def _grad_cases():
    """Every B with every network (n_critics, lo, noise and the handle cycling so that each value meets each network and several B), then the
    full cross of (n_critics, lo, noise) at 400-300, B 33."""
    out, k = [], 0
    for B in BATCHES:
        for net in tc.NETS:
            out.append((net, 1 + k % 2, (-1.0, 0.0)[(k // 2) % 2], (0.2, 0.0)[(k // 3) % 2], B, ("pst", "ppl")[(k // 5) % 2]))
            k += 1
    for nc in (1, 2):
        for lo in (-1.0, 0.0):
            for sigma in (0.2, 0.0):
                out.append(("400-300", nc, lo, sigma, 33, "ppl" if nc == 2 else "pst"))
    return out


class _Dev:
    """A case's rows on an engine, a policy object and a learner bound to it."""

    def __init__(self, eng, case, precision="fp32", rows=None, **cfg):
        self.eng, self.case = eng, case
        self.shape = (case["D"], case["h"][0], case["h"][1], case["P"], case["n_critics"])
        self.mlp = eng.mlp_create(*case["actor"], out_lo=case["lo"], precision=precision)
        self.t = eng.td3_create(self.mlp, case["actor"], case["critics"], seed=case["noise_seed"], n_critics=case["n_critics"],
                                target_policy_noise=case["sigma"], target_noise_clip=case["clip"], gamma=case["gamma"], **cfg)
        eng.td3_seed(self.t, case["noise_seed"], case["first_draw"])
        self.losses = eng.empty((2,), np.float32)
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
        return flat[:6], [flat[6 + 6 * j:12 + 6 * j] for j in range(self.shape[4])]

    def grads(self):
        return self.split(self.eng.td3_get_grads(self.t, self.shape))

    def weights(self, target=False):
        return self.split(self.eng.td3_get_weights(self.t, self.shape, target))

    def update(self):
        self.eng.td3_update(self.t, *self.bufs, self.B, self.losses)
        return self.losses.to_host()

    def forward(self, x, mlp=None, eng=None):
        eng = eng or self.eng
        xb, yb = _up(eng, np.ascontiguousarray(x, np.float32)), eng.empty((len(x), self.case["P"]), np.float32)
        eng.mlp_forward(mlp or self.mlp, xb, yb, len(x))
        y = yb.to_host()
        xb.free(); yb.free()
        return y

    def close(self):
        self.eng.mlp_destroy(self.mlp)   # (the learner goes with its policy)
        for b in self.bufs + [self.losses]:
            b.free()


def _flat(actor, critics):
    return list(actor) + [a for c in critics for a in c]


def _dp(net):
    """(D, P) of a case: a row of tc.EDGE_NETS brings its own, the others run at the "pst" handle's"""
    return tc.EDGE_NETS[net][0::3] if net in tc.EDGE_NETS else SHAPES["pst"]


# ---- 1. one staged step against the float64 reference ----
def _staged_step(eng, case, ref, ref32, tag):
    """The critics' stage, then the actor's, on `case`: y, both losses and every gradient under the idiom.  Returns the actor's gradient."""
    n_critics, sigma, B, P = case["n_critics"], case["sigma"], case["B"], case["P"]
    d = _Dev(eng, case)
    try:
        d.eng.td3_critic_grad(d.t, *d.bufs, B, d.losses)
        y = d.eng.td3_get_y(d.t, B)
        _, cg = d.grads()
        closs = d.losses.to_host()[0]
        assert d.eng.td3_counters(d.t) == (0, 0, 1000 + (B * P if sigma > 0.0 else 0))
        d.eng.td3_actor_grad(d.t, d.bufs[0], B, d.losses)
        ag, cg_after = d.grads()
        aloss = d.losses.to_host()[1]
        for a, b in zip(_flat([], cg), _flat([], cg_after)):   # the actor's stage leaves the critics' gradient alone
            assert np.array_equal(_bits(a), _bits(b))
        tc.check_arrays(tag + " y", [y], [ref["y"]], [ref32["y"]], values=True)
        tc.check_arrays(tag + " losses", [[closs], [aloss]], [[ref["critic_loss"]], [ref["actor_loss"]]], [[ref32["critic_loss"]], [ref32["actor_loss"]]], values=True)
        for j in range(n_critics):
            tc.check_arrays(tag + f" critic {j} grad", cg[j], ref["critic_grads"][j], ref32["critic_grads"][j])
        tc.check_arrays(tag + " actor grad", ag, ref["actor_grads"], ref32["actor_grads"])
        return ag
    finally:
        d.close()


@pytest.mark.parametrize("net,n_critics,lo,sigma,B,handle", _grad_cases())
def test_gradients_y_and_losses_against_float64(engines, net, n_critics, lo, sigma, B, handle):  # noqa: F811
    import torch
    D, P = SHAPES[handle]
    case = tc.make_case(D, P, net, n_critics, B, lo, sigma, seed=7 + B, first_draw=1000)
    ref, ref32 = tc.torch_grads(case, torch.float64), tc.torch_grads(case, torch.float32)
    tag = f"td3 {net} nc{n_critics} lo{lo:g} sigma{sigma:g} B{B} {handle} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']})"
    _staged_step(engines[handle], case, ref, ref32, tag)


# The plan's limits and the product kernel's tile edges (tests/td3_cases.EDGE_NETS; tests/test_td3_cpu.py pins the cases' conditions).  A learner
# binds to an eng.mlp_create policy of any shape, so the handle's own (D, P) does not matter.
@pytest.mark.parametrize("tag,n_critics,lo,sigma,B", tc.EDGE_GRAD_CASES)
def test_gradients_at_the_plans_limits_and_tile_edges(engines, tag, n_critics, lo, sigma, B):  # noqa: F811
    import torch
    case = tc.edge_grad_case(tag, n_critics, lo, sigma, B)
    name = f"td3 edge {tag} nc{n_critics} lo{lo:g} sigma{sigma:g} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']})"
    _staged_step(engines["pst"], case, case["ref64"], tc.torch_grads(case, torch.float32), name)


# A saturated actor: every second port's pre-tanh is beyond +-10 for every row (asserted by the builder in float64), where float32 tanh is exactly
# +-1 in torch and on the device alike.  The target's clamp a' in [-1, 1] acts on a quarter of the elements, and tanh_back's 1 - t^2 is exactly 0
# on the saturated ports: their rows of the actor's W3 gradient and their b3 entries are 0.0, not small.
@pytest.mark.parametrize("net,dp,n_critics,lo,sigma,B", tc.SATURATED_GRAD_CASES)
def test_gradients_with_a_saturated_actor(engines, net, dp, n_critics, lo, sigma, B):  # noqa: F811
    import torch
    case = tc.saturated_grad_case(net, dp, n_critics, lo, sigma, B)
    name = (f"td3 saturated {net} nc{n_critics} lo{lo:g} sigma{sigma:g} B{B} (redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}, "
            f"a' at +-1 {case['share_at_1']:.4f})")
    ag = _staged_step(engines["pst"], case, case["ref64"], tc.torch_grads(case, torch.float32), name)
    ports, _ = tc.saturated_ports(dp[1])
    live = np.setdiff1d(np.arange(dp[1]), ports)
    assert np.array_equal(ag[4][ports], np.zeros_like(ag[4][ports])) and np.array_equal(ag[5][ports], np.zeros(ports.size, np.float32))
    assert np.abs(ag[4][live]).max(axis=1).min() > 0.0 and np.abs(ag[5][live]).min() > 0.0


# ---- 2. the same update twice gives the same bits ----
# Gradients, masters and targets are read back and compared themselves.  The policy's packed images cannot be read through the ABI: they are
# compared through a PROXY, ev2g_mlp_forward of 33 rows on the refreshed bf16 policy.  The images' contents are held to pack_mlp bit for bit by
# tests/host/td3_check.cpp (every packing) and to a fresh policy object by test 4 below.
@pytest.mark.parametrize("net,B", [("400-300", 100), ("33-17", 257), ("limits", 1024)])
def test_an_update_is_reproducible_bit_for_bit(engines, net, B):  # noqa: F811
    D, P = _dp(net)
    case = tc.make_case(D, P, net, 2, B, 0.0, 0.2, seed=21)
    got = []
    for _ in range(2):
        d = _Dev(engines["pst"], case, precision="bf16", policy_delay=1)
        try:
            losses = d.update()
            got.append([losses] + _flat(*d.grads()) + _flat(*d.weights()) + _flat(*d.weights(True)) + [d.forward(case["obs"][:33])])
        finally:
            d.close()
    assert len(got[0]) == len(got[1]) == 2 + 3 * 18
    assert np.isfinite(got[0][0]).all()
    for a, b in zip(*got):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 3. three updates with policy_delay 2: Adam and Polyak bit for bit by the host twins, the loop under the idiom ----
@pytest.mark.parametrize("net,n_critics,B", [("64-64", 2, 33), ("400-300", 2, 100), ("33-17", 1, 31), ("tiny", 2, 33)])
def test_three_updates_adam_polyak_and_order(engines, net, n_critics, B):  # noqa: F811
    import torch
    from ev2gym_amd.engine import host_adam, host_normal, host_polyak
    D, P = _dp(net)
    case = tc.make_case(D, P, net, n_critics, 3 * B, -1.0, 0.2, seed=5, live=net in tc.EDGE_NETS)   # (tiny: no dead ReLU, tests/test_td3_cpu.py)
    batches = [(np.arange(k * B, (k + 1) * B), host_normal(B * P, case["noise_seed"], k * B * P).reshape(B, P)) for k in range(3)]
    ref, ref32 = tc.torch_loop(case, batches, torch.float64), tc.torch_loop(case, batches, torch.float32)
    d = _Dev(engines["pst"], case, rows=batches[0][0], policy_delay=2)
    try:
        masters, targets = _flat(*d.weights()), _flat(*d.weights(True))
        for a, b in zip(masters, targets):
            assert np.array_equal(_bits(a), _bits(b))
        m, v = [np.zeros_like(a) for a in masters], [np.zeros_like(a) for a in masters]
        x_probe = case["obs"][:8]
        y_probe = d.forward(x_probe)
        for k in range(3):
            d.load(batches[k][0])
            losses = d.update()
            grads, new, new_t = _flat(*d.grads()), _flat(*d.weights()), _flat(*d.weights(True))
            want = [a.copy() for a in masters]
            for i in range(6, len(want)):   # the critics step on every update, their Adam count is the update's
                host_adam(want[i], m[i], v[i], grads[i], k + 1, lr=1e-3, eps=1e-8)
            if k == 1:                      # the actor steps on the second update only: its Adam count is 1
                for i in range(6):
                    host_adam(want[i], m[i], v[i], grads[i], 1, lr=1e-3, eps=1e-8)
            for i, (a, b) in enumerate(zip(new, want)):
                assert np.array_equal(_bits(a), _bits(b)), (k, i)
            if k == 1:
                for i, (t_new, t_old, p) in enumerate(zip(new_t, targets, new)):
                    moved = t_old.copy()
                    host_polyak(moved, p, 0.005)
                    assert np.array_equal(_bits(t_new), _bits(moved)), i
                    assert not np.array_equal(t_new, t_old)
                y_new = d.forward(x_probe)
                assert not np.array_equal(y_new, y_probe)   # the bound policy reads the new actor
                y_probe = y_new
            else:                           # updates 1 and 3: the actor, every target and the policy's images are untouched
                for i in range(6):
                    assert np.array_equal(_bits(new[i]), _bits(masters[i])), (k, i)
                for a, b in zip(new_t, targets):
                    assert np.array_equal(_bits(a), _bits(b))
                assert np.array_equal(_bits(d.forward(x_probe)), _bits(y_probe))
            assert d.eng.td3_counters(d.t) == (k + 1, 1 if k >= 1 else 0, (k + 1) * B * P)
            tag = f"td3 loop {net} nc{n_critics} B{B} step {k}"
            tc.check_arrays(tag + " critic_loss", [[losses[0]]], [[ref[k]["critic_loss"]]], [[ref32[k]["critic_loss"]]], values=True)
            if k == 1:
                tc.check_arrays(tag + " actor_loss", [[losses[1]]], [[ref[k]["actor_loss"]]], [[ref32[k]["actor_loss"]]], values=True)
                tc.check_arrays(tag + " actor", new[:6], ref[k]["actor"], ref32[k]["actor"], values=True)
            for j in range(n_critics):
                tc.check_arrays(tag + f" critic {j}", new[6 + 6 * j:12 + 6 * j], ref[k]["critics"][j], ref32[k]["critics"][j], values=True)
            masters, targets = new, new_t
    finally:
        d.close()


# ---- 4. the refreshed actor ----
@pytest.mark.parametrize("net", ["400-300", "64-64"])
@pytest.mark.parametrize("precision", ["bf16", "fp32", "fp32x3"])
def test_the_bound_policy_equals_a_fresh_one_from_the_masters(engines, precision, net):  # noqa: F811
    eng = engines["pst"]
    D, P = SHAPES["pst"]
    case = tc.make_case(D, P, net, 2, 64, 0.0, 0.2, seed=9)
    d = _Dev(eng, case, precision=precision, policy_delay=1, lr=1e-2)
    twin = fresh = fresh_twin = None
    try:
        kind = eng.mlp_kernel_name(d.mlp)
        assert ("s16" in kind) == (net == "400-300"), kind   # the streaming packing and a generic one
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:40]])
        y0 = d.forward(x)
        d.update(); d.update()
        assert d.eng.td3_counters(d.t)[:2] == (2, 2)
        actor, _ = d.weights()
        assert all(not np.array_equal(a, b) for a, b in zip(actor, case["actor"]))
        fresh = eng.mlp_create(*actor, out_lo=case["lo"], precision=precision)
        y1, y2 = d.forward(x), d.forward(x, fresh)
        assert np.array_equal(_bits(y1), _bits(y2))
        assert not np.array_equal(y1, y0)
        # three collected steps through both, on twin engines (the streaming and the generic policy alike)
        twin = _gen_engine("pst")
        fresh_twin = twin.mlp_create(*actor, out_lo=case["lo"], precision=precision)
        rows = []
        for e, m in ((eng, d.mlp), (twin, fresh_twin)):
            bufs = [e.empty((4, e.E, D), np.float32), e.empty((3, e.E, P), np.float32), e.empty((3, e.E), np.float64), e.empty((3, e.E), np.uint8),
                    e.empty((3, e.E, P), np.uint8)]
            e.reset_f32(bufs[0], 0)
            e.collect(m, 3, *bufs)
            rows.append([b.to_host() for b in bufs])
            for b in bufs:
                b.free()
        for a, b in zip(*rows):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.abs(rows[0][1]).max() > 0.0
    finally:
        if fresh is not None:
            eng.mlp_destroy(fresh)
        if twin is not None:
            twin.mlp_destroy(fresh_twin)
            twin.close()
        d.close()


# The refreshed actor off the handles' shapes: the plan's limits on the generic bf16 kernel and on the float32 one, and a shape the plan gives a
# fixed-width kernel.  The forward comparison only: the collect half's shapes are the engine's.
@pytest.mark.parametrize("tag,shape,precision,kernel", tc.REFRESH_EDGE_CASES)
def test_the_bound_policy_off_the_handles_shapes_equals_a_fresh_one(engines, tag, shape, precision, kernel):  # noqa: F811
    from ev2gym_amd import _abi
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.td3 import init_critic_weights
    eng = engines["pst"]
    D, h1, h2, P = shape
    if tag == "fixed":   # 170-410-300-50 has the same tile counts, and the learner's plan refuses it on the host, ahead of any launch
        wide = eng.mlp_create(*init_mlp_weights(170, 50, 0, 410, 300), out_lo=0.0, precision="bf16")
        try:
            assert eng.mlp_kernel_name(wide) == kernel
            with pytest.raises(EngineError) as ei:
                eng.td3_create(wide, init_mlp_weights(170, 50, 0, 410, 300), [init_critic_weights(170, 50, 1 + j, 410, 300) for j in range(2)])
            assert ei.value.code == _abi.ERR_ARG and "h1 410 is outside 1 .. 400" in str(ei.value)
        finally:
            eng.mlp_destroy(wide)
    case = tc.make_case(D, P, (h1, h2), 2, 64, 0.0, 0.2, seed=9, live=True)
    d = _Dev(eng, case, precision=precision, policy_delay=1, lr=1e-2)
    fresh = None
    try:
        assert eng.mlp_kernel_name(d.mlp) == kernel
        x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:40]])
        y0 = d.forward(x)
        d.update(); d.update()
        assert d.eng.td3_counters(d.t)[:2] == (2, 2)
        actor, _ = d.weights()
        assert all(not np.array_equal(a, b) for a, b in zip(actor, case["actor"]))
        fresh = eng.mlp_create(*actor, out_lo=case["lo"], precision=precision)
        assert eng.mlp_kernel_name(fresh) == kernel
        y1, y2 = d.forward(x), d.forward(x, fresh)
        assert np.array_equal(_bits(y1), _bits(y2))
        assert not np.array_equal(y1, y0) and np.isfinite(y1).all() and y1.min() >= 0.0 and y1.max() <= 1.0
    finally:
        if fresh is not None:
            eng.mlp_destroy(fresh)
        d.close()


# ---- 4b. config edges the checks accept: policy_delay 3, tau in {0, 1}, gamma in {0, 1}, target_noise_clip 0 with sigma > 0 ----
def test_config_edges_delay_3_tau_1_gamma_0_clip_0(engines):  # noqa: F811
    """Three updates on 33-17.  The actor and the targets move on update 3 only, and the targets then EQUAL the masters bit for bit
    (target * 0 + 1 * param with finite weights); y is the reward bit for bit (gamma 0; no reward is -0.0); a clip of 0 silences the noise but its
    draws are still consumed, B P per update; Adam is bit for bit by host_adam, the loop under the idiom."""
    import torch
    from ev2gym_amd.engine import host_adam, host_normal
    D, P = SHAPES["pst"]
    B = 33
    case = tc.make_case(D, P, "33-17", 2, 3 * B, -1.0, 0.2, seed=5)
    case["clip"], case["gamma"] = 0.0, 0.0
    batches = [(np.arange(k * B, (k + 1) * B), host_normal(B * P, case["noise_seed"], k * B * P).reshape(B, P)) for k in range(3)]
    kw = dict(policy_delay=3, tau=1.0)
    ref, ref32 = tc.torch_loop(case, batches, torch.float64, **kw), tc.torch_loop(case, batches, torch.float32, **kw)
    d = _Dev(engines["pst"], case, rows=batches[0][0], **kw)
    try:
        masters, targets = _flat(*d.weights()), _flat(*d.weights(True))
        m, v = [np.zeros_like(a) for a in masters], [np.zeros_like(a) for a in masters]
        for k in range(3):
            d.load(batches[k][0])
            losses = d.update()
            y = d.eng.td3_get_y(d.t, B)
            r = case["reward"][batches[k][0]]
            assert not np.signbit(r[r == 0.0]).any() and np.array_equal(_bits(y), _bits(r)), k
            grads, new, new_t = _flat(*d.grads()), _flat(*d.weights()), _flat(*d.weights(True))
            want = [a.copy() for a in masters]
            for i in range(6, len(want)):
                host_adam(want[i], m[i], v[i], grads[i], k + 1, lr=1e-3, eps=1e-8)
            if k == 2:
                for i in range(6):
                    host_adam(want[i], m[i], v[i], grads[i], 1, lr=1e-3, eps=1e-8)
            for i, (a, b) in enumerate(zip(new, want)):
                assert np.array_equal(_bits(a), _bits(b)), (k, i)
            if k == 2:
                for i, (t_new, t_old, p_new) in enumerate(zip(new_t, targets, new)):
                    assert np.array_equal(_bits(t_new), _bits(p_new)) and not np.array_equal(t_new, t_old), i
                assert all(not np.array_equal(new[i], masters[i]) for i in range(6))
            else:
                for i in range(6):
                    assert np.array_equal(_bits(new[i]), _bits(masters[i])), (k, i)
                for a, b in zip(new_t, targets):
                    assert np.array_equal(_bits(a), _bits(b))
            assert d.eng.td3_counters(d.t) == (k + 1, 1 if k == 2 else 0, (k + 1) * B * P)
            tag = f"td3 config edges delay3 tau1 gamma0 clip0 step {k}"
            tc.check_arrays(tag + " critic_loss", [[losses[0]]], [[ref[k]["critic_loss"]]], [[ref32[k]["critic_loss"]]], values=True)
            if k == 2:
                tc.check_arrays(tag + " actor_loss", [[losses[1]]], [[ref[k]["actor_loss"]]], [[ref32[k]["actor_loss"]]], values=True)
                tc.check_arrays(tag + " actor", new[:6], ref[k]["actor"], ref32[k]["actor"], values=True)
            for j in range(2):
                tc.check_arrays(tag + f" critic {j}", new[6 + 6 * j:12 + 6 * j], ref[k]["critics"][j], ref32[k]["critics"][j], values=True)
            masters, targets = new, new_t
    finally:
        d.close()


@pytest.mark.parametrize("edge", ["tau0", "gamma1"])
def test_config_edges_tau_0_and_gamma_1(engines, edge):  # noqa: F811
    """Two updates with policy_delay 1.  tau 0: the actor and the critics step, the targets never move.  gamma 1: the loop under the idiom."""
    import torch
    from ev2gym_amd.engine import host_normal
    D, P = SHAPES["pst"]
    B = 33
    case = tc.make_case(D, P, "33-17", 2, 2 * B, 0.0, 0.2, seed=6)
    tau = 0.0 if edge == "tau0" else 0.005
    case["gamma"] = 1.0 if edge == "gamma1" else 0.99
    batches = [(np.arange(k * B, (k + 1) * B), host_normal(B * P, case["noise_seed"], k * B * P).reshape(B, P)) for k in range(2)]
    kw = dict(policy_delay=1, tau=tau)
    ref, ref32 = tc.torch_loop(case, batches, torch.float64, **kw), tc.torch_loop(case, batches, torch.float32, **kw)
    d = _Dev(engines["pst"], case, rows=batches[0][0], **kw)
    try:
        masters, targets = _flat(*d.weights()), _flat(*d.weights(True))
        for k in range(2):
            d.load(batches[k][0])
            losses = d.update()
            new, new_t = _flat(*d.weights()), _flat(*d.weights(True))
            assert all(not np.array_equal(a, b) for a, b in zip(new, masters)), k
            if edge == "tau0":
                for a, b in zip(new_t, targets):
                    assert np.array_equal(_bits(a), _bits(b))
            else:
                assert all(not np.array_equal(a, b) for a, b in zip(new_t, targets))
            assert d.eng.td3_counters(d.t) == (k + 1, k + 1, (k + 1) * B * P)
            tag = f"td3 config edges {edge} step {k}"
            tc.check_arrays(tag + " losses", [[losses[0]], [losses[1]]], [[ref[k]["critic_loss"]], [ref[k]["actor_loss"]]],
                            [[ref32[k]["critic_loss"]], [ref32[k]["actor_loss"]]], values=True)
            tc.check_arrays(tag + " actor", new[:6], ref[k]["actor"], ref32[k]["actor"], values=True)
            for j in range(2):
                tc.check_arrays(tag + f" critic {j}", new[6 + 6 * j:12 + 6 * j], ref[k]["critics"][j], ref32[k]["critics"][j], values=True)
                tc.check_arrays(tag + f" critic_target {j}", new_t[6 + 6 * j:12 + 6 * j], ref[k]["critics_target"][j], ref32[k]["critics_target"][j], values=True)
            tc.check_arrays(tag + " actor_target", new_t[:6], ref[k]["actor_target"], ref32[k]["actor_target"], values=True)
            masters, targets = new, new_t
    finally:
        d.close()


# ---- 5. the sampler ----
def _collector(eng, cap=3, seed=0):
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.sb3_vec_env import DeviceReplayCollector
    return DeviceReplayCollector(eng, init_mlp_weights(eng.D, eng.P, seed), lo=0.0, capacity_episodes=cap, use_torch=False)


def _gather(blocks, idx, T):
    """The rows of host copies of the complete blocks at idx [B, 3] (entry of the list, t, e)."""
    bi, t, e = idx[:, 0], idx[:, 1], idx[:, 2]
    pick = lambda k, tt: np.stack([blocks[b][k][x, y] for b, x, y in zip(bi, tt, e)])  # noqa: E731
    return pick(0, t), pick(1, t), pick(2, t).astype(np.float32), pick(0, t + 1), pick(3, t)


def test_replay_sample_matches_the_host_twin():
    from ev2gym_amd.engine import EngineError, host_replay_indices
    eng = _gen_engine("pst")
    col = _collector(eng)
    try:
        assert col.cap == 3
        col.collect_episode(); col.collect_episode()
        assert (col.head, col.filled) == (2, 2)
        complete = [1, 0]   # newest first; block 2 holds only the next reset observation
        T, E, D, P, B = col.T, col.E, col.D, col.P, 256
        ring = [(col.obs[b], col.actions[b], col.reward[b], col.done[b]) for b in complete]
        host = [[a.to_host() for a in r] for r in ring]
        out = [eng.empty((B, D), np.float32), eng.empty((B, P), np.float32), eng.empty((B,), np.float32), eng.empty((B, D), np.float32), eng.empty((B,), np.uint8)]
        index = eng.empty((B, 3), np.int32)
        seen = []
        for counter in (0, 1):
            eng.replay_sample(ring, T, E, D, P, B, 77, counter, *out, index)
            idx = index.to_host()
            assert np.array_equal(idx, host_replay_indices(B, 2, T, E, 77, counter))
            assert set(idx[:, 0]) == {0, 1} and idx[:, 1].max() == T - 1 and idx[:, 1].min() == 0
            want = _gather(host, idx, T)
            for a, b in zip([o.to_host() for o in out], want):
                assert np.array_equal(_bits(a), _bits(b))
            last = idx[:, 1] == T - 1   # s' of a block's last step is its terminal observation, row T
            assert last.any()
            nxt = out[3].to_host()
            for r in np.nonzero(last)[0]:
                assert np.array_equal(nxt[r], host[idx[r, 0]][0][T, idx[r, 2]])
            assert out[4].to_host()[last].all()   # (an episode's last step is done)
            seen.append(idx)
        assert not np.array_equal(seen[0], seen[1])
        eng.replay_sample(ring[:1], T, E, D, P, 5, 77, 0, *out, index)   # one complete block: only that one is drawn
        assert not index.to_host()[:5, 0].any()
        for bad in (0, 1025):
            with pytest.raises(EngineError) as ei:
                eng.replay_sample(ring, T, E, D, P, bad, 77, 0, *out, index)
            assert ei.value.code == -1 and "outside 1 .. 1024" in str(ei.value)
        for b in out + [index]:
            b.free()
    finally:
        col.close()
        eng.close()


def test_the_ring_wraps_and_the_sampler_reads_the_modular_block_list():
    from ev2gym_amd.td3 import TD3Learner
    eng = _gen_engine("pst", pool=4)   # four pool windows: four different episodes under one deterministic policy
    col = _collector(eng, seed=4)
    learner = TD3Learner(col, seed=3, batch_size=64)
    try:
        tc.check_ring_wrap(col, learner)
        out = learner.train(2)
        assert np.isfinite(out["critic_loss"]) and np.isfinite(out["actor_loss"]) and out["n_updates"] == 2
        assert learner.counters() == (2, 1, 2 * 64 * col.P) and learner.sample_counter == 2 and col.episodes == 4
    finally:
        learner.close(); col.close(); eng.close()


def test_a_wide_sampler_and_a_full_table():
    """D > 64: the 64-thread copy loops take a second trip.  A 32-entry list (two real blocks repeated) fills the sampler's table; 33 entries are
    refused on the host, and so is a learner on a ring that could hold 33 complete episodes."""
    from ev2gym_amd.engine import EngineError, host_replay_indices
    from ev2gym_amd.td3 import MAX_BLOCKS, TD3Learner
    eng = _gen_engine("ppl", pool=2)   # (two pool windows: two different episodes)
    col = _collector(eng)
    big, out = None, []
    try:
        assert col.D > 64 and col.P <= 64 and MAX_BLOCKS == 32
        snaps = [tc.snapshot(col, col.collect_episode()) for _ in range(2)]
        assert (col.head, col.filled) == (2, 2)
        assert not np.array_equal(snaps[0][0][1:], snaps[1][0][1:])   # two different episodes, by their observations
        dev = [(col.obs[b], col.actions[b], col.reward[b], col.done[b]) for b in (1, 0)]
        tc.check_sample(col, dev, [snaps[1], snaps[0]], 256, 77, (0, 1))
        table = [dev[i % 2] for i in range(32)]
        assert 31 in host_replay_indices(1024, 32, col.T, col.E, 77, 0)[:, 0]   # the last entry of the table is drawn at this seed
        idx = tc.check_sample(col, table, [snaps[1 - i % 2] for i in range(32)], 1024, 77, (0,))[0]
        assert 31 in idx[:, 0] and np.unique(idx[:, 0]).size == 32
        out = [eng.empty((8, col.D), np.float32), eng.empty((8, col.P), np.float32), eng.empty((8,), np.float32), eng.empty((8, col.D), np.float32), eng.empty((8,), np.uint8)]
        with pytest.raises(EngineError) as ei:
            eng.replay_sample(table + dev[:1], col.T, col.E, col.D, col.P, 8, 77, 0, *out)
        assert ei.value.code == -1 and "n_blocks must be 1 .. 32" in str(ei.value)
        big = _collector(eng, cap=34)
        with pytest.raises(ValueError, match="capacity_episodes must be at most 33"):
            TD3Learner(big)
    finally:
        for b in out:
            b.free()
        if big is not None:
            big.close()
        col.close()
        eng.close()


# ---- 6. end to end ----
@pytest.mark.parametrize("algo", ["td3", "ddpg"])
def test_learn_end_to_end(algo):
    import torch
    from ev2gym_amd.engine import host_normal, host_replay_indices
    from ev2gym_amd.td3 import DDPGLearner, TD3Learner, td3_state, td3_update_numpy
    eng = _gen_engine("pst")
    col = _collector(eng, seed=4)
    cls = TD3Learner if algo == "td3" else DDPGLearner
    learner = cls(col, seed=3, batch_size=64)
    try:
        T, E, D, P, B = col.T, col.E, col.D, col.P, 64
        nc, delay, sigma = (2, 2, 0.2) if algo == "td3" else (1, 1, 0.0)
        assert learner.shape == (D, 400, 300, P, nc)
        actor0, critics0 = learner.get_weights()
        out = learner.learn(2 * T * E, gradient_steps=3)
        assert len(out) == 2 and learner.num_timesteps == 2 * T * E and col.episodes == 2
        updates, actor_steps, next_draw = learner.counters()
        assert (updates, actor_steps) == (6, 6 // delay) and learner.sample_counter == 6
        assert next_draw == (6 * B * P if sigma > 0.0 else 0)
        assert [o["n_updates"] for o in out] == [3, 6]
        assert all(np.isfinite(o["critic_loss"]) and np.isfinite(o["actor_loss"]) for o in out)
        # the batches train() consumed, from the host twin's indices over host copies of the blocks
        host = {b: [a.to_host() for a in (col.obs[b], col.actions[b], col.reward[b], col.done[b])] for b in (0, 1)}
        lists = [[0]] * 3 + [[1, 0]] * 3
        rows = [_gather([host[b] for b in lst], host_replay_indices(B, len(lst), T, E, 3, k), T) for k, lst in enumerate(lists)]
        case = dict(lo=0.0, sigma=sigma, clip=0.5, gamma=0.99, n_critics=nc, actor=actor0, critics=critics0, P=P,
                    **{name: np.concatenate([r[i] for r in rows]) for i, name in enumerate(("obs", "actions", "reward", "next_obs", "done"))})
        batches = [(np.arange(k * B, (k + 1) * B), host_normal(B * P, 3, k * B * P).reshape(B, P) if sigma > 0.0 else None) for k in range(6)]
        st = td3_state(actor0, critics0)
        for rws, normals in batches:
            td3_update_numpy(st, case["obs"][rws], case["actions"][rws], case["reward"][rws], case["next_obs"][rws], case["done"][rws], normals, 0.0,
                             policy_delay=delay, target_policy_noise=sigma)
        ref32 = tc.torch_loop(case, batches, torch.float32, policy_delay=delay)[-1]
        actor, critics = learner.get_weights()
        for j in range(nc):
            tc.check_arrays(f"{algo} learn() critic {j}", critics[j], st.critics[j], ref32["critics"][j], values=True)
        tc.check_arrays(f"{algo} learn() actor", actor, st.actor, ref32["actor"], values=True)
        sd = learner.state_dict()
        assert len(sd) == 2 * (6 + 6 * nc) and "actor.mu.0.weight" in sd and f"critic_target.qf{nc - 1}.4.bias" in sd and sd["critic.qf0.4.weight"].shape == (1, 300)
        assert np.array_equal(sd["actor.mu.4.bias"], actor[5])
        # the collector's policy is the learner's actor: a fresh policy from the masters computes the same rows
        x = _up(eng, host[1][0][T]); ya, yb = eng.empty((E, P), np.float32), eng.empty((E, P), np.float32)
        fresh = eng.mlp_create(*actor, out_lo=0.0, precision="bf16")
        eng.mlp_forward(col.mlp, x, ya, E); eng.mlp_forward(fresh, x, yb, E)
        assert np.array_equal(_bits(ya.to_host()), _bits(yb.to_host()))
        eng.mlp_destroy(fresh)
    finally:
        if algo == "td3":      # close() in any order frees everything once
            learner.close(); col.close(); eng.close(); learner.close()
        else:
            col.close(); learner.close(); eng.close(); col.close()


def test_closing_the_engine_first_is_safe():
    from ev2gym_amd.td3 import TD3Learner
    eng = _gen_engine("pst")
    col = _collector(eng)
    learner = TD3Learner(col, batch_size=32)
    col.collect_episode()
    assert learner.train(1)["n_updates"] == 1
    eng.close(); learner.close(); col.close()


def test_both_halves_pending_and_lifetimes(engines):  # noqa: F811
    """ev2g_td3_apply with both gradients pending consumes both; a policy destroyed through a handle that does not own its learner leaves a learner
    that refuses; set_weights on a collector is refused while a learner is bound and keeps collector.weights current otherwise."""
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import EngineError, host_adam
    from ev2gym_amd.td3 import TD3Learner
    eng, other = engines["pst"], engines["ppl"]
    D, P = SHAPES["pst"]
    case = tc.make_case(D, P, "64-64", 2, 8, -1.0, 0.0)
    d = _Dev(eng, case)
    masters = _flat(*d.weights())
    eng.td3_critic_grad(d.t, *d.bufs, 8)
    eng.td3_actor_grad(d.t, d.bufs[0], 8)
    grads = _flat(*d.grads())
    eng.td3_apply(d.t)
    assert eng.td3_counters(d.t)[:2] == (1, 1)
    for a, g, b in zip(masters, grads, _flat(*d.weights())):   # every array stepped once, by its own gradient
        want, m, v = a.copy(), np.zeros_like(a), np.zeros_like(a)
        host_adam(want, m, v, g, 1, lr=1e-3, eps=1e-8)
        assert np.array_equal(_bits(want), _bits(b)) and np.abs(g).max() > 0.0
    with pytest.raises(EngineError) as ei:
        eng.td3_apply(d.t)
    assert ei.value.code == _abi.ERR_STATE
    eng.synchronize()
    other.mlp_destroy(d.mlp)          # the policy goes through a handle that does not own its learner: the learner stays, without a policy
    for call in (lambda: eng.td3_update(d.t, *d.bufs, 8), lambda: eng.td3_apply(d.t), lambda: eng.td3_get_weights(d.t, d.shape)):
        with pytest.raises(EngineError) as ei:
            call()
        assert ei.value.code == _abi.ERR_STATE and "policy was destroyed" in str(ei.value)
    eng.td3_destroy(d.t)
    for b in d.bufs + [d.losses]:
        b.free()

    own = _gen_engine("pst")
    col = _collector(own)
    try:
        w2 = [a + np.float32(0.01) for a in col.weights]
        col.set_weights(w2)           # no learner: a fresh policy object, and the collector remembers what it holds
        assert all(np.array_equal(a, b) for a, b in zip(col.weights, w2))
        learner = TD3Learner(col, batch_size=16)
        assert all(np.array_equal(a, b) for a, b in zip(learner.get_weights()[0], w2))
        with pytest.raises(RuntimeError, match="a device learner is bound"):
            col.set_weights(w2)
        with pytest.raises(ValueError, match="already has a learner"):
            TD3Learner(col)
        col.collect_episode()
        assert learner.train(2)["n_updates"] == 2   # the learner is still the policy's
        learner.close()
        col.set_weights(w2)
    finally:
        col.close()
        own.close()


# ---- 7. every refusal through the ABI ----
def test_refusals_through_the_abi(engines):  # noqa: F811
    from ev2gym_amd import _abi
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import EngineError
    from ev2gym_amd.td3 import init_critic_weights
    eng, other = engines["pst"], engines["ppl"]
    D, P = SHAPES["pst"]
    case = tc.make_case(D, P, "64-64", 2, 8, -1.0, 0.2)
    d = _Dev(eng, case)

    def refused(code, word, fn, *a, **kw):
        with pytest.raises(EngineError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    try:
        critics = lambda h1, h2, dd=D, pp=P: [init_critic_weights(dd, pp, 1 + j, h1, h2) for j in range(2)]  # noqa: E731
        free = eng.mlp_create(*case["actor"], out_lo=-1.0, precision="fp32")
        refused(_abi.ERR_ARG, "h1 32 is not the policy's 64", eng.td3_create, free, init_mlp_weights(D, P, 0, 32, 64), critics(32, 64))
        refused(_abi.ERR_ARG, "d_out 21 is not the policy's 20", eng.td3_create, free, init_mlp_weights(D, P + 1, 0, 64, 64), critics(64, 64, D, P + 1))
        refused(_abi.ERR_ARG, "tau must be in [0, 1]", eng.td3_create, free, case["actor"], case["critics"], tau=1.5)
        refused(_abi.ERR_ARG, "policy_delay must be finite and >= 1", eng.td3_create, free, case["actor"], case["critics"], policy_delay=0)
        refused(_abi.ERR_ARG, "n_critics 3 is outside 1 .. 2", eng.td3_create, free, case["actor"], case["critics"] + case["critics"][:1], n_critics=3)
        refused(_abi.ERR_STATE, "already has a learner", eng.td3_create, d.mlp, case["actor"], case["critics"])
        t2 = eng.td3_create(free, case["actor"], case["critics"])   # (the refusals left `free` unbound)
        eng.mlp_destroy(free)                                        # ... and its learner goes with it
        refused(_abi.ERR_ARG, "not created on this handle", eng.td3_apply, t2)
        for B in (0, 1025):
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.td3_update, d.t, *d.bufs, B)
            refused(_abi.ERR_ARG, f"B {B} is outside 1 .. 1024", eng.td3_actor_grad, d.t, d.bufs[0], B)
        refused(_abi.ERR_ARG, "not created on this handle", other.td3_update, d.t, *d.bufs, 8)
        refused(_abi.ERR_STATE, "no gradient to apply", eng.td3_apply, d.t)
        d.eng.td3_critic_grad(d.t, *d.bufs, 8)
        eng.td3_apply(d.t)
        refused(_abi.ERR_STATE, "no gradient to apply", eng.td3_apply, d.t)
        for lr in (float("nan"), -1.0, float("inf")):
            refused(_abi.ERR_ARG, "lr must be finite and >= 0", eng.td3_set_rate, d.t, lr)
        eng.td3_set_rate(d.t, 0.0)   # a zero rate is a rate: the masters stay
        before = _flat(*d.weights())
        d.update()
        for a, b in zip(before, _flat(*d.weights())):
            assert np.array_equal(_bits(a), _bits(b))
        refused(_abi.ERR_ARG, "null argument", eng.td3_update, d.t, None, *d.bufs[1:], 8)
        refused(_abi.ERR_ARG, "not the batch size", eng.td3_get_y, d.t, 9)
    finally:
        d.close()
