"""The TD3 / DDPG learner's arithmetic without a GPU (ev2gym_amd/td3.py, csrc/ev2g_td3.h's host twins, the host-only plan and element map):

  * `td3_update_numpy` and its two halves (float64, analytic backprop) against torch float64 autograd and torch.optim.Adam(eps=1e-8), to 1e-10 of
    each array's largest magnitude: critic and actor gradients, y, both losses, and three consecutive updates with policy_delay 2, targets
    included; both presets, B in {1, 37}, lo in {-1, 0};
  * tests/host/td3_check.cpp, a stand-alone C++17 program: for every packing plan_mlp can return, writing the masters through the element map
    reproduces pack_mlp's images bit for bit and touches no padding word; the config and shape refusals; the host twins against plain
    restatements;
  * `ev2g_host_replay_indices`: within bounds, a pure function of (seed, counter, row), different for different counters;
  * the host twins of the target and of Polyak through the library, and the Python-side refusals;
  * the cases tests/test_td3_gpu.py runs off the handles' shapes (tests/td3_cases.EDGE_NETS, the saturated actors): the redraw cap, a non-zero
    element in every float64 reference gradient array, |pre-tanh| >= 10 on the saturated ports, tolerances that a device of zeros would miss."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from tests import td3_cases as tc

PRESETS = {"td3": dict(n_critics=2, sigma=0.2, policy_delay=2), "ddpg": dict(n_critics=1, sigma=0.0, policy_delay=1)}


def _close(tag, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-300)
    dev = float(np.abs(got - ref).max())
    print(f"{tag}: deviation {dev:.3e} scale {scale:.3e}")
    assert dev <= 1e-10 * scale, (tag, dev, scale)


@pytest.mark.parametrize("lo", [-1.0, 0.0])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("preset", ["td3", "ddpg"])
def test_numpy_halves_match_torch_float64_autograd(preset, B, lo):
    import torch
    from ev2gym_amd.td3 import td3_actor_numpy, td3_critic_numpy
    p = PRESETS[preset]
    case = tc.make_case(63, 20, "64-64", p["n_critics"], B, lo, p["sigma"])
    ref = tc.torch_grads(case, torch.float64)
    cg, closs, aux = td3_critic_numpy(case["actor"], case["critics"], case["critics"], case["obs"], case["actions"], case["reward"], case["next_obs"],
                                      case["done"], case["normals"], lo, case["gamma"], case["sigma"], case["clip"])
    _close("y", aux.y, ref["y"])
    _close("critic_loss", closs, ref["critic_loss"])
    for j in range(p["n_critics"]):
        for i in range(6):
            _close(f"critic {j} grad {i}", cg[j][i], ref["critic_grads"][j][i])
    ag, aloss, _ = td3_actor_numpy(case["actor"], case["critics"][0], case["obs"])
    _close("actor_loss", aloss, ref["actor_loss"])
    for i in range(6):
        _close(f"actor grad {i}", ag[i], ref["actor_grads"][i])
    if p["sigma"] > 0.0 and B > 1:   # the noise is in play: it moved a' and some of it was clipped
        assert np.abs(aux.a_next - aux.a_target).max() > 0.1


@pytest.mark.parametrize("lo", [-1.0, 0.0])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("preset", ["td3", "ddpg"])
def test_three_numpy_updates_match_a_torch_float64_loop(preset, B, lo):
    import torch
    from ev2gym_amd.engine import host_normal
    from ev2gym_amd.td3 import td3_state, td3_update_numpy
    p = PRESETS[preset]
    case = tc.make_case(63, 20, "64-64", p["n_critics"], 3 * B, lo, p["sigma"])
    P = case["P"]
    batches = []
    for k in range(3):
        rows = np.arange(k * B, (k + 1) * B)
        batches.append((rows, host_normal(B * P, 11, k * B * P).reshape(B, P) if p["sigma"] > 0.0 else None))
    ref = tc.torch_loop(case, batches, torch.float64, policy_delay=2)   # (policy_delay 2 for both: the delay is what is under test)
    st = td3_state(case["actor"], case["critics"])
    for k, (rows, normals) in enumerate(batches):
        out = td3_update_numpy(st, case["obs"][rows], case["actions"][rows], case["reward"][rows], case["next_obs"][rows], case["done"][rows], normals, lo,
                               policy_delay=2, target_policy_noise=case["sigma"], target_noise_clip=case["clip"], gamma=case["gamma"])
        r = ref[k]
        _close(f"step {k} critic_loss", out.critic_loss, r["critic_loss"])
        assert (out.actor_loss is None) == (r["actor_loss"] is None) == (k != 1)
        if k == 1:
            _close("step 1 actor_loss", out.actor_loss, r["actor_loss"])
        for name, got, want in (("actor", st.actor, r["actor"]), ("actor_target", st.actor_target, r["actor_target"])):
            for i in range(6):
                _close(f"step {k} {name} {i}", got[i], want[i])
        for j in range(p["n_critics"]):
            for i in range(6):
                _close(f"step {k} critic {j} {i}", st.critics[j][i], r["critics"][j][i])
                _close(f"step {k} critic_target {j} {i}", st.critics_target[j][i], r["critics_target"][j][i])
    assert (st.n, st.t_critic, st.t_actor) == (3, 3, 1)


def test_td3_check_host_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "td3_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "td3_check.cpp"), "-o", exe], timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert "td3_check: ok" in run.stdout


def test_host_replay_indices_are_in_bounds_pure_and_counter_dependent():
    from ev2gym_amd.engine import EngineError, host_replay_indices
    B, n, T, E = 1024, 2, 12, 37
    a = host_replay_indices(B, n, T, E, 5, 0)
    assert a.shape == (B, 3) and a.min() >= 0
    assert a[:, 0].max() == n - 1 and a[:, 1].max() == T - 1 and a[:, 2].max() == E - 1   # (1024 rows reach every bound's last value)
    assert a[:, 0].min() == 0 and a[:, 1].min() == 0 and a[:, 2].min() == 0
    assert np.array_equal(a, host_replay_indices(B, n, T, E, 5, 0))
    assert np.array_equal(a[:100], host_replay_indices(100, n, T, E, 5, 0))   # a row's draw does not depend on B
    b = host_replay_indices(B, n, T, E, 5, 1)
    assert not np.array_equal(a, b) and not np.array_equal(a[1:], b[:-1])
    assert not np.array_equal(a, host_replay_indices(B, n, T, E, 6, 0))
    one = host_replay_indices(B, 1, 1, 1, 5, 3)
    assert not one.any()
    counts = np.bincount(host_replay_indices(B, n, T, E, 9, 2)[:, 1], minlength=T)
    assert counts.min() > B / T / 3   # uniform over the steps, roughly
    for bad in ((0, 2, 12, 37), (1025, 2, 12, 37), (8, 0, 12, 37), (8, 33, 12, 37), (8, 2, 0, 37), (8, 2, 12, 0)):
        with pytest.raises(EngineError):
            host_replay_indices(*bad, 1, 0)


def test_host_twins_of_target_and_polyak():
    from ev2gym_amd.engine import EngineError, host_normal, host_polyak, host_td3_target
    rng = np.random.default_rng(3)
    B, P = 33, 20
    at = rng.uniform(-1.2, 1.2, (B, P)).astype(np.float32)
    tq = rng.normal(size=(2, B)).astype(np.float32)
    r, d = rng.normal(size=B).astype(np.float32), (rng.uniform(size=B) < 0.4).astype(np.uint8)
    a_next, y = host_td3_target(at, tq, r, d, 0.2, 0.5, 0.99, 17, 1000)
    eps = np.clip(np.float32(0.2) * host_normal(B * P, 17, 1000).reshape(B, P), np.float32(-0.5), np.float32(0.5))
    assert np.array_equal(a_next, np.clip(at + eps, np.float32(-1), np.float32(1)))
    assert np.abs(eps).max() == 0.5 and (a_next == 1.0).any() and (a_next == -1.0).any()   # both clamps act
    assert np.array_equal(y, r + ((np.float32(1) - d.astype(np.float32)) * np.float32(0.99)) * tq.min(0))
    quiet, y1 = host_td3_target(at, tq[:1], r, d, 0.0, 0.5, 0.99, 17, 1000)
    assert np.array_equal(quiet, np.clip(at, np.float32(-1), np.float32(1)))
    assert np.array_equal(y1, r + ((np.float32(1) - d.astype(np.float32)) * np.float32(0.99)) * tq[0])
    t, p = rng.normal(size=500).astype(np.float32), rng.normal(size=500).astype(np.float32)
    want = t * np.float32(1.0 - 0.005) + np.float32(0.005) * p
    host_polyak(t, p, 0.005)
    assert np.array_equal(t, want)
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(EngineError):
            host_polyak(t, p, tau)


def test_python_refusals():
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.td3 import DDPGLearner, TD3Learner, make_learner
    col = types.SimpleNamespace(eng=None, weights=init_mlp_weights(5, 2, 0, 8, 8), mlp=None)
    for kw, word in ((dict(action_noise=object()), "action_noise"), (dict(learning_starts=100), "learning_starts"), (dict(lr=lambda f: 1e-3), "schedule"),
                     (dict(optimize_memory_usage=True), "optimize_memory_usage"), (dict(ent_coef="auto"), "ent_coef"), (dict(batch_size=0), "batch_size"),
                     (dict(batch_size=1025), "batch_size")):
        for cls in (TD3Learner, DDPGLearner):
            with pytest.raises(ValueError, match=word):
                cls(col, **kw)
    big = types.SimpleNamespace(eng=None, weights=col.weights, mlp=None, cap=34)   # 33 complete blocks: one more than the sampler's table holds
    with pytest.raises(ValueError, match="capacity_episodes must be at most 33"):
        TD3Learner(big)
    bound = types.SimpleNamespace(eng=None, weights=col.weights, mlp=None, learner=types.SimpleNamespace(learner=1))
    with pytest.raises(ValueError, match="already has a learner"):
        TD3Learner(bound)
    for algo in ("SAC", "TQC"):
        with pytest.raises(ValueError, match="SAC / TQC"):
            make_learner(algo, col)
    assert DDPGLearner.PRESET["n_critics"] == 1 and DDPGLearner.PRESET["batch_size"] == 100 and TD3Learner.PRESET["batch_size"] == 256


# ---- the cases of tests/test_td3_gpu.py off the handles' shapes: their conditions hold, without a GPU ----
def _tolerances_exclude_zeros(tag, ref, ref32):
    """Under the idiom a device that returned zeros would fail on every gradient array: 4 d32 + 4 * 2^-23 * s stays far below s."""
    for name, r, r32 in [(f"critic {j} grad {i}", g, ref32["critic_grads"][j][i]) for j, c in enumerate(ref["critic_grads"]) for i, g in enumerate(c)] + \
                        [(f"actor grad {i}", g, ref32["actor_grads"][i]) for i, g in enumerate(ref["actor_grads"])]:
        scale, d32 = float(np.abs(r).max()), float(np.abs(r32 - r).max())
        tol = tc.grad_tol(r, d32)
        print(f"{tag} {name}: scale {scale:.3e} d32 {d32:.3e} tol {tol:.3e}")
        assert scale > 0.0 and tol < 0.05 * scale, (tag, name, scale, tol)


@pytest.mark.parametrize("tag,n_critics,lo,sigma,B", tc.EDGE_GRAD_CASES)
def test_edge_cases_keep_the_redraw_cap_and_live_gradients(tag, n_critics, lo, sigma, B):
    case = tc.edge_grad_case(tag, n_critics, lo, sigma, B)
    print(f"td3 {tag} nc{n_critics} lo{lo:g} sigma{sigma:g} B{B}: redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}")
    assert (case["D"], *case["h"], case["P"]) == tc.EDGE_NETS[tag] and case["obs"].shape == (B, case["D"])
    assert case["redrawn"] < B / 4.0 and case["seeds_skipped"] <= 1   # (no case needed more than its second seed)
    assert tc.nonzero_grads(case["ref64"])
    assert len(case["ref64"]["critic_grads"]) == n_critics and (case["normals"] is not None) == (sigma > 0.0)


def test_edge_case_lists_cover_what_they_claim():
    for tag in tc.EDGE_NETS:
        rows = [c for c in tc.EDGE_GRAD_CASES if c[0] == tag]
        assert {c[4] for c in rows} == ({1, 33, 1023, 1024} if tag == "limits" else {33, 1024}), tag
        assert {c[1] for c in rows} == {1, 2} and {c[2] for c in rows} == {-1.0, 0.0} and {c[3] for c in rows} == {0.2, 0.0}, tag   # each value meets each network
    assert all(c[1] == 2 for c in tc.EDGE_GRAD_CASES if c[0] == "limits" and c[4] >= 1023)
    D, h1, h2, P = tc.EDGE_NETS["limits"]
    assert (D, h1, h2, P) == (192, 400, 400, 64) and all(x % 16 == 0 for x in (D, h1, h2, P, D + P))      # no ragged tile
    assert all(x == 16 for x in tc.EDGE_NETS["tile"]) and all(x % 16 == 1 for x in tc.EDGE_NETS["tile+1"])
    assert tc.EDGE_NETS["tiny"] == (1, 5, 2, 1)


@pytest.mark.parametrize("net,dp,n_critics,lo,sigma,B", tc.SATURATED_GRAD_CASES)
def test_saturated_cases_reach_the_clamp_and_keep_their_tolerances(net, dp, n_critics, lo, sigma, B):
    """The builder asserts |pre-tanh| >= 10 in float64 on every second port, for every row of obs and next_obs, and that a quarter of the a'
    elements are exactly +-1.  Here also: float32 torch has the saturated ports' W3 rows and b3 entries at exactly 0, and the idiom's tolerances
    stay non-degenerate."""
    import torch
    case = tc.saturated_grad_case(net, dp, n_critics, lo, sigma, B)
    print(f"td3 saturated {net} B{B}: redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}, share of a' at +-1 {case['share_at_1']:.4f}")
    assert case["share_at_1"] >= (0.25 if sigma > 0.0 else 0.5)
    ref32 = tc.torch_grads(case, torch.float32)
    ports, _ = tc.saturated_ports(dp[1])
    live = np.setdiff1d(np.arange(dp[1]), ports)
    assert not ref32["actor_grads"][4][ports].any() and not ref32["actor_grads"][5][ports].any()
    assert np.abs(ref32["actor_grads"][4][live]).max(axis=1).min() > 0.0 and np.abs(ref32["actor_grads"][5][live]).min() > 0.0
    _tolerances_exclude_zeros(f"td3 saturated {net} B{B}", case["ref64"], ref32)


def test_update_cases_off_the_handles_shapes_have_live_gradients_on_every_step():
    """tiny at B 33 over three updates (test_three_updates_adam_polyak_and_order): every critic array on every step and every actor array on the
    second have a non-zero gradient in float64; limits at B 1024 (the reproducibility test) keeps the cap."""
    from ev2gym_amd.engine import host_normal
    from ev2gym_amd.td3 import td3_state, td3_update_numpy
    case = tc.edge_case("tiny", 2, 99, -1.0, 0.2, seed=5)
    print(f"td3 tiny loop: redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}")
    st = td3_state(case["actor"], case["critics"])
    for k in range(3):
        rows = np.arange(k * 33, (k + 1) * 33)
        out = td3_update_numpy(st, case["obs"][rows], case["actions"][rows], case["reward"][rows], case["next_obs"][rows], case["done"][rows],
                               host_normal(33, 11, k * 33).reshape(33, 1), -1.0, policy_delay=2)
        assert all(np.any(g) for c in out.critic_grads for g in c), k
        assert (out.actor_grads is not None) == (k == 1) and (k != 1 or all(np.any(g) for g in out.actor_grads))
    big = tc.edge_case("limits", 2, 1024, 0.0, 0.2, seed=21)
    print(f"td3 limits B1024 seed 21: redrawn {big['redrawn']}, seeds skipped {big['seeds_skipped']}")
    assert big["seeds_skipped"] == 0 and case["seeds_skipped"] == 0   # the GPU tests' own cases: no seed was passed over
    plain = tc.make_case(192, 64, "limits", 2, 1024, 0.0, 0.2, seed=21)   # (as the reproducibility test builds it)
    assert all(np.array_equal(big[k], plain[k]) for k in ("obs", "actions", "reward", "next_obs", "done", "normals"))
    for tag, shape, _, _ in tc.REFRESH_EDGE_CASES:
        c = tc.make_case(shape[0], shape[3], shape[1:3], 2, 64, 0.0, 0.2, seed=9, live=True)
        print(f"td3 refresh {tag}: redrawn {c['redrawn']}, seeds skipped {c['seeds_skipped']}")
        assert c["seeds_skipped"] == 0 and c["redrawn"] < 16 and tc.nonzero_grads(c["ref64"]) and (c["D"], *c["h"], c["P"]) == tuple(shape)
