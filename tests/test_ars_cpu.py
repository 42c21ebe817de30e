"""The ARS learner's arithmetic without a GPU (ev2gym_amd/ars.py, csrc/ev2g_ars_host.h's host twins and plan):

  * `ars_update_numpy` (float64) against sb3_contrib's update lines restated in torch float64 (tests/ars_cases.torch_update), to 1e-9 of each
    array's largest magnitude (the project's float64 parity bound), with n_top = n_delta, n_top < n_delta, n_top = 1 and n_delta = 1, on cases
    whose scores are pairwise distinct (asserted);
  * the host twins through the library: perturb bit for bit theta +- float32(delta * float32(delta_std)) with delta from ev2g_ac_host_normal at
    the stated indices (iteration n + 1 continues the range); update within one float32 rounding of `ars_update_numpy`; the crafted updates
    (ties to the lower index, equal returns, NaN, infinity); the returns in the stated order against a numpy loop, bit for bit;
  * the cases of tests/test_ars_range_gpu.py, pinned on the float64 reference alone before the device is asked: on every ars_cases.EDGE_NETS
    network (both boxes, and the saturated one) the candidates' actions pairwise more than 1e-3 apart at every C and R, fewer than 10 % of the
    tanh pre-activations beyond 9, the linear policies' actions at both bounds and strictly inside, the shifted ports' pre-activations beyond
    10 (a seed that misses one is passed over among ten fixed seeds; the count is printed); the large updates' returns -- pairwise distinct
    scores; integer returns of eight values with equal scores on both sides of the n_top cut and directions k and k + 256 tied; one NaN at the
    last candidate; one +inf above candidate 256 -- and the twin within one float32 rounding of the float64 update at n_delta up to 4096;
  * tests/host/ars_check.cpp, a stand-alone C++17 program, plain and under -fsanitize=address,undefined;
  * the Python-side refusals, the policies' state-dict names and the pack -> unpack round trip;
  * the compiler's resource report of every ev2g_ars_* kernel: no spills, no scratch, the population actor within 128 VGPRs."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from tests import ars_cases as ac

BOUND = 1e-9
EPS32 = 2.0 ** -23
TINY32 = float(np.finfo(np.float32).tiny)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _close(tag, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-300)
    dev = float(np.abs(got - ref).max())
    print(f"{tag}: deviation {dev:.3e} scale {scale:.3e}")
    assert dev <= BOUND * scale, (tag, dev, scale)


@pytest.mark.parametrize("n_delta,n_top", ac.UPDATE_CASES)
def test_update_numpy_matches_torch_float64(n_delta, n_top):
    from ev2gym_amd.ars import ars_update_numpy
    case = ac.update_case(n_delta, n_top)
    s = ac.scores(case["returns"])
    assert len(set(s.tolist())) == n_delta, "the case's scores must be pairwise distinct"
    new, info = ars_update_numpy(case["theta"], case["delta"], case["returns"], n_top, case["lr"])
    ref, sigma, step, top_idx = ac.torch_update(case)
    assert np.array_equal(info["order"], top_idx)
    _close("theta", new, ref)
    _close("sigma_R", info["sigma_r"], sigma)
    _close("step", info["step"], step)
    assert np.abs(new - case["theta"]).max() > 0.0


def test_host_perturb_is_two_float32_roundings_of_the_stated_draws():
    from ev2gym_amd.engine import host_ars_perturb, host_normal
    rng = np.random.default_rng(3)
    n_delta, n, seed, std = 3, 41, 77, 0.05
    theta = rng.normal(size=n).astype(np.float32)
    for it in (5, 6):
        delta, cand = host_ars_perturb(theta, n_delta, std, seed, it)
        want = host_normal(n_delta * n, seed, it * n_delta * n).reshape(n_delta, n)   # draw (it n_delta + k) n + i
        assert np.array_equal(_bits(delta), _bits(want)), it
        d = (want * np.float32(std)).astype(np.float32)
        assert np.array_equal(_bits(cand[:n_delta]), _bits(theta + d)) and np.array_equal(_bits(cand[n_delta:]), _bits(theta - d)), it
    two = host_normal(2 * n_delta * n, seed, 5 * n_delta * n)
    assert np.array_equal(_bits(two[n_delta * n:]), _bits(delta.ravel()))   # iteration 6 continues iteration 5's index range
    assert float(np.float32(std)) != std and (cand[:n_delta] != theta).any()


@pytest.mark.parametrize("n_delta,n_top", ac.UPDATE_CASES + ac.LARGE_UPDATES)
def test_host_update_is_one_float32_rounding_from_the_float64_update(n_delta, n_top):
    from ev2gym_amd.ars import ars_update_numpy
    from ev2gym_amd.engine import host_ars_update
    if (n_delta, n_top) in ac.LARGE_UPDATES:   # the device's large updates (tests/test_ars_range_gpu.py): the bound holds for the twin before the device is asked
        case = dict(ac.large_update(n_delta), returns=ac.large_returns(n_delta, n_top, "distinct"))
    else:
        case = ac.update_case(n_delta, n_top)
    ref, info = ars_update_numpy(case["theta"], case["delta"], case["returns"], n_top, case["lr"])
    new, rep = host_ars_update(case["theta"], case["delta"], case["returns"], n_top, case["lr"])
    tol = EPS32 * np.maximum(np.abs(ref), TINY32)
    err = np.abs(new.astype(np.float64) - ref)
    print(f"n_delta {n_delta} n_top {n_top}: worst error / tolerance {(err / tol).max():.3f}")
    assert (err <= tol).all()
    rank_of = np.empty(n_delta, np.int64)
    rank_of[np.argsort(-ac.scores(case["returns"]), kind="stable")] = np.arange(n_delta)
    assert np.array_equal(rep["ranks"], rank_of) and not rep["refused"] and rep["first_bad"] == -1 and rep["n_top"] == n_top
    _close("sigma_R", rep["sigma_r"], info["sigma_r"])
    _close("step", rep["step"], info["step"])


def test_host_update_on_the_crafted_returns():
    from ev2gym_amd.engine import host_ars_update
    case = ac.update_case(4, 2)
    theta, delta, crafted = case["theta"], case["delta"], ac.crafted_returns(4)
    new, rep = host_ars_update(theta, delta, crafted["ties"], 2, 0.02)
    assert np.array_equal(rep["ranks"], np.arange(4)) and not rep["refused"] and (new != theta).any()   # equal scores: the lower index first
    new, rep = host_ars_update(theta, delta, crafted["equal"], 4, 0.02)
    assert np.array_equal(_bits(new), _bits(theta)) and rep["sigma_r"] == 0.0 and rep["step"] == 0.02 / 1e-6 and not rep["refused"]
    for name, bad in (("nan", 5), ("inf", 2)):
        new, rep = host_ars_update(theta, delta, crafted[name], 4, 0.02)
        assert rep["refused"] and rep["first_bad"] == bad and np.array_equal(_bits(new), _bits(theta)), name
    new, rep = host_ars_update(theta, delta, crafted["plain"], 4, 0.02)
    assert not rep["refused"] and np.array_equal(rep["ranks"], [2, 1, 0, 3])   # scores 3, 4, 7.5, 2.5: direction 2 first, then 1, 0, 3


def test_host_returns_run_in_the_stated_order():
    from ev2gym_amd.engine import EngineError, host_ars_returns
    rng = np.random.default_rng(9)
    E, C, k1, k2, offset = 24, 4, 7, 5, -0.375
    rew = rng.normal(0.0, 1e3, (k1 + k2, E)) + rng.normal(0.0, 1e-6, (k1 + k2, E))
    env = np.zeros(E)
    assert host_ars_returns(env, rew[:k1]) is None
    ret = host_ars_returns(env, rew[k1:], C, offset, k1 + k2)   # the second segment accumulates on the first
    want_env = np.zeros(E)
    for t in range(k1 + k2):
        want_env = want_env + rew[t]
    assert np.array_equal(_bits(env), _bits(want_env))
    R = E // C
    want = np.zeros(C)
    for c in range(C):
        s = 0.0
        for e in range(R):
            s = s + want_env[c * R + e]
        want[c] = s + offset * float(R * (k1 + k2))
    assert np.array_equal(_bits(ret), _bits(want))
    with pytest.raises(EngineError):
        host_ars_returns(env, None, 5)   # 24 envs are no multiple of 5 candidates


EDGE_PINS = [(tag, lo, False) for tag in sorted(ac.EDGE_NETS) for lo in (-1.0, 0.0)] + [("eighth", -1.0, True), ("eighth", 0.0, True)]


@pytest.mark.parametrize("tag,lo,saturate", EDGE_PINS)
def test_edge_cases_keep_their_pins_on_the_float64_reference(tag, lo, saturate):
    """What tests/test_ars_range_gpu.py's forward cases rely on, on the float64 reference alone (ars_cases.edge_case): candidates more than 1e-3
    apart at every C and R, tanh mostly unsaturated, the linear policies' actions at both bounds and inside, the shifted ports saturated."""
    from ev2gym_amd.ars import ars_forward_numpy, split_theta
    case = ac.edge_case(tag, lo, saturate)
    kind, D, h1, h2, P = ac.net_of(tag)
    print(f"ARS EDGE CASE {tag} lo {lo:g}{' saturated' if saturate else ''}: seeds skipped {case['seeds_skipped']}  " +
          "  ".join(f"C {C}: " + " ".join(f"{k} {v:.3g}" for k, v in fig.items()) for C, fig in case["figures"].items()))
    assert case["misses"] == [] and case["seeds_skipped"] < 10
    assert case["theta"].size == ac.n_params_of(tag) and sorted(case["cands"]) == list(ac.EDGE_C)
    for C in ac.EDGE_C:
        assert case["cands"][C].shape == (C, case["theta"].size)
        for R in ac.EDGE_R:
            ref = case["refs"][C, R]
            assert ref.shape == (C, R, P) and ref.min() >= lo and ref.max() <= 1.0
    if saturate:
        # |v| >= 10 (pinned by edge_case): tanh(v) is within 4.2e-9 of +-1 and rounds to exactly +-1 in float32, whose unscaled action is exactly
        # 1 or lo; the float64 action stays 1 - O(1e-10) (and, at lo = 0, a 1e-11 that float32 could hold: the device's tanhf cannot)
        assert np.float32(np.tanh(10.0)) == np.float32(1.0) and np.float32(np.tanh(-10.0)) == np.float32(-1.0) and 1.0 - np.tanh(10.0) < 4.2e-9
        ref = case["refs"][6, 33]
        for p, shift in case["sat"].items():
            want = 1.0 if shift > 0 else lo
            assert 0.0 < np.abs(ref[..., p] - want).max() < 5e-9, p
        assert len(case["sat"]) == 29 and sum(s > 0 for s in case["sat"].values()) == 15
    if kind == "LinearPolicy":   # (the reference clips: an element beyond a bound IS the bound)
        w = split_theta(case["cands"][2][0], kind, D, h1, h2, P)
        raw = case["rows"].astype(np.float64) @ w[0].astype(np.float64).T
        assert np.array_equal(ars_forward_numpy(case["rows"], w, kind, lo), np.clip(raw, lo, 1.0))


@pytest.mark.parametrize("n_delta,n_top", ac.LARGE_UPDATES)
def test_large_returns_are_distinct_tied_and_bad_as_stated(n_delta, n_top):
    distinct = ac.large_returns(n_delta, n_top, "distinct")
    assert distinct.shape == (2 * n_delta,) and len(set(ac.scores(distinct).tolist())) == n_delta and np.isfinite(distinct).all()
    ties = ac.large_returns(n_delta, n_top, "ties")
    s = ac.scores(ties)
    assert np.array_equal(ties, np.round(ties)) and len(set(ties.tolist())) == 8
    ranked = np.sort(s)[::-1]
    if n_top < n_delta:
        assert ranked[n_top - 1] == ranked[n_top], "equal scores must stand on both sides of the n_top cut"
    else:
        assert len(set(s.tolist())) < n_delta
    if n_delta > 256:
        assert any(s[k] == s[k + 256] for k in range(n_delta - 256)), "directions k and k + 256 must tie for some k"
        assert s[0] == s[256] and ac.stable_ranks(ties)[0] < ac.stable_ranks(ties)[256]
    rank = ac.stable_ranks(ties)
    assert sorted(rank.tolist()) == list(range(n_delta)) and all(s[a] >= s[b] for a, b in zip(np.argsort(rank)[:-1], np.argsort(rank)[1:]))
    nan, inf = ac.large_returns(n_delta, n_top, "nan"), ac.large_returns(n_delta, n_top, "inf")
    assert np.flatnonzero(~np.isfinite(nan)).tolist() == [2 * n_delta - 1] and np.isnan(nan[-1])
    assert np.flatnonzero(~np.isfinite(inf)).tolist() == [ac.LARGE_INF_AT] and inf[ac.LARGE_INF_AT] == np.inf and 256 < ac.LARGE_INF_AT < 2 * n_delta
    for bad in (nan, inf):
        keep = np.isfinite(bad)
        assert np.array_equal(bad[keep], distinct[keep])


def test_large_update_twin_on_ties_and_bad_returns():
    """host_ars_update at n_delta 257: ranks by "ties to the lower index" as numpy's stable argsort states it, and the refusals' first_bad"""
    from ev2gym_amd.engine import host_ars_update
    n_delta, n_top = 257, 1
    case = ac.large_update(n_delta)
    ties = ac.large_returns(n_delta, n_top, "ties")
    new, rep = host_ars_update(case["theta"], case["delta"], ties, n_top, case["lr"])
    assert np.array_equal(rep["ranks"], ac.stable_ranks(ties)) and not rep["refused"] and (new != case["theta"]).any()
    for kind, at in (("nan", 2 * n_delta - 1), ("inf", ac.LARGE_INF_AT)):
        new, rep = host_ars_update(case["theta"], case["delta"], ac.large_returns(n_delta, n_top, kind), n_top, case["lr"])
        assert rep["refused"] and rep["first_bad"] == at and np.array_equal(_bits(new), _bits(case["theta"])), kind


def test_ars_check_host_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    for tag, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(tmp_path / f"ars_check_{tag}")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", *extra, os.path.join(ROOT, "tests", "host", "ars_check.cpp"), "-o", exe], timeout=300)
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(run.stdout[-3000:])
        assert run.returncode == 0, tag + ": " + run.stdout[-3000:] + run.stderr[-3000:]
        assert "ars_check: ok" in run.stdout


def test_python_refusals_and_state_dict_names():
    from ev2gym_amd.ars import ARSLearner, ARSLinearPolicy, ARSPolicy, LINEAR_KEYS, MLP_KEYS
    from ev2gym_amd.engine import EngineError, ars_config, ars_query
    assert MLP_KEYS == ("action_net.0.weight", "action_net.0.bias", "action_net.2.weight", "action_net.2.bias", "action_net.4.weight", "action_net.4.bias")
    assert LINEAR_KEYS == ("action_net.0.weight",)
    pol = ARSPolicy.zeros(63, 20, net_arch=(33, 17), lo=0.0)
    theta = ac.random_theta("pst-33-17")
    pol.set_theta(theta)
    sd = pol.state_dict()
    assert tuple(sd) == MLP_KEYS and sd["action_net.2.weight"].shape == (17, 33) and sd["action_net.4.bias"].shape == (20,)
    again = ARSPolicy.from_state_dict(sd, lo=0.0)
    assert np.array_equal(_bits(again.theta()), _bits(theta)) and again.n_params == ars_query("MlpPolicy", 63, 33, 17, 20)["n_params"]
    lin = ARSLinearPolicy.from_state_dict({"action_net.0.weight": np.ones((20, 63), np.float32)})
    assert lin.n_params == 1260 and (lin.h1, lin.h2) == (0, 0)
    with pytest.raises(KeyError, match="action_net.2.bias"):
        ARSPolicy.from_state_dict({k: v for k, v in sd.items() if k != "action_net.2.bias"})
    with pytest.raises(ValueError, match="does not have"):
        ARSLinearPolicy.from_state_dict(sd)
    with pytest.raises(ValueError, match="lo"):
        ARSPolicy.zeros(5, 2, lo=0.5)
    with pytest.raises(ValueError, match="d_in 193"):
        ARSLinearPolicy.zeros(193, 2)
    with pytest.raises(ValueError, match="h1 257"):
        ARSPolicy.zeros(5, 2, net_arch=(257, 8))
    eng = types.SimpleNamespace(E=48, D=5, P=2, T=12, M=48)
    for kw, word in ((dict(policy="CnnPolicy"), "CnnPolicy"), (dict(zero_policy=False), "zero_policy"), (dict(learning_rate=lambda f: 0.02), "schedule"),
                     (dict(n_delta=4, n_top=5), "n_top"), (dict(n_delta=4, n_top=0), "n_top"), (dict(n_delta=5), "multiple of 2 n_delta"),
                     (dict(n_delta=4, n_eval_episodes=7), "n_eval_episodes"), (dict(n_delta=4, n_eval_episodes=0), "n_eval_episodes"),
                     (dict(policy=ARSPolicy.zeros(6, 2)), "maps 6 -> 2")):
        with pytest.raises(ValueError, match=word):
            ARSLearner(eng, **kw)
    for kw, word in ((dict(learning_rate=-1.0), "learning_rate must be finite and >= 0"), (dict(delta_std=0.0), "delta_std must be finite and > 0"),
                     (dict(alive_bonus_offset=float("nan")), "alive_bonus_offset must be finite"), (dict(n_delta=4097), "n_delta 4097"), (dict(n_top=9), "n_top 9")):
        with pytest.raises(EngineError, match=word):
            ars_query("MlpPolicy", 63, 64, 64, 20, ars_config(**kw))
    with pytest.raises(TypeError, match="gamma"):
        ars_config(gamma=0.99)
    info = ars_query("MlpPolicy", 162, 64, 64, 50, ars_config(n_delta=64, n_top=64))
    assert info["n_params"] == 162 * 64 + 64 + 64 * 64 + 64 + 64 * 50 + 50 and info["image_bytes"] == 129 * info["candidate_floats"] * 4
    assert info["lds_bytes"] <= 66560 and (info["max_in"], info["max_hidden"], info["max_out"], info["max_delta"]) == (192, 256, 256 // 4, 4096)


def test_forward_numpy_of_both_kinds_and_boxes():
    from ev2gym_amd.ars import ars_forward_numpy, split_theta
    rng = np.random.default_rng(2)
    x = rng.normal(size=(9, 63))
    kind, D, h1, h2, P = ac.NETS["pst-33-17"]
    w = split_theta(ac.random_theta("pst-33-17", scale=3.0), kind, D, h1, h2, P)
    a = ars_forward_numpy(x, w, kind, -1.0)
    assert np.allclose(ars_forward_numpy(x, w, kind, 0.0), 0.5 * (a + 1.0), rtol=0, atol=1e-15) and np.abs(a).max() <= 1.0 and np.abs(a).max() > 0.05
    wl = split_theta(ac.random_theta("pst-linear", scale=6.0), "LinearPolicy", 63, 0, 0, 20)
    raw = x @ wl[0].astype(np.float64).T
    for lo in (-1.0, 0.0):
        got = ars_forward_numpy(x, wl, "LinearPolicy", lo)
        assert np.array_equal(got, np.clip(raw, lo, 1.0)) and (got == lo).any() and (got == 1.0).any()


def test_ars_kernels_keep_their_register_budgets_and_do_not_spill():
    """The compiler's own figures (-Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): every ev2g_ars_* kernel without spills and
    without scratch; the population actor within 128 VGPRs, so that its weight ring stays in registers at four wavefronts per SIMD."""
    from ev2gym_amd import build
    cmd = [build.hipcc()] + [f for f in build.FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                                      "-o", os.devnull, build.SRC]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, res = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r" (VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            res.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    ars = {k: v for k, v in res.items() if "ev2g_ars_" in k}
    print(ars)
    names = ("ev2g_ars_act_kernel", "ev2g_ars_perturb_kernel", "ev2g_ars_returns_kernel", "ev2g_ars_candidates_kernel", "ev2g_ars_rank_kernel",
             "ev2g_ars_step_kernel", "ev2g_ars_repack_kernel")
    for n in names:
        assert sum(n in k for k in ars) == (2 if n == "ev2g_ars_act_kernel" else 1), (n, sorted(ars))
    assert len(ars) == len(names) + 1
    for k, v in ars.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        if "ev2g_ars_act_kernel" in k:
            assert v["VGPRs"] <= 128, (k, v)
