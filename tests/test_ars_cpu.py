"""The ARS learner's arithmetic without a GPU (ev2gym_amd/ars.py, csrc/ev2g_ars_host.h's host twins and plan):

  * `ars_update_numpy` (float64) against sb3_contrib's update lines restated in torch float64 (tests/ars_cases.torch_update), to 1e-9 of each
    array's largest magnitude (the project's float64 parity bound), with n_top = n_delta, n_top < n_delta, n_top = 1 and n_delta = 1, on cases
    whose scores are pairwise distinct (asserted);
  * the host twins through the library: perturb bit for bit theta +- float32(delta * float32(delta_std)) with delta from ev2g_ac_host_normal at
    the stated indices (iteration n + 1 continues the range); update within one float32 rounding of `ars_update_numpy`; the crafted updates
    (ties to the lower index, equal returns, NaN, infinity); the returns in the stated order against a numpy loop, bit for bit;
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


@pytest.mark.parametrize("n_delta,n_top", ac.UPDATE_CASES)
def test_host_update_is_one_float32_rounding_from_the_float64_update(n_delta, n_top):
    from ev2gym_amd.ars import ars_update_numpy
    from ev2gym_amd.engine import host_ars_update
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
