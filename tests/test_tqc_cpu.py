"""The TQC learner's arithmetic without a GPU (ev2gym_amd/tqc.py, csrc/ev2g_tqc.h's host twins, the host-only plan):

  * quantile_huber_loss_numpy on a hand case;
  * tqc_update_numpy -- the float64 analytic restatement the GPU tests lean on -- against the torch float64 restatement of sb3_contrib's
    TQC.train() (tests/tqc_cases.torch_loop) to 1e-9 of each array's largest magnitude: gradients, z, both log pi, the three losses, the gradient
    of log_ent_coef and every parameter over three consecutive updates with target_update_interval 2;
  * with one critic of one quantile and nothing dropped, z[:, 0] is sac_critic_numpy's y exactly;
  * tests/host/tqc_check.cpp, plain and under AddressSanitizer + UBSan: plan_tqc's refusals and layout, the host sort against std::stable_sort;
  * the host twins through the library; the Python-side refusals; the builder conditions of the GPU module's gradient and edge cases, and what
    those two lists cover."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import tqc_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantile_huber_loss_on_a_hand_case():
    from ev2gym_amd.tqc import quantile_huber_loss_numpy, quantile_huber_terms
    cur, tgt = np.zeros((1, 1, 1)), np.array([[0.5, 2.0, -3.0]])
    terms, delta = quantile_huber_terms(cur, tgt)
    assert np.array_equal(delta.reshape(-1), [0.5, 2.0, -3.0])
    assert np.array_equal(terms.reshape(-1), [0.0625, 0.75, 1.25])   # tau 0.5: 0.5 * 0.125, 0.5 * 1.5, 0.5 * 2.5
    assert quantile_huber_loss_numpy(cur, tgt) == 0.6875


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize("nc,nq,drop,lo,auto,B", [(2, 25, 2, -1.0, True, 37), (1, 25, 2, 0.0, False, 37), (5, 25, 2, 0.0, True, 37), (2, 7, 1, -1.0, False, 1),
                                                  (5, 3, 0, -1.0, True, 1), (1, 1, 0, 0.0, True, 37)])
def test_update_numpy_against_the_torch_float64_restatement(nc, nq, drop, lo, auto, B):
    """Three consecutive updates with target_update_interval 2 on batches of B rows: every quantity of every step to 1e-9 of its array's largest
    magnitude (values: of max(1, that))."""
    import torch
    from ev2gym_amd.tqc import tqc_state, tqc_update_numpy
    D, P = 11, 5
    case = tc.make_case(D, P, "33-17", nc, nq, drop, 3 * B, lo, 0.7, auto, seed=5)
    batches = tc.loop_batches(case, 3, B)
    ref = tc.torch_loop(case, batches, torch.float64, 2, grads=True)
    st = tqc_state(case["actor"], case["critics"], ent_coef=np.exp(case["log_ent_coef"]))
    worst = 0.0
    for k, (rows, eps, eps_next) in enumerate(batches):
        out = tqc_update_numpy(st, case["obs"][rows], case["actions"][rows], case["reward"][rows], case["next_obs"][rows], case["done"][rows], eps, eps_next, lo=lo,
                               target_update_interval=2, ent_coef_auto=auto, top_quantiles_to_drop_per_net=drop)
        r = ref[k]
        errs = [_rel(out.z, r["z"]), _rel(out.log_pi, r["log_pi"]), _rel(out.log_pi_next, r["log_pi_next"])]
        errs += [abs(getattr(out, n) - r[n]) / max(1.0, abs(r[n])) for n in ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef")]
        errs.append(abs(out.ent_coef_grad - r["ent_coef_grad"]) / max(1.0, abs(r["ent_coef_grad"])))
        errs += [_rel(a, b) for a, b in zip(out.actor_grads, r["actor_grads"])]
        errs += [_rel(a, b) for j in range(nc) for a, b in zip(out.critic_grads[j], r["critic_grads"][j])]
        errs += [_rel(a, b) for a, b in zip(st.actor, r["actor"])]
        errs += [_rel(a, b) for j in range(nc) for a, b in zip(st.critics[j], r["critics"][j])]
        errs += [_rel(a, b) for j in range(nc) for a, b in zip(st.critics_target[j], r["critics_target"][j])]
        errs.append(abs(float(st.log_ent_coef) - r["log_ent_coef"]))
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-9, (k, errs)
        moved = any(not np.array_equal(a, b) for a, b in zip(st.critics_target[0], case["critics"][0]))
        assert moved == (k >= 1)   # the Polyak step on the second update only
        if not auto:
            assert out.ent_coef_grad == 0.0 and out.ent_coef_loss == 0.0 and float(st.log_ent_coef) == np.log(np.exp(case["log_ent_coef"]))
    print(f"tqc numpy vs torch float64 nc{nc} nq{nq} d{drop} lo{lo:g} auto{int(auto)} B{B}: worst relative deviation {worst:.3e}")


@pytest.mark.parametrize("lo", [-1.0, 0.0])
def test_one_atom_is_sacs_target(lo):
    from ev2gym_amd.sac import sac_critic_numpy
    from ev2gym_amd.tqc import tqc_critic_numpy
    case = tc.make_case(11, 5, "33-17", 1, 1, 0, 37, lo, 0.7, True, seed=9)
    args = (case["actor"], case["critics"], case["critics"], case["obs"], case["actions"], case["reward"], case["next_obs"], case["done"], case["eps_next"],
            case["log_ent_coef"], lo, case["gamma"])
    z = tqc_critic_numpy(*args, 0)[2].z
    y = sac_critic_numpy(*args)[2].y
    assert z.shape == (37, 1) and np.array_equal(z[:, 0], y)


def test_tqc_check_host_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++")
                if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    for tag, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(tmp_path / f"tqc_check_{tag}")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", *extra, os.path.join(ROOT, "tests", "host", "tqc_check.cpp"), "-o", exe], timeout=300)
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        print(run.stdout[-3000:])
        assert run.returncode == 0, tag + ": " + run.stdout[-3000:] + run.stderr[-3000:]
        assert "tqc_check: ok" in run.stdout


@pytest.mark.parametrize("nc,nq,drop", tc.SORT_SHAPES)
def test_host_twins_of_the_target_and_of_the_critic_head(nc, nq, drop):
    """The library's twins against numpy in float64: z is one float32 rounding of the float64 expression on the stably sorted pool; dq and the loss
    to float32 rounding of the reference."""
    from ev2gym_amd.engine import host_tqc_critic_head, host_tqc_target
    from ev2gym_amd.tqc import quantile_huber_terms
    B, K, la = 33, nc * (nq - drop), np.float32(np.log(0.3))
    alpha = np.exp(np.float64(la))
    for kind in tc.SORT_KINDS:
        tq, lp, r, done = tc.sort_rows(kind, nc, nq, B)
        z = host_tqc_target(tq, lp, r, done, drop, 0.99, la)
        pool = tq.transpose(1, 0, 2).reshape(B, nc * nq)
        srt = np.take_along_axis(pool, np.argsort(pool, axis=1, kind="stable"), 1)[:, :K]
        want = (r.astype(np.float64)[:, None] + ((1.0 - done) * 0.99)[:, None] * (srt.astype(np.float64) - alpha * lp.astype(np.float64)[:, None])).astype(np.float32)
        assert z.shape == (B, K) and np.array_equal(z.view(np.uint32), want.view(np.uint32)), kind
        if kind == "done":
            assert np.array_equal(z, np.broadcast_to(r[:, None], (B, K)))
        q = np.random.default_rng(3).normal(0.0, 2.0, (nc, B, nq)).astype(np.float32)
        dq, loss = host_tqc_critic_head(z, q, drop)
        terms, delta = quantile_huber_terms(q.transpose(1, 0, 2), z)
        w = np.abs(((np.arange(nq) + 0.5) / nq)[None, None, :, None] - (delta < 0.0))
        dq64 = (-(w * np.clip(delta, -1.0, 1.0)).sum(3) / float(B * nc * nq * K)).transpose(1, 0, 2)
        assert np.abs(dq - dq64).max() <= 2.0 ** -23 * np.abs(dq64).max() and abs(loss - terms.mean()) <= 2.0 ** -23 * max(1.0, terms.mean()), kind


def test_host_twins_refuse_what_the_plan_refuses():
    from ev2gym_amd.engine import EngineError, host_tqc_critic_head, host_tqc_target
    z1 = np.zeros(4, np.float32)
    for shape, drop, word in (((6, 4, 2), 0, "n_critics 6 is outside 1 .. 5"), ((1, 4, 65), 0, "n_quantiles 65 is outside 1 .. 64"),
                              ((3, 4, 43), 0, "n_critics * n_quantiles 129 is outside 1 .. 128"), ((2, 4, 5), 5, "top_quantiles_to_drop_per_net 5 is outside 0 .. 4"),
                              ((2, 4, 5), -1, "top_quantiles_to_drop_per_net -1 is outside 0 .. 4")):
        with pytest.raises(EngineError, match=word.replace("*", r"\*").replace("..", r"\.\.")):
            host_tqc_target(np.zeros(shape, np.float32), z1, z1, np.zeros(4, np.uint8), drop, 0.99, 0.0)
        with pytest.raises(EngineError, match=word.replace("*", r"\*").replace("..", r"\.\.")):
            host_tqc_critic_head(np.zeros((4, 1), np.float32), np.zeros(shape, np.float32), drop)


def test_python_refusals_and_presets():
    from ev2gym_amd import sac, td3
    from ev2gym_amd.sac import init_sac_actor_weights
    from ev2gym_amd.tqc import TQCCollector, TQCLearner, make_learner
    col = types.SimpleNamespace(eng=None, weights=init_sac_actor_weights(5, 2, 0, 8, 8), tqc=None, cap=2, lo=-1.0)
    for kw, word in ((dict(use_sde=True), "use_sde"), (dict(action_noise=object()), "action_noise"), (dict(learning_starts=100), "learning_starts"),
                     (dict(lr=lambda f: 3e-4), "schedule"), (dict(optimize_memory_usage=True), "optimize_memory_usage"), (dict(ent_coef="automatic"), "ent_coef"),
                     (dict(ent_coef=0.0), "ent_coef"), (dict(target_entropy="half"), "target_entropy"), (dict(batch_size=0), "batch_size"),
                     (dict(batch_size=1025), "batch_size"), (dict(policy_delay=2), "policy_delay"), (dict(n_critics=6), r"n_critics 6 is outside 1 \.\. 5"),
                     (dict(n_quantiles=65), r"n_quantiles 65 is outside 1 \.\. 64"), (dict(n_critics=5, n_quantiles=26), r"n_critics \* n_quantiles 130 is outside 1 \.\. 128"),
                     (dict(top_quantiles_to_drop_per_net=25), r"top_quantiles_to_drop_per_net 25 is outside 0 \.\. 24"),
                     (dict(n_quantiles=0), "n_quantiles 0")):
        with pytest.raises(ValueError, match=word) as e:
            TQCLearner(col, **kw)
        assert "TQC's quantile critics" not in str(e.value)
    sac_col = types.SimpleNamespace(eng=None, weights=col.weights, sac=None, cap=2, lo=-1.0)
    with pytest.raises(ValueError, match="not a TQCCollector"):
        TQCLearner(sac_col)
    assert not hasattr(TQCCollector.__new__(TQCCollector), "sac")   # so SACLearner refuses a TQCCollector
    assert not hasattr(TQCLearner.__new__(TQCLearner), "sac") and hasattr(TQCLearner, "tqc")
    for algo in ("SAC", "TD3"):
        with pytest.raises(ValueError, match="not supported"):
            make_learner(algo, col)
    with pytest.raises(ValueError, match="TQC is out of scope"):   # the other modules' make_learner keep refusing it
        sac.make_learner("TQC", col)
    with pytest.raises(ValueError, match="SAC / TQC"):
        td3.make_learner("TQC", col)
    assert TQCLearner.PRESET == dict(n_critics=2, n_quantiles=25, top_quantiles_to_drop_per_net=2, lr=3e-4, tau=0.005, gamma=0.99, batch_size=256,
                                     target_update_interval=1, ent_coef="auto", target_entropy="auto")


def test_default_config_and_param_shapes():
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import tqc_default_config
    c = tqc_default_config()
    assert (c.lr, c.beta1, c.beta2, c.adam_eps, c.tau, c.gamma, c.ent_coef) == (3e-4, 0.9, 0.999, 1e-8, 0.005, 0.99, 1.0)
    assert (c.n_critics, c.target_update_interval, c.ent_coef_auto, c.target_entropy_auto, c.n_quantiles, c.top_quantiles_to_drop_per_net) == (2, 1, 1, 1, 25, 2)
    shapes = _abi.tqc_param_shapes(63, 64, 32, 20, 3, 7)
    assert len(shapes) == 8 + 18 and shapes[:8] == _abi.sac_param_shapes(63, 64, 32, 20, 0) and shapes[8:14] == [(64, 83), (64,), (32, 64), (32,), (7, 32), (7,)]


# ---- the cases of tests/test_tqc_gpu.py off NETS: their conditions hold, without a GPU ----
@pytest.mark.parametrize("tag,nc,nq,drop,lo,auto,B", tc.EDGE_GRAD_CASES)
def test_edge_cases_keep_the_builders_conditions(tag, nc, nq, drop, lo, auto, B):
    case = tc.edge_grad_case(tag, nc, nq, drop, lo, auto, B)
    print(f"tqc {tag} {nc}x{nq} d{drop} lo{lo:g} auto{int(auto)} B{B}: redrawn {case['redrawn']}, seeds skipped {case['seeds_skipped']}, regions "
          f"{np.round(case['regions'], 3)}, mixed drop {case['mixed_drop']}")
    assert (case["D"], *case["h"], case["P"]) == tc.EDGE_NETS[tag] and case["obs"].shape == (B, case["D"])
    assert case["redrawn"] < B / 4.0 and case["seeds_skipped"] <= 1
    assert tc.nonzero_grads(case["ref64"]) and len(case["ref64"]["critic_grads"]) == nc
    assert min(case["regions"]) >= tc.REGION_SHARE and (case["mixed_drop"] is None or case["mixed_drop"] >= tc.MIXED_DROP_SHARE)
    assert case["ref64"]["z"].shape == (B, nc * (nq - drop))


@pytest.mark.parametrize("net,dp,qs,lo,auto,B", tc.grad_cases())
def test_grad_cases_keep_the_builders_conditions(net, dp, qs, lo, auto, B):
    case = tc.grad_case(net, dp, qs, lo, auto, B)
    assert (case["D"], case["P"]) == dp and case["h"] == tc.NETS[net] and case["obs"].shape == (B, dp[0]) and tc.kept(case) == qs[0] * (qs[1] - qs[2])
    assert case["redrawn"] < B / 4.0 and case["seeds_skipped"] <= 1
    assert B < 17 or min(case["regions"]) >= tc.REGION_SHARE
    assert case["mixed_drop"] is None or case["mixed_drop"] >= tc.MIXED_DROP_SHARE


def test_grad_case_list_spreads_every_value_over_every_network():
    """tests/test_tqc_gpu.py's gradient cases: each (nc, nq, d), each (D, P), each B, both boxes and both kinds of coefficient meet each network,
    and the rate tool's shape -- 256-256, (162, 50), 2 x 25 with 2 dropped -- is among them."""
    cases = tc.grad_cases()
    assert len(cases) == len(set(cases)) == 18
    for net in tc.NETS:
        rows = [c for c in cases if c[0] == net]
        assert {c[1] for c in rows} == set(tc.DP) and {c[2] for c in rows} == set(tc.QUANTILES), net
        assert {c[5] for c in rows} == set(tc.BATCHES) and {c[3] for c in rows} == {-1.0, 0.0} and {c[4] for c in rows} == {True, False}, net
    assert {(c[1], c[2]) for c in cases} >= {(dp, (2, 25, 2)) for dp in tc.DP}   # the preset at every shape
    assert any(c[:3] == ("256-256", (162, 50), (2, 25, 2)) for c in cases)
    assert tc.QUANTILES == ((2, 25, 2), (1, 25, 2), (5, 25, 2), (2, 64, 0), (3, 7, 1), (1, 1, 0)) and tc.BATCHES == (1, 17, 37, 257)


def test_edge_case_list_covers_what_it_claims():
    atoms = {(c[0], c[1] * c[2], c[1] * (c[2] - c[3]), c[6]) for c in tc.EDGE_GRAD_CASES}
    assert ("limits", 125, 115, 1023) in atoms and ("limits", 128, 128, 1024) in atoms
    assert {m for _, m, _, _ in atoms} >= {1, 3, 6, 64, 65, 125, 128} and {k for _, _, k, _ in atoms} >= {1, 2}
    assert {c[4] for c in tc.EDGE_GRAD_CASES} == {-1.0, 0.0} and {c[5] for c in tc.EDGE_GRAD_CASES} == {True, False}
    assert sorted({nc * nq for nc, nq, _ in tc.SORT_SHAPES}) == [1, 2, 63, 64, 65, 125, 128]
