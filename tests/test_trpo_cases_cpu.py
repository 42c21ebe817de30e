"""tests/trpo_cases.py's step cases on the float64 reference, without a GPU: each meets tests/test_trpo_gpu.py's `_margins` as they stand (so the
device test that runs it compares like with like), and each has the shape it is in the table for -- the iteration its solve ends at, the
verdict of every try, a failed step that made no try.  Every case prints its margins, the r . r the exit was tested on and the tries."""
import numpy as np
import pytest

from tests import trpo_cases as tc
from tests.test_ppo_cpu import _record
from tests.test_trpo_cpu import TorchTrpo, decisions, trpo_reference
from tests.test_trpo_gpu import _margins


def _pin(tag, case, idx, cfg):
    import torch
    ref = trpo_reference(case, idx, **cfg)
    y32 = TorchTrpo(case, idx, torch.float32, normalize_advantage=cfg.get("normalize_advantage", True)).step(
        **{k: v for k, v in cfg.items() if k != "normalize_advantage"})
    target_kl = cfg.get("target_kl", 0.01)
    _margins(f"CASE {tag}", ref, y32, target_kl)
    _record(f"TRPO CASE {tag}: r.r {['%.3e' % r for r in ref['rho_history']]}  iterations {ref['cg_iterations']}  "
            f"(KL, J) {[('%.4e' % k, '%.4e' % j) for k, j in ref['tries']]}  J0 {ref['objective_before']:.4e}  verdicts {decisions(ref, target_kl)[0]}  "
            f"accepted {ref['accepted']}")
    return ref


@pytest.mark.parametrize("tag", tc.NET_IDS)
def test_every_network_steps_away_from_the_branches(tag):
    case = tc.net_case(tag)
    steps = tc.net_steps(tag)
    assert [len(ix) for _, ix in steps[:3]] == [1, 32, 97] and len(set(steps[2][1][5:9]) | {steps[2][1][0]}) == 1
    if tag == tc.LOOPING_NET:
        assert len(steps) == 4 and len(steps[3][1]) > 32 * tc.grid_cap(case) and case["h"] != (64, 64)
    for label, idx in steps:
        ref = _pin(label, case, idx, tc.NET_CFG)
        assert ref["accepted"] and not ref["failed"]
        if label in tc.ENDS_EARLY:   # a second solve that ends in mid-queue, at two of three iterations
            assert ref["cg_iterations"] == 2 and ref["rho_history"][-1] <= 1e-12
        else:
            assert ref["cg_iterations"] == 3


def test_the_mid_queue_solve_ends_at_its_third_iteration_of_fifteen():
    case, idx = tc.pst_case()
    ref = _pin("mid-queue", case, idx, tc.MID_QUEUE_CFG)
    assert ref["cg_iterations"] == 3 and len(ref["rho_history"]) == 4 and ref["rho_history"][2] >= 1e-8 and ref["rho_history"][3] <= 1e-12
    assert ref["line_search_tries"] == 1 and ref["accepted"]
    # three iterations asked for: the third is the last one, which updates x by the same expression
    short = trpo_reference(case, idx, cg_max_steps=3, **tc.MID_QUEUE_CFG)
    assert np.array_equal(short["x"], ref["x"]) and short["cg_iterations"] == 3
    for a, b in zip(short["params"], ref["params"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("tag", list(tc.DEEP_SEARCHES))
def test_deep_line_searches(tag):
    cfg, verdicts, accepted = tc.DEEP_SEARCHES[tag]
    case, idx = tc.pst_case()
    ref = _pin(tag, case, idx, cfg)
    target_kl, J0 = cfg["target_kl"], ref["objective_before"]
    assert decisions(ref, target_kl)[0] == verdicts and ref["accepted"] == accepted and not ref["failed"]
    shrink = cfg.get("line_search_shrinking_factor", 0.8)
    assert abs(ref["c"] - shrink ** (len(verdicts) - 1)) <= 1e-15
    if tag == "objective-alone":   # no rejected try breaks the KL condition
        assert all(KL < target_kl and J <= J0 for KL, J in ref["tries"][:3])
    else:
        assert all(KL > target_kl for KL, _ in ref["tries"][:len(verdicts) - accepted])   # every rejected try breaks the KL condition


@pytest.mark.parametrize("tag", tc.NON_FINITE)
def test_a_non_finite_gradient_fails_the_step(tag):
    bad, case, idx = tc.non_finite_case(tag)
    ref = tc.reference_quiet(bad, idx, normalize_advantage=False)
    assert not np.isfinite(ref["g"]).all() and np.isfinite(bad["obs"]).all()
    assert ref["failed"] and not ref["accepted"] and ref["cg_iterations"] == 15 and ref["line_search_tries"] == 0
    assert not np.isfinite(ref["xHx"])
    from ev2gym_amd.trpo import actor_arrays
    for a, b in zip(ref["params"], actor_arrays(case["weights"], case["log_std"])):
        assert np.array_equal(a, b)
    _record(f"TRPO CASE {tag}: failed {ref['failed']}  iterations {ref['cg_iterations']}  tries {ref['line_search_tries']}  x.Hx {ref['xHx']}")
    good = _pin(f"{tag}, the ordinary step afterwards", case, idx, dict(normalize_advantage=False))
    assert good["accepted"]
