"""What tests/test_trpo_cases_cpu.py and tests/test_trpo_edges_gpu.py share: the table of TRPO step cases that take the learner's kernels
(csrc/ev2g_trpo.h) off the one network, the one solve length and the two-try line searches tests/test_trpo_gpu.py runs them at, and their
builders.  A plain module.

A step case is the rows' case (tests/test_ppo_cpu.py's make_case), the row indices and the learner's settings.  The line search is
discontinuous in its two conditions and the conjugate-gradient exit in r . r, so every case is held ON THE REFERENCE to
tests/test_trpo_gpu.py's `_margins` as it stands (|KL - target| >= 1e-3 target, |J - J0| >= 1e-4 max(1, |J0|), torch float32 deciding alike,
every tested r . r >= 1e-8 or <= 1e-12) by tests/test_trpo_cases_cpu.py, which also pins the shape each case is there for: the iteration the
solve ends at, the verdict of every try.  A case that stops meeting them is replaced by another seed, B or setting; the margins stay.

  NET STEPS     every row of NET_CASES at cg_max_steps 3 and B 1 (no normalisation), 32 (one full chunk) and 97 with duplicates; lopsided-relu
                once more with every workgroup looping.  Three iterations: at fifteen some solves cross 1e-10 at an iteration float32 does
                not share.  tiny at B 1 ends its solve before the third iteration on its own.
  MID-QUEUE     cg_damping 1000: H is near 1000 I, r . r falls by 1e-4 per iteration and the solve ends at iteration 3 of 15.
  DEEP SEARCHES three tries rejected on the objective alone; six tries at a shrinking factor of 0.95; the same failed after four.
  NON-FINITE    one NaN advantage, one infinite ratio: NaN runs through all fifteen iterations and x . Hx fails the step."""
import numpy as np

from tests.learner_cases import N_ROWS, _shape
from tests.test_ppo_cpu import make_case, torch_params
from tests.test_trpo_cpu import trpo_reference
from tests.test_trpo_gpu import NET_CASES, VALUE

NET_IDS = [c[0] for c in NET_CASES]
STEP_B = (1, 32, 97)
NET_CFG = dict(cg_max_steps=3)
LOOPING_NET = "lopsided-relu"
ENDS_EARLY = ("tiny-tanh B 1", "tiny-relu B 1")   # the labels of net_steps whose solve ends before its third iteration
# The rows are drawn by default_rng(12) but for the labels here.  ppl-tanh B 1: seed 12's row puts the one try's KL at 0.0099949, 5.1e-4 of the
# target from the target (a one-row step is all but exactly quadratic), inside the 1e-3 margin; the seed below is the next that keeps it.
ROW_SEEDS = {"ppl-tanh B 1": 13}
MID_QUEUE_CFG = dict(cg_damping=1000.0)
# tag -> (settings, the verdicts of the tries, accepted)
DEEP_SEARCHES = {
    "objective-alone": (dict(target_kl=1000.0, cg_damping=100.0, cg_max_steps=3), [False, False, False, True], True),
    "six-tries": (dict(target_kl=16.0, line_search_shrinking_factor=0.95), [False] * 5 + [True], True),
    "failed-after-four": (dict(target_kl=16.0, line_search_shrinking_factor=0.95, line_search_max_iter=4), [False] * 4, False),
}
NON_FINITE = ("nan-advantage", "infinite-ratio")
CHANGING_B = (33, None, 1, 97)   # None: every workgroup looping
CRITIC_LRS = (1e-3, 3e-3, 1e-4)

_CASES = {}


def net_case(tag):
    """The rows of a row of NET_CASES (made once per run; nothing changes them)."""
    if tag not in _CASES:
        _, _, D, h, v, P, activation = NET_CASES[NET_IDS.index(tag)]
        case = make_case(D, P, h=h, v=v, activation=activation, n_rows=N_ROWS[activation])
        assert activation == "tanh" or case["zmin"] >= 1e-5
        _CASES[tag] = case
    return _CASES[tag]


def pst_case():
    """The (64, 64) tanh case of tests/test_trpo_gpu.py's step tests and its 97 rows."""
    if "pst-600" not in _CASES:
        _CASES["pst-600"] = make_case(63, 20, n_rows=600)
    return _CASES["pst-600"], np.random.default_rng(12).choice(600, 97)


def grid_cap(case):
    from ev2gym_amd.engine import trpo_query
    return trpo_query(*_shape(case))["grid_cap"]


def looping_rows(case):
    """The fewest rows that make every workgroup of a launch loop, and 37 more."""
    return 32 * grid_cap(case) + 37


def step_rows(case, B, seed=12):
    """B rows drawn with repeats; at 97, four of them the same row for certain."""
    idx = np.random.default_rng(seed).integers(0, case["obs"].shape[0], B)
    if B == 97:
        idx[5:9] = idx[0]
    return idx


def net_steps(tag):
    """The (label, idx) of a network's step cases."""
    case = net_case(tag)
    out = [(f"{tag} B {B}", step_rows(case, B, ROW_SEEDS.get(f"{tag} B {B}", 12))) for B in STEP_B]
    if tag == LOOPING_NET:
        B = looping_rows(case)
        out.append((f"{tag} B {B}", step_rows(case, B)))
    return out


def non_finite_case(tag):
    """(the case with one non-finite operand among the 97 rows of pst_case, the ordinary case, the rows): indices and observations stay
    ordinary.  Normalisation is off in these cases: it would spread a NaN advantage over every row."""
    case, idx = pst_case()
    bad = dict(case)
    row = int(idx[41])
    if tag == "nan-advantage":
        bad["advantages"] = case["advantages"].copy()
        bad["advantages"][row] = np.nan
    else:
        bad["old_log_prob"] = case["old_log_prob"].copy()
        bad["old_log_prob"][row] = -1e4   # exp(lp + 1e4) = inf
    return bad, case, idx


def reference_quiet(case, idx, **cfg):
    """trpo_reference on operands that are meant to be non-finite."""
    with np.errstate(all="ignore"):
        return trpo_reference(case, idx, **cfg)


def critic_torch_rates(case, sets, dtype, lrs):
    """tests/test_trpo_gpu.py's `_critic_torch` with a rate per minibatch, set in the optimiser's param group before the step as a schedule
    does: (the thirteen parameters after Adam(eps=1e-5) over every set, their value losses)"""
    import torch
    F = torch.nn.functional
    params = torch_params(case, dtype)
    vals = [params[i] for i in VALUE]
    act = torch.tanh if case["activation"] == "tanh" else torch.relu
    opt = torch.optim.Adam(vals, lr=lrs[0], eps=1e-5)
    losses = []
    for lr, idx in zip(lrs, sets):
        opt.param_groups[0]["lr"] = lr
        x, R = (torch.tensor(np.asarray(case[k])[np.asarray(idx)], dtype=dtype) for k in ("obs", "returns"))
        v = F.linear(act(F.linear(act(F.linear(x, params[4], params[5])), params[6], params[7])), params[10], params[11]).flatten()
        loss = F.mse_loss(R, v)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return [p.detach().numpy().astype(np.float64) for p in params], np.array(losses)
