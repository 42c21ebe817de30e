"""The TRPO learner on the device (csrc/ev2g_trpo.h) off the one shape tests/test_trpo_gpu.py steps it at: the whole policy step on every
network of its NET_CASES at B 1, 32 and 97 (and with every workgroup looping off width 64), a solve that ends in mid-queue, line searches of
four and six tries and one that fails after four shrinks, a non-finite gradient, one learner over changing row counts, the critic's gradient on
every network at every row count, the effect of the rate setter, replaced weights under a bound learner, and TRPOLearner.train() on given and on
sub-sampled rows.

Tolerance: the suite's (tests/test_trpo_gpu.py's docstring): reference = float64, d32 = torch-CPU float32's deviation from it, the device gets
4 d32 + 4 * 2^-23 * s; every figure goes through `_record` before it is asserted.  The step cases are tests/trpo_cases.py's, which
tests/test_trpo_cases_cpu.py holds to `_margins` on the reference without a GPU; `_compare_step` asserts them again.  Where two device runs
must be the same computation (a gated launch that wrote nothing, a restored theta0, a reused learner against a fresh one) the comparison is
bit for bit: the kernels have one fixed summation order and no float atomics."""
import numpy as np
import pytest

from tests import trpo_cases as tc
from tests.learner_cases import NAMES, _index_sets, _shape, engines  # noqa: F401 (engines: the fixture)
from tests.test_learner_shapes_gpu import _collected_case, _lr_is_seen, _policy_behind_a_collector, _state
from tests.test_onpolicy_gpu import _bits, _up
from tests.test_ppo_cpu import _record, make_case, value_tol
from tests.test_trpo_cpu import ACTOR, TorchTrpo, trpo_reference
from tests.test_trpo_gpu import NET_CASES, VALUE, _compare_step, _critic_torch, _margins, _Trpo, _val, _vec

pytestmark = pytest.mark.gpu

KIND = {c[0]: c[1] for c in NET_CASES}


def _same_bits(what, got, want):
    for name, a, b in zip(NAMES, got, want):
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: {name}"


def _same_report(a, b):
    """Two reports field by field, NaN equal to NaN."""
    return a.keys() == b.keys() and all(np.array_equal(_bits(np.float64(a[k])), _bits(np.float64(b[k]))) for k in a)


def _same_step(what, one, two):
    """(report, x, g, the thirteen arrays) of two device steps, bit for bit"""
    (ra, xa, ga, wa), (rb, xb, gb, wb) = one, two
    assert _same_report(ra, rb), (what, ra, rb)
    assert np.array_equal(_bits(xa), _bits(xb)), f"{what}: x"
    assert np.array_equal(_bits(ga), _bits(gb)), f"{what}: g"
    _same_bits(what, wa, wb)


def _stepped(dev, idx):
    rep, x, g = dev.step(idx)
    return rep, x, g, dev.weights()


def _means(eng, case, acs):
    """The mean of each policy object on the all-zero observation (biases and padding only), ordinary rows, and rows with large entries, which
    a non-zero padding weight would show up in."""
    D, P = case["D"], case["P"]
    x = np.concatenate([np.zeros((1, D), np.float32), case["obs"][:36], 50.0 * case["obs"][:40]])
    dx = _up(eng, x)
    out = [eng.empty((len(x), P), np.float32) for _ in acs]
    for ac, m in zip(acs, out):
        eng.ac_forward(ac, dx, len(x), mean=m)
    eng.synchronize()
    got = [m.to_host() for m in out]
    for b in [dx] + out:
        b.free()
    assert all(np.isfinite(m).all() for m in got)
    return got


def _twin_of(eng, case, arrays13=None):
    from ev2gym_amd.onpolicy import GaussianActorCritic
    w = list(case["weights"]) + [case["log_std"]] if arrays13 is None else arrays13
    return GaussianActorCritic(w[:12], w[12], activation=case["activation"], lo=-1.0, seed=5).attach(eng)


# ---- 1. the whole step on every network ----
@pytest.mark.parametrize("tag", tc.NET_IDS)
def test_the_whole_step_on_every_network(engines, tag):
    """g, x, beta, x . Hx, J(theta0), the last try's KL and J and the seven actor arrays against the float64 reference at three iterations, the
    six value arrays untouched; then the candidate kernel's placement into the padded images: a fresh policy object created from the read-back
    arrays computes the stepped policy's mean bit for bit."""
    eng, case = engines[KIND[tag]], tc.net_case(tag)
    ok = True
    for label, idx in tc.net_steps(tag):
        dev, fresh = _Trpo(eng, case, **tc.NET_CFG), None
        try:
            good, ref, before, after = _compare_step(f"EDGE STEP {label}", dev, case, idx, tc.NET_CFG)
            ok &= good
            assert ref["accepted"] and ref["cg_iterations"] == (2 if label in tc.ENDS_EARLY else 3)
            for i in ACTOR:
                assert not np.array_equal(after[i], before[i]), NAMES[i]
            fresh = _twin_of(eng, case, after)
            a, b = _means(eng, case, (dev.pol.ac, fresh.ac))
            assert np.array_equal(_bits(a), _bits(b)), label
        finally:
            if fresh is not None:
                fresh.close()
            dev.close()
    assert ok


# ---- 2. a solve that ends in mid-queue ----
def test_a_solve_that_ends_in_mid_queue_gates_the_remaining_launches(engines):
    """cg_damping 1000: the solve ends at its third iteration of fifteen.  A learner asked for three iterations runs the same three (its third
    is the `last` one, which updates x by the same expression), so the two agree bit for bit exactly when the twelve gated iterations' launches
    wrote nothing."""
    eng = engines["pst"]
    case, idx = tc.pst_case()
    full, short = _Trpo(eng, case, **tc.MID_QUEUE_CFG), _Trpo(eng, case, cg_max_steps=3, **tc.MID_QUEUE_CFG)
    try:
        ok, ref, _, after = _compare_step("EDGE MID-QUEUE", full, case, idx, tc.MID_QUEUE_CFG)
        assert ok and ref["cg_iterations"] == 3 and ref["accepted"] and ref["line_search_tries"] == 1
        x, g = eng.trpo_get_direction(full.trpo, full.n_actor)
        _same_step("fifteen iterations queued against three", (eng.trpo_get_report(full.trpo), x, g, after), _stepped(short, idx))
    finally:
        full.close()
        short.close()


# ---- 3. deep line searches ----
@pytest.mark.parametrize("tag", list(tc.DEEP_SEARCHES))
def test_deep_line_searches(engines, tag):
    cfg, verdicts, accepted = tc.DEEP_SEARCHES[tag]
    eng = engines["pst"]
    case, idx = tc.pst_case()
    dev, twin, fresh = _Trpo(eng, case, **cfg), None, None
    try:
        ok, ref, before, after = _compare_step(f"EDGE LINE SEARCH {tag}", dev, case, idx, cfg)
        assert ok and ref["line_search_tries"] == len(verdicts) and ref["accepted"] == accepted
        shrink = cfg.get("line_search_shrinking_factor", 0.8)
        assert abs(eng.trpo_get_report(dev.trpo)["c"] - shrink ** (len(verdicts) - 1)) <= 1e-15
        if accepted:
            twin = _twin_of(eng, case, after)
        else:   # masters, images and transposed images as before: bit-identical outputs, and a second step is a fresh learner's
            _same_bits("theta0 restored", after, before)
            twin = _twin_of(eng, case)
        a, b = _means(eng, case, (dev.pol.ac, twin.ac))
        assert np.array_equal(_bits(a), _bits(b))
        if not accepted:
            fresh = _Trpo(eng, case, **cfg)
            _same_step("a second step after the restore", _stepped(dev, idx), _stepped(fresh, idx))
    finally:
        for d in (twin, fresh, dev):
            if d is not None:
                d.close()


# ---- 4. a non-finite gradient ----
@pytest.mark.parametrize("tag", tc.NON_FINITE)
def test_a_non_finite_gradient_fails_the_step_and_leaves_theta0(engines, tag):
    """One non-finite operand value among ordinary rows (every index and observation is ordinary): NaN runs through all fifteen iterations,
    and the guard on x . Hx fails the step before any try.  The learner is whole afterwards."""
    eng = engines["pst"]
    bad, case, idx = tc.non_finite_case(tag)
    cfg = dict(normalize_advantage=False)
    ref = tc.reference_quiet(bad, idx, **cfg)
    assert ref["failed"] and not ref["accepted"] and ref["cg_iterations"] == 15 and ref["line_search_tries"] == 0
    dev, twin, fresh = _Trpo(eng, bad, **cfg), None, None
    try:
        before = dev.weights()
        rep, x, g = dev.step(idx)
        _record(f"TRPO EDGE NON-FINITE {tag}: report {rep}  finite elements of g {int(np.isfinite(g).sum())} of {g.size}")
        assert rep["failed"] and not rep["accepted"] and rep["line_search_tries"] == 0
        assert rep["cg_iterations"] == 15 and not np.isfinite(rep["xHx"]) and not np.isfinite(g).all()
        _same_bits("theta0 kept", dev.weights(), before)
        twin = _twin_of(eng, case)
        a, b = _means(eng, case, (dev.pol.ac, twin.ac))
        assert np.array_equal(_bits(a), _bits(b))
        dev.adv.upload(case["advantages"])   # the ordinary rows again
        dev.old.upload(case["old_log_prob"])
        fresh = _Trpo(eng, case, **cfg)
        one, two = _stepped(dev, idx), _stepped(fresh, idx)
        assert one[0]["accepted"] and np.isfinite(one[1]).all()
        _same_step("an ordinary step after the failed one", one, two)
    finally:
        for d in (twin, fresh, dev):
            if d is not None:
                d.close()


# ---- 5. one learner, changing B ----
def test_one_learner_over_changing_row_counts(engines):
    """33, every-workgroup-looping, 1 and 97 rows on one learner (mu0 regrown, partials and slabs holding what the larger launch left), a
    critic minibatch of the looping size and one of one row in between: each step is a fresh learner's on a fresh policy created from the
    arrays read back before it."""
    eng = engines["pst"]
    case, _ = tc.pst_case()
    many = tc.looping_rows(case)
    dev = _Trpo(eng, case)
    try:
        for k, B in enumerate(n or many for n in tc.CHANGING_B):
            idx = tc.step_rows(case, B, seed=40 + k)
            w = dev.weights()
            fresh = _Trpo(eng, dict(case, weights=w[:12], log_std=w[12]))
            try:
                one, two = _stepped(dev, idx), _stepped(fresh, idx)
                _record(f"TRPO EDGE CHANGING B {B}: report {one[0]}")
                assert np.isfinite(one[1]).all() and one[1].any() and one[0]["cg_iterations"] >= 1
                _same_step(f"step {k} of {B} rows", one, two)
                if k in (1, 2):   # (the fresh learner's Adam state is the reused one's at the first minibatch only)
                    ix = tc.step_rows(case, many if k == 1 else 1, seed=50 + k)
                    vl = [d.critic(ix) for d in (dev, fresh)]
                    grads = [eng.ppo_get_grads(d.trpo, _shape(case)) for d in (dev, fresh)]
                    assert np.isfinite(vl[0]) and np.array_equal(_bits(np.float32(vl[0])), _bits(np.float32(vl[1])))
                    for i in VALUE:
                        assert np.abs(grads[0][i]).max() > 0 and np.array_equal(_bits(grads[0][i]), _bits(grads[1][i])), NAMES[i]
                    if k == 1:
                        _same_bits(f"a critic minibatch of {len(ix)} rows", dev.weights(), fresh.weights())
            finally:
                fresh.close()
    finally:
        dev.close()


# ---- 6. the critic on every network, every row count, and its rate ----
@pytest.mark.parametrize("tag", tc.NET_IDS)
def test_the_critic_gradient_on_every_network_and_row_count(engines, tag):
    """At a rate of zero (ev2g_trpo_set_rate accepts it) one learner serves every index set: the six value gradients and value_loss against
    value_grad_numpy, the actor's entries of the gradient buffer and all thirteen arrays bit-identical throughout."""
    import torch
    from ev2gym_amd.trpo import value_grad_numpy
    eng, case = engines[KIND[tag]], tc.net_case(tag)
    sets = _index_sets(tc.grid_cap(case), case["obs"].shape[0])
    assert [len(ix) for ix in sets[:5]] == [1, 31, 32, 33, 97] and len(sets[5]) > 32 * tc.grid_cap(case)
    dev = _Trpo(eng, case)
    try:
        eng.trpo_set_rate(dev.trpo, 0.0)
        start = dev.weights()
        g0, _ = dev.grad(sets[3])   # the actor's entries of the gradient buffer hold g
        assert all(np.abs(g0[i]).max() > 0 for i in ACTOR)
        ok = True
        for idx in sets:
            label = f"EDGE CRITIC {tag} B {len(idx)}"
            vl64, g64 = value_grad_numpy(case["weights"], case["obs"], case["returns"], idx, activation=case["activation"])
            g32, _, l32 = _critic_torch(case, [idx], torch.float32)
            vl = dev.critic(idx)
            got = eng.ppo_get_grads(dev.trpo, _shape(case))
            for k, i in enumerate(VALUE):
                assert got[i].shape == g64[k].shape, NAMES[i]
                ok &= _vec(label, "d value_loss / d " + NAMES[i], got[i].astype(np.float64), g64[k], g32[k])
            ok &= _val(label, "value_loss", vl, vl64, l32[0])
            for i in ACTOR:
                assert np.array_equal(_bits(got[i]), _bits(g0[i])), NAMES[i]
            _same_bits(f"{label}, a rate of zero", dev.weights(), start)
        assert ok
    finally:
        dev.close()


def _minibatches(n_rows):
    rng = np.random.default_rng(21)
    return [rng.choice(n_rows, B, replace=False) for B in (64, 95, 33)]


def _rate_loops(tag, case, sets):
    """The float64 and float32 torch loops at tc.CRITIC_LRS, after asserting on float64 alone that a setter without effect cannot pass."""
    import torch
    train = lambda dtype, lrs: tc.critic_torch_rates(case, sets, dtype, lrs) + (None,)  # noqa: E731
    (ref, l64, _), (y32, l32, _) = train(torch.float64, tc.CRITIC_LRS), train(torch.float32, tc.CRITIC_LRS)
    _lr_is_seen(tag, ref, y32, train, tc.CRITIC_LRS)
    return ref, l64, y32, l32


def _value_params(tag, got, ref, y32, start):
    """The six value arrays after the steps, and the optimiser's effect got - start against ref - start (a rate that did not arrive shows up
    as a deviation near the distance moved); the actor's arrays as they started."""
    ok = True
    for i in VALUE:
        w0 = np.asarray(start[i], np.float64)
        ok &= _val(tag, NAMES[i], got[i], ref[i], y32[i])
        moved = float(np.abs(ref[i] - w0).max())
        tol = 4.0 * float(np.abs(y32[i] - ref[i]).max()) + 4.0 * 2.0 ** -23 * max(1.0, float(np.abs(ref[i]).max()))
        ok &= moved > 0.0 and float(np.abs((np.asarray(got[i], np.float64) - w0) - (ref[i] - w0)).max()) <= tol
    return ok


def test_set_rate_changes_the_learning_rate_of_the_next_critic_minibatch(engines):
    eng = engines["pst"]
    case, _ = tc.pst_case()
    sets = _minibatches(case["obs"].shape[0])
    ref, l64, y32, l32 = _rate_loops("trpo", case, sets)
    dev = _Trpo(eng, case, lr=tc.CRITIC_LRS[0])
    try:
        start, losses = dev.weights(), []
        for lr, ix in zip(tc.CRITIC_LRS, sets):
            eng.trpo_set_rate(dev.trpo, lr)
            losses.append(dev.critic(ix))
        got = dev.weights()
        ok = _value_params(f"EDGE RATES trpo lr {tc.CRITIC_LRS}", got, ref, y32, start)
        ok &= _val(f"EDGE RATES trpo lr {tc.CRITIC_LRS}", "value_loss of the three minibatches", losses, l64, l32)
        assert ok
        for i in ACTOR:
            assert np.array_equal(_bits(got[i]), _bits(start[i])), NAMES[i]
    finally:
        dev.close()


def test_trpolearner_set_rate_reaches_the_device():
    """TRPOLearner.set_rate before each of three train() calls of one critic minibatch each: the value arrays read back through state_dict()
    against the torch loop with the same rate per step (the policy steps in between touch the actor's arrays only)."""
    from ev2gym_amd.onpolicy import OnPolicyCollector
    from ev2gym_amd.trpo import TRPOLearner
    big, pol, start = _policy_behind_a_collector()
    try:
        col = OnPolicyCollector(big, pol, n_steps=5)
        batch = col.collect().clone()
        sets = _minibatches(5 * big.E)
        learner = TRPOLearner(col, learning_rate=tc.CRITIC_LRS[0], cg_max_steps=3)
        for lr, ix in zip(tc.CRITIC_LRS, sets):
            learner.set_rate(lr)
            learner.train(batch, minibatches=[ix])
        case = _collected_case(pol, batch, start[:12], start[12])
        ref, _, y32, _ = _rate_loops("TRPOLearner", case, sets)
        assert learner.lr == tc.CRITIC_LRS[-1]
        assert _value_params(f"EDGE RATES TRPOLearner lr {tc.CRITIC_LRS}", _state(learner), ref, y32, start)
    finally:
        pol.close()
        big.close()


# ---- 7. replaced weights under a bound learner; train() on given and on sub-sampled rows ----
def test_replaced_weights_reach_a_bound_trpo_learner_like_a_fresh_one(engines):
    """ev2g_ac_set_weights / ev2g_ac_set_log_std under a bound TRPO learner (masters, images, transposed images): a policy step and a critic
    minibatch are those of a learner created on a policy that had the arrays from the start.  The network pads every dimension."""
    eng = engines["pst"]
    new = tc.net_case("pst-odd")
    D, P, h, v = new["D"], new["P"], new["h"], new["v"]
    old = make_case(D, P, h=h, v=v, n_rows=8, seed=8)
    idx = tc.step_rows(new, 97)
    moved, fresh = _Trpo(eng, dict(new, weights=old["weights"], log_std=old["log_std"]), **tc.NET_CFG), _Trpo(eng, new, **tc.NET_CFG)
    try:
        assert all((_bits(a) != _bits(b)).any() for a, b in zip(moved.weights(), fresh.weights()))
        eng.ac_set_weights(moved.pol.ac, new["weights"])
        eng.ac_set_log_std(moved.pol.ac, new["log_std"])
        _same_bits("the masters after set_weights / set_log_std", moved.weights(), fresh.weights())
        one, two = _stepped(moved, idx), _stepped(fresh, idx)
        assert two[0]["accepted"] and np.isfinite(two[1]).all()
        _same_step("the policy step", one, two)
        vl = [d.critic(idx) for d in (moved, fresh)]
        assert np.isfinite(vl[1]) and np.array_equal(_bits(np.float32(vl[0])), _bits(np.float32(vl[1])))
        after = fresh.weights()
        assert all((_bits(after[i]) != _bits(two[3][i])).any() for i in VALUE), "the minibatch moved every value array"
        _same_bits("the masters after the critic minibatch", moved.weights(), after)
        a, b = _means(eng, new, (moved.pol.ac, fresh.pol.ac))
        assert np.array_equal(_bits(a), _bits(b))
    finally:
        moved.close()
        fresh.close()


@pytest.mark.parametrize("how", ["policy_rows", "sub_sampling_factor"])
def test_train_steps_over_exactly_the_rows_it_is_given(how):
    """TRPOLearner.train(batch, policy_rows=an odd number of rows), and sub_sampling_factor 2 with explicit minibatches (the generator is then
    used once: the rows are randperm(N)[::2] of a second generator with the same seed on the same device): the report and the actor's arrays
    against the reference over exactly those rows."""
    import torch
    from ev2gym_amd.onpolicy import OnPolicyCollector
    from ev2gym_amd.trpo import TRPOLearner
    big, pol, start = _policy_behind_a_collector()
    try:
        col = OnPolicyCollector(big, pol, n_steps=5)
        batch = col.collect().clone()
        N = 5 * big.E
        pieces = [np.random.default_rng(3).choice(N, 64, replace=False)]
        if how == "policy_rows":
            learner = TRPOLearner(col, **tc.NET_CFG)
            rows = np.random.default_rng(2).choice(N, 77, replace=False)
            stats = learner.train(batch, policy_rows=rows, minibatches=pieces)
        else:
            learner = TRPOLearner(col, sub_sampling_factor=2, seed=4, **tc.NET_CFG)
            again = torch.Generator(device=learner.device)
            again.manual_seed(4)
            rows = torch.randperm(N, generator=again, device=learner.device)[::2].cpu().numpy()
            assert len(rows) == (N + 1) // 2 and len(set(rows.tolist())) == len(rows)
            stats = learner.train(batch, minibatches=pieces)
        case = _collected_case(pol, batch, start[:12], start[12])
        ref, y32 = trpo_reference(case, rows, **tc.NET_CFG), TorchTrpo(case, rows, torch.float32).step(**tc.NET_CFG)
        tag = f"EDGE TRAIN {how} {len(rows)} rows"
        _margins(tag, ref, y32, 0.01)
        # a step over every row is another step, a hundred tolerances away in some array: a learner that ignored the rows cannot pass
        every = trpo_reference(case, np.arange(N), **tc.NET_CFG)
        far = max(float(np.abs(e - r).max()) / float(value_tol(r, float(np.abs(y - r).max())).max()) for e, r, y in zip(every["params"], ref["params"], y32["params"]))
        _record(f"TRPO {tag}: the reference over every row ends {far:.1f} tolerances from the one over the rows given")
        assert far >= 100.0
        rep = learner.last_report
        assert stats["is_line_search_success"] == ref["accepted"] and stats["line_search_tries"] == ref["line_search_tries"]
        assert stats["cg_iterations"] == ref["cg_iterations"] and np.isfinite(stats["value_loss"])
        ok = _val(tag, "policy_objective", stats["policy_objective"], ref["objective_before"], y32["objective_before"])
        ok &= _val(tag, "kl_divergence_loss", stats["kl_divergence_loss"], ref["kl"] if ref["accepted"] else 0.0, y32["kl"] if y32["accepted"] else 0.0)
        ok &= _val(tag, "beta", rep["beta"], ref["beta"], y32["beta"]) & _val(tag, "x.Hx", rep["xHx"], ref["xHx"], y32["xHx"])
        got = _state(learner)
        for k, i in enumerate(ACTOR):
            ok &= _val(tag, NAMES[i], got[i], ref["params"][k], y32["params"][k])
        assert ok
    finally:
        pol.close()
        big.close()
