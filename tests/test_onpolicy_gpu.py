"""The on-policy collector on the device (csrc/ev2g_ac.h; ev2g_ac_*, ev2g_gae; ev2gym_amd/onpolicy.py): the Gaussian actor-critic's forward
against a float64 numpy forward, row independence, the sample and its log-probability against the host twin of the noise, the step that consumed
the clipped action against a twin engine, the launch counter, GAE against its host twin, the RolloutBuffer-shaped collector across an episode end,
and every refusal.

Engines: the single-env PublicPST and V2G_profit_max_loads fixtures of tests/golden (both on ev2g_step_wave), and generated pools of 37 envs with
12-step episodes.  Forward tolerance, per case: d32 = the largest deviation of a torch-CPU float32 forward from the float64 forward on the same
rows (the reference stack's own rounding); the device gets 4 d32 + 4 * 2^-23 * max(1, |y|) -- the margin covers another summation order and a
tanh that differs by a few ulp.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_golden
from tests.test_onpolicy_cpu import _gae_case

pytestmark = pytest.mark.gpu

ARG, DONE = -1, -4
EPS32 = 2.0 ** -23
T_SHORT = 12
E_GEN = 37
FIXTURES = {"pst": ("pst_rand_s2", 0.0), "ppl": ("v2gppl_rand_s2", -1.0)}   # name, lower edge of the action box


def _fixture_engine(kind):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    _, batch, rk, sk = load_golden(os.path.join(GOLDEN_DIR, FIXTURES[kind][0] + ".npz"))
    eng = Engine(batch, rk, sk, device=0, flags=_abi.FLAG_LOG_SOC)
    assert eng.kernel_name.startswith("ev2g_step_wave")
    return eng


def _gen_engine(kind, pool=1):
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    if kind == "pst":
        cfg, kinds = GenConfig.public_pst(E_GEN * pool, 20, seed=31, spawn_multiplier=10, simulation_length=T_SHORT), ("SquaredTrackingErrorReward", "PublicPST")
    else:
        cfg, kinds = GenConfig.v2g_profit_plus_loads(E_GEN * pool, 30, 1, seed=32, simulation_length=T_SHORT), ("ProfitMax_TrPenalty_UserIncentives", "V2G_profit_max_loads")
    eng = Engine(generate_native(cfg), _abi.REWARD_KINDS[kinds[0]], _abi.STATE_KINDS[kinds[1]], device=0, flags=_abi.FLAG_LOG_SOC, n_active_envs=E_GEN)
    assert (eng.E, eng.T) == (E_GEN, T_SHORT)
    return eng


@pytest.fixture(scope="module")
def fixture_engines():
    engs = {k: _fixture_engine(k) for k in FIXTURES}
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def gen_eng():
    eng = _gen_engine("pst")
    yield eng
    eng.close()


def _record(line):
    """A figure of this run: printed, and appended to the file EV2G_ONPOLICY_RECORD names when it is set (how the numerics part of
    profiles/r14_onpolicy.txt is taken; an ordinary run of the suite writes nothing into the tree)."""
    print(line)
    path = os.environ.get("EV2G_ONPOLICY_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def _up(eng, arr):
    arr = np.ascontiguousarray(arr)
    return eng.empty(arr.shape, arr.dtype).upload(arr)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _policy(eng, D, P, h=(64, 64), v=(64, 64), activation="tanh", lo=-1.0, log_std=None, seed=3, noise_seed=5):
    from ev2gym_amd.onpolicy import GaussianActorCritic, init_ac_weights
    ls = np.zeros(P, np.float32) if log_std is None else log_std
    return GaussianActorCritic(init_ac_weights(D, P, seed=seed, h=h, v=v), ls, activation=activation, lo=lo, seed=noise_seed).attach(eng)


def _torch32(x, w, activation):
    import torch
    F = torch.nn.functional
    act = torch.tanh if activation == "tanh" else torch.relu
    t = [torch.from_numpy(a) for a in w]
    X = torch.from_numpy(x)
    with torch.no_grad():
        hp = act(F.linear(act(F.linear(X, t[0], t[1])), t[2], t[3]))
        hv = act(F.linear(act(F.linear(X, t[4], t[5])), t[6], t[7]))
        return F.linear(hp, t[8], t[9]).numpy(), F.linear(hv, t[10], t[11]).numpy()[:, 0]


def _forward_tol(x, pol):
    """(mean_ref, value_ref, tol_mean, tol_value, d32) of rows x: the float64 forward and the tolerance of the module docstring"""
    mean64, value64 = pol.forward_numpy(x)
    mean32, value32 = _torch32(x, pol.weights, pol.activation)
    d32 = max(float(np.abs(mean32 - mean64).max()), float(np.abs(value32 - value64).max()))
    tol = lambda y: 4.0 * d32 + 4.0 * EPS32 * np.maximum(1.0, np.abs(y))  # noqa: E731
    return mean64, value64, tol(mean64), tol(value64), d32


def _device_forward(eng, pol, x):
    n = x.shape[0]
    dx, dm, dv = _up(eng, x), eng.empty((n, pol.d_out), np.float32), eng.empty((n,), np.float32)
    eng.ac_forward(pol.ac, dx, n, mean=dm, value=dv)
    eng.synchronize()
    out = dm.to_host(), dv.to_host()
    for b in (dx, dm, dv):
        b.free()
    return out


# ---- forward ----
NETWORKS = [("pst", None), ("ppl", None), ("tiny", (5, 8, 8, 1)), ("odd", (63, 48, 72, 20)), ("max", (192, 256, 256, 64))]


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("net,shape", NETWORKS, ids=[n for n, _ in NETWORKS])
def test_forward_matches_the_float64_forward(fixture_engines, net, shape, activation):
    eng = fixture_engines[net] if shape is None else fixture_engines["pst"]
    D, h1, h2, P = (eng.D, 64, 64, eng.P) if shape is None else shape
    pol = _policy(eng, D, P, h=(h1, h2), v=(h2, h1), activation=activation)
    x_all = np.random.default_rng(D * 7 + P).normal(size=(200, D)).astype(np.float32)
    try:
        for n in (1, 37, 200):
            x = x_all[:n]
            mean64, value64, tol_m, tol_v, d32 = _forward_tol(x, pol)
            mean, value = _device_forward(eng, pol, x)
            dm, dv = np.abs(mean - mean64), np.abs(value - value64)
            _record(f"FORWARD {net} {D}->{h1}->{h2}->{P} {activation} rows {n}: d32 {d32:.3e}  |mean - f64| {dm.max():.3e} (tol {tol_m.min():.3e})  "
                    f"|value - f64| {dv.max():.3e} (tol {tol_v.min():.3e})")
            assert np.isfinite(mean).all() and np.isfinite(value).all()
            assert (dm <= tol_m).all() and (dv <= tol_v).all()
    finally:
        pol.close()


# ---- row independence ----
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_a_rows_results_do_not_depend_on_the_launch(fixture_engines, activation):
    eng = fixture_engines["ppl"]
    D, P, n = eng.D, eng.P, 70
    rng = np.random.default_rng(4)
    pol = _policy(eng, D, P, activation=activation, log_std=rng.uniform(-1, 0, P).astype(np.float32))
    x = rng.normal(size=(n, D)).astype(np.float32)
    perm = rng.permutation(n)
    try:
        mean, value = _device_forward(eng, pol, x)
        mean_p, value_p = _device_forward(eng, pol, x[perm])
        assert np.array_equal(_bits(mean_p), _bits(mean[perm])) and np.array_equal(_bits(value_p), _bits(value[perm]))
        for i in (0, 31, 32, 45, 69):   # alone: row 0 of a one-row launch
            m1, v1 = _device_forward(eng, pol, x[i:i + 1])
            assert np.array_equal(_bits(m1[0]), _bits(mean[i])) and np.array_equal(_bits(v1), _bits(value[i:i + 1])), i
        # the sampling launch's value is the forward launch's, and its deterministic action is the mean
        dx = _up(eng, x)
        da, dc, dv, dl = eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n,), np.float32), eng.empty((n,), np.float32)
        for det in (False, True):
            eng.ac_act(pol.ac, dx, n, actions=da, clipped=dc, value=dv, log_prob=dl, deterministic=det)
            eng.synchronize()
            assert np.array_equal(_bits(dv.to_host()), _bits(value)), det
            if det:
                assert np.array_equal(_bits(da.to_host()), _bits(mean))
    finally:
        pol.close()


# ---- sampling ----
@pytest.mark.parametrize("kind", ["pst", "ppl"])
def test_sample_and_log_prob_against_the_host_noise(fixture_engines, kind):
    from ev2gym_amd.engine import host_normal
    from ev2gym_amd.onpolicy import log_prob_numpy
    eng, lo = fixture_engines[kind], FIXTURES[kind][1]
    D, P, n, seed, first = eng.D, eng.P, 37, 11, 3
    rng = np.random.default_rng(8)
    log_std = rng.uniform(-1.0, 0.0, P).astype(np.float32)
    pol = _policy(eng, D, P, lo=lo, log_std=log_std)
    x = rng.normal(size=(n, D)).astype(np.float32)
    mean64, _, tol_m, _, d32 = _forward_tol(x, pol)
    sigma = np.exp(log_std.astype(np.float64))
    dx = _up(eng, x)
    da, dc, dv, dl = eng.empty((n, P), np.float32), eng.empty((n, P), np.float32), eng.empty((n,), np.float32), eng.empty((n,), np.float32)
    try:
        eng.ac_seed(pol.ac, seed, first)
        eng.ac_act(pol.ac, dx, n, actions=da, clipped=dc, value=dv, log_prob=dl)
        eng.synchronize()
        a, c, lp = da.to_host(), dc.to_host(), dl.to_host()
        noise = sigma * host_normal(n * P, seed, first * n * P).astype(np.float64).reshape(n, P)   # draw (first * n + e) * P + p
        err = np.abs(a - (mean64 + noise))
        bound = tol_m + 4.0 * EPS32 * np.abs(noise)
        _record(f"SAMPLE {kind}: |a - (mean_ref + sigma eps_host)| max {err.max():.3e}, smallest margin {(bound - err).min():.3e}")
        assert (err <= bound).all()
        assert np.abs(noise).max() > 1.0   # (noise was added)
        assert np.array_equal(_bits(c), _bits(np.clip(a, np.float32(lo), np.float32(1.0))))
        lp64 = log_prob_numpy(a, mean64, log_std)
        lp_bound = (np.abs(a - mean64) / sigma ** 2 * tol_m).sum(axis=1) + P * 2.0 ** -20
        lp_err = np.abs(lp - lp64)
        _record(f"LOGPROB {kind}: |log_prob - f64| max {lp_err.max():.3e}, smallest bound {lp_bound.min():.3e}")
        assert (lp_err <= lp_bound).all()
        # deterministic: the mean itself, and the density at the mode
        dm = eng.empty((n, P), np.float32)
        eng.ac_forward(pol.ac, dx, n, mean=dm)
        eng.ac_act(pol.ac, dx, n, actions=da, clipped=dc, value=dv, log_prob=dl, deterministic=True)
        eng.synchronize()
        assert np.array_equal(_bits(da.to_host()), _bits(dm.to_host()))
        mode = float((-log_std.astype(np.float64) - 0.5 * np.log(2.0 * np.pi)).sum())
        lp_det = dl.to_host()
        _record(f"DETERMINISTIC {kind}: log_prob {lp_det[0]!r} vs {mode!r}")
        assert (np.abs(lp_det - mode) <= np.spacing(np.float32(abs(mode)))).all()
    finally:
        pol.close()


# ---- the step consumed the clipped action ----
class Rows:
    def __init__(self, eng, k):
        E, D, P = eng.E, eng.D, eng.P
        self.eng, self.k = eng, k
        self.obs, self.act = eng.empty((k + 1, E, D), np.float32), eng.empty((k, E, P), np.float32)
        self.val, self.lp = eng.empty((k, E), np.float32), eng.empty((k, E), np.float32)
        self.rew, self.done, self.mask = eng.empty((k, E)), eng.empty((k, E), np.uint8), eng.empty((k, E, P), np.uint8)

    def collect(self, pol, k=None, first=0, **kw):
        """k steps whose rows start at row `first` of the blocks"""
        eng, (E, D, P) = self.eng, (self.eng.E, self.eng.D, self.eng.P)
        eng.ac_collect(pol.ac, self.k if k is None else k, self.obs.at(first * E * D), self.act.at(first * E * P), self.val.at(first * E),
                       self.lp.at(first * E), self.rew.at(first * E), self.done.at(first * E), self.mask.at(first * E * P), **kw)

    def host(self):
        self.eng.synchronize()
        return {n: getattr(self, n).to_host() for n in ("obs", "act", "val", "lp", "rew", "done", "mask")}


def _same_rows(a, b, k=None):
    """every block of two segments bit for bit; k: their first k steps only (the blocks are longer than the segment)"""
    cut = lambda n, x: x if k is None else x[:k + 1 if n == "obs" else k]  # noqa: E731
    return all(np.array_equal(_bits(cut(n, a[n])), _bits(cut(n, b[n]))) for n in a)


T0 = 24   # the fixtures' first EVs arrive at steps 9 .. 22: the segments start where ports are occupied and rewards are not zero


def _advance(eng, rows=None):
    """A fresh episode stepped T0 steps on the constant action 0.5 through a float32 hand-over pair (cleared again); the observation of step
    T0 goes to row 0 of `rows` and is returned."""
    E, D, P = eng.E, eng.D, eng.P
    o, a = eng.empty((E, D), np.float32), _up(eng, np.full((E, P), 0.5, np.float32))
    rew, done, mask = eng.empty((E,)), eng.empty((E,), np.uint8), eng.empty((E, P), np.uint8)
    eng.set_extras(obs_f32=o, actions_f32=a)
    eng.reset_f32(o, 0)
    eng.step_n(T0, None, 0, None, 0, rew, 0, done, 0, mask, 0, auto_reset=False, persistent=False)
    eng.synchronize()
    row = o.to_host()
    eng.set_extras()
    assert eng.current_step == T0 and mask.to_host().any()
    if rows is not None:
        eng._check(eng._lib.ev2g_memcpy_h2d(eng._h, rows.obs.ptr, row.ctypes.data, row.nbytes))
    return row


@pytest.mark.parametrize("kind", ["pst", "ppl"])
def test_collect_steps_on_the_clipped_action(fixture_engines, kind):
    eng, lo = fixture_engines[kind], FIXTURES[kind][1]
    E, D, P, k = eng.E, eng.D, eng.P, 6
    pol = _policy(eng, D, P, lo=lo, log_std=np.full(P, 0.5, np.float32), noise_seed=21)   # sigma 1.65: many samples leave the box
    twin = _fixture_engine(kind)
    rows = Rows(eng, k)
    try:
        _advance(eng, rows)
        rows.collect(pol)
        r = rows.host()
        assert eng.current_step == T0 + k and eng.last_launch_specialisation > 0   # (the per-launch float32 rows of the fast path)
        clipped = np.clip(r["act"], np.float32(lo), np.float32(1.0))
        n_clipped = int((clipped != r["act"]).sum())
        _record(f"COLLECT {kind}: {n_clipped} of {r['act'].size} actions clipped")
        assert n_clipped > 0 and (clipped == r["act"]).any()
        # the twin: the same scenarios stepped on clip(actions, lo, 1) through the registered float32 hand-over
        x_obs, x_act = twin.empty((E, D), np.float32), twin.empty((E, P), np.float32)
        rew, done, mask = twin.empty((E,)), twin.empty((E,), np.uint8), twin.empty((E, P), np.uint8)
        assert np.array_equal(_bits(_advance(twin)), _bits(r["obs"][0]))
        twin.set_extras(obs_f32=x_obs, actions_f32=x_act)
        for i in range(k):
            x_act.upload(clipped[i])
            twin.step_n(1, None, 0, None, 0, rew, 0, done, 0, mask, 0, auto_reset=False, persistent=False)
            twin.synchronize()
            assert np.array_equal(_bits(x_obs.to_host()), _bits(r["obs"][i + 1])), i
            assert np.array_equal(_bits(rew.to_host()), _bits(r["rew"][i])) and np.array_equal(done.to_host(), r["done"][i]), i
            assert np.array_equal(mask.to_host(), r["mask"][i]), i
        assert np.abs(r["rew"]).max() > 0 and r["mask"].any()
        # values and log-probabilities are those of the observation rows the steps wrote
        mean, value = _device_forward(eng, pol, r["obs"][:k].reshape(k * E, D))
        assert np.array_equal(_bits(value.reshape(k, E)), _bits(r["val"]))
        from ev2gym_amd.onpolicy import log_prob_numpy
        assert np.allclose(r["lp"], log_prob_numpy(r["act"], mean.reshape(k, E, P), pol.log_std), rtol=0, atol=P * 2.0 ** -20)
        # the other route: the registered hand-over pair with device-to-device copies gives the same rows
        h_obs, h_act = eng.empty((E, D), np.float32), eng.empty((E, P), np.float32)
        _advance(eng, rows)
        eng.set_extras(obs_f32=h_obs, actions_f32=h_act)
        eng.ac_seed(pol.ac, 21, 0)
        rows.collect(pol)
        assert _same_rows(rows.host(), r)
        eng.set_extras()
    finally:
        pol.close()
        twin.close()


# ---- the launch counter ----
def test_segments_continue_the_noise_stream(gen_eng):
    eng = gen_eng
    pol = _policy(eng, eng.D, eng.P, lo=0.0, log_std=np.full(eng.P, -0.5, np.float32), noise_seed=7)
    whole, parts = Rows(eng, 7), Rows(eng, 7)
    try:
        eng.reset_f32(whole.obs, 0)
        whole.collect(pol)
        w = whole.host()
        eng.reset_f32(parts.obs, 0)
        eng.ac_seed(pol.ac, 7, 0)   # back to the start of the stream
        parts.collect(pol, 3)
        parts.collect(pol, 4, first=3)
        assert _same_rows(parts.host(), w)
        eng.reset_f32(parts.obs, 0)
        eng.ac_seed(pol.ac, 8, 0)
        parts.collect(pol)
        other = parts.host()
        assert not np.array_equal(other["act"], w["act"]) and np.array_equal(_bits(other["obs"][0]), _bits(w["obs"][0]))
        # the counter alone: the same seed from launch 2 on gives rows 2.. of the noise, so another first row
        eng.reset_f32(parts.obs, 0)
        eng.ac_seed(pol.ac, 7, 2)
        parts.collect(pol, 1)
        assert not np.array_equal(parts.host()["act"][0], w["act"][0])
        # deterministic segments draw nothing and leave the counter where it was
        eng.reset_f32(parts.obs, 0)
        eng.ac_seed(pol.ac, 7, 0)
        parts.collect(pol, 2, deterministic=True)
        eng.reset_f32(parts.obs, 0)
        parts.collect(pol)
        assert _same_rows(parts.host(), w)
    finally:
        pol.close()


# ---- GAE ----
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
@pytest.mark.parametrize("k", [1, 7])
def test_device_gae_equals_the_host_twin_bit_for_bit(gen_eng, k, gamma, lam):
    from ev2gym_amd.engine import host_gae
    eng = gen_eng
    case = _gae_case(k, 200 + k)
    bufs = [_up(eng, a) for a in case]
    adv, ret = eng.empty((k, E_GEN), np.float32), eng.empty((k, E_GEN), np.float32)
    eng.gae(*bufs, k, E_GEN, gamma, lam, adv, ret)
    eng.synchronize()
    adv_h, ret_h = host_gae(*case, gamma, lam)
    assert np.array_equal(_bits(adv.to_host()), _bits(adv_h)) and np.array_equal(_bits(ret.to_host()), _bits(ret_h))
    for b in bufs + [adv, ret]:
        b.free()


# ---- the collector ----
def test_collector_crosses_an_episode_end():
    import torch
    from ev2gym_amd.onpolicy import OnPolicyCollector, gae_numpy
    eng, twin = _gen_engine("pst", pool=2), _gen_engine("pst", pool=2)
    pol = _policy(eng, eng.D, eng.P, lo=0.0, log_std=np.full(eng.P, -0.5, np.float32))
    n, T, E = T_SHORT + 5, T_SHORT, E_GEN
    try:
        col = OnPolicyCollector(eng, pol, n, gamma=0.99, gae_lambda=0.95)
        col.last_episode_stats.fill_(-7.0)
        b = col.collect()
        for f in b.FIELDS:
            t = b[f]
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape[:2]) == (n, E), f
        assert b.observations.shape == (n, E, eng.D) and b.actions.shape == (n, E, eng.P)
        starts = b.episode_starts.cpu().numpy()
        want = np.zeros((n, E), np.float32)
        want[0], want[T] = 1, 1
        assert np.array_equal(starts, want)
        assert col.episodes == 1 and eng.current_step == 5 and eng.scenario_offset == E
        assert b.dones.cpu().numpy()[T - 1].all() and not b.dones.cpu().numpy()[:T - 1].any() and not b.dones.cpu().numpy()[T:].any()
        # the new episode's first observation is the reset observation of the window the collector moved to
        reset_obs = twin.empty((E, eng.D), np.float32)
        twin.reset_f32(reset_obs, E)
        twin.synchronize()
        assert np.array_equal(_bits(b.observations[T].cpu().numpy()), _bits(reset_obs.to_host()))
        twin.reset_f32(reset_obs, 0)
        twin.synchronize()
        assert np.array_equal(_bits(b.observations[0].cpu().numpy()), _bits(reset_obs.to_host()))
        # the statistics of the finished episode were taken
        stats = col.last_episode_stats.cpu().numpy()
        assert not (stats == -7.0).any() and np.isfinite(stats[:, 0]).all()
        # advantages: the numpy twin on the returned tensors, bootstrapped with the value of the row behind the buffer
        last_v = np.empty(E, np.float32)
        _, v = _device_forward(eng, pol, b.all_observations[n].cpu().numpy())
        last_v[:] = v
        assert np.array_equal(_bits(col.last_values.cpu().numpy()), _bits(last_v))
        adv, ret = gae_numpy(col.reward.cpu().numpy(), b.values.cpu().numpy(), starts, last_v, np.zeros(E, np.uint8), 0.99, 0.95)
        assert np.array_equal(_bits(b.advantages.cpu().numpy()), _bits(adv)) and np.array_equal(_bits(b.returns.cpu().numpy()), _bits(ret))
        assert np.array_equal(b.rewards.cpu().numpy(), col.reward.cpu().numpy().astype(np.float32))
        assert np.abs(adv).max() > 0 and np.abs(b.log_probs.cpu().numpy()).max() > 0
        # the next buffer goes on from the last observation, inside the running episode
        last_obs = b.all_observations[n].cpu().numpy().copy()
        b2 = col.collect()
        assert np.array_equal(_bits(b2.observations[0].cpu().numpy()), _bits(last_obs))
        starts2 = b2.episode_starts.cpu().numpy()
        assert not starts2[0].any() and starts2[T - 5].all() and starts2.sum() == E
    finally:
        pol.close()
        eng.close()
        twin.close()


# ---- refusals ----
def _raises(eng, code, *words):
    from ev2gym_amd.engine import EngineError

    class Ctx:
        def __enter__(self):
            return self

        def __exit__(self, et, ev, tb):
            assert et is EngineError, f"expected EngineError {code}, got {et}"
            assert ev.code == code, (ev.code, str(ev))
            for w in words:
                assert w in str(ev), (w, str(ev))
            return True
    return Ctx()


def test_refusals_leave_the_handle_usable(gen_eng):
    from ev2gym_amd.onpolicy import init_ac_weights
    eng = gen_eng
    D, P = eng.D, eng.P
    ls = np.zeros(P, np.float32)
    pol = _policy(eng, D, P, lo=0.0, log_std=np.full(P, -0.5, np.float32), noise_seed=7)
    rows, again = Rows(eng, T_SHORT + 1), Rows(eng, T_SHORT + 1)
    try:
        eng.reset_f32(rows.obs, 0)
        rows.collect(pol, 4)
        good = rows.host()
        # a segment past the episode end
        eng.reset_f32(again.obs, 0)
        with _raises(eng, DONE, "ev2g_ac_collect", "past the episode end"):
            again.collect(pol, T_SHORT + 1)
        assert eng.current_step == 0
        # actor shape != (D, P)
        wide = _policy(eng, D, P + 1)
        with _raises(eng, ARG, "d_out", str(P + 1)):
            again.collect(wide, 2)
        wide.close()
        narrow = _policy(eng, D - 1, P)
        with _raises(eng, ARG, "d_in", str(D - 1)):
            again.collect(narrow, 2)
        narrow.close()
        # shapes outside the range, settings
        with _raises(eng, ARG, "ev2g_ac_create", "d_in", "192"):
            eng.ac_create(init_ac_weights(193, P), ls)
        with _raises(eng, ARG, "ev2g_ac_create", "v2", "256"):
            eng.ac_create(init_ac_weights(D, P, v=(64, 257)), ls)
        with _raises(eng, ARG, "ev2g_ac_create", "d_out", "64"):
            eng.ac_create(init_ac_weights(D, 65), np.zeros(65, np.float32))
        bad = ls.copy()
        bad[1] = np.nan
        with _raises(eng, ARG, "ev2g_ac_create", "log_std[1]", "not finite"):
            eng.ac_create(init_ac_weights(D, P), bad)
        with _raises(eng, ARG, "activation"):
            eng.ac_create(init_ac_weights(D, P), ls, activation=7)
        with _raises(eng, ARG, "lo must be -1 or 0"):
            eng.ac_create(init_ac_weights(D, P), ls, lo=0.5)
        with _raises(eng, ARG, "ev2g_ac_set_log_std", "log_std[1]"):
            eng.ac_set_log_std(pol.ac, bad)
        # together with a link: ev2g_ac_collect takes none -- there is no argument to stack one through, and the chain refuses the pair
        # internally -- and a link that lives on the handle is neither applied nor touched: the rows are those without it
        link = eng.link_create(1.0, 0.0, seed_act=5)   # (p_fail 1: applied, it would hold every command at zero)
        eng.ac_seed(pol.ac, 7, 0)
        again.collect(pol, 4)
        assert _same_rows(again.host(), good, 4)
        eng.link_destroy(link)
        eng.reset_f32(again.obs, 0)
        # a policy of another handle
        far = _gen_engine("pst")
        far_pol = _policy(far, D, P, lo=0.0)
        with _raises(eng, ARG, "not created on this handle"):
            again.collect(far_pol, 2)
        far_pol.close()
        far.close()
        # the handle and the policy are as they were: the first segment again, bit for bit
        assert eng.current_step == 0
        eng.ac_seed(pol.ac, 7, 0)
        again.collect(pol, 4)
        assert _same_rows(again.host(), good, 4)
    finally:
        pol.close()


# ---- through an EV2GymVec ----
def test_collector_drives_a_vec_envs_engine():
    """OnPolicyCollector(vec, ...) as INTEGRATION.md has it: the vec's armed episode is taken over, the next window comes from the vec's own
    order and is noted in the vec, and the vec's gym surface works again after its reset(); what the chain does not apply is refused."""
    from ev2gym_amd.onpolicy import GaussianActorCritic, OnPolicyCollector, init_ac_weights
    from ev2gym_amd.scenario_gen import GenConfig, generate_native
    from ev2gym_amd.vec_env import EV2GymVec
    pool = generate_native(GenConfig.public_pst(E_GEN * 3, 20, seed=31, spawn_multiplier=10, simulation_length=T_SHORT))
    kw = dict(scenarios=pool, num_envs=E_GEN, state_function="PublicPST", reward_function="SquaredTrackingErrorReward", seed=3)
    vec, twin = EV2GymVec(**kw), _gen_engine("pst", pool=3)
    eng = vec.engine
    n, T = T_SHORT + 5, T_SHORT
    pol = GaussianActorCritic(init_ac_weights(eng.D, eng.P, seed=3), np.full(eng.P, -0.5, np.float32), lo=0.0, seed=5)
    try:
        first = eng.scenario_offset
        col = OnPolicyCollector(vec, pol, n)
        b = col.collect()
        second = eng.scenario_offset
        assert vec._last_offset == second and eng.current_step == 5 and col.episodes == 1
        reset_obs = twin.empty((E_GEN, eng.D), np.float32)
        for row, off in ((0, first), (T, second)):
            twin.reset_f32(reset_obs, off)
            twin.synchronize()
            assert np.array_equal(_bits(b.observations[row].cpu().numpy()), _bits(reset_obs.to_host())), row
        assert b.episode_starts.cpu().numpy().sum() == 2 * E_GEN
        kept = b.clone()
        before = kept.actions.cpu().numpy().copy()
        b2 = col.collect()
        assert b2.actions.data_ptr() == b.actions.data_ptr() and np.array_equal(kept.actions.cpu().numpy(), before)   # views, and the clone
        # back to the gym surface: the vec's reset draws a window other than the one the collector ran last
        obs, _ = vec.reset()
        assert eng.current_step == 0 and eng.scenario_offset == vec._last_offset
        out = vec.step(vec.full_like_actions(0.5))
        assert eng.current_step == 1 and np.isfinite(np.asarray(out[1].cpu() if hasattr(out[1], "cpu") else out[1])).all()
        costly = EV2GymVec(cost_function="ProfitMax_TrPenalty_UserIncentives_safety", **kw)
        try:
            with pytest.raises(ValueError, match="cost function"):
                OnPolicyCollector(costly, pol, n)
        finally:
            costly.close()
    finally:
        pol.close()
        vec.close()
        twin.close()
