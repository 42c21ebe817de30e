"""One policy per kind of plan (csrc/ev2g_policy_host.h: plan_mlp): the actor kernel ev2g_mlp_kernel_name reports is the one the plan's rules
give the shape, and one ev2g_mlp_forward on it agrees with the reference forward of its precision.  37 rows: a ragged last tile for 16- and
32-row workgroups alike."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 37
S16_WIDE, S16_NARROW = "ev2g_mlp3_s16<6,25,19,4,%d,%d>", "ev2g_mlp3_s16<2,25,19,2,%d,%d>"
CASES = [
    # the streaming kernel, both shapes, all three precisions (terms per weight, wavefronts per workgroup)
    ((162, 400, 300, 50), "bf16", S16_WIDE % (1, 8)), ((162, 400, 300, 50), "fp32", S16_WIDE % (2, 4)), ((162, 400, 300, 50), "fp32x3", S16_WIDE % (3, 4)),
    ((63, 400, 300, 20), "bf16", S16_NARROW % (1, 8)), ((63, 400, 300, 20), "fp32", S16_NARROW % (2, 4)), ((63, 400, 300, 20), "fp32x3", S16_NARROW % (3, 4)),
    # small (both hidden layers under 128), and wider than the fixed kernels unroll for
    ((17, 40, 70, 3), "bf16", "ev2g_mlp3_any"), ((20, 520, 64, 5), "bf16", "ev2g_mlp3_any"),
    ((17, 40, 70, 3), "fp32", "ev2g_mlp3_f32"),
    # a first hidden layer of 401..416 misses the streaming kernel and pads to the fixed kernels' 26 tiles of 16
    ((170, 410, 300, 50), "bf16", "ev2g_mlp3_fixed<11,26,20>"), ((63, 410, 300, 20), "bf16", "ev2g_mlp3_fixed<4,26,20>"),
]


@pytest.fixture(scope="module")
def eng():
    from ev2gym_amd import _abi
    from ev2gym_amd.engine import Engine
    from ev2gym_amd.scenario_gen import GenConfig, generate
    e = Engine(generate(GenConfig.v2g_profit_plus_loads(8, 50, 1, seed=1)), _abi.REWARD_KINDS["ProfitMax_TrPenalty_UserIncentives"],
               _abi.STATE_KINDS["V2G_profit_max_loads"], device=0)
    yield e
    e.close()


@pytest.mark.parametrize("shape,prec,kernel", CASES, ids=["-".join(map(str, c[0])) + "-" + c[1] for c in CASES])
def test_policy_runs_the_kernel_its_plan_names(eng, shape, prec, kernel):
    """ev2g_mlp_kernel_name is the instantiation the plan's rules give (shape, precision), and a forward of 37 rows on it agrees with the
    precision's reference: the bf16-rounded numpy forward to 3e-3, the float64 forward to 1e-5 (fp32) / 1e-6 (fp32x3); rows behind the batch
    stay untouched."""
    from ev2gym_amd.actor import init_mlp_weights, mlp_forward_numpy
    d_in, h1, h2, d_out = shape
    rng = np.random.default_rng(d_in * 7 + h1)
    w = init_mlp_weights(d_in, d_out, seed=5, h1=h1, h2=h2)
    x = (rng.normal(0, 1, (N_ROWS, d_in)) * rng.uniform(0.1, 3.0, d_in)).astype(np.float32)
    m = eng.mlp_create(*w, out_lo=-1.0, precision=prec)
    name = eng.mlp_kernel_name(m)
    if prec == "bf16" and "s16" in kernel:   # large batches run the 32-row variant of the same shape
        first, _, rest = name.partition("; from ")
        rows, _, big = rest.partition(" rows ")
        assert first == kernel and int(rows) > 16 and big == kernel.replace(",1,8>", ",1,4,2>"), name
    else:
        assert name == kernel, name
    dx = eng.empty((N_ROWS, d_in), np.float32).upload(x)
    guard = np.full((N_ROWS + 2, d_out), 7.0, np.float32)   # two rows behind the batch: must stay untouched
    dy = eng.empty((N_ROWS + 2, d_out), np.float32).upload(guard)
    eng.mlp_forward(m, dx, dy, N_ROWS)
    y = dy.to_host()
    eng.mlp_destroy(m)
    assert np.all(y[N_ROWS:] == 7.0)
    if prec == "bf16":
        ref = mlp_forward_numpy(x, w, -1.0, bf16=True)
    else:   # float64 forward
        W1, b1, W2, b2, W3, b3 = [a.astype(np.float64) for a in w]
        ref = np.tanh(np.maximum(np.maximum(x.astype(np.float64) @ W1.T + b1, 0) @ W2.T + b2, 0) @ W3.T + b3)
    err = np.abs(y[:N_ROWS] - ref).max()
    print("max |device - reference| = %.3e" % err)
    assert err <= {"bf16": 3e-3, "fp32": 1e-5, "fp32x3": 1e-6}[prec], err


def test_too_wide_a_network_is_refused(eng):
    from ev2gym_amd.actor import init_mlp_weights
    from ev2gym_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        eng.mlp_create(*init_mlp_weights(20, 5, seed=5, h1=3000, h2=64))
    assert e.value.code == -1 and "ev2g_mlp_create: layers too wide for the LDS-resident activations" in str(e.value)   # EV2G_ERR_ARG
