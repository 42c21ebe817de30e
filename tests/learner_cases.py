"""What tests/test_ppo_gpu.py, tests/test_a2c_gpu.py and tests/test_learner_shapes_gpu.py share: the array names, the networks' shapes per
handle, the row counts, the engines, the index sets of a gradient case, one device harness parameterised by the learner's kind, and the table of
networks that take the learner's kernels off width 64 (tests/test_ppo_plan_cpu.py pins its LDS figures without a GPU).  A plain module: each
test module imports what it uses (the `engines` fixture included)."""
import numpy as np
import pytest

from tests.test_onpolicy_gpu import _fixture_engine, _gen_engine, _up
from tests.test_ppo_cpu import CLIP

NAMES = ("pi_W1", "pi_b1", "pi_W2", "pi_b2", "vf_W1", "vf_b1", "vf_W2", "vf_b2", "action_W", "action_b", "value_W", "value_b", "log_std")
SHAPES = {"pst": (63, 20), "ppl": (162, 50)}   # (D, P) of the networks run on each handle
N_ROWS = {"tanh": 600, "relu": 96}   # distinct rows of a case (ReLU: few enough that a seed with no pre-activation near 0 exists)

# Networks that reach what the (64, 64) learners never run (csrc/ev2g_ppo.h; padded widths k1 = ceil8(d_in), k1r = ceil32(d_in), n1 / n2 / m1 /
# m2 / n3 = ceil32 of h / v / d_out; the gradient kernel has 4 wavefronts): tag -> (d_in, h, v, d_out, activations, the plan's LDS bytes).
#   wide         8 tiles in both trunk stages, forward and back: every wavefront's second trip.  Back tiles of KG 16, dW decode with kn 4,
#                output tile rows 2 and 3 of both packed images.
#   lopsided     9 tiles in the first stage (8 + 1) and 4 in the second (1 + 3): a 256-wide layer, KG 32 forward and 4 back, unequal trunks.
#   limits       1,664 bytes under the LDS limit; k1r == d_in (no zero-filled x column); n3 == P (no padded port); tile counts 3 and 5.
#   tiny         kx 1; k1 8 < k1r 32 (only the dW tiles read x columns 8..31); P 1: seven of a row's eight head lanes have no port; one tile
#                per stage, so three wavefronts idle.
#   past-a-tile  d_in and d_out both 33: 31 zero-filled input columns, 31 padded ports.
# (128, 128) / (128, 128) runs tanh only: no seed of RELU_SEEDS keeps its ReLU pre-activations away from 0.
LEARNER_NETS = {
    "wide": (63, (128, 128), (128, 128), 20, ("tanh",), 153728),
    "lopsided": (162, (256, 32), (32, 96), 50, ("relu",), 153984),
    "limits": (192, (96, 160), (160, 32), 64, ("relu",), 162176),
    "tiny": (5, (8, 8), (8, 8), 1, ("tanh", "relu"), 51328),
    "past-a-tile": (33, (64, 64), (64, 64), 33, ("tanh",), 96640),
}
NEAREST_THE_LDS_LIMIT = "limits"


def net_shape(tag):
    """(d_in, h1, h2, v1, v2, d_out) of a row of LEARNER_NETS, the order ev2g_ppo_query takes"""
    d_in, h, v, d_out, _, _ = LEARNER_NETS[tag]
    return (d_in, h[0], h[1], v[0], v[1], d_out)


# per kind: the create call with its fixed arguments, the case's arrays a call reads, the gradient call, the grad-then-apply call
KINDS = {
    "ppo": dict(create="ppo_create", fixed=dict(clip_range=CLIP), rows=("obs", "actions", "old_log_prob", "advantages", "returns"), grad="ppo_grad",
                step="ppo_minibatch"),
    "a2c": dict(create="a2c_create", fixed={}, rows=("obs", "actions", "advantages", "returns"), grad="a2c_grad", step="a2c_update"),
}


@pytest.fixture(scope="module")
def engines():
    engs = {"pst": _gen_engine("pst"), "ppl": _fixture_engine("ppl")}
    assert (engs["pst"].D, engs["pst"].P) == SHAPES["pst"]
    yield engs
    for e in engs.values():
        e.close()


def _shape(case):
    return (case["D"], case["h"][0], case["h"][1], case["v"][0], case["v"][1], case["P"])


class _Device:
    """A case's rows, a policy object and a learner of `kind` on an engine; the learner is also the attribute named after its kind."""

    def __init__(self, kind, eng, case, lo=-1.0, **cfg):
        from ev2gym_amd.onpolicy import GaussianActorCritic
        self.eng, self.case, self.calls = eng, case, KINDS[kind]
        self.pol = GaussianActorCritic(case["weights"], case["log_std"], activation=case["activation"], lo=lo, seed=5).attach(eng)
        self.learner = getattr(eng, self.calls["create"])(self.pol.ac, **self.calls["fixed"], **cfg)
        setattr(self, kind, self.learner)
        self.bufs = [_up(eng, case[k]) for k in self.calls["rows"]]
        self.stats = eng.empty((6,), np.float32)

    def grad(self, idx):
        ix = _up(self.eng, np.asarray(idx, np.int32))
        getattr(self.eng, self.calls["grad"])(self.learner, *self.bufs, ix, len(idx), self.stats)
        g = self.eng.ppo_get_grads(self.learner, _shape(self.case))
        st = self.stats.to_host()
        ix.free()
        return g, st

    def step(self, idx):
        ix = _up(self.eng, np.asarray(idx, np.int32))
        getattr(self.eng, self.calls["step"])(self.learner, *self.bufs, ix, len(idx), self.stats)
        st = self.stats.to_host()   # (synchronises)
        ix.free()
        return st

    minibatch = update = step

    def weights(self):
        w, ls = self.eng.ac_get_weights(self.pol.ac, _shape(self.case))
        return w + [ls]

    def close(self):
        self.pol.close()   # (the learner goes with its policy)
        for b in self.bufs + [self.stats]:
            b.free()


def _index_sets(cap, n_rows, skip_one_row=False):
    rng = np.random.default_rng(12)
    sets = [rng.choice(n_rows, B, replace=False) for B in (1, 31, 32, 33)]
    dup = rng.integers(0, n_rows, 97)
    dup[5:9] = dup[0]                                      # duplicates for certain
    sets += [dup, rng.integers(0, n_rows, 32 * cap + 37)]   # the last: every workgroup loops and the cross-workgroup reduction runs
    return sets[1:] if skip_one_row else sets               # (A2C refuses one normalised row: its test_refusals_through_the_abi)
