"""tests/cat_stage_rules.py is the reference of tests/test_gpu_cat_stages.py: here (no GPU) its stages, chained in float64, are tied to
the oracle and to the goldens the reference module wrote, its site counts are checked for the tile cases they must reach, and its
convolution bounds are held against a numpy emulation of the three arithmetics."""
import numpy as np
import pytest
import torch

from tests import cat_stage_rules as R
from tests.helpers import PROB_ATOL, golden, seeded_cat_weights, synth_cat_groups


@pytest.fixture(scope="module")
def ws():
    return seeded_cat_weights(R.SEED)


@pytest.fixture(scope="module")
def chain3(ws):
    """the float64 chain at N = 3 on the inputs of the GPU file"""
    g0, g1 = R.stage_inputs(3)
    return R.chain(R.weights_as(ws, torch.float64), g0, g1)


def test_chain_reproduces_the_oracle(ws):
    from oracle import oracle
    g0, g1 = synth_cat_groups(1024, 24)
    got = R.chain(R.weights_as(ws, torch.float64), g0, g1)["prob"].numpy()
    want = oracle.cat_forward(ws, g0, g1, nthreads=4)
    d = np.abs(got - want).max()
    print("float64 chain vs oracle", d)
    assert d < PROB_ATOL
    g0, g1 = R.stage_inputs(5)                                  # the crafted rows too: the empty tag, every base code
    d = np.abs(R.chain(R.weights_as(ws, torch.float64), g0, g1)["prob"].numpy() - oracle.cat_forward(ws, g0, g1, nthreads=4)).max()
    assert d < PROB_ATOL


@pytest.mark.parametrize("name", ["cat_fwd.npz", "cat_fwd_large.npz"])
def test_chain_reproduces_the_reference_goldens(name):
    z = np.load(golden(name))
    w = R.weights_as(seeded_cat_weights(int(z["seed"])), torch.float64)
    got = R.chain(w, z["g0"].astype(np.float32), z["g1"].astype(np.float32))["prob"].numpy()
    d = np.abs(got - z["gt"]).max()
    print(name, "float64 chain vs golden", d)
    assert d < PROB_ATOL


def test_stage_shapes_and_six_step_rows(chain3, ws):
    from nanosnp_amd._lib import Context
    for name in R.ORDER[:-1]:
        assert tuple(chain3[name].shape) == Context.cat_stage_shape(name, 3)[1], name
    # a six-step layer is the full layer's rows: forward column s, backward column 10 - s
    w = R.weights_as(ws, torch.float64)
    full = R.bilstm(w[94:102], chain3["rnn0_emb"], R.L)
    six = chain3["rnn1_h"]
    for s in range(6):
        assert torch.equal(six[s, :, :256], full[s, :, :256]) and torch.equal(six[s, :, 256:], full[10 - s, :, 256:])
    assert torch.equal(six[5], full[5])


def test_site_counts():
    assert R.SITE_COUNTS == (1, 3, 5, 129)
    props = R.site_count_properties()
    assert all(props.values()), props
    # each property is lost by some smaller set: the counts are not redundant for them
    assert not R.site_count_properties((1, 3, 129))["block1_even_and_odd_tiles"]
    assert not R.site_count_properties((1, 5, 129))["block0_even_and_odd_tiles"]
    assert not R.site_count_properties((1, 3, 5))["crosses_site_tile"]
    assert not R.site_count_properties((128,))["partly_filled_everywhere"]


def test_inputs_reach_the_edges(chain3):
    g0, g1 = R.stage_inputs(3)
    pct = chain3["pct_features"].numpy()
    assert pct.dtype == np.float32
    assert np.all(pct[:, 0, 0:5] == 0)                                               # the tag without reads: 0 / 1e-9
    last = pct[0, 2, 15:20]                                                            # group 1, tag 1 of the last site, column 0
    assert np.array_equal(last, (np.array([2, 2, 2, 3, 4], np.float32) / (np.float32(16) + np.float32(1e-9))).astype(np.float32))
    # the pools that drop rows (10 -> 3, 3 -> 1) meet inputs whose maxima sit in the dropped rows
    assert R.dropped_rows_dominate(chain3["block3_out"], 3) > 0.02
    assert R.dropped_rows_dominate(chain3["block5_out"], 2) > 0.02
    assert R.dropped_rows_dominate(chain3["block0_out"], 2) == 0.0
    for name in R.CONV_STAGES:                                                         # no map is trivially zero
        assert float((chain3[name] > 0).double().mean()) >= 0.1, name


def test_storage_formats():
    v = np.array([1 / 3, 0.1, 3.0, 1e-6, 60000.0, -0.7], np.float32)
    p = R.f16_pair(v)
    assert np.all(np.abs(p - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25))
    assert np.array_equal(R.f16_pair(p), p)                                            # a decoded pair splits into itself
    p0, p1, p2 = R.bf16_planes(v)
    assert np.all(np.abs((p0.astype(np.float64) + p1 + p2) - v) <= 2.0 ** -26 * np.abs(v))
    assert np.all((p0.view(np.uint32) & 0xffff) == 0)


@pytest.mark.parametrize("prec", [0, 2, 1], ids=["fp32", "bf16x3", "f16x3"])
def test_bounds_hold_for_an_emulation_of_the_arithmetic(prec, ws, chain3):
    """every convolution stage at N = 3: the emulation (operands split as the packers split them, float32 products, a float32 accumulator,
    shuffled order) on the float64 chain's maps as that arithmetic stores them, against the float64 stage on the same maps"""
    w64 = R.weights_as(ws, torch.float64)
    rng = np.random.default_rng(38)
    for name in R.CONV_STAGES:
        deps = R.STAGES[name][0]
        inp = {d: R.stored(prec, chain3[d].numpy().astype(np.float32)) for d in deps}
        got = R.emulate_conv(ws, name, inp, prec, rng)
        tin = {d: torch.from_numpy(v) for d, v in inp.items()}
        ref = R.stage(name, w64, tin)
        A, S, K = R.conv_magnitude(w64, name, tin)
        err = (torch.from_numpy(got).double() - ref).abs()
        bound = R.conv_bound(prec, A, S, K, ref)
        print(name, "K", K, "max(err / A) / 2^-24 =", float((err / A).max() / R.U), "max(err / bound) =", float((err / bound).max()))
        assert bool((err <= bound).all()), name
        assert float((ref > 0).double().mean()) >= 0.1
