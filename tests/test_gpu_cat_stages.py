"""Every launch of the legacy CatModel forward held to its ONE operation: Context.cat_forward_stage returns the image a stage left, and the
stage's float64 restatement (tests/cat_stage_rules.py, tied to the oracle and the goldens by tests/test_cat_stage_rules.py) is applied to
the GPU's own input of that stage, so errors do not compound, every element is compared and the bounds are derived there, not measured.

In each context the forward runs at N = 129 first, so that stale maps lie behind the end of the small ones; at N = 129 the references
cover the sites R.BIG_SITES only (sites are independent), at N = 1, 3, 5 every element.

Measured on an MI355X (docs/rounds/r38.md): the convolution ratios max(err / A) / 2^-24 and the distances of the recurrent stages."""
import numpy as np
import pytest
import torch

from tests import cat_stage_rules as R
from tests.helpers import seeded_cat_weights

pytestmark = pytest.mark.gpu

PREC_IDS = {0: "fp32", 1: "f16x3", 2: "bf16x3"}
_W = {}
_REF = {}                       # references, per module: (precision, lds, N, stage, dtype) -> tensor


def _weights(dtype):
    if dtype not in _W:
        _W[dtype] = R.weights_as(seeded_cat_weights(R.SEED), dtype)
    return _W[dtype]


class Taps:
    """one context in one arithmetic; every tapped image is fetched once per (N, stage, options)"""

    def __init__(self, prec):
        from nanosnp_amd import _lib
        self.prec = prec
        self.ctx = _lib.Context(0)
        self.ctx.cat_load_weights(seeded_cat_weights(R.SEED))
        self.ctx.set_option("cat_precision", prec)
        self.opts = {"cat_conv_lds": 1, "cat_conv_pix2": 1}
        self.g = {}
        self.cache = {}
        for N in (R.BIG_N,) + tuple(n for n in R.SITE_COUNTS if n != R.BIG_N):
            g0, g1 = R.stage_inputs(N)
            self.g[N] = (torch.from_numpy(g0).cuda(), torch.from_numpy(g1).cuda(), g0, g1)
        self.prime()

    def prime(self):
        """the whole forward at the largest N: what it leaves in the workspace lies behind every smaller run"""
        self.forward(R.BIG_N)

    def options(self, lds=1, pix2=1):
        want = {"cat_conv_lds": lds, "cat_conv_pix2": pix2}
        if want != self.opts:
            for k, v in want.items():
                self.ctx.set_option(k, v)
            self.opts = want
            self.prime()

    def forward(self, N):
        out = self.ctx.cat_forward(self.g[N][0], self.g[N][1])
        torch.cuda.synchronize()
        return out.cpu()

    def run(self, N, name, lds=1, pix2=1):
        """a fresh run, not cached"""
        self.options(lds, pix2)
        if name in ("g0", "g1"):
            return torch.from_numpy(self.g[N][2 if name == "g0" else 3])
        if name == "prob":
            return self.forward(N)
        out = self.ctx.cat_forward_stage(self.g[N][0], self.g[N][1], name)
        torch.cuda.synchronize()
        return out.cpu()

    def tap(self, N, name, lds=1, pix2=1):
        key = (N, name, lds, pix2)
        if key not in self.cache:
            self.cache[key] = self.run(N, name, lds, pix2)
        return self.cache[key]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["fp32", "f16x3", "bf16x3"])
def taps(request):
    t = Taps(request.param)
    yield t
    t.close()


def _site_axis(t):
    return 1 if t.dim() == 3 else 0


def _sites(t, N):
    """the compared sites of an image: all of them, or R.BIG_SITES of the large run"""
    if N != R.BIG_N:
        return t
    return t.index_select(_site_axis(t), torch.tensor(R.BIG_SITES))


def _inputs(taps, N, name, lds=1):
    return {d: _sites(taps.tap(N, d, lds), N) for d in R.STAGES[name][0]}


def _reference(taps, N, name, lds, dtype):
    key = (taps.prec, lds, N, name, dtype)
    if key not in _REF:
        _REF[key] = R.stage(name, _weights(dtype), _inputs(taps, N, name, lds))
    return _REF[key]


# ---- a. exact stages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.SITE_COUNTS)
def test_pack_and_percentage_are_exact(taps, N):
    g = {"g0": taps.run(N, "g0"), "g1": taps.run(N, "g1")}
    w32 = _weights(torch.float32)
    assert torch.equal(taps.tap(N, "pixels"), R.pack(w32, g["g0"], g["g1"]))
    want = R.stored(taps.prec, R.percentage(w32, g["g0"], g["g1"]).numpy())
    got = taps.tap(N, "pct_features").numpy()
    assert np.array_equal(got, want)
    assert np.all(got[:, 0, 0:5] == 0)                                      # the tag without reads
    assert np.array_equal(got[0, N - 1, 15:20], R.stored(taps.prec, (np.array([2, 2, 2, 3, 4], np.float32) / (np.float32(16) + np.float32(1e-9)))))


@pytest.mark.parametrize("N", R.SITE_COUNTS)
@pytest.mark.parametrize("name", list(R.POOL_STAGES))
def test_pools_are_the_max_of_their_input(taps, N, name):
    src, kh = R.POOL_STAGES[name]
    x = taps.tap(N, src)
    want = R.maxpool(x, kh)
    if name == "seq0":
        want = R.to_sequence(want)                                          # the last pool writes the LSTM's input: [11,N,256]
    assert torch.equal(taps.tap(N, name), want)
    assert float((want > 0).double().mean()) >= 0.1
    if name in ("pool3", "seq0"):                                           # heights 10 -> 3 and 3 -> 1: the dropped rows hold larger values
        assert R.dropped_rows_dominate(x, kh) > 0.02


# ---- b. convolutions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [1, 0], ids=["lds", "gather"])
@pytest.mark.parametrize("name", R.CONV_STAGES)
def test_convolution_within_derived_bound(taps, name, lds):
    w64 = _weights(torch.float64)
    worst = 0.0
    for N in (R.BIG_N,) + tuple(n for n in R.SITE_COUNTS if n != R.BIG_N):
        got = _sites(taps.tap(N, name, lds), N).double()
        inp = _inputs(taps, N, name, lds)
        ref = _reference(taps, N, name, lds, torch.float64)
        A, S, K = R.conv_magnitude(w64, name, inp)
        err = (got - ref).abs()
        bound = R.conv_bound(taps.prec, A, S, K, ref)
        ratio = float((err / A).max() / R.U)
        worst = max(worst, ratio)
        print(f"cat stage {name} {PREC_IDS[taps.prec]} lds={lds} N={N} K={K}: max(err / A) / 2^-24 = {ratio:.2f}, "
              f"max(err / bound) = {float((err / bound).max()):.4f}")
        assert got.shape == ref.shape
        assert bool((err <= bound).all()), (name, N, float((err / bound).max()))
        assert float((ref > 0).double().mean()) >= 0.1                       # not trivially zero after ReLU
    print(f"cat stage {name} {PREC_IDS[taps.prec]} lds={lds}: worst ratio {worst:.2f}")


# ---- c. bit equality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.SITE_COUNTS)
def test_two_pixel_tiles_per_workgroup_give_the_same_bits(taps, N):
    """cat_conv_pix2 1 against 0: blocks 0 and 1 (<= 64 output channels) on 256-pixel workgroups, "bit-identical" in cat_forward.hip"""
    for name in ("block0_y", "block0_out", "block1_y", "block1_out", "prob"):
        a, b = taps.tap(N, name, 1, 1), taps.tap(N, name, 1, 0)
        assert a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("N", [R.BIG_N, 3])
def test_every_stage_is_bit_equal_to_a_second_run(taps, N):
    for name in R.ORDER:
        assert torch.equal(taps.tap(N, name), taps.run(N, name)), name
    # the 512-vector is its two halves' own stages
    assert torch.equal(taps.tap(N, "cat")[:, :256], taps.tap(N, "pct_linear"))


# ---- d. recurrent stages, Linears and the head ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.RECURRENT_STAGES)
def test_recurrent_stage_against_float64(taps, name):
    """each BiLSTM layer (the six-step ones too), each Linear and the head (nsnp_cat_forward's probabilities against the head of the tapped
    512-vector) on the tapped input: at most 8 d32 + 2^-23 from float64 (six times that in f16x3), d32 the distance of the same stage in
    float32 torch on the CPU (tests/cat_stage_rules.py)"""
    for N in (R.BIG_N,) + tuple(n for n in R.SITE_COUNTS if n != R.BIG_N):
        got = _sites(taps.tap(N, name), N).double()
        ref = _reference(taps, N, name, 1, torch.float64)
        d32 = float((_reference(taps, N, name, 1, torch.float32).double() - ref).abs().max())
        d = float((got - ref).abs().max())
        bound = R.recurrent_bound(taps.prec, d32)
        print(f"cat stage {name} {PREC_IDS[taps.prec]} N={N}: d32 = {d32:.3e}, |gpu - f64| = {d:.3e}, bound {bound:.3e}, max |ref| = {float(ref.abs().max()):.3f}")
        assert got.shape == ref.shape
        assert d <= bound, (name, N, d, bound)
    if name == "prob":
        assert float((got.sum(1) - 1).abs().max()) < 1e-5


def test_stage_entry_rejects_bad_arguments(taps):
    from nanosnp_amd._lib import NanoSNPError
    g0, g1 = taps.g[1][0], taps.g[1][1]
    with pytest.raises(NanoSNPError):
        taps.ctx.cat_forward_stage(g0, g1, "no_such_stage")
    lib, h = taps.ctx.lib, taps.ctx.handle
    out = torch.empty(512, device="cuda")
    assert lib.nsnp_cat_forward_stage(h, g0.data_ptr(), g1.data_ptr(), 1, 25, out.data_ptr(), 511, None) == -1      # size of another shape
    assert lib.nsnp_cat_forward_stage(h, g0.data_ptr(), g1.data_ptr(), 1, 26, out.data_ptr(), 512, None) == -1      # no such stage
    assert lib.nsnp_cat_forward_stage(h, g0.data_ptr(), g1.data_ptr(), 4097, 25, out.data_ptr(), 4097 * 512, None) == -1   # more than one pass
    assert lib.nsnp_cat_forward_stage(h, g0.data_ptr(), g1.data_ptr(), 0, 25, out.data_ptr(), 0, None) == -1
