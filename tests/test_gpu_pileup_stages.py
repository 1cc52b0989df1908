"""Every launch of the PileupModel forward held to its ONE operation.  Context.pileup_forward_stage returns the image a layer left (h0:
layer 0's h at all 33 positions, h1c: layer 1's h at position 16), and the stage's float64 restatement (tests/pileup_stage_rules.py, tied
to eval_rules, the oracle and the goldens by tests/test_pileup_stage_rules.py) is applied to the GPU's own input of that stage: h0 from
the integer counts, h1c from the tapped h0, the probabilities of nsnp_pileup_forward and the 90 logits of nsnp_pileup_forward_logits2 from
the tapped h1c.  Errors do not compound, every element is compared, and the bound is the project's rule for recurrent stages
(cat_stage_rules.recurrent_bound: 8 d32 + 2^-23, six times that in f16x3, d32 the distance of the same stage in float32 torch on the CPU
from float64 on the same inputs) - not a figure measured on a kernel.

One context per arithmetic; in each the largest N runs first, so that what it leaves in the workspace lies behind every smaller run.
Each layer's kernel variants are tested on their own (layer-1 variants behind the default layer 0, on the h0 that run left), and
where an existing test asserts two variants bit-equal in their probabilities their stage images are asserted bit-equal here.

Measured on an MI355X: docs/rounds/r40.md."""
import numpy as np
import pytest
import torch

from tests import pileup_stage_rules as R
from tests.helpers import golden

pytestmark = pytest.mark.gpu

PREC_IDS = {0: "fp32", 1: "f16x3", 2: "bf16x3"}
DEFAULTS = {"l0_register_stationary": 2, "l0_weave": 1, "l0_prestage": 1, "l0_site_groups": 0, "l0_input_weights_in_lds": 0,
            "l1_register_stationary": 1, "l1_weave": 1, "l1_stagger": 0, "l1_site_groups": 0, "fused_l1": 1, "fused_waves": 0,
            "recurrence_waves": 0, "head_split": 1}       # the library's defaults today; every context SETS them all (Taps), so a
                                                          # case with no options of its own runs these kernels whatever the defaults become
CHUNK = 16384                                             # sites of a pass, reserved by every context: above the largest N run (16 * 2 * n_cu + 17)

# layer-0 variants per arithmetic: (id, options, bit-equality class - variants of one class give the same h0, asserted by
# test_gpu_pileup_forward.py / test_gpu_l0_weave.py / test_gpu_l0_prestage.py on the probabilities)
L0 = {
    0: [(f"lds-image-{w}w", {"l0_register_stationary": 0, "recurrence_waves": w}, "fp32-chain") for w in (1, 2, 4, 8)]
       + [(f"rs-{g}g", {"l0_register_stationary": 1, "l0_site_groups": g}, "fp32-chain") for g in (1, 2, 4)]
       + [("rs-wx-lds", {"l0_register_stationary": 1, "l0_site_groups": 1, "l0_input_weights_in_lds": 1}, "fp32-chain"),
          ("rsx", {"l0_weave": 0}, "bf16-input"), ("rsx-weave", {"l0_prestage": 0}, "bf16-input"), ("rsx-weave-prestage", {}, "bf16-input")],
    1: [(f"lds-image-{w}w", {"l0_register_stationary": 0, "recurrence_waves": w}, None) for w in (1, 2, 4, 8)]
       + [(f"rs-{g}g", {"l0_site_groups": g}, "rs") for g in (1, 2, 4)],
    2: [("1g", {"l0_site_groups": 1}, "b3"), ("2g", {"l0_site_groups": 2, "l0_register_stationary": 0}, "b3"),
        ("4g", {"l0_site_groups": 4}, "b3"), ("2g-skewed", {"l0_site_groups": 2}, "b3")],
}
L1 = {
    0: [(f"lds-image-{w}w", {"l1_register_stationary": 0, "recurrence_waves": w}, "fp32") for w in (1, 2, 4, 8)]
       + [("rs4-1g", {"l1_weave": 0, "l1_site_groups": 1}, "fp32"), ("rs4-2g", {"l1_weave": 0, "l1_site_groups": 2}, "fp32"),
          ("rs4-weave", {}, "fp32")]
       + [(f"rs8-{g}g-stagger{st}", {"l1_register_stationary": 2, "l1_site_groups": g, "l1_stagger": st}, "fp32") for g in (2, 4) for st in (0, 1)],
    1: [("rs4", {}, "rs"), ("rs8-2g", {"l1_site_groups": 2}, "rs"), ("rs8-4g", {"l1_site_groups": 4}, "rs"),
        ("rs8", {"l1_register_stationary": 2}, "rs")]
       + [(f"fused-{w}w", {"l1_register_stationary": 0, "fused_waves": w}, None) for w in (4, 8, 12)]
       + [("unfused", {"fused_l1": 0}, None)]
       + [(f"unfused-{w}w", {"fused_l1": 0, "recurrence_waves": w}, None) for w in (1, 2, 4, 8)],
    2: [(f"{g}g", {"l1_site_groups": g}, "b3") for g in (1, 2, 4)],
}


def _params(table):
    return [pytest.param(p, opts, id=f"{PREC_IDS[p]}-{name}") for p in (0, 1, 2) for name, opts, _ in table[p]]


def _key(opts):
    return tuple(sorted(opts.items()))


class Taps:
    """one context in one arithmetic; every image is fetched once per (stage, N, options)"""

    def __init__(self, prec, weights, indel):
        from nanosnp_amd import _lib
        self.prec = prec
        self.ctx = _lib.Context(0)
        self.ctx.pileup_load_weights(weights)
        self.ctx.pileup_load_indel_heads(indel)
        self.ctx.set_option("pileup_precision", prec)
        self.ctx.reserve(CHUNK)
        for k, v in DEFAULTS.items():
            self.ctx.set_option(k, v)
        self.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        self.opts = dict(DEFAULTS)
        self.x_host = R.stage_inputs(prec)
        self.x = torch.from_numpy(self.x_host).cuda()
        self.counts = R.site_counts(prec)
        self.cache = {}
        self.w = {dt: R.weights_as(weights, indel, dt) for dt in (torch.float64, torch.float32)}
        self.h0_ref = {dt: R.layer0(self.w[dt], self.x_host) for dt in (torch.float64, torch.float32)}    # once: sites are independent
        self.prime()

    def prime(self):
        """the forward at the largest N: what it leaves in the workspace lies behind every smaller run"""
        self.ctx.pileup_forward(self.x)
        torch.cuda.synchronize()

    def options(self, opts):
        want = {**DEFAULTS, **opts}
        if want != self.opts:
            for k, v in want.items():
                if self.opts[k] != v:
                    self.ctx.set_option(k, v)
            self.opts = want
            self.prime()

    def run(self, stage, N, opts, x=None):
        """a fresh run, not cached.  stage: h0, h1c (the tap), prob ((gt | zy) of nsnp_pileup_forward), logits (nsnp_pileup_forward_logits2)"""
        self.options(opts)
        x = self.x[:N].contiguous() if x is None else x
        if stage == "prob":
            out = torch.cat(self.ctx.pileup_forward(x), 1)
        elif stage == "logits":
            out = self.ctx.pileup_forward_logits(x, precision=self.prec)
        else:
            out = self.ctx.pileup_forward_stage(x, stage, precision=self.prec)
        torch.cuda.synchronize()
        return out.cpu()

    def tap(self, stage, N, opts):
        key = (stage, N, _key(opts))
        if key not in self.cache:
            self.cache[key] = self.run(stage, N, opts)
        return self.cache[key]

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def contexts(pileup_weights):
    z = np.load(golden("pileup_eval.npz"))
    indel = [z["indel1_weight"], z["indel1_bias"], z["indel2_weight"], z["indel2_bias"]]
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = Taps(prec, pileup_weights, indel)
        return made[prec]
    yield get
    for t in made.values():
        t.close()


def _held(what, prec, got, ref64, ref32):
    """got within recurrent_bound of ref64, every element; prints the figures docs/rounds/r40.md tabulates"""
    assert got.shape == ref64.shape and got.dtype == torch.float32
    d32 = R.dist(ref32, ref64)
    d = R.dist(got, ref64)
    bound = R.recurrent_bound(prec, d32)
    print(f"pileup stage {what}: d32 = {d32:.3e}, |gpu - f64| = {d:.3e}, bound {bound:.3e}, share {d / bound:.3f}")
    assert bool(torch.isfinite(got).all())
    assert d <= bound, (what, d, bound)
    return d / bound


# ---- layer 0 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,opts", _params(L0))
def test_layer0_against_float64(contexts, prec, opts, request):
    """h0 of every layer-0 kernel from the integer counts (the reference is exact on them), at every site count"""
    taps = contexts(prec)
    for N in taps.counts:
        got = taps.tap("h0", N, opts)
        _held(f"h0 {request.node.callspec.id} N={N}", prec, got, taps.h0_ref[torch.float64][:N], taps.h0_ref[torch.float32][:N])


# ---- layer 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,opts", _params(L1))
def test_layer1_against_float64(contexts, prec, opts, request):
    """h1c of every layer-1 kernel against layer 1 of the h0 the same run left"""
    taps = contexts(prec)
    for N in taps.counts:
        h0 = taps.tap("h0", N, opts)
        got = taps.tap("h1c", N, opts)
        _held(f"h1c {request.node.callspec.id} N={N}", prec, got, R.layer1_centre(taps.w[torch.float64], h0), R.layer1_centre(taps.w[torch.float32], h0))


# ---- heads ----------------------------------------------------------------------------------------------------------------------------
def _heads_held(taps, what, h1c, prob, logits):
    l64, g64, z64 = R.heads(taps.w[torch.float64], h1c)
    l32, g32, z32 = R.heads(taps.w[torch.float32], h1c)
    _held(f"prob {what}", taps.prec, prob, torch.cat((g64, z64), 1), torch.cat((g32, z32), 1))
    _held(f"logits {what}", taps.prec, logits, l64, l32)
    assert float((prob[:, :21].sum(1) - 1).abs().max()) < 1e-5 and float((prob[:, 21:].sum(1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("prec,opts", [pytest.param(p, o, id=f"{PREC_IDS[p]}-head_split{o['head_split']}")
                                       for p in (0, 1, 2) for o in ({"head_split": 1}, {"head_split": 0})])
def test_heads_against_float64(contexts, prec, opts, request):
    """the probabilities of nsnp_pileup_forward and the 90 logits of nsnp_pileup_forward_logits2 against the heads of the tapped h1c
    ("head_split" chooses between the two fp32 probability kernels; the other arithmetics have one, and the scoring heads kernel is
    one per arithmetic)"""
    taps = contexts(prec)
    for N in taps.counts:
        _heads_held(taps, f"{request.node.callspec.id} N={N}", taps.tap("h1c", N, opts), taps.tap("prob", N, opts), taps.tap("logits", N, opts))
    if prec == 0:                                                        # same chains in both kernels: test_gpu_pileup_forward.py
        for N in taps.counts:
            assert torch.equal(taps.tap("prob", N, {"head_split": 1}), taps.tap("prob", N, {"head_split": 0}))


@pytest.mark.parametrize("prec", [0, 1, 2], ids=list(PREC_IDS.values()))
def test_heads_where_the_persistent_kernel_loops(contexts, prec):
    """N = 16 * 2 * n_cu + 17: k_pileup_head_rs runs two workgroups per CU and walks the rest - here every workgroup's first tile, a
    second tile for one of them and a partial one.  The inputs tile the pool; the heads alone are compared, at 256 sampled sites"""
    taps = contexts(prec)
    N = 16 * 2 * taps.n_cu + 17
    assert N <= CHUNK
    pool = taps.x.shape[0]
    x = taps.x[torch.arange(N, device="cuda") % pool].contiguous()
    h1c = taps.run("h1c", N, {}, x)
    prob = taps.run("prob", N, {}, x)
    logits = taps.run("logits", N, {}, x)
    taps.prime()
    pick = torch.from_numpy(np.unique(np.concatenate([np.random.default_rng(40).integers(0, N, 244), np.arange(N - 12, N)])))
    assert pick.numel() <= 256 and int(pick.max()) == N - 1 and int((pick >= 16 * 2 * taps.n_cu).sum()) >= 12
    _heads_held(taps, f"{PREC_IDS[prec]} N={N}", h1c[pick], prob[pick], logits[pick])
    # and the tiled sites repeat their pool site bit for bit, wherever they stand
    idx = torch.arange(N) % pool
    assert torch.equal(h1c, h1c[:pool][idx]) and torch.equal(prob, prob[:pool][idx]) and torch.equal(logits, logits[:pool][idx])


# ---- bit equality -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1, 2], ids=list(PREC_IDS.values()))
def test_variants_that_share_their_arithmetic_share_their_bits(contexts, prec):
    """where the end-to-end tests assert two variants bit-equal in their probabilities, the stage images are bit-equal too"""
    taps = contexts(prec)
    for stage, table in (("h0", L0), ("h1c", L1)):
        first = {}
        for name, opts, cls in table[prec]:
            if cls is None:
                continue
            if cls not in first:
                first[cls] = (name, opts)
                continue
            for N in taps.counts:
                assert torch.equal(taps.tap(stage, N, opts), taps.tap(stage, N, first[cls][1])), (stage, name, first[cls][0], N)


@pytest.mark.parametrize("prec", [0, 1, 2], ids=list(PREC_IDS.values()))
def test_second_run_tap_between_forwards_and_site_independence(contexts, prec):
    taps = contexts(prec)
    n_all = taps.counts[0]
    for N in (n_all, 17):
        before = taps.run("prob", N, {})
        for stage in ("h0", "h1c"):
            assert torch.equal(taps.tap(stage, N, {}), taps.run(stage, N, {})), stage         # every stage equals a second run
        assert torch.equal(taps.run("prob", N, {}), before)                                   # a forward after a tap: the same bits
        assert torch.equal(taps.run("logits", N, {}), taps.tap("logits", N, {}))
    for stage in ("h0", "h1c"):                                                               # a site does not depend on its batch
        for N in taps.counts[1:]:
            assert torch.equal(taps.tap(stage, N, {}), taps.tap(stage, n_all, {})[:N]), (stage, N)


def test_counts_read_in_place_give_the_same_images(contexts):
    """center_idx: the windows straight out of a count matrix (nsnp_pileup_forward_windows' addressing) -> the images of the gathered call"""
    taps = contexts(0)
    rng = np.random.default_rng(41)
    counts = torch.from_numpy(rng.integers(-15, 61, (200, 18)).astype(np.int32)).cuda()
    centers = torch.from_numpy(rng.permutation(np.arange(16, 184, dtype=np.int64))[:37].copy()).cuda()
    x = taps.ctx.pileup_gather_windows(counts, centers)
    for prec in (0, 1, 2):
        for stage in ("h0", "h1c"):
            a = taps.ctx.pileup_forward_stage(counts, stage, center_idx=centers, precision=prec)
            b = taps.ctx.pileup_forward_stage(x, stage, precision=prec)
            assert torch.equal(a, b), (prec, stage)
    taps.prime()


# ---- the entry's argument rules ---------------------------------------------------------------------------------------------------------
def test_stage_entry_rejects_bad_arguments_and_launches_nothing(contexts):
    from nanosnp_amd._lib import NanoSNPError
    taps = contexts(0)
    x = taps.x[:2].contiguous()
    with pytest.raises(NanoSNPError):
        taps.ctx.pileup_forward_stage(x, "heads")
    with pytest.raises(NanoSNPError):
        taps.ctx.pileup_forward_stage(x, "h0", precision=None)
    lib, h = taps.ctx.lib, taps.ctx.handle
    good = taps.run("h1c", 2, {})
    marks = torch.full((4 * 33 * 128,), -7.0, device="cuda")
    p = lambda t: t.data_ptr()

    def refused(*args):
        assert lib.nsnp_pileup_forward_stage(h, *args, None) == -1
        torch.cuda.synchronize()
        assert bool((marks == -7.0).all())                               # nothing written
    refused(p(x), None, 2, 0, 1, p(marks), 2 * 128 - 1)                  # not the image's size
    refused(p(x), None, 2, 0, 1, p(marks), 2 * 33 * 128)                 # the size of the other stage
    refused(p(x), None, 2, 0, 2, p(marks), 2 * 128)                      # no such stage
    refused(p(x), None, 2, 3, 1, p(marks), 2 * 128)                      # no such arithmetic
    refused(p(x), None, 2, -2, 1, p(marks), 2 * 128)
    refused(p(x), None, 0, 0, 1, p(marks), 0)                            # no sites
    refused(p(x), None, -1, 0, 1, p(marks), -128)
    refused(p(x), None, CHUNK + 1, 0, 1, p(marks), (CHUNK + 1) * 128)    # more than one pass of the reserved chunk
    refused(None, None, 2, 0, 1, p(marks), 2 * 128)
    assert lib.nsnp_pileup_forward_stage(h, p(x), None, 2, 0, 1, None, 2 * 128, None) == -1
    assert lib.nsnp_pileup_forward_stage(None, p(x), None, 2, 0, 1, p(marks), 2 * 128, None) == -1
    # no layer launch either: the context's launch counters saw none (and do see those of an accepted call)
    taps.ctx.enable_timing(True)
    try:
        taps.ctx.read_timing()
        refused(p(x), None, 2, 0, 1, p(marks), 2 * 128 + 1)
        refused(p(x), None, 2, 0, 5, p(marks), 2 * 128)
        seen = taps.ctx.read_timing()
        assert seen["pileup_l0"][1] == 0 and seen["pileup_l1"][1] == 0 and seen["pileup_head"][1] == 0, seen
        assert torch.equal(taps.run("h1c", 2, {}), good)
        seen = taps.ctx.read_timing()
        assert seen["pileup_l0"][1] == 1 and seen["pileup_l1"][1] == 1 and seen["pileup_head"][1] == 0, seen      # and no heads launch
    finally:
        taps.ctx.enable_timing(False)
    # "context" follows the option
    assert torch.equal(taps.ctx.pileup_forward_stage(x, "h1c").cpu(), good)
