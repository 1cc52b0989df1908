"""The bf16x3 LSTM step kernel on 256 x 256 workgroup tiles (k_hap_lstm_b3x, nanosnp_amd/csrc/hap_gemm.hpp) at the pass sizes where
launch_hap_gemm selects it, at every K-chunk count a feature count can give it, with outputs that differ from site to site; and the LDS
ballast regimes of k_hap_gemm in fp32 and f16x3.  Every site count is derived from tests/hap_tile_rules.py and the CU count of the device;
tests/test_hap_tile_rules.py pins what they are at 256 CUs.  A case whose regime is not reached on the device fails.

Contracts: the big kernel gives the bits of k_hap_gemm<MODE_LSTM, 2> (its header comment), sites are independent of each other and of the
pass size, and every arithmetic stays within PROB_ATOL of the CPU oracle.  Weights: the scaled seeded weights (helpers.HAP_DIMS_WEIGHTS);
inputs: standard_normal * 300, so that a swap of two site tiles, two row halves, layers, steps or directions shows as O(0.1).

Every context sets "hap_pass_sites" to 128 * tiles_all (8,192 at 256 CUs) BEFORE it loads weights: the workspace is sized at load time.

Measured on an MI355X: docs/rounds/r37.md."""
import functools

import numpy as np
import pytest

from tests import hap_eval_rules as hr
from tests import hap_tile_rules as tr
from tests.helpers import HAP_DIMS_WEIGHTS, PROB_ATOL, seeded_hap_weights

pytestmark = pytest.mark.gpu

CLASSES = [(10, 3), (15, 1), (1, 15), (13, 3)]
F_LIST = [1, 16, 17, 32, 33, 105, 128]            # 1, 1, 2, 2, 3, 7, 8 input chunks
CASES = [(F,) + CLASSES[i % len(CLASSES)] for i, F in enumerate(F_LIST)]
IDS = ["F%d-%d+%d" % c for c in CASES]
SCORING_CASES = [(105, 10, 3), (17, 13, 3)]
SAMPLE = 96                                       # sites given to the oracle


def site_cases(n_cu):
    """name -> (sites, the regime of each of its passes at pass size 128 * tiles_all): "all" launches on the big kernel, the "four"-slice
    launches only (the hand-over to k_hap_gemm inside every layer), or "none" """
    A, Q = tr.tiles_all(n_cu), tr.tiles_four(n_cu)
    return {"all": (128 * A, ["all"]),
            "all_one_site_tile": (128 * A - 127, ["all"]),            # the last tile holds one site
            "odd_control": (128 * (A - 1), ["none"]),                 # an odd tile count: the control
            "handover": (128 * Q, ["four"]),
            "handover_ragged": (128 * (Q + 2) - 5, ["four"]),
            "two_passes": (128 * A + 129, ["all", "none"])}           # a full big-kernel pass, then two tiles in the same workspace


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pass_sites():
    return 128 * tr.tiles_all(_n_cu())


def _require_regimes():
    """the rules, applied to this device, give every case the regime it is named for - otherwise the case fails, it does not skip"""
    n_cu, ps = _n_cu(), _pass_sites()
    for name, (n, regimes) in site_cases(n_cu).items():
        assert [tr.regime(p, n_cu) for p in tr.passes(n, ps)] == regimes, (name, n, n_cu)


@functools.lru_cache(maxsize=None)
def _inputs(F):
    """device fp32 [n, F, 33] and [n, F, 11] at the largest site count; the smaller ones are slices"""
    import torch
    n = max(n for n, _ in site_cases(_n_cu()).values())
    rng = np.random.default_rng(3700 + F)
    xp = rng.standard_normal((n, F, 33), dtype=np.float32) * np.float32(300)
    xh = rng.standard_normal((n, F, 11), dtype=np.float32) * np.float32(300)
    return torch.from_numpy(xp).cuda(), torch.from_numpy(xh).cuda()


def _weights(F, n_gt, n_zy):
    return seeded_hap_weights(900 + F + 1000 * n_gt, F=F, n_gt=n_gt, n_zy=n_zy, **HAP_DIMS_WEIGHTS)


def _ctx(prec, F, n_gt, n_zy):
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    c.set_option("hap_pass_sites", _pass_sites())
    c.set_option("hap_precision", prec)
    c.hap_load_weights(_weights(F, n_gt, n_zy), n_features=F, n_gt=n_gt, n_zy=n_zy)
    return c


def _forward(c, xp, xh, b3x=None):
    import torch
    if b3x is not None:
        c.set_option("hap_b3x", b3x)
    out = c.hap_forward(xp, xh)
    torch.cuda.synchronize()
    return out


def _assert_same_bits(got, want, what):
    import torch
    for head, (g, w) in enumerate(zip(got, want)):
        if not torch.equal(g, w):
            d = (g.double() - w.double()).abs()
            raise AssertionError("%s, head %d: %d of %d sites differ, max |d| = %.3g" % (what, head, int((d.max(1).values > 0).sum()), g.shape[0],
                                                                                        float(d.max())))


@functools.lru_cache(maxsize=None)
def _full_run(F, n_gt, n_zy):
    """128 * tiles_all sites in one pass, every launch on the big kernel, on a context of its own -> device (gt, zy)"""
    xp, xh = _inputs(F)
    n = _pass_sites()
    c = _ctx(2, F, n_gt, n_zy)
    try:
        return _forward(c, xp[:n], xh[:n], b3x=1)
    finally:
        c.close()


def sample_sites(n, seed, cap=SAMPLE):
    """at most `cap` of n sites: the edges of the wave and workgroup tiles, the last two tiles, a tile pair in the middle, a seeded draw"""
    T = tr.n_tiles(n)
    m = 2 * (T // 4)
    fixed = [0, 31, 32, 127, 128, 255, 256, 128 * m, 128 * m + 127, 128 * m + 128, 128 * m + 255]
    for t in (T - 2, T - 1):
        fixed += [128 * t, min(128 * t + 127, n - 1)]
    fixed = sorted({s for s in fixed if 0 <= s < n})
    rest = np.setdiff1d(np.arange(n), fixed)
    draw = np.random.default_rng(seed).choice(rest, size=max(0, min(cap, n) - len(fixed)), replace=False)
    return np.sort(np.concatenate([np.asarray(fixed, np.int64), draw.astype(np.int64)]))


def _oracle(F, n_gt, n_zy, idx):
    from oracle import oracle
    import torch
    xp, xh = _inputs(F)
    i = torch.from_numpy(idx).cuda()
    return oracle.hap_forward(_weights(F, n_gt, n_zy), xp[i].cpu().numpy(), xh[i].cpu().numpy(), n_gt=n_gt, n_zy=n_zy, nthreads=16)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_device_tensors():
    yield
    _inputs.cache_clear(); _full_run.cache_clear(); _scoring_runs.cache_clear()


# ---- a. the big kernel gives the small kernel's bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n_gt,n_zy", CASES, ids=IDS)
def test_big_kernel_gives_the_bits_of_the_small_kernel(F, n_gt, n_zy):
    """hap_precision 2, per site count of site_cases: hap_b3x 1 == hap_b3x 0 == hap_b3x 1 again, bit for bit on both heads; every prefix
    equals the first rows of the all-big-kernel pass of another context; the 129 sites behind a full pass equal a forward of their own"""
    _require_regimes()
    xp, xh = _inputs(F)
    full = _full_run(F, n_gt, n_zy)
    ps = _pass_sites()
    c = _ctx(2, F, n_gt, n_zy)
    try:
        for name, (n, _) in site_cases(_n_cu()).items():
            what = "F %d, %s (N = %d)" % (F, name, n)
            big = _forward(c, xp[:n], xh[:n], b3x=1)
            small = _forward(c, xp[:n], xh[:n], b3x=0)
            again = _forward(c, xp[:n], xh[:n], b3x=1)
            assert big[0].shape == (n, n_gt) and big[1].shape == (n, n_zy)
            _assert_same_bits(big, small, what + ": hap_b3x 1 against 0")
            _assert_same_bits(again, big, what + ": hap_b3x 1 a second time")
            k = min(n, ps)
            _assert_same_bits((big[0][:k], big[1][:k]), (full[0][:k], full[1][:k]), what + ": against the first rows of the full pass")
            if n > ps:
                own = _forward(c, xp[ps:n], xh[ps:n], b3x=1)
                _assert_same_bits((big[0][ps:], big[1][ps:]), own, what + ": the second pass against a forward of its own")
    finally:
        c.close()


# ---- b. the big kernel against the CPU oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n_gt,n_zy", CASES, ids=IDS)
def test_big_kernel_against_the_oracle(F, n_gt, n_zy):
    """96 sites of the all-big-kernel pass (sample_sites) within PROB_ATOL of the oracle on both heads.  Measured max |dp| on an MI355X
    (docs/rounds/r37.md), F = 1, 16, 17, 32, 33, 105, 128: 2.4e-6, 4.6e-6, 3.6e-6, 3.3e-6, 2.5e-6, 3.8e-6, 3.3e-6."""
    _require_regimes()
    n = _pass_sites()
    idx = sample_sites(n, 4100 + F)
    assert idx.size == min(SAMPLE, n) and np.unique(idx).size == idx.size
    gt, zy = (a.cpu().numpy()[idx] for a in _full_run(F, n_gt, n_zy))
    ogt, ozy = _oracle(F, n_gt, n_zy, idx)
    assert (ogt if n_gt >= n_zy else ozy).std(0).max() > 1e-3             # outputs that differ from site to site: a constant cannot pass
    d = max(np.abs(gt - ogt).max(), np.abs(zy - ozy).max())
    print("F %d, classes %d + %d, k_hap_lstm_b3x at N = %d: max |dp| vs the oracle over %d sites = %.3g" % (F, n_gt, n_zy, n, idx.size, d))
    assert d < PROB_ATOL
    assert np.abs(gt.sum(1) - 1).max() < 1e-5 and np.abs(zy.sum(1) - 1).max() < 1e-5


# ---- c. the scoring path ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scoring_runs(F, n_gt, n_zy):
    """nsnp_hap_eval at N = 128 * tiles_all - 127 with seeded classes, hap_b3x 1, 0 and 1 again -> [(loss, pred, logits, counters)] as numpy"""
    import torch
    n = site_cases(_n_cu())["all_one_site_tile"][0]
    xp, xh = _inputs(F)
    rng = np.random.default_rng(4300 + F)
    cls = np.stack([rng.integers(0, n_gt, n), rng.integers(0, n_zy, n)], axis=1).astype(np.uint8)
    cls_d = torch.from_numpy(cls).cuda()
    c = _ctx(2, F, n_gt, n_zy)
    runs = []
    try:
        for b3x in (1, 0, 1):
            c.set_option("hap_b3x", b3x)
            counters = c.hap_eval_counters()
            loss, pred, z = c.hap_eval(xp[:n], xh[:n], cls_d, counters, want_logits=True)
            torch.cuda.synchronize()
            runs.append((loss.cpu().numpy(), pred.cpu().numpy(), z.cpu().numpy(), counters.cpu().numpy()))
    finally:
        c.close()
    return cls, runs


@pytest.mark.parametrize("F,n_gt,n_zy", SCORING_CASES, ids=["F%d-%d+%d" % c for c in SCORING_CASES])
def test_scoring_on_the_big_kernel_gives_the_bits_of_the_small_kernel(F, n_gt, n_zy):
    _require_regimes()
    cls, (big, small, again) = _scoring_runs(F, n_gt, n_zy)
    n = cls.shape[0]
    assert big[0].shape == (n, 2) and big[1].shape == (n, 2) and big[2].shape == (n, n_gt + n_zy)
    for name, other in (("hap_b3x 0", small), ("hap_b3x 1 again", again)):
        for what, a, b in zip(("site losses", "predictions", "logits"), big, other):
            # (bits through an integer view and a verdict of its own: pytest's report of two unequal byte strings of this size is a
            # difflib run that does not end within minutes)
            same = a.shape == b.shape and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))
            if not same:
                raise AssertionError("%s, %s: %d of %d sites differ, max |d| = %.3g" % (name, what, int((a != b).any(-1).sum()), n,
                                                                                   float(np.abs(a.astype(np.float64) - b).max())))
        same_counters = bool(np.array_equal(big[3], other[3]))
        assert same_counters, name
    # the counters are those of the entry's own predictions, one count per site and head
    gcm, zcm = hr.confusion(cls, big[1], n_gt, n_zy)
    assert np.array_equal(big[3], np.concatenate([gcm.reshape(-1), zcm.reshape(-1)])) and big[3].sum() == 2 * n
    assert np.array_equal(big[1], hr.predictions(big[2], n_gt))
    assert np.count_nonzero(gcm.sum(0)) >= 2                              # predictions that differ from site to site


def _softmax64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


@pytest.mark.parametrize("F,n_gt,n_zy", SCORING_CASES, ids=["F%d-%d+%d" % c for c in SCORING_CASES])
def test_scoring_logits_against_the_oracle(F, n_gt, n_zy):
    """the sampled sites of test_big_kernel_against_the_oracle that lie below N: the scoring logits within PROB_ATOL of the oracle's values
    in front of its softmaxes (oracle.hap_forward_logits) and of the float64 restatement tests/hap_eval_rules.forward_logits_f64.
    Printed beside them, not asserted: the float64 softmax of the logits against the oracle's probabilities, and the oracle's own
    distance to float64 - the fp32 oracle stands 1.7e-6 .. 2.2e-6 from the float64 probabilities itself, so no bound under that could be
    held against it.  Measured on an MI355X (docs/rounds/r37.md), F = 105 / F = 17: |logits - oracle| 1.6e-5 / 1.7e-5;
    |logits - float64| 1.3e-5 / 1.1e-5; |softmax64(logits) - oracle probabilities| 3.2e-6 / 3.7e-6."""
    from oracle import oracle
    import torch
    _require_regimes()
    cls, (big, _, _) = _scoring_runs(F, n_gt, n_zy)
    n = cls.shape[0]
    idx = sample_sites(_pass_sites(), 4100 + F)
    idx = idx[idx < n]
    assert idx.size >= SAMPLE - 8 and idx[-1] == n - 1                     # the one site of the last tile is among them
    z = big[2][idx]
    xp, xh = _inputs(F)
    i = torch.from_numpy(idx).cuda()
    xs, hs, ws = xp[i].cpu().numpy(), xh[i].cpu().numpy(), _weights(F, n_gt, n_zy)
    zo = np.concatenate(oracle.hap_forward_logits(ws, xs, hs, n_gt=n_gt, n_zy=n_zy, nthreads=16), axis=1)
    ogt, ozy = oracle.hap_forward(ws, xs, hs, n_gt=n_gt, n_zy=n_zy, nthreads=16)
    z64 = hr.forward_logits_f64(ws, xs, hs)
    assert ogt.std(0).max() > 1e-3 and zo.std(0).max() > 1e-3
    do, dz = np.abs(z - zo).max(), np.abs(z - z64).max()
    dp = max(np.abs(_softmax64(z[:, :n_gt]) - ogt).max(), np.abs(_softmax64(z[:, n_gt:]) - ozy).max())
    d64 = max(np.abs(_softmax64(z64[:, :n_gt]) - ogt).max(), np.abs(_softmax64(z64[:, n_gt:]) - ozy).max())
    print("F %d, classes %d + %d, nsnp_hap_eval on k_hap_lstm_b3x, %d sites: max |logits - oracle| = %.3g, max |logits - float64| = %.3g, "
          "max |softmax64(logits) - oracle probabilities| = %.3g (the oracle's probabilities against float64: %.3g; its logits: %.3g)"
          % (F, n_gt, n_zy, idx.size, do, dz, dp, d64, np.abs(zo - z64).max()))
    assert do <= PROB_ATOL
    assert dz <= PROB_ATOL
    assert dp <= PROB_ATOL


# ---- d. the LDS ballast regimes of k_hap_gemm in fp32 and f16x3 -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "f16x3"])
def test_ballast_regimes_do_not_change_a_bit(prec):
    """F = 105, one context at pass 128 * tiles_all: the four-slice launches at three workgroups per CU (N = 2,560 at 256 CUs), without
    ballast beside two-slice launches at two (4,096), and no ballast at all (8,192) - each equal, bit for bit, to the same sites at
    "hap_pass_sites" 256, and its first 64 sites within PROB_ATOL of the oracle (measured: fp32 2.8e-6, f16x3 1.4e-5 at each N)"""
    F, n_gt, n_zy = 105, 10, 3
    n_cu = _n_cu()
    sites = tr.ballast_sites(n_cu)
    assert [(tr.ballast_per_cu(n, 4, n_cu), tr.ballast_per_cu(n, 2, n_cu)) for n in sites] == [(3, 2), (0, 2), (0, 0)], n_cu
    assert sites[2] == _pass_sites() and sites[0] < sites[1] < sites[2]
    xp, xh = _inputs(F)
    assert float(xp[:sites[2]].abs().max()) < 2048 and float(xh[:sites[2]].abs().max()) < 2048         # where f16x3 keeps the 1e-4 bound
    idx = np.arange(64)
    ogt, ozy = _oracle(F, n_gt, n_zy, idx)
    assert ogt.std(0).max() > 1e-3
    c = _ctx(prec, F, n_gt, n_zy)
    try:
        got = {n: _forward(c, xp[:n], xh[:n]) for n in sites}
        c.set_option("hap_pass_sites", 256)
        small = _forward(c, xp[:sites[2]], xh[:sites[2]])
    finally:
        c.close()
    for n in sites:
        _assert_same_bits(got[n], (small[0][:n], small[1][:n]), "hap_precision %d, N = %d against pass 256" % (prec, n))
        d = max(np.abs(got[n][0][:64].cpu().numpy() - ogt).max(), np.abs(got[n][1][:64].cpu().numpy() - ozy).max())
        print("hap_precision %d, N = %d: max |dp| vs the oracle over the first 64 sites = %.3g" % (prec, n, d))
        assert d < PROB_ATOL
