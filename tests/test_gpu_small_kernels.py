"""The small integer-exact kernels at their edges: nsnp_pileup_postprocess, nsnp_pileup_gather_windows / nsnp_pileup_forward_windows /
nsnp_pileup_call_rows, nsnp_cat_groups.  Every comparison is array_equal against plain numpy written here from the sentences of
include/nanosnp.h, and against the CPU oracle where it has the operation: grid tails, N = 0, the first and last legal centre, unsorted and
repeated centres, other window lengths and depths of exactly 20."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COV = [0, 1, 2, 3, 9, 10, 11, 12]                  # predict.py:63: x[:, 16, [0, 1, 2, 3, 9, 10, 11, 12]]
LIM = (2 ** 31 - 1) // 8                            # eight channels of -LIM still sum inside int32


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- nsnp_pileup_postprocess -------------------------------------------------------------------------------------------------------
def _synthetic_probabilities(rng, n, k):
    """[n,k] float32 rows of eight kinds, cycling: distinct values; a tie for the maximum at a pair of positions that walks through all
    pairs; exactly 1.0 beside exact 0.0s; 1.0 twice; all equal; denormals only (distinct); denormals with a tied maximum; a normal
    maximum tied with itself among denormals"""
    p = rng.random((n, k)).astype(np.float32) * np.float32(0.5) + np.float32(0.01)
    pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
    tiny = np.float32(1e-45)                                          # the smallest denormal
    for r in range(n):
        kind, a, b = r % 8, *pairs[(r // 8) % len(pairs)]
        if kind == 1:
            p[r, a] = p[r, b] = np.float32(0.75)
        elif kind == 2:
            p[r] = 0; p[r, r % k] = 1.0
        elif kind == 3:
            p[r] = 0; p[r, a] = p[r, b] = 1.0
        elif kind == 4:
            p[r] = np.float32(1.0) / np.float32(k)
        elif kind == 5:
            p[r] = (rng.permutation(k) + 1).astype(np.float32) * tiny
        elif kind == 6:
            p[r] = tiny; p[r, a] = p[r, b] = np.float32(7) * tiny
        elif kind == 7:
            p[r] = (rng.permutation(k) + 1).astype(np.float32) * tiny; p[r, a] = p[r, b] = np.float32(0.25)
    return p


@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "no-depth"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100_003])
def test_postprocess_on_synthetic_probabilities(gpu_ctx, n, with_depth):
    """argmax = the FIRST maximum, max = its bits, depth = -(sum of the negative entries of x[n,16,{0,1,2,3,9,10,11,12}]); a grid of 256
    threads per block at its tail; nothing written behind row N (three guard rows per output keep their fill)"""
    import torch
    from nanosnp_amd import _lib
    rng = np.random.default_rng(1000 + n)
    gt, zy = _synthetic_probabilities(rng, n, 21), _synthetic_probabilities(rng, n, 3)
    x = rng.integers(-40, 60, (n, 33, 18), dtype=np.int32)
    if n:
        # the centre column: zeros, positives and large negatives whose eight-channel sum stays inside int32; the other channels and
        # the other columns hold negatives that must not be counted
        big = rng.integers(-LIM, 0, (n, 8))
        mix = rng.integers(0, 4, (n, 8))
        x[:, 16, COV] = np.where(mix == 0, 0, np.where(mix == 1, rng.integers(1, 2 ** 31 - 1, (n, 8)), np.where(mix == 2, big, rng.integers(-60, 0, (n, 8)))))
        x[0, 16, COV] = -LIM
        if n > 1:
            x[n - 1, 16, COV] = 0
    g = 3                                                              # guard rows
    d_gt, d_zy, d_x = _cuda(gt), _cuda(zy), _cuda(x)
    outs = [torch.full((n + g,), 201, dtype=torch.uint8, device="cuda"), torch.full((n + g,), 202, dtype=torch.uint8, device="cuda"),
            torch.full((n + g,), -5.0, dtype=torch.float32, device="cuda"), torch.full((n + g,), -6.0, dtype=torch.float32, device="cuda"),
            torch.full((n + g,), -77, dtype=torch.int32, device="cuda")]
    P = ctypes.c_void_p
    rc = _lib.load().nsnp_pileup_postprocess(gpu_ctx.handle, P(d_gt.data_ptr()), P(d_zy.data_ptr()), P(d_x.data_ptr()) if with_depth else None, n,
                                             *[P(t.data_ptr()) for t in outs[:4]], P(outs[4].data_ptr()) if with_depth else None,
                                             P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    ga, za, gm, zm, depth = [t.cpu().numpy() for t in outs]
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(ga[:n], np.argmax(gt, 1).astype(np.uint8) if n else ga[:0]) and np.array_equal(za[:n], np.argmax(zy, 1).astype(np.uint8) if n else za[:0])
    assert np.array_equal(u(gm[:n]), u(np.max(gt, 1)) if n else u(gm[:0])) and np.array_equal(u(zm[:n]), u(np.max(zy, 1)) if n else u(zm[:0]))
    if n:
        # the same, said without np.argmax: no earlier entry is >= the chosen one, no later entry is > it
        for prob, arg in ((gt, ga[:n]), (zy, za[:n])):
            best = prob[np.arange(n), arg]
            k = np.arange(prob.shape[1])[None]
            assert not ((prob >= best[:, None]) & (k < arg[:, None])).any() and not (prob > best[:, None]).any()
    want_depth = -np.where(x[:, 16][:, COV] < 0, x[:, 16][:, COV].astype(np.int64), 0).sum(1) if n else np.zeros(0, np.int64)
    assert n == 0 or (want_depth.max() == 8 * LIM < 2 ** 31 and (n == 1 or want_depth.min() == 0))
    if with_depth:
        assert np.array_equal(depth[:n].astype(np.int64), want_depth)
    else:
        assert (depth == -77).all()
    assert (ga[n:] == 201).all() and (za[n:] == 202).all() and (gm[n:] == -5.0).all() and (zm[n:] == -6.0).all() and (depth[n:] == -77).all()


def test_postprocess_of_no_sites_through_the_python_binding(gpu_ctx):
    """N = 0 is a no-op like every other call of the ABI, with the NULL pointers empty tensors have - not an argument error"""
    import torch
    e = gpu_ctx.pileup_postprocess(torch.empty((0, 21), device="cuda"), torch.empty((0, 3), device="cuda"),
                                   torch.empty((0, 33, 18), dtype=torch.int32, device="cuda"))
    assert [t.shape[0] for t in e] == [0] * 5
    e = gpu_ctx.pileup_postprocess(torch.empty((0, 21), device="cuda"), torch.empty((0, 3), device="cuda"))
    assert e[4] is None
    lib = __import__("nanosnp_amd._lib", fromlist=["load"]).load()
    assert lib.nsnp_pileup_postprocess(gpu_ctx.handle, None, None, None, 0, None, None, None, None, None, None) == 0
    assert lib.nsnp_pileup_postprocess(gpu_ctx.handle, None, None, None, 1, None, None, None, None, None, None) == -1
    assert lib.nsnp_pileup_postprocess(None, None, None, None, 0, None, None, None, None, None, None) == -1


# ---- windows out of the count matrix -----------------------------------------------------------------------------------------------
def _centres(rng, m, n):
    """n legal centres of a count matrix of m columns (16 .. m - 17), unsorted, with repeats, the first and the last legal one among them"""
    lo, hi = 16, m - 17
    c = rng.integers(lo, hi + 1, n).astype(np.int64)
    if n >= 1:
        c[0] = hi
    if n >= 2:
        c[-1] = lo
    if n >= 5:
        c[2] = c[1]; c[n // 2] = c[1]; c[3] = hi; c[4] = lo            # the same centre side by side and far apart, the ends again
    return c


@pytest.mark.parametrize("m", [33, 5000])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_gather_forward_windows_and_call_rows_at_the_edges(gpu_ctx, pileup_weights, m, n):
    """x[n][t][c] = counts[center_idx[n] - 16 + t][c] for the first and last legal centre (16 and M - 17; M = 33 has only one), unsorted and
    repeated centres; forward_windows = forward on the gathered copy, bit for bit, in fp32 and bf16x3; call_rows = the float64 array
    assembled in numpy"""
    import torch
    from oracle import oracle
    rng = np.random.default_rng(m * 10 + n)
    counts = rng.integers(-30, 40, (m, 18)).astype(np.int32)
    cen = _centres(rng, m, n)
    assert n < 2 or (cen.min() == 16 and cen.max() == m - 17)
    assert n < 5 or (m == 33) or (np.any(np.diff(cen) < 0) and len(set(cen.tolist())) < n)
    want_x = counts[cen[:, None] + np.arange(-16, 17)[None]]           # [n,33,18]
    d_counts, d_cen = _cuda(counts), _cuda(cen)
    x = gpu_ctx.pileup_gather_windows(d_counts, d_cen)
    torch.cuda.synchronize()
    assert x.shape == (n, 33, 18) and np.array_equal(x.cpu().numpy(), want_x)
    assert np.array_equal(oracle.gather_windows(counts, cen), want_x)
    gpu_ctx.pileup_load_weights(pileup_weights)
    try:
        for prec in (0, 2):
            gpu_ctx.set_option("pileup_precision", prec)
            g1, z1 = gpu_ctx.pileup_forward(x)
            g2, z2 = gpu_ctx.pileup_forward_windows(d_counts, d_cen)
            torch.cuda.synchronize()
            assert g1.shape == (n, 21) and z2.shape == (n, 3)
            assert torch.equal(g1, g2) and torch.equal(z1, z2), prec
            if n:
                assert bool(torch.isfinite(g1).all()) and float((g1.sum(1) - 1).abs().max()) < 1e-5
                same = np.flatnonzero(cen == cen[0])                   # a repeated centre gives the same row wherever it stands
                assert np.array_equal(g2.cpu().numpy()[same], np.broadcast_to(g2.cpu().numpy()[same[0]], (same.size, 21)))
    finally:
        gpu_ctx.set_option("pileup_precision", 0)
    pos = rng.integers(1, 2 ** 40, m).astype(np.int64)
    ga = rng.integers(0, 21, n).astype(np.uint8); za = rng.integers(0, 3, n).astype(np.uint8)
    gm = rng.random(n).astype(np.float32); zm = rng.random(n).astype(np.float32)
    rows = gpu_ctx.pileup_call_rows(d_counts, d_cen, _cuda(pos), _cuda(ga), _cuda(za), _cuda(gm), _cuda(zm))
    torch.cuda.synchronize()
    want = np.concatenate([pos[cen][:, None].astype(np.float64), ga[:, None].astype(np.float64), za[:, None].astype(np.float64),
                           gm[:, None].astype(np.float64), zm[:, None].astype(np.float64), counts[cen][:, COV].astype(np.float64)], axis=1)
    assert rows.shape == (n, 13) and np.array_equal(rows.cpu().numpy(), want)


def test_keys_of_high_contig_indices_survive_call_rows_and_rows_unpack(gpu_ctx):
    """the "position" of a call over several contigs is the key (contig index << 36) | position (include/nanosnp.h,
    nsnp_mpileup_tokenise_contigs): nsnp_pileup_call_rows stores it in column 0 of its float64 rows, nsnp_pileup_rows_unpack hands it back
    as int64 - exactly, for the lowest and the highest contig index (2^17 - 1) and position (2^36 - 1) the limits allow"""
    import torch
    keys = np.array([(c << 36) | p for c in (0, 1, (1 << 17) - 1) for p in (1, (1 << 36) - 1)], np.int64)
    assert keys.max() == (1 << 53) - 1 and len(set(keys.tolist())) == 6
    rng = np.random.default_rng(36)
    m, n = 40, 6
    counts = rng.integers(-30, 40, (m, 18)).astype(np.int32)
    cen = np.array([21, 16, 19, 17, 20, 18], np.int64)                 # unsorted: row i holds the key of column cen[i]
    pos = rng.integers(1, 1 << 40, m).astype(np.int64)
    pos[16:22] = keys
    ga = rng.integers(0, 21, n).astype(np.uint8); za = rng.integers(0, 3, n).astype(np.uint8)
    gm = rng.random(n).astype(np.float32); zm = rng.random(n).astype(np.float32)
    rows = gpu_ctx.pileup_call_rows(_cuda(counts), _cuda(cen), _cuda(pos), _cuda(ga), _cuda(za), _cuda(gm), _cuda(zm))
    torch.cuda.synchronize()
    want = keys[cen - 16]
    col0 = rows.cpu().numpy()[:, 0]
    assert col0.dtype == np.float64 and [int(v) for v in col0] == want.tolist()
    for pinned in (False, True):
        kw = dict(pin_memory=True) if pinned else dict(device="cuda")
        outs = (torch.full((n + 2,), -7, dtype=torch.int64, **kw), torch.zeros(n, dtype=torch.uint8, **kw), torch.zeros(n, dtype=torch.uint8, **kw),
                torch.zeros(n, dtype=torch.float32, **kw), torch.zeros(n, dtype=torch.float32, **kw), torch.zeros((n, 8), dtype=torch.float32, **kw))
        gpu_ctx.pileup_rows_unpack(rows, outs)
        torch.cuda.synchronize()
        got = outs[0].cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got[:n], want) and (got[n:] == -7).all()
        assert np.array_equal(got[:n] >> 36, want >> 36) and np.array_equal(outs[1].cpu().numpy(), ga) and np.array_equal(outs[3].cpu().numpy(), gm)


# ---- nsnp_cat_groups ---------------------------------------------------------------------------------------------------------------
def _tag_planes(rng, n, d, L):
    """(read, baseq, mapq) int32 [n,d,L] of one tag.  Rows from a random count of real reads on are -2 padding in all three planes (a tag
    with fewer than 20 reads is what the bins hold), so padding lies INSIDE the first 20 rows; rows behind row 20 hold values that must
    not appear in the output"""
    read = rng.integers(-1, 5, (n, d, L)).astype(np.int32)
    bq = rng.integers(0, 94, (n, d, L)).astype(np.int32)
    mq = rng.integers(0, 61, (n, d, L)).astype(np.int32)
    real = rng.integers(0, 21, n)
    if n == 1:
        real[0] = 7
    else:
        real[0], real[-1] = 0, 20
    pad = np.arange(d)[None, :, None] >= real[:, None, None]
    if d > 20:
        pad = pad & (np.arange(d)[None, :, None] < 20)                 # the rows behind the cut keep other values
        read[:, 20:] += 1000; bq[:, 20:] += 1000; mq[:, 20:] += 2000
    for a in (read, bq, mq):
        a[np.broadcast_to(pad, a.shape)] = -2
    return read, bq, mq


@pytest.mark.parametrize("n", [1, 37, 4099])
@pytest.mark.parametrize("d1,d2", [(20, 20), (21, 64), (64, 20)])
@pytest.mark.parametrize("L", [1, 11, 33])
def test_cat_groups_shapes_and_padding(gpu_ctx, L, d1, d2, n):
    """[N,40,L,5]: the first 20 rows of tag 1, then of tag 2; planes base, baseq, mapq, mask = base != -2, phase 1 | 2 (include/nanosnp.h)"""
    import torch
    from oracle import oracle
    rng = np.random.default_rng(L * 10000 + d1 * 100 + d2 + n)
    t1, t2 = _tag_planes(rng, n, d1, L), _tag_planes(rng, n, d2, L)
    got = gpu_ctx.cat_groups([_cuda(a) for a in t1], [_cuda(a) for a in t2])
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = np.empty((n, 40, L, 5), np.float32)
    for k, t in enumerate((t1, t2)):
        rows = slice(20 * k, 20 * k + 20)
        for plane in range(3):
            want[:, rows, :, plane] = t[plane][:, :20]
        want[:, rows, :, 3] = t[0][:, :20] != -2
        want[:, rows, :, 4] = k + 1
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(oracle.cat_groups(t1, t2), want)
    assert (want[..., 3] == 0).any() and (want[..., 3] == 1).any() and want[..., :3].max() < 100        # padding inside, nothing from behind row 20


def test_cat_groups_refuses_a_depth_below_20_on_either_tag(gpu_ctx):
    from nanosnp_amd import _lib
    rng = np.random.default_rng(9)
    ok, short = _tag_planes(rng, 5, 20, 11), _tag_planes(rng, 5, 19, 11)
    for a, b in ((short, ok), (ok, short), (short, short)):
        with pytest.raises(_lib.NanoSNPError, match="unsupported model dimensions"):
            gpu_ctx.cat_groups([_cuda(t) for t in a], [_cuda(t) for t in b])
    assert gpu_ctx.cat_groups([_cuda(t) for t in ok], [_cuda(t) for t in ok]).shape == (5, 40, 11, 5)
