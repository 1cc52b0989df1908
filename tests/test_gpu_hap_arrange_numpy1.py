"""k_hap_arrange_numpy1 (nsnp_hap_arrange_reads2, NSNP_TIE_NUMPY1) on the GPU: the reference's HP sort row for row
(tests/golden/hap_arrange_numpy1.npz), NumPy's scalar argsort permutations (tests/golden/argsort_numpy1.npz, the heapsort
fallback included), a fuzz against the restatement tests/numpy1_sort.py, and the stable mode through the new entry."""
import ctypes

import numpy as np
import pytest

from nanosnp_amd import readmatrix
from tests import numpy1_sort
from tests.helpers import FakeSamfile, golden, synth_groups, synth_reads

pytestmark = pytest.mark.gpu

PLANES = ("seq", "bq", "mq", "hap")


def _arrange(ctx, mats, D, n_reads=None, tie_order="numpy1"):
    import torch
    outs = ctx.hap_arrange_reads(*[torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in mats], int(D),
                                 n_reads=None if n_reads is None else torch.from_numpy(np.asarray(n_reads, np.int32)).cuda(),
                                 tie_order=tie_order)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _fixture_sites(z, tag):
    mats = [z[f"in_{nm}"].astype(np.int32) for nm in PLANES]
    n = int(z["n_groups"])
    ins = [np.stack([m[:, z[f"g{g}_{tag}_cols"]] for g in range(n)]) for m in mats]        # [N, R, L]
    want = [[z[f"g{g}_{tag}_out_{nm}"].astype(np.int32) for nm in PLANES] for g in range(n)]
    return ins, want


@pytest.mark.parametrize("tag", ["h", "p"])
def test_numpy1_equals_the_reference_function_row_for_row(gpu_ctx, tag):
    z = np.load(golden("hap_arrange_numpy1.npz"))
    ins, want = _fixture_sites(z, tag)
    depths = [w[0].shape[0] for w in want]
    D = max(depths) + 4
    outs = _arrange(gpu_ctx, ins, D)
    for g, w in enumerate(want):
        d = depths[g]
        assert int(outs[4][g]) == d, g
        for k in range(4):
            assert np.array_equal(outs[k][g][:d], w[k]), (g, PLANES[k])
            assert (outs[k][g][d:] == -2).all()
    # a cut below the depth keeps the reference's own prefix (write_to_bins.py:54-61)
    for D in (17, 40, 90):
        outs = _arrange(gpu_ctx, ins, D)
        for g, w in enumerate(want):
            d = min(depths[g], D)
            assert int(outs[4][g]) == d
            for k in range(4):
                assert np.array_equal(outs[k][g][:d], w[k][:d]), (D, g, PLANES[k])
                assert (outs[k][g][d:] == -2).all()


def test_numpy1_is_not_the_stable_order_on_the_fixture(gpu_ctx):
    z = np.load(golden("hap_arrange_numpy1.npz"))
    ins, want = _fixture_sites(z, "p")
    D = max(w[0].shape[0] for w in want)
    a = _arrange(gpu_ctx, ins, D)
    b = _arrange(gpu_ctx, ins, D, tie_order="stable")
    assert np.array_equal(a[4], b[4])
    assert all(not np.array_equal(a[1][g], b[1][g]) for g in range(len(want)))


def _perm_site(keys, L=3):
    """one site whose centre HP is `keys` and whose bq plane holds the row index: the arranged bq column is the permutation"""
    K = len(keys)
    R = max(K, 1)
    seq = np.ones((1, R, L), np.int32)
    hap = np.zeros((1, R, L), np.int32); hap[0, :K, L // 2] = keys
    bq = np.broadcast_to(np.arange(R, dtype=np.int32)[None, :, None], (1, R, L)).copy()
    mq = np.full((1, R, L), 7, np.int32)
    return (seq, bq, mq, hap), K, R


def test_numpy_permutations_through_the_kernel(gpu_ctx):
    z = np.load(golden("argsort_numpy1.npz"))
    off = z["offsets"]
    heap = set(int(h) for h in z["heapsort"])
    seen_heap = 0
    for i in range(len(off) - 1):
        keys, perm = z["keys"][off[i]:off[i + 1]], z["perms"][off[i]:off[i + 1]]
        mats, K, R = _perm_site(keys)
        outs = _arrange(gpu_ctx, mats, R, n_reads=[K])
        assert int(outs[4][0]) == K, i
        assert np.array_equal(outs[1][0][:K, 1], perm), i
        assert np.array_equal(outs[3][0][:K, 1], keys[perm]), i
        seen_heap += i in heap
    assert seen_heap == len(heap) > 0


@pytest.mark.parametrize("L", [11, 33])
def test_numpy1_fuzz_against_the_restatement(gpu_ctx, L):
    rng = np.random.default_rng(1000 + L)
    extremes = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, 1, 2, 3], np.int64)
    for R in (17, 40, 64, 65, 150, 257, 1000):
        N = 12
        seq = rng.integers(-1, 5, (N, R, L)).astype(np.int32)
        seq[rng.random((N, R)) < 0.2, L // 2] = 0
        hap = rng.integers(1, 4, (N, R, L)).astype(np.int32)
        for n in range(N // 2, N):                                        # half the sites: extreme int32 keys, few distinct values
            hap[n, :, L // 2] = rng.choice(extremes[: 3 + n % 5], R)
        hap[0, :, L // 2] = rng.integers(-2 ** 31, 2 ** 31 - 1, R, endpoint=True)
        bq = rng.integers(0, 94, (N, R, L)).astype(np.int32); mq = rng.integers(0, 61, (N, R, L)).astype(np.int32)
        n_reads = rng.integers(0, R + 1, N); n_reads[:3] = R
        for D in sorted({max(1, R // 3), R, R + 5}):
            outs = _arrange(gpu_ctx, (seq, bq, mq, hap), D, n_reads=n_reads)
            for n in range(N):
                rows = int(n_reads[n])
                keep = np.nonzero(seq[n, :rows, L // 2] != 0)[0]
                order = keep[numpy1_sort.argsort(hap[n, keep, L // 2])][:D]
                d = len(order)
                assert int(outs[4][n]) == d, (R, L, D, n)
                for k, m in enumerate((seq, bq, mq, hap)):
                    assert np.array_equal(outs[k][n][:d], m[n][order]), (R, L, D, n, k)
                    assert (outs[k][n][d:] == -2).all(), (R, L, D, n, k)


def test_group_planes_numpy1_equal_the_reference_function(gpu_ctx):
    import torch
    z = np.load(golden("hap_arrange_numpy1.npz"))
    reads = synth_reads(int(z["deep_seed"]), n_reads=int(z["deep_reads"]))
    groups = synth_groups(int(z["deep_seed"]) + 1, centres=tuple(int(c) for c in z["deep_centres"]))
    rm = readmatrix.read_matrices(FakeSamfile(reads), groups, max_coverage=10000)
    Dh, Dp = (int(v) for v in z["max_depths"])
    cand, hpos, hplanes, pplanes, dh, dp = readmatrix.group_planes(gpu_ctx, rm, Dh, Dp, tie_order="numpy1")
    torch.cuda.synchronize()
    assert cand == z["candidates"].tolist() and hpos == z["haplotype_positions"].tolist()
    for g in range(len(cand)):
        for tag, planes, depth in (("h", hplanes, dh), ("p", pplanes, dp)):
            d = int(depth[g].item())
            assert d == z[f"g{g}_{tag}_out_seq"].shape[0]
            for k, nm in enumerate(PLANES):
                o = planes[k][g].cpu().numpy()
                assert np.array_equal(o[:d], z[f"g{g}_{tag}_out_{nm}"].astype(np.int32)), (g, tag, nm)
                assert (o[d:] == -2).all()


def test_stable_mode_through_the_new_entry_is_bit_identical(gpu_ctx):
    import torch
    from nanosnp_amd import _lib
    rng = np.random.default_rng(9)
    N, R, L, D = 40, 150, 33, 90
    seq = rng.integers(-1, 5, (N, R, L)).astype(np.int32)
    seq[rng.random((N, R)) < 0.25, L // 2] = 0
    hap = rng.choice([1, 2, 3, -2 ** 31, 2 ** 31 - 1], (N, R, L)).astype(np.int32)
    bq = rng.integers(0, 60, (N, R, L)).astype(np.int32); mq = rng.integers(0, 61, (N, R, L)).astype(np.int32)
    ins = [torch.from_numpy(a).cuda() for a in (seq, bq, mq, hap)]
    nr = torch.from_numpy(rng.integers(0, R + 1, N).astype(np.int32)).cuda()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = gpu_ctx.lib

    def run(tie_order):
        outs = [torch.full((N, D, L), 99, dtype=torch.int32, device="cuda") for _ in range(4)]
        dep = torch.full((N,), 99, dtype=torch.int32, device="cuda")
        if tie_order is None:
            rc = lib.nsnp_hap_arrange_reads(gpu_ctx.handle, *[P(t) for t in ins], P(nr), N, R, L, D, *[P(o) for o in outs], P(dep), None)
        else:
            rc = lib.nsnp_hap_arrange_reads2(gpu_ctx.handle, *[P(t) for t in ins], P(nr), N, R, L, D, tie_order,
                                             *[P(o) for o in outs], P(dep), None)
        torch.cuda.synchronize()
        return rc, [o.cpu().numpy() for o in outs] + [dep.cpu().numpy()]

    rc0, old = run(None)
    rc1, new = run(0)
    assert rc0 == rc1 == 0
    assert all(np.array_equal(a, b) for a, b in zip(old, new))
    _, np1 = run(1)
    assert np.array_equal(np1[4], old[4])
    rc2, untouched = run(2)
    assert rc2 == -1                                                          # NSNP_EINVAL, nothing launched
    assert all((u == 99).all() for u in untouched)
    with pytest.raises(_lib.NanoSNPError):
        gpu_ctx.hap_arrange_reads(*ins, D, tie_order="numpy2")
