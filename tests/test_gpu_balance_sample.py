"""ctx.pileup_balance_samples (nsnp_pileup_balance_samples: the training sample list of a PileupModel pass under balance_dataset upsampling)
bit for bit against the numpy restatement tests/balance_rules.py: samples, sizes and meta.

Row counts: 0, 1, 2 (less than a lane each), 63 / 64 / 65 around a wave, 255 / 256 / 257 around a block of the count and list kernels,
511 / 512 / 513 around two, 1,000, 4,095 / 4,096 / 4,097 (the scan kernel's 16 segments take one block each up to 4,096 rows and a run of
two from 4,097), 70,001 (274 blocks, runs of 18).  Layouts: two categories; all 63; one dominating; three tied at the maximum; a category of one row;
every row in one category and equal sizes (status 1: the poisoned buffer stays untouched); runs of one category of 70 rows (longer than a
wave) and of 300 (longer than a block), so that ranks cross waves and blocks; strictly alternating categories; rows with gt >= 21 or
zy >= 3 (counted, never sampled).  Two seeds above 2^32 that differ in the high key word only; two draw counters."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import balance_rules as br

pytestmark = pytest.mark.gpu

SEEDS = ((3 << 32) | 2022, (4 << 32) | 2022)
DRAWS = (0, 7)
ROWS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4095, 4096, 4097, 70001)
LAYOUTS = ("two", "all_63", "dominating", "tied", "single_row", "one_category", "equal_sizes", "runs_70", "runs_300", "alternating", "no_category")
EINVAL = -1                                                              # include/nanosnp.h
POISON = -7


def layout(name, n, rng):
    """cls uint8 [n,4]"""
    i = np.arange(n)
    none = np.zeros(n, bool)
    if name == "two":
        c = np.where(rng.random(n) < 0.8, 0, 5)
    elif name == "all_63":
        c = rng.permutation(np.concatenate([np.arange(63), rng.integers(0, 63, max(n - 63, 0))])[:n]) if n else i
    elif name == "dominating":
        c = np.where(rng.random(n) < 0.9, 0, rng.integers(1, 11, n) * 4)
    elif name == "tied":
        c = rng.permutation(np.concatenate([np.repeat([2, 30, 61], n // 4), rng.integers(40, 50, n - 3 * (n // 4))]))
    elif name == "single_row":
        c = np.where(i % 3 == 0, 12, 13)
        if n:
            c[n // 2] = 59
    elif name == "one_category":
        c = np.full(n, 7)
    elif name == "equal_sizes":
        c = np.concatenate([np.repeat([0, 9, 62], n // 3), np.zeros(n - 3 * (n // 3), np.int64)])
    elif name == "runs_70":
        c = 3 + 41 * ((i // 70) % 2)
    elif name == "runs_300":
        c = 20 * ((i // 300) % 3) + (i < 5)
    elif name == "alternating":
        c = 10 + i % 2
    elif name == "no_category":
        c = rng.integers(0, 8, n) * 9
        none = rng.random(n) < 0.2
    cls = np.zeros((n, 4), np.uint8)
    cls[:, 0], cls[:, 1] = c // 3, c % 3
    cls[:, 2:] = rng.integers(0, 33, (n, 2))
    if name == "equal_sizes":                                            # the rows behind three equal categories are in no category
        none = np.zeros(n, bool)
        none[3 * (n // 3):] = True
        order = rng.permutation(n)
        cls, none = cls[order], none[order]
    k = int(none.sum())
    if k:
        bad = np.arange(k)
        cls[none, 0] = np.where(bad % 2 == 0, 21 + bad % 200, bad % 21)        # gt >= 21, or
        cls[none, 1] = np.where(bad % 2 == 0, bad % 3, 3 + bad % 250)          # zy >= 3
    return np.ascontiguousarray(cls)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if len(a) else torch.empty((0, 4), dtype=torch.uint8, device="cuda")


def _run(ctx, cls, seed, draw, cap=None, meta=None, stream=None, sizes=None):
    """-> (the whole samples buffer, sizes, meta, the restatement's three) with the buffer poisoned first and `cap` entries long
    (default: M + 3)"""
    import torch
    want = br.balance_samples(cls, seed, draw)
    cap = want[0].size + 3 if cap is None else cap
    samples = torch.full((max(cap, 1),), POISON, dtype=torch.int64, device="cuda")[:cap]
    d = _dev(cls)
    torch.cuda.current_stream().synchronize()                             # (the buffers are ready whichever stream runs the entry)
    got, sz, meta = ctx.pileup_balance_samples(d, len(cls), seed, draw=draw, samples=samples, sizes=sizes, meta=meta, stream=stream)
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    return got.cpu().numpy(), None if sz is None else sz.cpu().numpy(), meta.cpu().numpy() if meta.is_cuda else meta.numpy().copy(), want


def _check(res, what):
    got, sizes, meta, (want, want_sizes, want_meta) = res
    assert np.array_equal(meta, want_meta), (what, meta, want_meta)
    if sizes is not None:
        assert np.array_equal(sizes, want_sizes), what
    assert np.array_equal(got[:want.size], want), what
    assert (got[want.size:] == POISON).all(), what                        # nothing behind M; nothing at all with status 1


@pytest.mark.parametrize("n", ROWS)
def test_matches_the_restatement(gpu_ctx, n):
    statuses = set()
    for j, name in enumerate(LAYOUTS):
        cls = layout(name, n, np.random.default_rng([n, j]))
        full = name == "dominating"                                       # both seeds x both draws on one layout, one pair on the others
        lists = {}
        for seed in (SEEDS if full else SEEDS[j % 2:j % 2 + 1]):
            for draw in (DRAWS if full else DRAWS[(j // 2) % 2:(j // 2) % 2 + 1]):
                res = _run(gpu_ctx, cls, seed, draw)
                _check(res, (name, n, seed, draw))
                lists[seed, draw] = res[3][0]
                statuses.add(int(res[2][5]))
                if name in ("one_category", "equal_sizes"):
                    assert res[2][5] == 1 and res[2][0] == 0
                if name == "no_category" and n >= 64:
                    assert res[2][4] > 0 and (br.categories(cls)[res[0][:res[2][0]]] < 63).all()
        if full and n >= 255:                                             # (24 or more draws: two lists cannot agree by chance)
            assert lists[SEEDS[0], 0].size >= 24
            assert not np.array_equal(lists[SEEDS[0], 0], lists[SEEDS[1], 0])            # the high key word reaches the draws
            assert not np.array_equal(lists[SEEDS[0], 0], lists[SEEDS[0], 7])            # and so does the draw counter
    assert 1 in statuses and (n < 63 or 0 in statuses)


def test_meta_in_pinned_and_device_memory_a_side_stream_no_sizes_and_two_runs(gpu_ctx):
    import torch
    cls = layout("dominating", 5000, np.random.default_rng(11))
    pinned = torch.zeros(8, dtype=torch.int64).pin_memory()
    a = _run(gpu_ctx, cls, SEEDS[0], 1, meta=pinned)
    b = _run(gpu_ctx, cls, SEEDS[0], 1, meta=torch.zeros(8, dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = _run(gpu_ctx, cls, SEEDS[0], 1, stream=side)
    d = _run(gpu_ctx, cls, SEEDS[0], 1, sizes=False)                      # sizes NULL
    for i, res in enumerate((a, b, c, d)):
        _check(res, i)
    assert d[1] is None and a[1] is not None
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() == d[0].tobytes()
    auto, sizes, meta = gpu_ctx.pileup_balance_samples(_dev(cls), 5000, SEEDS[0], draw=1)            # the binding's own buffers
    assert auto.numel() == 10000 and np.array_equal(auto[:int(meta[0])].cpu().numpy(), a[3][0]) and np.array_equal(sizes.cpu().numpy(), a[3][1])


def test_refusals_write_nothing(gpu_ctx):
    import torch
    from nanosnp_amd import _lib
    lib = _lib.load()
    cls_np = layout("dominating", 1400, np.random.default_rng(5))
    want, want_sizes, want_meta = br.balance_samples(cls_np, 9, 0)
    M = int(want_meta[0])
    assert M > 100
    cls = _dev(cls_np)
    samples = torch.full((M + 8,), POISON, dtype=torch.int64, device="cuda")
    sizes = torch.full((63,), POISON, dtype=torch.int64, device="cuda")
    meta = torch.full((8,), POISON, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda c, n, s, cap, z, m: lib.nsnp_pileup_balance_samples(gpu_ctx.handle, p(c), n, 9, 0, p(s), cap, p(z), p(m), None)
    assert call(cls, 1400, samples, M - 1, sizes, meta) == EINVAL
    assert call(cls, -1, samples, M + 8, sizes, meta) == EINVAL
    assert call(cls, 1 << 32, samples, M + 8, sizes, meta) == EINVAL
    assert call(cls, 1400, None, M + 8, sizes, meta) == EINVAL
    assert call(None, 1400, samples, M + 8, sizes, meta) == EINVAL
    assert call(cls, 1400, samples, M + 8, sizes, None) == EINVAL
    torch.cuda.synchronize()
    assert (samples == POISON).all() and (sizes == POISON).all() and (meta == POISON).all()
    assert call(cls, 1400, samples, M, sizes, meta) == 0                  # cap == M
    torch.cuda.synchronize()
    assert np.array_equal(samples[:M].cpu().numpy(), want) and (samples[M:] == POISON).all()
    assert np.array_equal(meta.cpu().numpy(), want_meta) and np.array_equal(sizes.cpu().numpy(), want_sizes)
    assert call(None, 0, None, 0, None, meta) == 0                        # no row: status 1, no buffer needed
    torch.cuda.synchronize()
    assert meta.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    one = _dev(layout("one_category", 300, np.random.default_rng(1)))
    assert call(one, 300, None, 0, sizes, meta) == 0                      # status 1 needs no samples buffer either
    torch.cuda.synchronize()
    assert meta.tolist() == [0, 1, 0, 300, 0, 1, 0, 0] and int(sizes[7]) == 300 and int(sizes.sum()) == 300
    with pytest.raises(_lib.NanoSNPError, match="nsnp_pileup_balance_samples"):
        gpu_ctx.pileup_balance_samples(cls, 1400, 9, samples=samples[:M - 1])
    for bad in (dict(cls=cls.cpu()), dict(cls=cls.to(torch.int32)), dict(cls=cls[::2]), dict(meta=torch.zeros(8, dtype=torch.int64)),
                dict(meta=meta[:4]), dict(samples=samples.to(torch.int32)), dict(sizes=sizes[:10]), dict(n=1401), dict(seed=1 << 64),
                dict(draw=1 << 32)):
        kw = dict(cls=cls, n=1400, seed=9, samples=samples, sizes=sizes, meta=meta)
        kw.update(bad)
        with pytest.raises(_lib.NanoSNPError, match="pileup_balance_samples:"):
            gpu_ctx.pileup_balance_samples(**kw)
