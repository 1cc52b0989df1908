"""ctx.hap_train_samples (nsnp_hap_train_samples: the training sample list of a HaplotypeModel pass under pn_value upsampling) bit for bit
against the numpy restatement tests/hap_sample_rules.py.

Sizes: kept 0, 1, 5 (less than a lane each), 1025 (a scan lane's share becomes 2 rows), 5000 (5 rows per scan lane, 20 workgroups of the
flag kernels, up to 69 of the placing kernel); refcall counts 90 (int(90 * 0.7) == 62), 999, 1000, 1001 and 2090 around the block cut;
all-refcall, all-variant and single-variant inputs; pn_value 0 (no draws), 0.7 (the shipped one), 1.0 and 2.5 (more draws than refcalls);
two seeds above 2^32 that differ in the high key word only; two draw counters."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import hap_sample_rules as sr

pytestmark = pytest.mark.gpu

PN_VALUES = (0.0, 0.7, 1.0, 2.5)
SEEDS = ((3 << 32) | 2021, (4 << 32) | 2021)
DRAWS = (0, 7)
CASES = [(0, 0), (1, 1), (1, 0), (5, 3), (5, 5), (5, 0), (1025, 90), (1025, 999), (1025, 1024), (1400, 1000), (1400, 1001), (5000, 2090),
         (5000, 4999), (5000, 5000), (5000, 0)]
EINVAL = -1                                                              # include/nanosnp.h
POISON = -7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ctx, cls, pn, seed, draw, cap=None, meta=None, stream=None):
    """-> (the whole samples buffer, meta) with the buffer poisoned first and `cap` entries long (default: M + 3)"""
    import torch
    want, want_meta = sr.train_samples(cls, pn, seed, draw)
    cap = want.size + 3 if cap is None else cap
    samples = torch.full((max(cap, 1),), POISON, dtype=torch.int64, device="cuda")[:cap]
    d = _dev(cls) if len(cls) else torch.empty((0, 2), dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()                             # (the buffers are ready whichever stream runs the entry)
    got, meta = ctx.hap_train_samples(d, len(cls), pn, seed, draw=draw, samples=samples, meta=meta, stream=stream)
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    return got.cpu().numpy(), meta.cpu().numpy() if meta.is_cuda else meta.numpy().copy(), want, want_meta


@pytest.mark.parametrize("kept,n_ref", CASES)
def test_matches_the_restatement(gpu_ctx, kept, n_ref):
    cls = sr.flags(kept, n_ref, np.random.default_rng(1000 * kept + n_ref))
    lists = {}
    for pn in PN_VALUES:
        for seed in SEEDS:
            for draw in DRAWS:
                got, meta, want, want_meta = _run(gpu_ctx, cls, pn, seed, draw)
                assert np.array_equal(meta, want_meta), (pn, seed, draw)
                assert np.array_equal(got[:want.size], want), (pn, seed, draw)
                assert (got[want.size:] == POISON).all()                  # nothing behind M
                lists[pn, seed, draw] = want
    if n_ref >= 90 and kept - n_ref >= 100:                               # (62 or more draws among 100 or more variants: two lists cannot agree
        # by chance)  the high key word and the draw counter reach the device's draws
        assert not np.array_equal(lists[0.7, SEEDS[0], 0], lists[0.7, SEEDS[1], 0])
        assert not np.array_equal(lists[0.7, SEEDS[0], 0], lists[0.7, SEEDS[0], 7])


def test_meta_in_pinned_and_device_memory_a_side_stream_and_two_runs(gpu_ctx):
    import torch
    cls = sr.flags(5000, 2090, np.random.default_rng(11))
    pinned = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    a = _run(gpu_ctx, cls, 0.7, SEEDS[0], 1, meta=pinned)
    b = _run(gpu_ctx, cls, 0.7, SEEDS[0], 1, meta=torch.zeros(4, dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = _run(gpu_ctx, cls, 0.7, SEEDS[0], 1, stream=side)
    for got, meta, want, want_meta in (a, b, c):
        assert np.array_equal(meta, want_meta) and np.array_equal(got[:want.size], want)
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes()
    assert a[2].size == 2090 + 2 * 700 + 62
    auto, meta = gpu_ctx.hap_train_samples(_dev(cls), 5000, 0.7, SEEDS[0], draw=1)                   # the binding's own buffer
    assert auto.numel() >= a[2].size and np.array_equal(auto[:int(meta[0])].cpu().numpy(), a[2])


def test_refusals_write_nothing(gpu_ctx):
    import torch
    from nanosnp_amd import _lib
    lib = _lib.load()
    cls_np = sr.flags(1400, 1001, np.random.default_rng(5))
    want, want_meta = sr.train_samples(cls_np, 0.7, 9, 0)
    M = int(want_meta[0])
    assert M == 1001 + 700
    cls = _dev(cls_np)
    samples = torch.full((M + 8,), POISON, dtype=torch.int64, device="cuda")
    meta = torch.full((4,), POISON, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda c, kept, pn, s, cap, m: lib.nsnp_hap_train_samples(gpu_ctx.handle, p(c), kept, C.c_double(pn), 9, 0, p(s), cap, p(m), None)
    assert call(cls, 1400, 0.7, samples, M - 1, meta) == EINVAL
    assert call(cls, 1400, -0.5, samples, M + 8, meta) == EINVAL
    assert call(cls, 1400, float("nan"), samples, M + 8, meta) == EINVAL
    assert call(cls, 1400, float("inf"), samples, M + 8, meta) == EINVAL
    assert call(cls, -1, 0.7, samples, M + 8, meta) == EINVAL
    assert call(cls, 1400, 0.7, None, M + 8, meta) == EINVAL
    assert call(None, 1400, 0.7, samples, M + 8, meta) == EINVAL
    assert call(cls, 1400, 0.7, samples, M + 8, None) == EINVAL
    torch.cuda.synchronize()
    assert (samples == POISON).all() and (meta == POISON).all()
    assert call(cls, 1400, 0.7, samples, M, meta) == 0                    # cap == M
    torch.cuda.synchronize()
    assert np.array_equal(samples[:M].cpu().numpy(), want) and (samples[M:] == POISON).all() and np.array_equal(meta.cpu().numpy(), want_meta)
    assert call(None, 0, 0.7, None, 0, meta) == 0                         # nothing kept: an empty list, no buffer needed
    torch.cuda.synchronize()
    assert meta.tolist() == [0, 0, 0, 0]
    with pytest.raises(_lib.NanoSNPError, match="nsnp_hap_train_samples"):
        gpu_ctx.hap_train_samples(cls, 1400, 0.7, 9, samples=samples[:M - 1])
    for bad in (dict(cls=cls.cpu()), dict(cls=cls.to(torch.int32)), dict(cls=cls[::2]), dict(meta=torch.zeros(4, dtype=torch.int64)),
                dict(samples=samples.to(torch.int32)), dict(pn_value=-1.0), dict(kept=1401)):
        kw = dict(cls=cls, kept=1400, pn_value=0.7, seed=9, samples=samples, meta=meta)
        kw.update(bad)
        with pytest.raises(_lib.NanoSNPError, match="hap_train_samples:"):
            gpu_ctx.hap_train_samples(**kw)
