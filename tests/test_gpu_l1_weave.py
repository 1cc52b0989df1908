"""The software-pipelined fp32 layer-1 kernel (k_pileup_l1_rs4w, context option "l1_weave" 1: the cell of step s in the MFMA gaps of
the input projection of step s+1, half of W_hh in LDS - docs/rounds/r19.md) returns, bit for bit, what k_pileup_l1_rs4 returns on the
same context for the same seeded integer windows.  Every case runs the 17-step pipeline's prologue and its drain (the h0 rows of
steps s+2 and s+3 beyond the last step); the sizes cover a partial last workgroup and the rows past N that restage the last site."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 33, 200)


def _counts(seed, shape):
    return np.random.default_rng(seed).integers(-15, 61, shape).astype(np.int32)


@pytest.fixture(scope="module")
def ctx(pileup_weights):
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    c.pileup_load_weights(pileup_weights)
    yield c
    c.close()


def _both(ctx, run):
    """run() under l1_weave 0 and 1 -> the two tuples of host arrays"""
    import torch
    out = []
    for weave in (0, 1):
        ctx.set_option("l1_weave", weave)
        try:
            res = run()
            torch.cuda.synchronize()
        finally:
            ctx.set_option("l1_weave", 1)               # the default
        out.append(tuple(t.cpu().numpy() for t in res))
    return out


def _same(off, on):
    assert len(off) == len(on)
    for a, b in zip(off, on):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    assert np.isfinite(off[0]).all() and np.isfinite(off[1]).all()


@pytest.mark.parametrize("n", SIZES)
def test_same_bits_as_the_unwoven_kernel(n, ctx):
    import torch
    x = torch.from_numpy(_counts(1900 + n, (n, 33, 18))).cuda()
    off, on = _both(ctx, lambda: ctx.pileup_forward(x))
    assert off[0].shape == (n, 21) and off[1].shape == (n, 3)
    _same(off, on)


@pytest.fixture(scope="module")
def windows():
    import torch
    rng = np.random.default_rng(1950)
    counts = rng.integers(-15, 61, (120, 18)).astype(np.int32)
    idx = rng.permutation(np.arange(16, 104, dtype=np.int64))[:50].copy()       # overlapping windows, in no order
    return torch.from_numpy(counts).cuda(), torch.from_numpy(idx).cuda()


def test_windows_read_in_place(ctx, windows):
    counts, idx = windows
    off, on = _both(ctx, lambda: ctx.pileup_forward_windows(counts, idx))
    assert off[0].shape == (50, 21)
    _same(off, on)


def test_windows_calls(ctx, windows):
    counts, idx = windows
    off, on = _both(ctx, lambda: ctx.pileup_forward_windows_calls(counts, idx))
    assert len(off) == 6 and off[2].dtype == np.uint8 and off[2].shape == (50,)
    _same(off, on)


def test_two_forwards_back_to_back(ctx):
    """different N on one stream, no synchronisation between them: nothing of the first launch (the LDS weight image, a staging
    buffer) may reach the second"""
    import torch
    xa = torch.from_numpy(_counts(1961, (200, 33, 18))).cuda()
    xb = torch.from_numpy(_counts(1962, (17, 33, 18))).cuda()

    def run():
        ga, za = ctx.pileup_forward(xa)
        gb, zb = ctx.pileup_forward(xb)
        return ga, za, gb, zb
    off, on = _both(ctx, run)
    _same(off, on)
    # and the second forward alone gives what it gave behind the first
    alone_off, alone_on = _both(ctx, lambda: ctx.pileup_forward(xb))
    _same(alone_off, on[2:])
    _same(alone_on, on[2:])
