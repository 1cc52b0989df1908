"""The software-pipelined fp32 layer-0 kernel (k_pileup_l0_rsxw, context option "l0_weave" 1: the count projection of step s+1 issued
in step s, under the cell and in front of the barrier - docs/rounds/r21.md) returns, bit for bit, what k_pileup_l0_rsx returns on the
same context for the same integer windows.  Every case runs the 33-step pipeline's prologue (x of steps 0 and 1 staged, step 0
projected) and its drain (the staging of steps s+2 and s+3 beyond the last step); the sizes cover a partial last workgroup and the rows
past N that restage the last site; the split-level case puts counts beyond +-256 on the steps at which the pipeline changes shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 33, 200)
DEFAULT = 1                                             # nsnp_ctx_create's "l0_weave"


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
    """run() under l0_weave 0 and 1 -> the two tuples of host arrays"""
    import torch
    out = []
    for weave in (0, 1):
        ctx.set_option("l0_weave", weave)
        try:
            res = run()
            torch.cuda.synchronize()
        finally:
            ctx.set_option("l0_weave", DEFAULT)
        out.append(tuple(t.cpu().numpy() for t in res))
    return out


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(off, on):
    assert len(off) == len(on)
    for a, b in zip(off, on):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n", SIZES)
def test_same_bits_as_the_unwoven_kernel(n, ctx):
    import torch
    x = torch.from_numpy(_counts(2100 + n, (n, 33, 18))).cuda()
    off, on = _both(ctx, lambda: ctx.pileup_forward(x))
    assert off[0].shape == (n, 21) and off[1].shape == (n, 3)
    _same(off, on)
    assert np.isfinite(off[0]).all() and np.isfinite(off[1]).all()


@pytest.fixture(scope="module")
def windows():
    import torch
    rng = np.random.default_rng(2150)
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


# Split level of a (16-site group, step): 257 = 256 + 1 needs two bf16 terms (level 1), 65,536 is one bf16 beyond +-256 (the split
# path at level 0), 2^24 + 3 casts to the float 2^24 + 4 (level 1), 65,793 = 65,536 + 256 + 1 needs three terms (level 2).  The
# forward direction reads column t in step t, the backward direction in step 32 - t: a count at column t tests both.
# (site, column, channel, count); sites 0-15, 16-31 and 32-47 are three workgroups per direction, channels 0-7 / 8-15 / 16-17 the
# three staging waves
SPLIT_COUNTS = (
    # group 0: the prologue's projection (step 0) and the last step, which projects nothing, in both directions; a step alone
    # between level-0 neighbours; the split path at level 0
    (3, 0, 3, 257), (9, 32, 12, (1 << 24) + 3), (0, 10, 17, 257), (15, 14, 5, 65536),
    # group 1: step 1, the first projection issued inside a step, and step 31; two consecutive steps of different non-zero level,
    # one in each x buffer, 1 -> 2 forwards and 2 -> 1 backwards
    (17, 1, 12, 257), (30, 31, 17, (1 << 24) + 3), (16, 20, 3, 257), (31, 21, 12, 65793),
    # group 2: level 2 in the prologue and on the last step; two consecutive steps of level 1; a negative count
    (32, 0, 17, 65793), (40, 32, 3, 65793), (47, 5, 12, (1 << 24) + 3), (33, 6, 0, 257), (36, 16, 9, -257),
)


def test_split_levels_at_every_shape_of_the_pipeline(ctx):
    import torch
    x = _counts(2160, (48, 33, 18))
    for site, t, ch, v in SPLIT_COUNTS:
        x[site, t, ch] = v
    xd = torch.from_numpy(x).cuda()
    off, on = _both(ctx, lambda: ctx.pileup_forward(xd))
    _same(off, on)
    # the sites of a group whose own counts stay small do not see their neighbours' split level (planes 1 and 2 add exact zeros)
    plain = _counts(2160, (48, 33, 18))
    ref, _ = _both(ctx, lambda: ctx.pileup_forward(torch.from_numpy(plain).cuda()))
    untouched = np.setdiff1d(np.arange(48), [s for s, _, _, _ in SPLIT_COUNTS])
    for a, b in zip(ref, on):
        assert np.array_equal(_bits(a)[untouched], _bits(b)[untouched])


def test_two_forwards_back_to_back(ctx):
    """different N on one stream, no synchronisation between them: nothing the first launch staged two steps ahead may reach the
    second"""
    import torch
    xa = torch.from_numpy(_counts(2161, (200, 33, 18))).cuda()
    xb = torch.from_numpy(_counts(2162, (17, 33, 18))).cuda()

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


def test_option_values(ctx):
    import torch
    assert ctx.lib.nsnp_ctx_set_option(ctx.handle, b"l0_weave", 2) == -1            # NSNP_EINVAL
    assert ctx.lib.nsnp_ctx_set_option(ctx.handle, b"l0_weave", -1) == -1
    # "l0_weave" shapes the kernel of "l0_register_stationary" 2 only
    x = torch.from_numpy(_counts(2170, (33, 33, 18))).cuda()
    ctx.set_option("l0_register_stationary", 1)
    try:
        off, on = _both(ctx, lambda: ctx.pileup_forward(x))
    finally:
        ctx.set_option("l0_register_stationary", 2)
    _same(off, on)
