"""The fp32 layer-0 kernel that stages the whole window once (k_pileup_l0_rsxp, context option "l0_prestage" 1: the workgroup's 16
windows converted to a read-only LDS image in front of the step loop, the loop without staging - docs/rounds/r24.md) returns, bit for
bit, what k_pileup_l0_rsxw ("l0_prestage" 0) returns on the same context for the same integer windows.  A workgroup with a count beyond
+-256 runs k_pileup_l0_rsxw's own loop; the choice is per workgroup, so the split case puts such workgroups beside one that takes the
fast loop."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 33, 200)
DEFAULT = 1                                             # nsnp_ctx_create's "l0_prestage"


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
    """run() under l0_prestage 0 and 1 -> the two tuples of host arrays"""
    import torch
    out = []
    for pre in (0, 1):
        ctx.set_option("l0_prestage", pre)
        try:
            res = run()
            torch.cuda.synchronize()
        finally:
            ctx.set_option("l0_prestage", DEFAULT)
        out.append(tuple(t.cpu().numpy() for t in res))
    return out


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(off, on):
    assert len(off) == len(on)
    for a, b in zip(off, on):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n", SIZES)
def test_same_bits_as_per_step_staging(n, ctx):
    import torch
    x = torch.from_numpy(_counts(2400 + n, (n, 33, 18))).cuda()
    off, on = _both(ctx, lambda: ctx.pileup_forward(x))
    assert off[0].shape == (n, 21) and off[1].shape == (n, 3)
    _same(off, on)
    assert np.isfinite(off[0]).all() and np.isfinite(off[1]).all()


@pytest.fixture(scope="module")
def windows():
    """50 overlapping windows in no order over exactly 120 columns: centre 16 starts at offset 0, centre 103 ends on the array's
    last element; odd centres start 8-byte aligned only ((c - 16) * 72 bytes), even ones 16-byte aligned"""
    import torch
    rng = np.random.default_rng(2450)
    counts = rng.integers(-15, 61, (120, 18)).astype(np.int32)
    rest = rng.permutation(np.arange(17, 103, dtype=np.int64))[:48]
    idx = rng.permutation(np.concatenate([np.array([16, 103], dtype=np.int64), rest])).copy()
    assert len(idx) == 50 and (idx % 2 == 0).any() and (idx % 2 == 1).any()
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


# Counts beyond +-256 at columns 0, 1, 16, 31 and 32 (the prologue's projection, the first step, the centre, the last projection and
# the last step, in both directions) in groups 0 (sites 0-15) and 2 (sites 32-47); group 1 stays within +-256 and takes the fast loop
# between two workgroups that do not.  257 and -257 need two bf16 terms, 65,536 is one bf16 beyond +-256, 2^24 + 3 casts to the float
# 2^24 + 4, 65,793 needs three terms.  (site, column, channel, count)
SPLIT_COUNTS = (
    (3, 0, 3, 257), (9, 1, 12, -257), (0, 16, 17, 65536), (15, 31, 5, (1 << 24) + 3), (7, 32, 0, 65793),
    (32, 0, 17, 65793), (40, 1, 3, (1 << 24) + 3), (47, 16, 12, -257), (33, 31, 0, 257), (36, 32, 9, 65536),
)


def test_split_counts_take_the_general_loop(ctx):
    import torch
    x = _counts(2460, (48, 33, 18))
    for site, t, ch, v in SPLIT_COUNTS:
        x[site, t, ch] = v
    assert np.abs(x[16:32]).max() <= 256
    xd = torch.from_numpy(x).cuda()
    off, on = _both(ctx, lambda: ctx.pileup_forward(xd))
    _same(off, on)
    # the sites whose own counts were not changed equal the run without any large count
    plain = torch.from_numpy(_counts(2460, (48, 33, 18))).cuda()
    _, ref = _both(ctx, lambda: ctx.pileup_forward(plain))
    untouched = np.setdiff1d(np.arange(48), [s for s, _, _, _ in SPLIT_COUNTS])
    assert len(untouched) == 38
    for a, b in zip(ref, on):
        assert np.array_equal(_bits(a)[untouched], _bits(b)[untouched])


def test_counts_of_exactly_256_take_the_fast_loop(ctx):
    """+-256 is split level 0: one bf16 term, the fast loop's arithmetic"""
    import torch
    x = _counts(2470, (33, 33, 18))
    x[2, 0, 0] = 256
    x[2, 32, 17] = -256
    x[20, 16, 8] = -256
    x[32, 1, 16] = 256
    xd = torch.from_numpy(x).cuda()
    off, on = _both(ctx, lambda: ctx.pileup_forward(xd))
    _same(off, on)


def test_two_forwards_back_to_back(ctx):
    """different N on one stream, no synchronisation between them: nothing of the first launch's image may reach the second"""
    import torch
    xa = torch.from_numpy(_counts(2461, (200, 33, 18))).cuda()
    xb = torch.from_numpy(_counts(2462, (17, 33, 18))).cuda()

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
    assert ctx.lib.nsnp_ctx_set_option(ctx.handle, b"l0_prestage", 2) == -1         # NSNP_EINVAL
    assert ctx.lib.nsnp_ctx_set_option(ctx.handle, b"l0_prestage", -1) == -1
    # "l0_prestage" shapes the kernel of "l0_register_stationary" 2 with "l0_weave" 1 only
    x = torch.from_numpy(_counts(2480, (33, 33, 18))).cuda()
    for name, value, back in (("l0_weave", 0, 1), ("l0_register_stationary", 1, 2)):
        ctx.set_option(name, value)
        try:
            off, on = _both(ctx, lambda: ctx.pileup_forward(x))
        finally:
            ctx.set_option(name, back)
        _same(off, on)
