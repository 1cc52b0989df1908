"""fp32 PileupModel layer 0 with the input block on the bf16 matrix pipe, exact ("l0_register_stationary" 2, the default of
pileup_precision 0): fp32 weights as three bf16 terms times integer counts as one to three bf16 terms, every partial product exact
in the fp32 accumulator.  Against the oracle, against the fp32-MFMA kernel ("l0_register_stationary" 1) and against float64."""
import numpy as np
import pytest

from tests.helpers import PROB_ATOL, golden

pytestmark = pytest.mark.gpu

CKPTS = {"ont_pileup": None, "hg001_e186": "pileup_fwd_hg001_e186.npz"}


def _ctx(weights, l0=None):
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    c.pileup_load_weights(weights)
    if l0 is not None:
        c.set_option("l0_register_stationary", l0)
    return c


def _fwd(c, x):
    import torch
    g, z = c.pileup_forward(x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda())
    torch.cuda.synchronize()
    return g, z


def _synth30(n, seed):
    from nanosnp_amd import host
    from oracle import oracle
    cols = host.synth_columns(seed, n + 32, coverage=30, window=33)
    counts, _, _ = oracle.encode_columns(cols.bases, cols.col_off, cols.ref)
    centers = np.arange(16, 16 + n, dtype=np.int64)
    return np.ascontiguousarray(oracle.gather_windows(counts, centers), np.int32)


def test_option_values(pileup_weights):
    from nanosnp_amd import _lib
    c = _ctx(pileup_weights)
    for v in (0, 1, 2):
        c.set_option("l0_register_stationary", v)
    for bad in (3, -1):
        with pytest.raises(_lib.NanoSNPError):
            c.set_option("l0_register_stationary", bad)
    c.close()


@pytest.mark.parametrize("ckpt", list(CKPTS))
def test_goldens_synthetic_and_float64(ckpt):
    from oracle import oracle
    from tests.helpers import load_pileup_weights
    w = load_pileup_weights(golden(CKPTS[ckpt]) if CKPTS[ckpt] else None)
    new, old = _ctx(w), _ctx(w, 1)
    z = np.load(golden("pileup_fwd.npz"))
    if ckpt == "ont_pileup":
        g, zz = _fwd(new, z["x"])
        assert np.abs(g.cpu().numpy() - z["gt"]).max() < PROB_ATOL and np.abs(zz.cpu().numpy() - z["zy"]).max() < PROB_ATOL
    x = _synth30(1100, 20261016)
    gn, zn = _fwd(new, x)
    go, zo = _fwd(old, x)
    gn, zn, go, zo = (t.cpu().numpy() for t in (gn, zn, go, zo))
    og, oz = oracle.pileup_forward(w, x, nthreads=8)
    assert np.abs(gn - og).max() < PROB_ATOL and np.abs(zn - oz).max() < PROB_ATOL
    assert np.abs(gn - go).max() < 5e-6 and np.abs(zn - zo).max() < 5e-6
    fg, fz = oracle.pileup_forward_f64(w, x)
    err_new = max(np.abs(gn - fg).max(), np.abs(zn - fz).max())
    err_old = max(np.abs(go - fg).max(), np.abs(zo - fz).max())
    assert err_new <= max(1.2 * err_old, 1e-6), (err_new, err_old)
    new.close(); old.close()


SPLIT_COUNTS = [256, -256, 257, -257, 65536, -40000, 2**20 + 3, 2**24 + 3]


@pytest.mark.parametrize("ckpt", list(CKPTS))
def test_split_levels_alone_and_mixed(ckpt):
    """counts that take one, two and three bf16 terms, in a site group alone and among small-count sites of other groups and of the
    same group: every site equals, bit for bit, its result in a 16-site batch of its own group, and matches the oracle"""
    import torch
    from oracle import oracle
    from tests.helpers import load_pileup_weights
    w = load_pileup_weights(golden(CKPTS[ckpt]) if CKPTS[ckpt] else None)
    rng = np.random.default_rng(7)
    n = 16 * 24
    x = (rng.integers(0, 40, (n, 33, 18)) - 8).astype(np.int32)
    for i, v in enumerate(SPLIT_COUNTS):
        x[16 * i + 3, 5 + i, i % 18] = v                      # group i: one large count at one step
        x[16 * (8 + i) + (i % 16), :, (i + 3) % 18] = v        # group 8 + i: at every step
    x[16 * 20 + 1, 7, 2] = 2**24 + 3; x[16 * 20 + 2, 7, 2] = 257   # group 20: two levels in one step
    xt = torch.from_numpy(x).cuda()
    c = _ctx(w)
    g, z = _fwd(c, xt)
    for grp in range(n // 16):
        a = 16 * grp
        gs, zs = _fwd(c, xt[a:a + 16].contiguous())
        assert torch.equal(gs, g[a:a + 16]) and torch.equal(zs, z[a:a + 16]), grp
    # a site whose own counts are small gives the same bits in a group that runs the extra products
    clean = x.copy(); clean[16 * 20 + 1, 7, 2] = 1; clean[16 * 20 + 2, 7, 2] = 1
    gc, zc = _fwd(c, clean[16 * 20:16 * 21])
    keep = [k for k in range(16) if k not in (1, 2)]
    assert torch.equal(gc[keep], g[16 * 20 + np.array(keep)]) and torch.equal(zc[keep], z[16 * 20 + np.array(keep)])
    og, oz = oracle.pileup_forward(w, x, nthreads=8)
    assert np.abs(g.cpu().numpy() - og).max() < PROB_ATOL and np.abs(z.cpu().numpy() - oz).max() < PROB_ATOL
    c.close()


@pytest.mark.parametrize("ckpt", list(CKPTS))
def test_stale_split_planes_of_another_staging_wave(ckpt):
    """Counts are staged by three waves (thread 9 site + piece: sites 1 and 4 by wave 0, 10 by wave 1, channel 17 of site 15 by
    wave 2) into two buffers.  Site 10 (wave 1)
    is large at position 5, site 1 (wave 0) at position 7: the same buffer two steps apart in either direction.  At the later step
    the workgroup runs the extra products while the other wave's own counts are small, so its planes 1 and 2 must hold zeros and
    not its large count of two steps before.  Every site but the one changed must keep its bits when site 1 or site 10 is made
    small."""
    import torch
    from oracle import oracle
    from tests.helpers import load_pileup_weights
    w = load_pileup_weights(golden(CKPTS[ckpt]) if CKPTS[ckpt] else None)
    rng = np.random.default_rng(17)
    x = (rng.integers(0, 40, (48, 33, 18)) - 8).astype(np.int32)
    for g in range(3):                                   # three groups: two and three bf16 terms, and a negative count
        v = (70000, 2**24 + 3, -40000)[g]
        x[16 * g + 10, 5, 3] = v; x[16 * g + 1, 7, 3] = v
        x[16 * g + 15, 9, 17] = v; x[16 * g + 4, 11, 17] = v            # wave 2 against wave 0 as well
    c = _ctx(w)
    g0, z0 = _fwd(c, x)
    for site, pos, ch in ((1, 7, 3), (10, 5, 3), (15, 9, 17), (4, 11, 17)):
        y = x.copy()
        for g in range(3):
            y[16 * g + site, pos, ch] = 5
        g1, z1 = _fwd(c, y)
        keep = np.array([k for k in range(48) if k % 16 != site])
        assert torch.equal(g1[keep], g0[keep]) and torch.equal(z1[keep], z0[keep]), site
    og, oz = oracle.pileup_forward(w, x, nthreads=8)
    assert np.abs(g0.cpu().numpy() - og).max() < PROB_ATOL and np.abs(z0.cpu().numpy() - oz).max() < PROB_ATOL
    c.close()


def test_int32_extremes_are_finite_and_agree_with_the_fp32_kernel(pileup_weights):
    import torch
    rng = np.random.default_rng(3)
    x = (rng.integers(0, 40, (64, 33, 18)) - 8).astype(np.int32)
    x[2, 4, 1] = 2**31 - 1; x[20, 30, 17] = -2**31; x[40, :, 0] = 2**31 - 1; x[41, :, 9] = -2**31
    # near the top of the int32 range with two and three bf16 terms (the casts are exact: multiples of 128 below 2^31)
    x[8, 6, 2] = 2**30 + 2**21 + 2**13 + 384; x[24, 12, 5] = -(2**31 - 640); x[45, :, 7] = 2**31 - 2**23 - 2**14
    new, old = _ctx(pileup_weights), _ctx(pileup_weights, 1)
    gn, zn = _fwd(new, x)
    go, zo = _fwd(old, x)
    assert torch.isfinite(gn).all() and torch.isfinite(zn).all()
    assert (gn - go).abs().max().item() < 5e-6 and (zn - zo).abs().max().item() < 5e-6
    for a in (0, 16, 32):
        gs, zs = _fwd(new, torch.from_numpy(x[a:a + 16].copy()).cuda())
        assert torch.equal(gs, gn[a:a + 16]) and torch.equal(zs, zn[a:a + 16])
    new.close(); old.close()


def test_deterministic_permutation_and_chunking_invariant(pileup_weights):
    import torch
    x = _synth30(4096 + 77, 99)
    x[100, 3, 4] = 70000; x[2000, 20, 11] = -300
    xt = torch.from_numpy(x).cuda()
    c = _ctx(pileup_weights)
    g, z = _fwd(c, xt)
    g2, z2 = _fwd(c, xt)
    assert torch.equal(g, g2) and torch.equal(z, z2)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(len(x))).cuda()
    gp, zp = _fwd(c, xt[perm].contiguous())
    assert torch.equal(gp, g[perm]) and torch.equal(zp, z[perm])
    for n in (1, 15, 16, 17, 33, 4096 + 77):
        gs, zs = _fwd(c, xt[:n].contiguous())
        assert torch.equal(gs, g[:n]) and torch.equal(zs, z[:n]), n
    c.reserve(1024)                                             # internal chunks of 1024 sites
    gc, zc = _fwd(c, xt)
    assert torch.equal(gc, g) and torch.equal(zc, z)
    c.close()
