"""nsnp_pileup_label_sites_keys beyond the sizes tests/test_gpu_train_bins.py gives it (3,077 sites, 1,000 truth keys), against the rules of
tests/label_rules.py, exact.

k_label_write is launched with at most 4,096 workgroups of 256 lanes, a lane owning 16 bytes: 4,194,304 ints a trip, which is 46,603 label
rows of 90 ints and 34 ints of the next.  More kept rows than that are written by the grid-stride loop's second (at 93,207 rows: third)
trip; the rows below, at and above the seams are the cases here.  90 is not a multiple of 4, so a lane's four ints straddle two rows at
every second row whatever the trip.  A 64 MiB chunk of a 30x mpileup selects more sites than 46,603: this is what production runs.

The truth table of the binary search in k_label_sites: 2^20 + 3 keys (a real truth VCF holds millions), hits at key 0 and at the last key."""
import numpy as np
import pytest

from nanosnp_amd import _lib
from tests import label_rules as lr
from tests.test_gpu_train_bins import KS, _run_entry, _site_keys, _truth_for

pytestmark = pytest.mark.gpu
POS = (1 << KS) - 1
ROWS_PER_TRIP = 4096 * 256 * 4 // 90                         # 46,603 whole rows
CONTIG = 60_000


@pytest.fixture(scope="module")
def big_table():
    """two contigs of 60,000 bases: c0 = ACGTacgt over and over, c1 seeded, both cases of every letter"""
    rng = np.random.default_rng(20261020)
    letters = np.frombuffer(b"ACGTacgt", np.uint8)
    seqs = {"c0": np.tile(letters, CONTIG // 8), "c1": rng.choice(letters, CONTIG).astype(np.uint8)}
    assert all(s.size == CONTIG and set(s.tolist()) == set(b"ACGTacgt") for s in seqs.values())
    return _lib.ContigTable(contigs=seqs, device=0), seqs


def _bases(seqs, keys):
    pos = (keys & POS) - 1
    return np.where(keys >> KS == 0, seqs["c0"][pos], seqs["c1"][pos]).astype(np.uint8)


@pytest.mark.parametrize("n", [ROWS_PER_TRIP - 1, ROWS_PER_TRIP, ROWS_PER_TRIP + 1, 2 * ROWS_PER_TRIP + 1, 100_003])
def test_kept_rows_around_the_write_grid(gpu_ctx, big_table, n):
    """every site kept, 1,000 of them truth sites: one row short of a trip, a trip's whole rows, one more, two trips and a row, 100,003.
    The label on the device, and in pinned host memory filled with -7 that is three rows longer than the entry is told."""
    table, seqs = big_table
    assert n in (46602, 46603, 46604, 93207, 100003) and 4096 * 256 * 4 - ROWS_PER_TRIP * 90 == 34
    keys = _site_keys(n)
    rng = np.random.default_rng([28, n])
    tk, truth = _truth_for(keys, 1000, "all", rng)
    quads, hit = lr.site_quads(keys, _bases(seqs, keys), truth)
    assert tk.size == 1000 == hit.sum() and len(set(quads)) > 500
    want = lr.one_hot(quads)
    for pinned in (False, True):
        kept, label, meta, whole = _run_entry(gpu_ctx, table, keys, np.arange(n), tk, truth, None, 0, pinned=pinned, extra_rows=3)
        assert meta.tolist() == [n, 1000, n - 1000, 0], (n, pinned)
        assert np.array_equal(kept, np.arange(n)), (n, pinned)
        assert label.shape == want.shape and np.array_equal(label, want), (n, pinned, np.flatnonzero((label != want).any(axis=1))[:8])
        if pinned:
            rest = whole.numpy().reshape(-1)[n * 90:]
            assert rest.size == 3 * 90 and (rest == -7).all(), n


def test_fewer_kept_rows_than_sites_beyond_the_write_grid(gpu_ctx, big_table):
    """120,000 sites, the seeded draw keeps two thirds of c0 and all of c1: N' < N, and N' itself lies in the third trip"""
    table, seqs = big_table
    n = 120_000
    keys = _site_keys(n)
    rng = np.random.default_rng([28, n])
    tk, truth = _truth_for(keys, 1000, "seeded", rng)
    seed = int(rng.integers(0, 1 << 62))
    thr = [(2 << 53) // 3, 1 << 53]                          # (hash >> 11 is below 2^53: the second keeps everything)
    quads, hit = lr.site_quads(keys, _bases(seqs, keys), truth)
    keep = lr.kept_mask(keys, hit, {0: thr[0], 1: thr[1]}, seed)
    assert hit.sum() == 1000 and keep[keys >> KS == 1].all() and 0.64 < keep[(keys >> KS == 0) & ~hit].mean() < 0.69
    assert 2 * ROWS_PER_TRIP < keep.sum() < n
    want = lr.one_hot([q for q, k in zip(quads, keep) if k])
    for pinned in (False, True):
        kept, label, meta, whole = _run_entry(gpu_ctx, table, keys, np.arange(n), tk, truth, thr, seed, pinned=pinned)
        assert meta.tolist() == [int(keep.sum()), 1000, n - 1000, 0], pinned
        assert np.array_equal(kept, np.flatnonzero(keep)), pinned
        assert np.array_equal(label, want), (pinned, np.flatnonzero((label != want).any(axis=1))[:8])
        if pinned:
            rest = whole.numpy().reshape(-1)[int(keep.sum()) * 90:]
            assert rest.size == (n - int(keep.sum())) * 90 and (rest == -7).all()


def test_a_truth_table_of_a_million_keys(gpu_ctx, big_table):
    """2^20 + 3 truth keys, 5,000 sites in any order: two sites below the first key, one AT it, about half of the others at a key
    somewhere in the table, one at the last key, two above it.  The keys no site has lie between them - most of them in c0 at positions
    beyond its 60,000 bases, where no site can be.  Codes: random bits of LAB_CODE_MASK, fields a truth VCF never gives included."""
    table, seqs = big_table
    n_truth = (1 << 20) + 3
    rng = np.random.default_rng(20)
    sites = np.concatenate([np.sort(rng.choice(CONTIG, 2500, replace=False)) + 1, 1 << KS | (np.sort(rng.choice(CONTIG, 2500, replace=False)) + 1)]).astype(np.int64)
    lo, hi = int(sites[2]), int(sites[-3])
    inner = sites[3:-3]
    chosen = inner[rng.random(inner.size) < 0.5]
    free = np.concatenate([np.arange(lo + 1, 2_000_001, dtype=np.int64), 1 << KS | np.arange(1, hi & POS, dtype=np.int64)])
    free = free[~np.isin(free, sites)]
    tk = np.sort(np.concatenate([[lo, hi], chosen, rng.choice(free, n_truth - 2 - chosen.size, replace=False)])).astype(np.int64)
    assert tk.size == n_truth and (np.diff(tk) > 0).all() and tk[0] == lo and tk[-1] == hi
    codes = (rng.integers(0, 1 << 32, n_truth, dtype=np.uint64) & 0x3f3f031f).astype(np.uint32)
    fields = [(codes & 0x1f).tolist(), (codes >> 8 & 3).tolist(), (codes >> 16 & 0x3f).tolist(), (codes >> 24 & 0x3f).tolist()]
    asked = np.isin(tk, sites)                               # (the rules look a site's key up: only those keys need an entry)
    truth = {k: q for k, q, a in zip(tk.tolist(), zip(*fields), asked.tolist()) if a}
    keys = sites[rng.permutation(sites.size)]
    quads, hit = lr.site_quads(keys, _bases(seqs, keys), truth)
    assert hit[keys == lo].all() and hit[keys == hi].all() and not hit[keys < lo].any() and not hit[keys > hi].any()
    assert (keys < lo).sum() == 2 == (keys > hi).sum() and 0.45 < hit.mean() < 0.55 and hit.sum() == chosen.size + 2
    assert max(q[3] for q, h in zip(quads, hit) if h) > 32                          # (a length column beyond 89: three ones in that row)
    want = lr.one_hot(quads)
    kept, label, meta, _ = _run_entry(gpu_ctx, table, keys, np.arange(keys.size), tk, truth, None, 0, codes=codes)
    assert meta.tolist() == [keys.size, int(hit.sum()), int((~hit).sum()), 0]
    assert np.array_equal(kept, np.arange(keys.size)) and np.array_equal(label, want), np.flatnonzero((label != want).any(axis=1))[:8]


def test_count_mode_at_100003_sites(gpu_ctx, big_table):
    """the contig changes at site 50,001, lane 81 of workgroup 195: that workgroup adds c0's sites in LDS and c1's straight to the
    counters; two calls, the counters are ADDED"""
    import torch
    table, _ = big_table
    dev = torch.device("cuda", 0)
    keys = np.concatenate([np.arange(1, 50_002, dtype=np.int64), 1 << KS | np.arange(1, 50_003, dtype=np.int64)])
    assert keys.size == 100_003 and 50_001 % 256 == 81 and 50_001 // 256 == 195
    rng = np.random.default_rng(4)
    tk = np.unique(np.concatenate([rng.choice(keys, 1000, replace=False), np.arange(55_000, 55_040, dtype=np.int64), 1 << KS | np.arange(55_000, 55_040, dtype=np.int64)]))
    hit = np.isin(keys, tk)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    totals = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    for _ in range(2):
        kept, label, meta = gpu_ctx.pileup_label_sites_keys(up(keys), up(np.arange(keys.size)), table, up(tk), up(np.zeros(tk.size, np.int32)),
                                                            counts=totals, want_label=False)
    assert kept is None and label is None and meta.cpu().tolist() == [keys.size, int(hit.sum()), int((~hit).sum()), 0]
    want = np.bincount((keys >> KS) * 2 + (~hit), minlength=4).reshape(2, 2)
    assert hit.sum() == 1000 and tk.size == 1080 and want.min() > 300 and np.array_equal(totals.cpu().numpy(), 2 * want)
