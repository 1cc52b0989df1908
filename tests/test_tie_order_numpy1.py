"""The numpy-1.x tie order of the stage-4 read arrangement, on the CPU: the restatement tests/numpy1_sort.py against NumPy's scalar
argsort (tests/golden/argsort_numpy1.npz) and against the reference's own HP sort, and the reference's row order out of
readmatrix.read_matrices (tests/golden/hap_arrange_numpy1.npz; both written by tests/golden/make_golden_numpy1.py)."""
import numpy as np

from nanosnp_amd import readmatrix
from tests import numpy1_sort
from tests.helpers import FakeSamfile, golden, synth_groups, synth_reads


def _vectors(z):
    off = z["offsets"]
    for i in range(len(off) - 1):
        yield i, z["keys"][off[i]:off[i + 1]], z["perms"][off[i]:off[i + 1]]


def test_restatement_reproduces_numpy_scalar_argsort():
    z = np.load(golden("argsort_numpy1.npz"))
    lengths, differ = set(), 0
    for i, keys, perm in _vectors(z):
        assert numpy1_sort.argsort(keys) == perm.tolist(), i
        lengths.add(len(keys))
        differ += not np.array_equal(perm, np.argsort(keys, kind="stable"))
    assert {0, 1, 2, 15, 16, 17, 18, 33, 64, 65, 150, 257, 1000} <= lengths
    assert differ > 50                                      # ties are not the stable order: the fixture tells the two apart
    assert (z["keys"] == -2 ** 31).any() and (z["keys"] == 2 ** 31 - 1).any()


def test_fixture_reaches_the_heapsort_fallback():
    z = np.load(golden("argsort_numpy1.npz"))
    heap = set(int(h) for h in z["heapsort"])
    assert heap
    for i, keys, perm in _vectors(z):
        st = {}
        numpy1_sort.argsort(keys, st)
        assert (st["heapsort"] > 0) == (i in heap), i


def test_up_to_16_keys_is_the_stable_order():
    rng = np.random.default_rng(5)
    for n in range(17):
        for _ in range(20):
            k = rng.integers(1, 4, n)
            assert numpy1_sort.argsort(k) == np.argsort(k, kind="stable").tolist()


def _deep_matrices():
    z = np.load(golden("hap_arrange_numpy1.npz"))
    reads = synth_reads(int(z["deep_seed"]), n_reads=int(z["deep_reads"]))
    groups = synth_groups(int(z["deep_seed"]) + 1, centres=tuple(int(c) for c in z["deep_centres"]))
    return z, readmatrix.read_matrices(FakeSamfile(reads), groups, max_coverage=10000)


def test_read_matrices_yield_the_reference_row_order():
    """the rows come out in the order in which the reference's pileup pass first sees each read (create_pileup_haplotype.py:86-134),
    which is not the order of the alignment file's read list"""
    z, rm = _deep_matrices()
    assert rm.names == z["names"].tolist()
    assert rm.positions == z["ext_positions"].tolist()
    for nm, m in (("seq", rm.seq), ("bq", rm.baseq), ("mq", rm.mapq), ("hap", rm.hap)):
        assert np.array_equal(m, z[f"in_{nm}"].astype(np.int32)), nm
    assert rm.names != [f"r{i}" for i in range(len(rm.names))]


def test_restatement_orders_rows_as_the_reference_function():
    """centre filter then the restated NumPy 1.x argsort on the centre HP: the reference's output matrices row for row, and at
    every one of these deep sites a different order from the stable one"""
    z, rm = _deep_matrices()
    sl = readmatrix.group_slices(rm)
    assert [s["candidate"] for s in sl] == z["candidates"].tolist()
    for g, s in enumerate(sl):
        for tag, key in (("h", "hap_cols"), ("p", "pile_cols")):
            assert np.array_equal(s[key], z[f"g{g}_{tag}_cols"])
            seq, hap = rm.seq[:, s[key]], rm.hap[:, s[key]]
            mid = seq.shape[1] // 2
            keep = np.nonzero(seq[:, mid] != 0)[0]
            order = keep[numpy1_sort.argsort(hap[keep, mid])]
            assert len(order) > 16
            for nm, m in (("seq", rm.seq), ("bq", rm.baseq), ("mq", rm.mapq), ("hap", rm.hap)):
                assert np.array_equal(m[:, s[key]][order], z[f"g{g}_{tag}_out_{nm}"].astype(np.int32)), (g, tag, nm)
            assert not np.array_equal(order, keep[np.argsort(hap[keep, mid], kind="stable")]), (g, tag)
