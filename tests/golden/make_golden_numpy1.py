#!/usr/bin/env python3
"""Generate the numpy-1.x tie-order fixtures under tests/golden/ from NumPy's scalar sort and from the reference itself.

The reference's environment (Miniconda py38) holds NumPy <= 1.24, whose argsort(kind="quicksort") is the scalar introsort
aquicksort_ on every CPU.  Later NumPy runs the same code only with SIMD sort dispatch off, so every group runs in a child
interpreter started with NPY_DISABLE_CPU_FEATURES below, and asserts there that AVX512_SKX and AVX2 report off: no fixture can
record a CPU-dependent SIMD order.

    python tests/golden/make_golden_numpy1.py            # both fixtures
    python tests/golden/make_golden_numpy1.py argsort    # one group: argsort | haparrange

Groups:
  argsort     numpy.argsort(kind="quicksort") on int32 key vectors (lengths 0 .. ~1000, HP-like ties, sorted / reverse / organ
              pipe, random int32 with INT_MIN / INT_MAX, and a McIlroy adversary that reaches the heapsort fallback)
                                                        -> argsort_numpy1.npz
  haparrange  create_pileup_haplotype.single_group_pileup_haplotype_feature on a deep stand-in alignment file
              (tests/helpers.py synth_reads(DEEP_SEED, n_reads=DEEP_READS)): the reads in the reference's own row order
              (first seen over its pileup pass, :86-134) and its HP-sorted output matrices -> hap_arrange_numpy1.npz
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NANOSNP_REFERENCE", "/root/reference")
GOLD = HERE
sys.path.insert(0, ROOT)

NPY_SCALAR_SORT = ("AVX512F AVX512CD AVX512VL AVX512BW AVX512DQ AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR "
                   "AVX512VPOPCNTDQ AVX512VNNI AVX512IFMA AVX512VBMI AVX512VBMI2 AVX512BITALG AVX512FP16 AVX2 FMA3 F16C AVX")
DEEP_SEED, DEEP_READS = 91, 300
DEEP_CENTRES = (130, 180, 250, 330, 400, 470, 540, 620, 700, 765)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _assert_scalar_sort():
    try:
        from numpy._core._multiarray_umath import __cpu_features__ as feats
    except ImportError:                                   # NumPy 1.x
        from numpy.core._multiarray_umath import __cpu_features__ as feats
    assert not feats.get("AVX512_SKX") and not feats.get("AVX2"), "SIMD sort dispatch is on: set NPY_DISABLE_CPU_FEATURES"


def _np_argsort(keys):
    """the permutation pandas' sort_values(by=col) takes on an int64 column (nargsort, kind="quicksort")"""
    p = np.argsort(np.asarray(keys, np.int64), kind="quicksort")
    assert np.array_equal(p, np.argsort(np.asarray(keys, np.int32), kind="quicksort"))
    return p


def mcilroy_adversary(n):
    """McIlroy's "A killer adversary for quicksort": values frozen lazily while the restatement sorts, so that every pivot is as bad
    as the comparisons so far allow.  Returns int32 keys on which the restatement reaches its heapsort fallback."""
    from tests import numpy1_sort
    gas = n
    val = [gas] * n
    state = {"solid": 0, "cand": None}

    class Item:
        __slots__ = ("i",)

        def __init__(self, i):
            self.i = i

        def __lt__(self, other):
            x, y = self.i, other.i
            if val[x] == gas and val[y] == gas:
                z = x if x == state["cand"] else y
                val[z] = state["solid"]; state["solid"] += 1
            if val[x] == gas:
                state["cand"] = x
            elif val[y] == gas:
                state["cand"] = y
            return val[x] < val[y]

    numpy1_sort.argsort([Item(i) for i in range(n)])
    return np.asarray(val, np.int32)


def group_argsort():
    _assert_scalar_sort()
    from tests import numpy1_sort
    rng = np.random.default_rng(2024)
    vecs = []
    lengths = (0, 1, 2, 15, 16, 17, 18, 33, 64, 65, 150, 257, 1000)
    for n in lengths:
        vecs.append(rng.integers(1, 4, n))                                       # HP tags
        vecs.append(np.full(n, 2))                                               # one key
        s = rng.integers(-50, 51, n)
        vecs.append(np.sort(s)); vecs.append(np.sort(s)[::-1])                   # sorted, reverse-sorted
        h = np.arange(n) % max(1, (n + 1) // 2)
        vecs.append(np.concatenate([np.arange((n + 1) // 2), np.arange(n // 2)[::-1]]))   # organ pipe
        vecs.append(h)                                                           # saw tooth
        r = rng.integers(INT_MIN, INT_MAX, n, endpoint=True)
        if n >= 2:
            r[rng.integers(0, n, max(1, n // 8))] = INT_MIN
            r[rng.integers(0, n, max(1, n // 8))] = INT_MAX
        vecs.append(r)
        vecs.append(rng.choice([1, 2, 3, INT_MIN, INT_MAX, 0], n))               # extreme ties
    for n in rng.integers(17, 400, 40):                                          # HP tags at pileup depths
        vecs.append(rng.choice([1, 2, 3], int(n), p=[0.3, 0.3, 0.4]))
    adversary = []
    for n in (300, 1000):
        adversary.append(len(vecs))
        vecs.append(mcilroy_adversary(n))
    heap = []                                                                    # every vector that reaches the fallback
    for i, v in enumerate(vecs):
        st = {}
        numpy1_sort.argsort(np.asarray(v, np.int32), st)
        if st["heapsort"]:
            heap.append(i)
    assert set(adversary) <= set(heap), ("the adversary did not reach the heapsort fallback", adversary, heap)
    keys = np.concatenate([np.asarray(v, np.int64) for v in vecs]).astype(np.int32)
    assert np.array_equal(keys, np.concatenate([np.asarray(v, np.int64) for v in vecs]))
    off = np.cumsum([0] + [len(v) for v in vecs]).astype(np.int64)
    perms = np.concatenate([_np_argsort(np.asarray(v, np.int32)) for v in vecs]).astype(np.int32) if len(keys) else np.zeros(0, np.int32)
    for i, v in enumerate(vecs):                                                 # the restatement is what the tests hold the kernel to
        assert numpy1_sort.argsort(np.asarray(v, np.int32)) == perms[off[i]:off[i + 1]].tolist(), i
    stable_differs = sum(not np.array_equal(perms[off[i]:off[i + 1]], np.argsort(np.asarray(v), kind="stable")) for i, v in enumerate(vecs))
    np.savez_compressed(os.path.join(GOLD, "argsort_numpy1.npz"), keys=keys, perms=perms, offsets=off,
                        heapsort=np.asarray(heap, np.int64), numpy_version=np.array(np.__version__))
    print("argsort_numpy1:", len(vecs), "vectors,", len(keys), "keys;", stable_differs, "differ from the stable order; heapsort vectors", heap)


def group_haparrange():
    _assert_scalar_sort()
    import types
    for name in ("ranger", "ranger21", "tables", "pysam"):
        sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, os.path.join(REF, "HaplotypeModel"))
    import pandas as pd
    import create_pileup_haplotype as cph        # noqa: E402  (reference module)
    from select_hetesnp_homosnp import SNPItem   # noqa: E402
    from tests.helpers import FakeSamfile, synth_groups, synth_reads
    from tests import numpy1_sort
    reads = synth_reads(DEEP_SEED, n_reads=DEEP_READS)
    groups_cp = synth_groups(DEEP_SEED + 1, centres=DEEP_CENTRES)
    groups = [[SNPItem(c, p, "0/1", 10.0 if k == 5 else 20.0) for k, (c, p) in enumerate(g)] for g in groups_cp]
    # the read dictionaries of :86-134 as the reference builds them: the four dicts handed to pd.DataFrame at :135-138
    seen = []
    real_df = cph.pd.DataFrame

    def recording_df(data=None, *a, **k):
        if isinstance(data, dict):
            seen.append((data, list(k.get("index", a[0] if a else []))))
        return real_df(data, *a, **k)
    cph.pd = types.SimpleNamespace(DataFrame=recording_df)
    import contextlib, io
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = cph.single_group_pileup_haplotype_feature(FakeSamfile(reads), groups, 10000, 5, 16)
    finally:
        cph.pd = pd
    cand, hpos, hseq, hbq, hmq, hhap, maxh, pseq, pbq, pmq, phap, maxp = out
    assert len(cand) == len(groups) and len(seen) == 4, (len(cand), len(seen))
    (snp, ext), (hp, _), (bq, _), (mq, _) = seen
    names = list(snp.keys())
    assert names == list(hp.keys()) == list(bq.keys()) == list(mq.keys())
    mats = [np.array([d[q] for q in names], np.int32) for d in (snp, bq, mq, hp)]     # seq, bq, mq, hap [R, P] in the reference's order
    col = {p: i for i, p in enumerate(ext)}
    fx = {"n_groups": len(groups), "names": np.array(names), "ext_positions": np.array(ext, np.int64),
          "candidates": np.array(cand), "haplotype_positions": np.array(hpos), "max_depths": np.array([maxh, maxp]),
          "deep_seed": DEEP_SEED, "deep_reads": DEEP_READS, "deep_centres": np.array(DEEP_CENTRES),
          "numpy_version": np.array(np.__version__), "pandas_version": np.array(pd.__version__)}
    for nm, m in zip(("seq", "bq", "mq", "hap"), mats):
        fx[f"in_{nm}"] = m.astype(np.int16)
    depths, differs = [], 0
    for g, grp in enumerate(groups):
        gp = [int(it.position) for it in grp]
        wp = list(range(gp[5] - 16, gp[5] + 17))
        for tag, cols, outs in (("h", gp, (hseq[g], hbq[g], hmq[g], hhap[g])), ("p", wp, (pseq[g], pbq[g], pmq[g], phap[g]))):
            ci = np.array([col[p] for p in cols], np.int64)
            fx[f"g{g}_{tag}_cols"] = ci
            for nm, o in zip(("seq", "bq", "mq", "hap"), outs):
                fx[f"g{g}_{tag}_out_{nm}"] = np.asarray(o, np.int16)
            # the restatement reproduces the reference's rows in order (and they are not the stable order)
            s, h = mats[0][:, ci], mats[3][:, ci]
            keep = np.nonzero(s[:, len(ci) // 2] != 0)[0]
            order = keep[numpy1_sort.argsort(h[keep, len(ci) // 2])]
            assert np.array_equal(s[order], np.asarray(outs[0])) and np.array_equal(h[order], np.asarray(outs[3])), (g, tag)
            stable = keep[np.argsort(h[keep, len(ci) // 2], kind="stable")]
            differs += not np.array_equal(order, stable)
            depths.append(len(keep))
    assert 40 <= min(depths) and max(depths) <= 200, depths
    np.savez_compressed(os.path.join(GOLD, "hap_arrange_numpy1.npz"), **fx)
    print("hap_arrange_numpy1:", len(groups), "groups,", len(names), "reads; depths", depths, ";", differs, "of", len(depths),
          "sites differ from the stable order; numpy", np.__version__, "pandas", pd.__version__)


GROUPS = {"argsort": group_argsort, "haparrange": group_haparrange}

if __name__ == "__main__":
    which = sys.argv[1:] or list(GROUPS)
    if "haparrange" in which and not os.path.isdir(REF):
        sys.exit(f"{REF} is not mounted: the haparrange fixture can only be generated where the reference tree is")
    if len(which) == 1 and os.environ.get("NPY_DISABLE_CPU_FEATURES") == NPY_SCALAR_SORT:
        GROUPS[which[0]]()
    else:
        env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=NPY_SCALAR_SORT)
        for g in which:
            subprocess.run([sys.executable, os.path.abspath(__file__), g], check=True, env=env)
