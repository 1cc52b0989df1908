#!/usr/bin/env python3
"""Generate tests/golden/pileup_balance.npz from the REFERENCE's own balance_dataset (PileupModel/dataset.py:32-66).

Runs only in the development container, where the upstream tree is mounted read-only (NANOSNP_REFERENCE, default /root/reference); the
fixture is data only: small label sets and what the reference's function returned for them.

    python tests/golden/make_golden_balance.py

Per set i: gt_i, zy_i (uint8 [N]); m_i = len(final_index) of a call, or -1 where the call raised ZeroDivisionError (U == 0); rows_i
(int64 [N]) = how often each row was returned over RUNS calls under np.random.seed(SEED0 + 1000 i + run); cats_i (int64 [63]) = the same
per category 3 gt + zy.  The sets: 2 to 63 nonempty categories, ties at the maximum, single-row categories, one dominating category, and
the three U == 0 shapes (no row, one category, equal sizes)."""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("NANOSNP_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
RUNS, SEED0 = 200, 20240


def size_sets():
    """(name, {category: rows}) per set"""
    rng = np.random.default_rng(35)
    sets = [
        ("two", {0: 50, 5: 7}),
        ("two_near_bound", {0: 10, 1: 1}),
        ("all_63", {c: 1 + (7 * c) % 20 for c in range(63)}),
        ("all_63_one_large", {c: (120 if c == 31 else 1 + c % 4) for c in range(63)}),
        ("dominating", {0: 300, 4: 3, 7: 2, 30: 5, 62: 1}),
        ("ties_at_max", {0: 40, 3: 40, 6: 40, 10: 5, 11: 9}),
        ("tie_and_one", {0: 10, 1: 10, 2: 1}),
        ("single_rows", {0: 30, 1: 1, 2: 1, 61: 1}),
        ("reference_like", {0: 200, 15: 180, 27: 150, 36: 120, 1: 6, 2: 9, 16: 4, 17: 7, 28: 3, 29: 5, 37: 2, 38: 8, 4: 1, 5: 2, 13: 1, 44: 3}),
        ("empty", {}),
        ("one_category", {8: 17}),
        ("equal_sizes", {0: 5, 9: 5, 62: 5}),
        ("two_tied", {1: 1, 2: 1}),
    ]
    for i, K in enumerate((2, 3, 5, 9, 17, 33, 62, 63)):
        cats = np.sort(rng.choice(63, K, replace=False))
        big = rng.integers(20, 80)
        sizes = np.minimum(rng.geometric(0.15, K), big)
        sizes[rng.integers(0, K)] = big
        sets.append((f"random_{K}", {int(c): int(s) for c, s in zip(cats, sizes)}))
    return sets


def main():
    for name, attrs in (("tables", {"Filters": lambda **k: None}),):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    sys.path.insert(0, os.path.join(REF, "PileupModel"))
    import dataset                                                            # the reference's module
    from tests import balance_rules as br
    out = {"runs": np.int64(RUNS), "seed0": np.int64(SEED0)}
    names = []
    for i, (name, d) in enumerate(size_sets()):
        sizes = np.zeros(63, np.int64)
        for c, s in d.items():
            sizes[c] = s
        cls = br.labels_from_sizes(sizes, np.random.default_rng(100 + i))
        gt, zy = cls[:, 0].astype(np.int64), cls[:, 1].astype(np.int64)
        cat = 3 * gt + zy
        rows = np.zeros(cls.shape[0], np.int64)
        m = None
        for run in range(RUNS):
            np.random.seed(SEED0 + 1000 * i + run)
            try:
                idx = np.asarray(dataset.balance_dataset(gt_label=gt, zy_label=zy), np.int64)
            except ZeroDivisionError:
                assert m in (None, -1)
                m = -1
                continue
            assert m in (None, idx.size)
            m = idx.size
            rows += np.bincount(idx, minlength=rows.size)
        out.update({f"gt_{i}": cls[:, 0].copy(), f"zy_{i}": cls[:, 1].copy(), f"m_{i}": np.int64(m), f"rows_{i}": rows,
                    f"cats_{i}": np.bincount(cat, weights=rows, minlength=63).astype(np.int64)})
        names.append(name)
        print(f"{i:2d} {name:18s} N {cls.shape[0]:5d} K {int((sizes > 0).sum()):2d} max {int(sizes.max()) if sizes.size else 0:4d} M {m}")
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(GOLD, "pileup_balance.npz"), **out)
    print("wrote", os.path.join(GOLD, "pileup_balance.npz"), os.path.getsize(os.path.join(GOLD, "pileup_balance.npz")), "bytes")


if __name__ == "__main__":
    main()
