"""The training sample list of a PileupModel pass under balance_dataset upsampling, restated in numpy: the rules of
nsnp_pileup_balance_samples (include/nanosnp.h), which follow balance_dataset (PileupModel/dataset.py:32-66).

Category of a row: c = 3 gt + zy (gt 0..20, zy 0..2), in ascending c; a row with gt >= 21 or zy >= 3 is in no category.  size[c], max = the
largest, K = categories with size > 0, U = categories with 0 < size < max (the reference's non_zero_categories: those at max are NOT
counted).  Every nonempty category owns max slots: slot r < size[c] is its r-th row in row order, slot r >= size[c] the row number
index(w[0], size[c]) with w = Philox at counter {r - size[c], c, draw, 1}.  M = int(K max / U) samples; sample m takes v = Philox at counter
{m low, m high, draw, 0}: nonempty category number index(v[0], K), slot index(v[1], max).  index(r, n) = (r n) >> 32.  U == 0: status 1,
no samples."""
from __future__ import annotations

import numpy as np

from tests.hap_sample_rules import MASK, philox4x32_10

N_GT, N_ZY = 21, 3
CATEGORIES = N_GT * N_ZY                                                  # 63


def categories(cls):
    """cls uint8 [N,4] (or [N,2]) -> int64 [N]: 3 gt + zy, 63 for a row in no category"""
    cls = np.asarray(cls, np.uint8)
    cls = cls.reshape(-1, cls.shape[-1] if cls.ndim == 2 else 4)
    gt, zy = cls[:, 0].astype(np.int64), cls[:, 1].astype(np.int64)
    return np.where((gt < N_GT) & (zy < N_ZY), 3 * gt + zy, CATEGORIES)


def sample_count(sizes):
    """sizes [63] -> (M, K, U, max); M is None when U == 0.  M = int(L / U), Python's float division truncated, as dataset.py:65 writes it"""
    sizes = [int(s) for s in sizes]
    mx = max(sizes) if sizes else 0
    K = sum(1 for s in sizes if s > 0)
    U = sum(1 for s in sizes if 0 < s < mx)
    return (int(K * mx / U) if U else None), K, U, mx


def index(r, n):
    return ((np.asarray(r, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def slot_rows(c, rows, slots, seed, draw):
    """the rows (of category c, `rows` in row order) the slots hold"""
    slots = np.asarray(slots, np.int64)
    size = rows.size
    up = slots >= size
    within = np.where(up, 0, slots)
    if up.any():
        w = philox4x32_10((slots[up] - size, c, draw, 1), (seed & MASK, seed >> 32))[0]
        within[up] = index(w, size)
    return rows[within]


def balanced_list(cls, seed, draw):
    """the whole balanced list: K blocks of max slots in ascending category (what total_indexes holds before the reference shuffles it)"""
    c = categories(cls)
    sizes = np.bincount(c, minlength=CATEGORIES + 1)[:CATEGORIES]
    _, K, U, mx = sample_count(sizes)
    return [slot_rows(k, np.flatnonzero(c == k), np.arange(mx), seed, draw) for k in range(CATEGORIES) if sizes[k] > 0]


def balance_samples(cls, seed, draw):
    """cls uint8 [N,4] -> (samples int64 [M], sizes int64 [63], meta int64 [8] = {M, K, U, max, rows in no category, status, 0, 0})"""
    c = categories(cls)
    counts = np.bincount(c, minlength=CATEGORIES + 1)
    sizes = counts[:CATEGORIES].astype(np.int64)
    M, K, U, mx = sample_count(sizes)
    if M is None:
        return np.zeros(0, np.int64), sizes, np.array([0, K, U, mx, counts[CATEGORIES], 1, 0, 0], np.int64)
    m = np.arange(M, dtype=np.uint64)
    v = philox4x32_10((m & np.uint64(MASK), m >> np.uint64(32), draw, 0), (seed & MASK, seed >> 32))
    nz = np.flatnonzero(sizes > 0)
    cat, slot = nz[index(v[0], K)], index(v[1], mx)
    size = sizes[cat]
    # (all categories at once; balanced_list goes category by category through slot_rows, and the rules test holds the two together)
    w = philox4x32_10((np.maximum(slot - size, 0), cat, draw, 1), (seed & MASK, seed >> 32))[0]
    within = np.where(slot < size, slot, (w * size.astype(np.uint64) >> np.uint64(32)).astype(np.int64))
    by_category = np.argsort(c, kind="stable")                              # the rows of category 0 in row order, then of 1, ...
    samples = by_category[(np.cumsum(sizes) - sizes)[cat] + within].astype(np.int64)
    return samples, sizes, np.array([M, K, U, mx, counts[CATEGORIES], 0, 0, 0], np.int64)


def labels_from_sizes(sizes, rng=None, none=0):
    """cls uint8 [N,4] with sizes[c] rows of category c (63 entries) and `none` rows in no category, at seeded places (rng None: sorted)"""
    sizes = np.asarray(sizes, np.int64)
    c = np.repeat(np.arange(CATEGORIES), sizes)
    cls = np.zeros((c.size + none, 4), np.uint8)
    cls[:c.size, 0], cls[:c.size, 1] = c // 3, c % 3
    bad = np.arange(none)
    cls[c.size:, 0] = np.where(bad % 2 == 0, 21 + bad % 200, bad % 21)           # gt >= 21, or
    cls[c.size:, 1] = np.where(bad % 2 == 0, bad % 3, 3 + bad % 250)            # zy >= 3
    if rng is not None:
        cls = cls[rng.permutation(cls.shape[0])]
        cls[:, 2:] = rng.integers(0, 33, (cls.shape[0], 2))
    return np.ascontiguousarray(cls)
