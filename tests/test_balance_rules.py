"""The rules of nsnp_pileup_balance_samples (tests/balance_rules.py, train.balance_sample_count) against the reference's own balance_dataset
as tests/golden/pileup_balance.npz recorded it (tests/golden/make_golden_balance.py): the sample count M with K, U and max, the U == 0
shapes where the reference divides by zero, int(L / U) == L // U, the bound M <= 2 N, the slot structure, and the distribution.

Distribution bound, five standard deviations, for the restatement's totals over the recorded number of runs (draw = 0, 1, ...) and for the
reference's recorded totals alike.  Every nonempty category owns max of the K max slots, so a category's total is Binomial(runs M, 1 / K).
A row j of a category of `size` rows holds n_j = 1 + Binomial(max - size, 1 / size) slots (its own and the upsampled slots that drew it) and
collects Binomial(M, n_j p), p = 1 / (K max), per run: mean M / (K size), variance M p E[n] - M p^2 E[n^2] + M^2 p^2 Var[n] - two samples in
one upsampled slot get the same row, which is what the last term is.  Every row of every nonempty category of every set with U > 0 is
held against its bound: 3,777 rows and 357 categories on each side.  The sets and the seeds (SEED here, seed0 of the fixture) are ones
for which the restatement and the reference both pass."""
from __future__ import annotations

import numpy as np
import pytest

from tests import balance_rules as br
from tests.helpers import golden

SEED = (5 << 32) | 2022
CHECKED_CATEGORIES, CHECKED_ROWS = 357, 3777                            # the nonempty categories and the rows of the 17 sets with U > 0


@pytest.fixture(scope="module")
def fx():
    z = np.load(golden("pileup_balance.npz"))
    sets = []
    for i, name in enumerate(z["names"]):
        cls = np.zeros((z[f"gt_{i}"].size, 4), np.uint8)
        cls[:, 0], cls[:, 1] = z[f"gt_{i}"], z[f"zy_{i}"]
        sets.append(dict(name=str(name), cls=cls, m=int(z[f"m_{i}"]), rows=z[f"rows_{i}"], cats=z[f"cats_{i}"]))
    return dict(runs=int(z["runs"]), sets=sets)


@pytest.fixture(scope="module")
def totals(fx):
    """the restatement's per-row totals over the recorded number of runs, per set (None where U == 0): computed once"""
    out = []
    for s in fx["sets"]:
        if s["m"] < 0:
            out.append(None)
            continue
        t = np.zeros(s["cls"].shape[0], np.int64)
        for draw in range(fx["runs"]):
            t += np.bincount(br.balance_samples(s["cls"], SEED, draw)[0], minlength=t.size)
        out.append(t)
    return out


def test_the_fixture_covers_the_shapes(fx):
    names = [s["name"] for s in fx["sets"]]
    assert len(names) >= 20 and {"empty", "one_category", "equal_sizes"} <= set(names)
    K = [int((br.balance_samples(s["cls"], 0, 0)[1] > 0).sum()) for s in fx["sets"]]
    assert 2 in K and 63 in K
    assert sum(1 for s in fx["sets"] if s["m"] < 0) >= 3 and sum(1 for s in fx["sets"] if s["m"] > 0) >= 15


def test_counts_equal_the_reference(fx):
    from nanosnp_amd import train
    for s in fx["sets"]:
        samples, sizes, meta = br.balance_samples(s["cls"], SEED, 0)
        M, K, U, mx = br.sample_count(sizes)
        assert train.balance_sample_count(sizes) == (M, K, U, mx), s["name"]
        assert sizes.sum() == s["cls"].shape[0] and meta[4] == 0
        if s["m"] < 0:                                                       # the reference raised ZeroDivisionError
            assert M is None and U == 0 and meta[5] == 1 and meta[0] == 0 and samples.size == 0, s["name"]
        else:
            assert M == s["m"] == meta[0] == samples.size and meta[5] == 0 and U > 0, s["name"]
            assert M <= 2 * s["cls"].shape[0], s["name"]
        assert meta.tolist() == [samples.size, K, U, mx, 0, int(s["m"] < 0), 0, 0]


def test_truncated_float_division_is_integer_division():
    """int(L / U) of dataset.py:65 against L // U: every U in 1..62 at L around 2^38, around the multiples of U, and at seeded places"""
    rng = np.random.default_rng(3)
    for U in range(1, 63):
        top = 1 << 38
        Ls = list(range(top - 130, top)) + [q * U + d for q in (1, 2, top // U - 1, top // U) for d in (-1, 0, 1, U - 1)]
        Ls += rng.integers(1, top, 200).tolist()
        for L in Ls:
            if 0 < L < top:
                assert int(L / U) == L // U, (L, U)


def test_sample_count_and_its_bound_on_random_sizes():
    from nanosnp_amd import train
    rng = np.random.default_rng(8)
    for trial in range(2000):
        K = int(rng.integers(0, 64))
        sizes = np.zeros(63, np.int64)
        hi = int(rng.choice([2, 5, 100, 70000, 1 << 31]))
        sizes[rng.choice(63, K, replace=False)] = rng.integers(1, hi + 1, K)
        if K and trial % 3 == 0:
            sizes[sizes > 0] = np.where(rng.random(K) < 0.5, sizes.max(), sizes[sizes > 0])      # ties at the maximum
        M, k, U, mx = train.balance_sample_count(sizes)
        assert (M, k, U, mx) == br.sample_count(sizes)
        assert k == K and mx == sizes.max(initial=0) and U == int(((sizes > 0) & (sizes < mx)).sum())
        if M is None:
            assert U == 0
        else:
            assert M == k * mx // U and M <= 2 * int(sizes.sum())
    assert train.balance_sample_count([0] * 63) == (None, 0, 0, 0) and train.balance_sample_count([]) == (None, 0, 0, 0)
    assert train.balance_sample_count([4, 0, 1]) == (8, 2, 1, 4) and train.balance_sample_count([4, 4, 1]) == (12, 3, 1, 4)
    with pytest.raises(ValueError):
        train.balance_sample_count([1, -1])


def test_slot_structure_and_placement(fx):
    for s in fx["sets"]:
        if s["m"] < 0:
            continue
        cat = br.categories(s["cls"])
        for draw in (0, 3):
            samples, sizes, meta = br.balance_samples(s["cls"], SEED, draw)
            M, K, U, mx = (int(v) for v in meta[:4])
            blocks = br.balanced_list(s["cls"], SEED, draw)
            nz = np.flatnonzero(sizes > 0)
            assert len(blocks) == K and all(b.size == mx for b in blocks)
            for k, b in zip(nz, blocks):
                own = np.flatnonzero(cat == k)
                assert np.array_equal(b[:own.size], own)                    # slot r < size: the r-th row of the category, in row order
                assert (cat[b[own.size:]] == k).all()                       # an upsampled slot: a row of its own category
            # sample m is slot index(v[1], max) of nonempty category number index(v[0], K)
            m = np.arange(M, dtype=np.uint64)
            v = br.philox4x32_10((m & np.uint64(br.MASK), m >> np.uint64(32), draw, 0), (SEED & br.MASK, SEED >> 32))
            flat = np.concatenate(blocks)
            assert np.array_equal(samples, flat[br.index(v[0], K) * mx + br.index(v[1], mx)]), s["name"]
        assert not np.array_equal(br.balance_samples(s["cls"], SEED, 0)[0], br.balance_samples(s["cls"], SEED, 1)[0])


def test_rows_in_no_category_are_counted_and_never_sampled():
    sizes = np.zeros(63, np.int64)
    sizes[[0, 4, 62]] = 40, 3, 9
    cls = br.labels_from_sizes(sizes, np.random.default_rng(2), none=25)
    samples, got, meta = br.balance_samples(cls, SEED, 0)
    assert np.array_equal(got, sizes) and meta.tolist() == [3 * 40 // 2, 3, 2, 40, 25, 0, 0, 0]
    assert (br.categories(cls)[samples] < 63).all()


def _row_sigma(runs, M, K, mx, size):
    p = 1.0 / (K * mx)
    q = 1.0 / size
    en = 1.0 + (mx - size) * q
    vn = (mx - size) * q * (1.0 - q)
    return np.sqrt(runs * (M * p * en - M * p * p * (vn + en * en) + M * M * p * p * vn))


@pytest.mark.parametrize("who", ["restatement", "reference"])
def test_totals_within_five_standard_deviations(fx, totals, who):
    runs, checked_rows, checked_cats = fx["runs"], 0, 0
    for s, own in zip(fx["sets"], totals):
        if s["m"] < 0:
            continue
        rows = own if who == "restatement" else s["rows"]
        cat = br.categories(s["cls"])
        sizes = np.bincount(cat, minlength=64)[:63]
        M, K, U, mx = br.sample_count(sizes)
        assert rows.sum() == runs * M
        cats = np.bincount(cat, weights=rows, minlength=63)
        if who == "reference":
            assert np.array_equal(cats, s["cats"])
        mean, sd = runs * M / K, np.sqrt(runs * M * (1.0 / K) * (1.0 - 1.0 / K))
        for c in np.flatnonzero(sizes > 0):
            assert abs(cats[c] - mean) <= 5.0 * sd, (who, s["name"], c, cats[c], mean, sd)
            checked_cats += 1
            row_mean = mean / sizes[c]
            sigma = _row_sigma(runs, M, K, mx, int(sizes[c]))
            worst = np.abs(rows[cat == c] - row_mean).max()
            assert worst <= 5.0 * sigma, (who, s["name"], c, worst, row_mean, sigma)
            checked_rows += int(sizes[c])
        assert (cats[sizes == 0] == 0).all()
    print(f"{who}: {checked_cats} categories and {checked_rows} rows within five standard deviations")
    assert checked_cats == CHECKED_CATEGORIES and checked_rows == CHECKED_ROWS
