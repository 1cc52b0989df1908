"""merge.group_cuts: a QUAL threshold as the float32 probability at which the library's own score first reaches it, so that the
device (nanosnp_amd/csrc/pileup_groups.hip) compares bit patterns and evaluates no logarithm - and the generator of tests/group_rules.py,
whose cases the GPU tests run: every branch of the rule occurs and the yardstick finds groups."""
import numpy as np
import pytest

from nanosnp_amd import host, merge
from tests import group_rules as gr

THRESHOLDS = (19.0, 14.0, 15.5, 13.004, 0.0, 3010.3, -1.0, 1e9)
MODES = (host.SCORE_FLOAT32, host.SCORE_FLOAT64)


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _bits(p):
    return int(np.array([p], np.float32).view(np.uint32)[0])


def _scores(p, mode):
    """(score, ok) arrays of the float32 array p"""
    l = host._bind_vcf()
    import ctypes as C
    ok = C.c_int(0)
    s = np.empty(p.size)
    has = np.empty(p.size, bool)
    for i, v in enumerate(p.tolist()):
        s[i] = l.nsnp_calculate_score(v, mode, C.byref(ok))
        has[i] = bool(ok.value)
    return s, has


@pytest.mark.parametrize("mode", MODES)
def test_the_table_has_the_layout_the_kernel_reads(mode):
    c = merge.group_cuts(19.0, 14.0, mode)
    assert c.dtype == np.float32 and c.shape == (8,)
    assert c[0] == merge.group_cuts(19.0, 3.0, mode)[0] and c[1] == merge.group_cuts(1.0, 14.0, mode)[1]
    assert 0.5 < c[1] < c[0] < 1.0 and c[2] == 0.0 and not np.signbit(c[2]) and not c[5:].any()
    # p == 1: skipped where NumPy scalars stay float32, scored where they widen (nsnp_vcf.c)
    assert c[3] == (np.float32(1.0) if mode == host.SCORE_FLOAT64 else np.nextafter(np.float32(1), np.float32(0)))
    assert c[4] == (1.0 if mode == host.SCORE_FLOAT64 else 0.0) == float(host.calculate_score(np.float32(-0.0), mode)[1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_the_cut_is_the_first_probability_whose_score_reaches_the_threshold(threshold, mode):
    c = merge.group_cuts(threshold, threshold, mode)
    assert c[0] == c[1] or (np.isinf(c[0]) and np.isinf(c[1]))
    lo, hi = c[2], c[3]
    if np.isinf(c[0]):                                       # no probability reaches it: not even the last one that has a score
        s, ok = host.calculate_score(hi, mode)
        assert ok and not s >= threshold and threshold > 80
        return
    s, ok = host.calculate_score(c[0], mode)
    assert ok and s >= threshold
    if c[0] == lo:                                           # every probability that has a score reaches it; the one below has none
        assert threshold <= 0 and not host.calculate_score(-np.nextafter(np.float32(0), np.float32(1)), mode)[1]
    else:
        s, ok = host.calculate_score(np.nextafter(c[0], np.float32(-1)), mode)
        assert ok and not s >= threshold


@pytest.mark.parametrize("mode", MODES)
def test_the_score_never_decreases_round_the_cuts(mode):
    """2^17 consecutive bit patterns round every cut: one `p >= p_cut` per threshold is the whole comparison"""
    for threshold in THRESHOLDS:
        c = merge.group_cuts(threshold, threshold, mode)
        if np.isinf(c[0]):
            continue
        b = _bits(c[0])
        first = max(_bits(c[2]), b - (1 << 16))
        last = min(_bits(c[3]), first + (1 << 17) - 1)
        p = np.arange(first, last + 1, dtype=np.uint32).view(np.float32)
        s, ok = _scores(p, mode)
        assert ok.all() and (np.diff(s) >= 0).all(), threshold
        assert ((s >= threshold) == (p >= c[0])).all(), threshold


@pytest.mark.parametrize("mode", MODES)
def test_the_score_never_decreases_over_random_probabilities(mode):
    rng = np.random.default_rng(20264101)
    p = np.concatenate([rng.random(500_000), 1.0 - rng.random(400_000) ** 4, rng.random(100_000) ** 6]).astype(np.float32)
    p = np.sort(p[p < 1.0])
    assert p.size > 990_000
    s, ok = _scores(p, mode)
    assert ok.all() and (np.diff(s) >= 0).all()
    for threshold in (19.0, 14.0, 15.5, 13.004):
        assert ((s >= threshold) == (p >= merge.group_cuts(threshold, 14.0, mode)[0])).all()


@pytest.mark.parametrize("mode", MODES)
def test_the_interval_that_has_a_score(mode):
    c = merge.group_cuts(19.0, 14.0, mode)
    rng = np.random.default_rng(20264102)
    tiny = np.nextafter(np.float32(0), np.float32(1))
    p = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32).view(np.float32),     # any bit pattern
                        np.array([0.0, -0.0, tiny, -tiny, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)),
                                  np.inf, -np.inf, np.nan, -np.nan, 0.5, -0.5, 2.0], np.float32)])
    _, ok = _scores(p, mode)
    bits = p.view(np.uint32)
    inside = (bits >= _bits(c[2])) & (bits <= _bits(c[3]))
    if c[4]:
        inside |= bits == 0x80000000
    assert (ok == inside).all()
    assert inside.sum() > 10_000


@pytest.mark.parametrize("mode", MODES)
def test_the_generator_reaches_every_branch(mode):
    got = gr.branches(gr.default_case(mode)) | gr.branches(gr.short_batch_case(mode))
    assert got == set(gr.BRANCHES)
    assert {"tail7", "tail8", "tail9", "tail10", "tail_T"} <= gr.branches(gr.short_batch_case(mode))


@pytest.mark.parametrize("mode", MODES)
def test_the_yardstick_finds_groups(mode):
    case = gr.default_case(mode)
    groups = gr.yardstick(case)
    assert gr.n_groups(groups) >= 20 and sum(bool(v) for v in groups.values()) >= 3
    assert all(len(g) == 11 for v in groups.values() for g in v)
    # a short last batch takes rows away: the text depends on the batch size, and so do the groups' members
    assert gr.vcf_text(case, batch_size=1000) != gr.vcf_text(case, batch_size=1012)
    assert gr.n_groups(gr.yardstick(gr.short_batch_case(mode))) >= 20


def test_the_row_entries_exist():
    from nanosnp_amd import _lib, pipeline
    assert "nsnp_pileup_select_groups" in _lib.EXPORTS and "nsnp_pileup_groups_scratch_bytes" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.nsnp_pileup_groups_scratch_bytes(-1) == 0 and lib.nsnp_pileup_groups_scratch_bytes(1 << 31) == 0
    assert lib.nsnp_pileup_groups_scratch_bytes(0) >= 32 and lib.nsnp_pileup_groups_scratch_bytes(2049) >= 17 * 2049
    assert callable(merge.select_groups_rows) and callable(pipeline.call_mpileup_groups) and hasattr(merge.DeviceGroups, "to_lists")
