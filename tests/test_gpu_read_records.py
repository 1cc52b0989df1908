"""readmatrix.read_matrices_device (nanosnp_amd/csrc/hap_reads.hip: nsnp_hap_read_depths, nsnp_hap_read_matrices) on the GPU against
readmatrix.read_matrices on tests/record_rules.py's per-base stand-in for the same reads: exact, no tolerance."""
import zlib

import numpy as np
import pytest

from nanosnp_amd import readmatrix
from nanosnp_amd._lib import NanoSNPError
from tests import record_rules as rr
from tests.helpers import golden, synth_groups, synth_reads

pytestmark = pytest.mark.gpu
MAXCOV = 10000
GROUPS = synth_groups(78)


def _host(records, groups=GROUPS, max_coverage=MAXCOV):
    return readmatrix.read_matrices(rr.RecordSamfile(records), groups, max_coverage)


def _device(ctx, records, groups=GROUPS, max_coverage=MAXCOV):
    return readmatrix.read_matrices_device(ctx, rr.to_alignment_records(records), groups, max_coverage)


def _equal(ctx, records, groups=GROUPS, max_coverage=MAXCOV):
    """both sides not None (a case cannot pass as None == None) and equal in names, positions, groups and all four matrices"""
    import torch
    want = _host(records, groups, max_coverage)
    assert want is not None, "the host yardstick returns None: the case checks nothing"
    got = _device(ctx, records, groups, max_coverage)
    assert got is not None
    assert all(isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.int32 for m in (got.seq, got.hap, got.baseq, got.mapq))
    rr.same_matrices(got, want)
    return got, want


def _none(ctx, records, groups=GROUPS, max_coverage=MAXCOV):
    assert _host(records, groups, max_coverage) is None, "the host yardstick does not return None"
    assert _device(ctx, records, groups, max_coverage) is None


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("variant", ["plain", "mixed", "unit"])
def test_equals_the_host_function(gpu_ctx, variant, seed):
    records = rr.synth_records(10 * seed + 400, variant)
    if variant == "unit":                                  # single reads with more than 64, more than 256 and about 700 ops
        n = sorted(len(rd["cigar"]) for rd in records)
        assert n[0] > 64 and any(256 < k < 400 for k in n) and n[-1] > 700
    if variant == "mixed":
        assert {op for rd in records for op, _ in rd["cigar"]} == set(range(9))
    groups = synth_groups(seed + 500)
    _equal(gpu_ctx, records, groups)


@pytest.mark.parametrize("seed", [4, 5])
def test_300_reads_cross_a_workgroup_of_records(gpu_ctx, seed):
    _equal(gpu_ctx, rr.synth_records(seed, "mixed", n_reads=300))


def test_a_cigar_longer_than_a_tile(gpu_ctx):
    """reads of 1500 and 2600 ops of length 1: two and three tiles of 1024 ops with carried prefixes, among ordinary reads"""
    rng = np.random.default_rng(9)
    records = rr.synth_records(9, "mixed", n_reads=40)
    for k, span in enumerate((1200, 2100)):
        records.append(rr.make_record(rng, f"long{k}", 3 + k, rr._cigar(rng, "unit", span)))
    assert sorted(len(rd["cigar"]) for rd in records)[-2] > 1024 and max(len(rd["cigar"]) for rd in records) > 2048
    records.sort(key=lambda rd: rd["a"])
    groups = synth_groups(78, centres=(260, 700, 1150, 1500))
    _equal(gpu_ctx, records, groups)


def _edge_records(ext):
    """reads placed against the wanted columns `ext` (sorted): name -> what it is there for"""
    rng = np.random.default_rng(12)
    have = set(ext)
    w = next(p for p in ext if p > 200)                                                     # some wanted column
    lone = next(p for p in ext if not have & {p - 2, p - 1, p + 1, p + 2})                   # a wanted column with no wanted neighbour
    gap = next(p for p, q in zip(ext, ext[1:]) if q - p >= 5)                                # gap + 1 .. gap + 4 are not wanted
    mk = lambda name, a, cigar, **kw: rr.make_record(rng, name, a, cigar, **kw)             # noqa: E731
    return [
        mk("one_base", w, [(rr.M, 1)]),
        mk("one_base_off", gap + 2, [(rr.M, 1)]),
        mk("starts_on", w, [(rr.M, 50)]),
        mk("ends_on", w - 49, [(rr.M, 50)]),
        mk("covers_none_front", 5, [(rr.M, 20)]),
        mk("covers_none_between", gap + 1, [(rr.M, 3)]),
        mk("only_under_n", lone - 2, [(rr.M, 2), (rr.N, 1), (rr.M, 2)]),
        mk("ins_in_front", w - 10, [(rr.M, 10), (rr.I, 3), (rr.M, 10)]),
        mk("clip_in_front", w, [(rr.S, 5), (rr.M, 20)]),
        mk("hard_clip_in_front", w, [(rr.H, 5), (rr.M, 20), (rr.H, 2)]),
        mk("del_on", w - 3, [(rr.M, 3), (rr.D, 1), (rr.M, 3)]),
        mk("lower_case", w - 20, [(rr.M, 40)], lower=True),
        mk("no_reference_op", w, [(rr.S, 4), (rr.I, 2)]),
    ]


def test_edge_reads(gpu_ctx):
    base = rr.synth_records(11, "mixed", n_reads=30)
    ext = _host(base).positions
    assert min(ext) > 30
    records = sorted(base + _edge_records(ext), key=lambda rd: rd["a"])
    got, want = _equal(gpu_ctx, records)
    assert got.positions == ext
    for absent in ("covers_none_front", "covers_none_between", "one_base_off", "no_reference_op"):
        assert absent not in got.names
    row = got.names.index("only_under_n")
    assert not any(m[row].any().item() for m in (got.seq, got.hap, got.baseq, got.mapq))
    for present in ("one_base", "starts_on", "ends_on", "ins_in_front", "clip_in_front", "hard_clip_in_front", "del_on", "lower_case"):
        assert got.seq[got.names.index(present)].ne(0).any().item(), present


# ---- the None cases of tests/test_readmatrix.py::test_coverage_filter_and_foreign_bases ----------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    records = rr.from_helper_reads(synth_reads(77))
    cov = {col.pos + 1: col.n for col in rr.RecordSamfile(records).pileup("c", 1, 900)}
    return records, cov


def test_a_group_dropped_by_the_first_pass(gpu_ctx, plain):
    records, cov = plain
    survived = 0
    for g in GROUPS:
        limit = max(cov[p] for _, p in g) - 1
        want = _host(records, GROUPS, limit)
        got = _device(gpu_ctx, records, GROUPS, limit)
        assert (want is None) == (got is None)
        if want is not None:
            assert g not in want.groups and 0 < len(want.groups) < len(GROUPS)
            rr.same_matrices(got, want)
            survived += 1
    assert survived, "no limit leaves a group behind: the case checks nothing"
    _none(gpu_ctx, records, GROUPS, 0)


def test_a_window_column_too_deep_and_exactly_at_the_limit(gpu_ctx, plain):
    records, cov = plain
    gpos = {p for g in GROUPS for _, p in g}
    centre = GROUPS[0][5][1]
    wcol = next(p for p in range(centre - 16, centre + 17) if p not in gpos)
    lim = max(cov.values())
    rng = np.random.default_rng(3)
    extra = [rr.make_record(rng, f"x{k}", wcol, [(rr.M, 1)], hp=1) for k in range(lim - cov[wcol] + 1)]
    by_start = lambda rs: sorted(rs, key=lambda rd: rd["a"])                               # noqa: E731
    _none(gpu_ctx, by_start(records + extra), GROUPS, lim)
    _equal(gpu_ctx, by_start(records + extra[:-1]), GROUPS, lim)


def test_hp_tags_outside_1_to_3(gpu_ctx, plain):
    records, _ = plain
    k = next(i for i, rd in enumerate(records) if rd["a"] <= 260 <= rr._RecAlignment(rd).end)
    for tag in (7, 0):
        odd = [dict(rd) for rd in records]
        odd[k]["hp"] = tag
        _none(gpu_ctx, odd)
    rng = np.random.default_rng(4)
    aside = sorted(records + [rr.make_record(rng, "aside", 5, [(rr.M, 20)], hp=7)], key=lambda rd: rd["a"])
    got, _ = _equal(gpu_ctx, aside)                        # a read that covers no wanted column is never looked at
    assert "aside" not in got.names


def test_foreign_bases(gpu_ctx, plain):
    records, _ = plain
    ext = set(_host(records).positions)
    k = next(i for i, rd in enumerate(records) if rr._RecAlignment(rd).at.get(260, ("", None))[0] == "M")
    at = rr._RecAlignment(records[k]).at

    def with_n(p):
        bad = [dict(rd) for rd in records]
        q = at[p][1]
        bad[k]["seq"] = bad[k]["seq"][:q] + "N" + bad[k]["seq"][q + 1:]
        return bad
    _none(gpu_ctx, with_n(260))
    elsewhere = next(p for p, (kind, _) in at.items() if kind == "M" and p not in ext)
    _equal(gpu_ctx, with_n(elsewhere))


def test_meta_names_the_first_offence(gpu_ctx, plain):
    """the status word of the raw entry: the first offence in the host function's order (column, then record)"""
    import torch
    records, _ = plain
    ext = _host(records).positions
    covering = [i for i, rd in enumerate(records) if rr._RecAlignment(rd).at.get(260, ("", None))[0] == "M"]
    k1, k2 = covering[0], covering[-1]
    bad = [dict(rd) for rd in records]
    for k in (k1, k2):
        q = rr._RecAlignment(records[k]).at[260][1]
        bad[k]["seq"] = bad[k]["seq"][:q] + "n" + bad[k]["seq"][q + 1:]
    bad[k2]["hp"] = 5                                      # met at the first wanted column that record k2 covers
    first_col = min(p for p in ext if p in rr._RecAlignment(records[k2]).at)
    rec = rr.to_alignment_records(bad).to_device(torch.device("cuda", gpu_ctx.device))
    cols = torch.tensor(ext, dtype=torch.int64, device="cuda")
    depth, rows = gpu_ctx.hap_read_depths(rec, cols, want_rows=True)
    want_depth = [sum(1 for rd in records if p in rr._RecAlignment(rd).at) for p in ext[:40]]
    assert depth[:40].tolist() == want_depth
    *_, meta = gpu_ctx.hap_read_matrices(rec, cols, MAXCOV, int(rows.item()))
    n_rows, status, record, column = meta.tolist()
    assert n_rows == int(rows.item()) > 0
    if first_col < 260 or (first_col == 260 and k2 == k1):
        assert (status, record, column) == (2, k2, first_col)
    else:
        assert (status, record, column) == (3, k1, 260)
    *_, meta = gpu_ctx.hap_read_matrices(rec, cols, int(depth.max().item()) - 1, int(rows.item()))
    deep = next(p for p, d in zip(ext, depth.tolist()) if d == int(depth.max().item()))
    n_rows, status, record, column = meta.tolist()
    if deep <= min(first_col, 260):
        assert (status, record, column) == (1, -1, deep)
    else:
        assert status in (2, 3) and column < deep


# ---- downstream ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie_order", ["stable", "numpy1"])
def test_group_planes_from_device_matrices(gpu_ctx, tie_order):
    import torch
    records = rr.synth_records(21, "mixed")
    got, want = _equal(gpu_ctx, records)
    D = len(want.names) - 3                                 # a cut where a site is that deep
    a = readmatrix.group_planes(gpu_ctx, got, D, D, tie_order=tie_order)
    b = readmatrix.group_planes(gpu_ctx, want, D, D, tie_order=tie_order)
    torch.cuda.synchronize()
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2] + a[3] + (a[4], a[5]), b[2] + b[3] + (b[4], b[5])):
        assert x.dtype == y.dtype and torch.equal(x, y)
    pplanes = a[3]
    ref_row = torch.zeros((len(a[0]), 33), dtype=torch.int32, device="cuda")
    feat = gpu_ctx.hap_features(pplanes[0], pplanes[1], pplanes[2], pplanes[3], ref_row)
    assert feat.shape == (len(a[0]), 105, 33) and torch.isfinite(feat).all()


def test_group_planes_equal_the_reference_function(gpu_ctx):
    """tests/golden/hap_records.npz (make_golden_records.py): what the reference's function returns for these reads"""
    import torch
    from tests.test_readmatrix import _compare_with_reference
    z = np.load(golden("hap_records.npz"))
    records = rr.synth_records(int(z["seed"]), "mixed")
    arrays = rr.to_arrays(records)
    crc = zlib.crc32(b"".join(np.ascontiguousarray(arrays[k]).tobytes() for k in
                              ("start", "mapq", "hp", "cigar", "cigar_off", "seq", "qual", "seq_off")))
    assert crc == int(z["records_crc32"]), "hap_records.npz: the rebuilt records are not the recorded ones (another numpy random stream?)"
    rm = readmatrix.read_matrices_device(gpu_ctx, rr.to_alignment_records(records), synth_groups(int(z["group_seed"])), MAXCOV)
    Dh, Dp = (int(v) + 2 for v in z["max_depths"])
    cand, hpos, hplanes, pplanes, dh, dp = readmatrix.group_planes(gpu_ctx, rm, Dh, Dp)
    torch.cuda.synchronize()
    assert cand == z["candidates"].tolist() and hpos == z["haplotype_positions"].tolist()
    for g in range(len(cand)):
        _compare_with_reference(z, g, "h", tuple(p[g].cpu().numpy() for p in hplanes), int(dh[g].item()))
        _compare_with_reference(z, g, "p", tuple(p[g].cpu().numpy() for p in pplanes), int(dp[g].item()))


# ---- determinism, refusals ------------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_again_and_on_another_stream(gpu_ctx):
    import torch
    ar = rr.to_alignment_records(rr.synth_records(31, "mixed", n_reads=300))
    first = readmatrix.read_matrices_device(gpu_ctx, ar, GROUPS, MAXCOV)
    second = readmatrix.read_matrices_device(gpu_ctx, ar, GROUPS, MAXCOV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = readmatrix.read_matrices_device(gpu_ctx, ar, GROUPS, MAXCOV)
    side.synchronize()
    torch.cuda.synchronize()
    assert first is not None and first.names == second.names == third.names
    for other in (second, third):
        for x, y in zip((first.seq, first.hap, first.baseq, first.mapq), (other.seq, other.hap, other.baseq, other.mapq)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_refusals(gpu_ctx):
    import torch
    records = rr.synth_records(32, "mixed", n_reads=20)
    good = rr.to_arrays(records)
    swapped = dict(good, start=good["start"][::-1].copy())
    with pytest.raises(NanoSNPError):
        readmatrix.AlignmentRecords.from_arrays(**swapped)
    with pytest.raises(NanoSNPError):
        readmatrix.AlignmentRecords.from_arrays(**dict(good, seq_off=good["seq_off"] + 1))
    with pytest.raises(NanoSNPError):
        readmatrix.AlignmentRecords.from_arrays(**dict(good, cigar_off=good["cigar_off"][:-1]))
    # cap_rows below the row count: NSNP_EINVAL from the raw binding, and nothing written
    rec = rr.to_alignment_records(records).to_device(torch.device("cuda", gpu_ctx.device))
    cols = torch.tensor(_host(records).positions, dtype=torch.int64, device="cuda")
    _, rows = gpu_ctx.hap_read_depths(rec, cols, want_rows=True)
    rows = int(rows.item())
    assert rows > 1
    P = cols.shape[0]
    outs = [torch.full((rows - 1, P), 77, dtype=torch.int32, device="cuda") for _ in range(4)]
    row_record = torch.full((rows - 1,), 77, dtype=torch.int64, device="cuda")
    meta = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    lib = gpu_ctx.lib
    scratch = torch.empty(lib.nsnp_hap_read_scratch_bytes(rec.n, P), dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr()                           # noqa: E731
    args = [ptr(rec.start), ptr(rec.mapq), ptr(rec.hp), ptr(rec.cigar), ptr(rec.cigar_off), ptr(rec.seq), ptr(rec.qual), ptr(rec.seq_off),
            rec.n, ptr(cols), P, MAXCOV, *[ptr(o) for o in outs]]
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.nsnp_hap_read_matrices(gpu_ctx.handle, *args, rows - 1, ptr(row_record), ptr(meta), ptr(scratch), stream)
    torch.cuda.synchronize()
    assert rc == -1                                         # NSNP_EINVAL
    assert all((o == 77).all().item() for o in outs) and (row_record == 77).all().item()
    assert lib.nsnp_hap_read_matrices(gpu_ctx.handle, *args, -1, ptr(row_record), ptr(meta), ptr(scratch), stream) == -1
    assert lib.nsnp_hap_read_matrices(gpu_ctx.handle, *args, rows - 1, ptr(row_record), None, ptr(scratch), stream) == -1
