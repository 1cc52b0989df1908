"""readmatrix.AlignmentRecords (packing, validation) and the helpers of tests/record_rules.py, on the CPU: the per-base stand-in
against tests.helpers.FakeSamfile, and the numpy restatement of the device rules against readmatrix.read_matrices."""
import numpy as np
import pytest

from nanosnp_amd import readmatrix
from nanosnp_amd._lib import NanoSNPError
from tests import record_rules as rr
from tests.helpers import FakeSamfile, synth_groups, synth_reads

FIELDS = ("start", "mapq", "hp", "cigar", "cigar_off", "seq", "qual", "seq_off")


def test_record_samfile_on_plain_reads_equals_the_fake_samfile():
    reads = sorted(synth_reads(77), key=lambda r: r["a"])
    groups = synth_groups(78)
    want = readmatrix.read_matrices(FakeSamfile(reads), groups, max_coverage=10000)
    got = readmatrix.read_matrices(rr.RecordSamfile(rr.from_helper_reads(reads)), groups, max_coverage=10000)
    assert want is not None and got is not None
    rr.same_matrices(got, want)


@pytest.mark.parametrize("variant", ["plain", "mixed", "unit"])
def test_from_alignments_round_trips_to_from_arrays(variant):
    records = rr.synth_records(5, variant, n_reads=20)
    a = rr.to_alignment_records(records)
    b = readmatrix.AlignmentRecords.from_alignments(rr.RecordSamfile(records).fetch(), contig="c")
    assert b.contig == "c" and a.names == b.names and len(a) == len(b) == 20
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert a.cigar.dtype == np.uint32 and a.start.dtype == np.int64 and a.hp.dtype == np.int32 and a.seq.dtype == np.uint8


def test_from_alignments_drops_what_the_pileup_stepper_drops():
    records = rr.synth_records(6, "mixed", n_reads=12)
    flags = [0, 0x4, 0x100, 0x200, 0x400, 0x1, 0x1 | 0x2, 0x10, 0x800, 0x1 | 0x2 | 0x400, 0x1 | 0x40, 0x2]
    for rd, f in zip(records, flags):
        rd["flag"] = f
    keep = [rd["name"] for rd, f in zip(records, flags) if not f & 0x704 and not (f & 0x1 and not f & 0x2)]
    assert len(keep) == 5
    got = readmatrix.AlignmentRecords.from_alignments(rr.RecordSamfile(records).fetch())
    assert got.names == keep
    want = rr.to_alignment_records([rd for rd in records if rd["name"] in keep])
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


def test_an_hp_tag_outside_1_to_3_stays_refusable():
    records = rr.synth_records(7, "plain", n_reads=4)
    records[1]["hp"], records[2]["hp"], records[3]["hp"] = -1, 7, None
    got = readmatrix.AlignmentRecords.from_alignments(rr.RecordSamfile(records).fetch())
    assert got.hp[3] == -1 and not 1 <= got.hp[1] <= 3 and got.hp[1] != -1 and not 1 <= got.hp[2] <= 3


def test_every_refusal():
    records = rr.synth_records(8, "mixed", n_reads=10)
    good = rr.to_arrays(records)
    readmatrix.AlignmentRecords.from_arrays(**good)

    def refused(**change):
        kw = {k: (v.copy() if hasattr(v, "copy") else list(v)) for k, v in good.items()}
        for k, f in change.items():
            kw[k] = f(kw[k])
        with pytest.raises(NanoSNPError):
            readmatrix.AlignmentRecords.from_arrays(**kw)

    def put(i, v):
        def f(a):
            a[i] = v
            return a
        return f
    refused(cigar_off=put(3, int(good["cigar_off"][4]) + 1))              # not monotone
    refused(seq_off=put(3, int(good["seq_off"][2]) - 1))                  # not monotone
    refused(cigar_off=lambda a: a[:-1])                                   # not R + 1 offsets
    refused(seq_off=put(-1, int(good["seq_off"][-1]) + 1))                # the last offset is not the array's length
    refused(cigar_off=put(0, 1))
    refused(qual=lambda a: a[:-1])
    k = next(i for i, w in enumerate(good["cigar"]) if int(w) & 15 == rr.M)
    refused(cigar=put(k, int(good["cigar"][k]) + 16))                     # query-consuming lengths no longer sum to the sequence
    refused(seq_off=put(5, int(good["seq_off"][5]) + 1))                  # monotone, but two reads' lengths are off by one
    refused(cigar=put(0, (int(good["cigar"][0]) & ~15) | 9))              # op code 9
    refused(cigar=put(0, (int(good["cigar"][0]) & ~15) | 15))
    refused(start=put(4, int(good["start"][3]) - 1))                      # starts decrease
    refused(names=lambda n: n[:-1] + [n[0]])                              # a name twice
    refused(mapq=lambda a: a[:-1])
    refused(hp=lambda a: a.astype(np.float64))


CASES = [(seed, variant) for variant in ("plain", "mixed", "unit") for seed in range(4)]


@pytest.mark.parametrize("seed,variant", CASES)
def test_the_restated_rules_equal_read_matrices(seed, variant):
    records = rr.synth_records(100 + seed, variant)
    groups = synth_groups(200 + seed)
    want = readmatrix.read_matrices(rr.RecordSamfile(records), groups, max_coverage=10000)
    assert want is not None
    if variant == "unit":
        assert max(len(rd["cigar"]) for rd in records) > 600
    rr.same_matrices(rr.rules_matrices(rr.to_alignment_records(records), groups, 10000), want)


def test_the_stand_in_and_the_rules_equal_the_reference_function():
    """tests/golden/hap_records.npz (make_golden_records.py): the reference's own function on RecordSamfile over reads with every op;
    the matrices of read_matrices on the stand-in and of the restated rules, arranged by the oracle, per group as
    tests/test_readmatrix.py compares them"""
    import zlib
    from oracle import oracle
    from tests.helpers import golden
    from tests.test_readmatrix import _compare_with_reference
    z = np.load(golden("hap_records.npz"))
    records = rr.synth_records(int(z["seed"]), "mixed")
    arrays = rr.to_arrays(records)
    assert zlib.crc32(b"".join(np.ascontiguousarray(arrays[k]).tobytes() for k in FIELDS)) == int(z["records_crc32"])
    groups = synth_groups(int(z["group_seed"]))
    rm = readmatrix.read_matrices(rr.RecordSamfile(records), groups, max_coverage=10000)
    names, ext, seq, hap, bq, mq, kept = rr.rules_matrices(rr.to_alignment_records(records), groups, 10000)
    rm2 = readmatrix.ReadMatrices("c", ext, names, seq, hap, bq, mq, kept)
    for m in (rm, rm2):
        sl = readmatrix.group_slices(m)
        assert [s["candidate"] for s in sl] == z["candidates"].tolist()
        assert [s["haplotype_positions"] for s in sl] == z["haplotype_positions"].tolist()
        depths = {"h": [], "p": []}
        for g, s in enumerate(sl):
            for tag, key in (("h", "hap_cols"), ("p", "pile_cols")):
                ins = [x[:, s[key]] for x in (m.seq, m.baseq, m.mapq, m.hap)]
                *planes, depth = oracle.hap_arrange(*ins, z[f"g{g}_{tag}_out_seq"].shape[0] + 3)
                _compare_with_reference(z, g, tag, tuple(planes), depth)
                depths[tag].append(depth)
        assert [max(depths["h"]), max(depths["p"])] == z["max_depths"].tolist()


def test_the_restated_rules_return_none_where_read_matrices_does():
    records = rr.synth_records(300, "mixed")
    groups = synth_groups(301)
    ar = rr.to_alignment_records(records)
    cov = {col.pos + 1: col.n for col in rr.RecordSamfile(records).pileup("c", 1, 900)}
    limit = max(cov.get(p, 0) for _, p in groups[0]) - 1
    want = readmatrix.read_matrices(rr.RecordSamfile(records), groups, max_coverage=limit)
    got = rr.rules_matrices(ar, groups, limit)
    assert (want is None) == (got is None)
    if want is not None:
        assert len(want.groups) < len(groups)
        rr.same_matrices(got, want)
    assert rr.rules_matrices(ar, groups, 0) is None and readmatrix.read_matrices(rr.RecordSamfile(records), groups, 0) is None
    odd = [dict(rd) for rd in records]
    k = next(i for i, rd in enumerate(odd) if rd["a"] <= 260 <= rr._RecAlignment(rd).end)      # 260 is a centre: a wanted column
    odd[k]["hp"] = 7
    assert readmatrix.read_matrices(rr.RecordSamfile(odd), groups, 10000) is None
    assert rr.rules_matrices(rr.to_alignment_records(odd), groups, 10000) is None
