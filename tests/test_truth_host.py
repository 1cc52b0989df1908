"""nanosnp_amd.truth: the truth VCF of a training run, against what the reference's compiled DNA_SplitVcf and DNA_CreateTrainData wrote
(tests/golden/train_*: make_golden_train.py) and against the numpy restatement of the rules (tests/label_rules.py), every refusal, and
the threshold arithmetic of the subsample against the reference's logged ratios.  No GPU."""
import gzip
import json

import numpy as np
import pytest

from nanosnp_amd import truth
from tests import label_rules as lr
from tests.helpers import golden

CASES = (("train_g1", "chrS"), ("train_cut", "chrC"), ("train_g1_bed", "chrS"))
HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"


def _row(pos=b"100", ref=b"A", alt=b"C", gt=b"0/1", contig=b"chr1", fmt=b"GT"):
    return b"\t".join([contig, pos, b".", ref, alt, b"50", b"PASS", b".", fmt, gt]) + b"\n"


def _fixture(case):
    return (open(golden(case + ".vcf"), "rb").read(), open(golden(case + ".true_var"), "rb").read(),
            gzip.open(golden(case + ".td.gz")).read().decode(), json.load(open(golden(case + ".json"))))


@pytest.mark.parametrize("case,contig", CASES)
def test_split_rows_equal_the_reference_true_var(case, contig):
    vcf, true_var, _, _ = _fixture(case)
    assert truth.true_var_text(vcf, contig) == true_var
    assert truth.true_var_text(vcf, "chrOther").count(b"\n") == 1 and truth.true_var_text(vcf, "chrNone") == b""


@pytest.mark.parametrize("case,contig", CASES)
def test_load_truth_gives_the_labels_of_the_reference_td(case, contig):
    vcf, true_var, td, counts = _fixture(case)
    keys, codes, per_contig = truth.load_truth(vcf, ["unused", contig])               # (the contig is entry 1 of the table)
    assert keys.dtype == np.int64 and codes.dtype == np.uint32 and per_contig.tolist() == [0, counts["ratio_1000000"]["truth"]]
    assert np.all(np.diff(keys) > 0) and np.all(keys >> 36 == 1) and keys.size == true_var.count(b"\n")
    names, labels, has_truth = lr.parse_td(td)
    pos = np.array([int(n.split(":")[1]) for n in names], np.int64)
    at = np.searchsorted(keys, (1 << 36) | pos)
    hit = (at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == ((1 << 36) | pos))
    assert np.array_equal(hit, has_truth) and int(hit.sum()) == counts["ratio_1000000"]["variants"]
    assert np.array_equal(truth.labels_of(codes[at[hit]]), labels[hit])
    # the labels of the other rows: the homozygous-reference code of the centre base
    ref33 = [line.split("\t")[2].rsplit(":", 1)[1] for line in td.split("\n") if line.strip()]
    ref_codes = np.array([truth.reference_code(r[16]) for r, h in zip(ref33, hit) if not h], np.uint32)
    assert np.array_equal(truth.labels_of(ref_codes), labels[~hit])
    # and the restated rules say the same about every truth row, candidate site or not
    table = lr.truth_table(vcf.decode(), ["unused", contig])
    assert sorted(table) == keys.tolist()
    assert [tuple(int(v[i]) for v in truth.unpack_codes(codes)) for i in range(keys.size)] == [table[k] for k in keys.tolist()]


def test_genotype_quirks():
    assert truth.genotype_of(b"./.") == (0, 0) and truth.genotype_of(b"2|1:7:x") == (1, 2) and truth.genotype_of(b"1/.") == (0, 1)
    assert truth.genotype_of(b"x|1") == (0, 1) and truth.genotype_of(b"0/1:0/0") == (0, 1)
    assert truth.fix_alternate(b"G,*", 1, 2) == (b"G,", 0, 1) and truth.fix_alternate(b"*,G", 1, 2) == (b",G", 0, 1)
    assert truth.fix_alternate(b"*", 0, 1) is None and truth.fix_alternate(b"G,*", 0, 1) is None and truth.fix_alternate(b"G,*,T", 1, 2) is None
    gt = lambda *a: truth.GT21_LABELS[truth.label_code(*a) & 0x1f]
    assert gt(b"C", b"G,", 0, 1) == "CIns" and gt(b"C", b",G", 0, 1) == "CIns"              # one allele of length 2 against a 1-base REF
    assert gt(b"A", b"C", 0, 1) == "AC" and gt(b"T", b"C", 0, 1) == "CT" and gt(b"A", b"C", 1, 1) == "CC" and gt(b"A", b"G,C", 1, 2) == "CG"
    assert gt(b"A", b"ATT", 1, 1) == "InsIns" and gt(b"ATT", b"A", 0, 1) == "ADel" and gt(b"AT", b"ATTT,A", 1, 2) == "InsDel"
    assert gt(b"A", b"C,G,T", 1, 2) == "CG"                                                   # more than two alleles: the first two
    zy = lambda *a: (truth.label_code(*a) >> 8) & 3
    assert [zy(b"A", b"C", *g) for g in ((0, 0), (1, 1), (0, 1), (1, 2), (2, 2), (0, 2))] == [0, 1, 2, 2, 1, 2]
    assert truth.label_code(b"A", b"C", 0, 1) >> 16 == 32 | 32 << 8 and truth.reference_code("G") == 7 | 16 << 16 | 16 << 24


@pytest.mark.parametrize("row,what", [
    (_row(gt=b"1"), "genotype without"),
    (_row(alt=b"N"), "no gt21 label"),
    (_row(alt=b"c"), "no gt21 label"),
    (_row(ref=b"N", alt=b"NA"), "no gt21 label"),
    (_row(pos=b"0100"), "canonical"),
    (_row(pos=b"+5"), "canonical"),
    (_row(pos=b"1e3"), "canonical"),
    (_row(pos=str(1 << 36).encode()), "canonical"),
    (_row() + _row(alt=b"G"), "occurs twice"),
    (b"chr1\t100\t.\tA\n", "fewer than five"),
])
def test_refusals_name_the_row(row, what):
    with pytest.raises(ValueError, match=what):
        truth.load_truth(HEAD + row, ["chr1"])


def test_rows_that_are_passed_over_and_the_key_layout():
    vcf = HEAD + _row(contig=b"chrZ", gt=b"1") + _row(pos=b"7", contig=b"chr2") + _row(alt=b"*") + b"\n" + _row(pos=str((1 << 36) - 1).encode())
    keys, codes, counts = truth.load_truth(vcf, ["chr1", "chr2"])                       # (the row of chrZ is not even parsed)
    assert keys.tolist() == [(1 << 36) - 1, (1 << 36) | 7] and counts.tolist() == [1, 1] and codes.tolist() == [truth.label_code(b"A", b"C", 0, 1)] * 2
    keys, codes, counts = truth.load_truth(HEAD, ["chr1"])
    assert keys.size == 0 and codes.size == 0 and keys.dtype == np.int64 and codes.dtype == np.uint32 and counts.tolist() == [0]
    assert truth.load_truth(gzip.compress(vcf), ["chr2"])[0].tolist() == [7]


@pytest.mark.parametrize("case,contig", CASES)
def test_threshold_arithmetic_against_the_reference_log(case, contig):
    c = _fixture(case)[3]["ratio_5"]
    thr, ratio = truth.keep_thresholds([c["variants"]], [c["non_variants"]], 5.0)
    assert "%g" % ratio[0] == c["ratio"] and "%g" % (c["variants"] / c["truth"]) == c["recall"]
    max_nv = int(c["variants"] * 5.0)
    assert thr[0] == ((max_nv << 53) // c["non_variants"] if max_nv < c["non_variants"] else 1 << 53)
    assert lr.threshold(c["variants"], c["non_variants"], 5.0) == (thr[0] if thr[0] < 1 << 53 else None, ratio[0])


def test_thresholds_truncate_and_keep_nothing_without_truth():
    thr, ratio = truth.keep_thresholds([0, 3, 3, 1], [40, 7, 8, 0], 2.5)                # int(7.5) = 7: 7 < 7 is false, 7 < 8 subsamples
    assert thr == [0, 1 << 53, (7 << 53) // 8, 1 << 53] and ratio == [0.0, 1.0, 7 / 8, 1.0]
