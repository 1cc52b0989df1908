"""BED region filters without a GPU: the BED reader, the bitmap, and the two rules restated in numpy (tests/bed_rules.py) against the
fixtures the reference's own programs wrote (tests/golden/make_golden_bed.py)."""
import gzip

import numpy as np
import pytest

from nanosnp_amd import bed, host
from nanosnp_amd._lib import NanoSNPError
from tests import bed_rules
from tests.helpers import golden

FAI = "chr1\t1000\t6\t60\t61\nchr2\t77\t1100\t60\t61\n"
CASES = [(tag, case) for tag in ("g1", "cut") for case in ("ext", "conf", "both")]


def load_case(tag, case):
    """-> (mpileup text, sequence, contig, the reference's .pd, extended intervals or None, confident intervals or None)"""
    text = gzip.open(golden(f"encode_{tag}.mpileup.gz")).read()
    fa = gzip.open(golden(f"encode_{tag}.fa.gz")).read()
    contig = fa.split(b"\n")[0][1:].split()[0].decode()
    seq = np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8).copy()
    pd = gzip.open(golden(f"bed_{tag}_{case}.pd.gz")).read()
    iv = {}
    for kind in ("ext", "conf"):
        iv[kind] = None
        if case in (kind, "both"):
            iv[kind] = bed.load_bed(golden(f"bed_{tag}_{case}.{kind}.bed"), {contig: seq.size})[contig]
    return text, seq, contig, pd, iv["ext"], iv["conf"]


def test_bed_reader_comments_overlaps_and_fields(tmp_path):
    text = (b"# a comment\nchr1\t10\t20\n#chr1\t0\t1000\nchr1\t15\t30\textra\tfields\nchr2\t0\t77\r\nchr1\t\t40\t41\n"
            b"chr1\t 50x\t60.9\nchr1\t+7\t9\n")
    got = bed.load_bed(text, FAI)
    assert sorted(got) == ["chr1", "chr2"]
    # runs of tabs are one separator (split_line), from / to as atoi reads them (leading blanks, a sign, digits up to the first other byte)
    assert got["chr1"].tolist() == [[10, 20], [15, 30], [40, 41], [50, 60], [7, 9]] and got["chr2"].tolist() == [[0, 77]]
    p = tmp_path / "a.bed"
    p.write_bytes(text)
    assert all(np.array_equal(got[k], v) for k, v in bed.load_bed(str(p), FAI).items())
    assert bed.load_bed(p, {"chr1": 1000, "chr2": 77})["chr2"].tolist() == [[0, 77]]
    assert bed.load_bed(b"", FAI) == {} and bed.load_bed(b"#only\n", FAI) == {}
    # one contig of a larger file, checked against its own length alone
    assert sorted(bed.load_bed(text, {"chr2": 77}, skip_unknown=True)) == ["chr2"]
    assert bed.contig_intervals(str(p), "chr2", 77).tolist() == [[0, 77]]
    assert bed.contig_intervals(got, "chr9", 5).shape == (0, 2) and bed.contig_intervals(None, "chr1", 5) is None


@pytest.mark.parametrize("line", [b"chr1\t10\n", b"chr1\n", b"\n", b"chr1\t20\t20\n", b"chr1\t30\t10\n", b"chr1\t10\t1001\n", b"chr3\t1\t2\n",
                                  b"chr1\tx\ty\n", b"chr1\t-5\t10\n"])
def test_bed_reader_errors(line):
    """what BedIntvList's constructor asserts on: fewer than three fields, from >= to, to beyond the contig, an unknown contig"""
    with pytest.raises(NanoSNPError):
        bed.load_bed(b"chr1\t1\t2\n" + line, FAI)


def test_bitmap_equals_a_plain_loop():
    rng = np.random.default_rng(7)
    for chr_len in (1, 31, 32, 33, 64, 65, 1000, 4097):
        for _ in range(20):
            n = int(rng.integers(0, 9))
            lo = rng.integers(0, chr_len, n)
            iv = np.stack([lo, np.minimum(chr_len, lo + rng.integers(1, max(2, chr_len // 2), n))], 1)
            w = bed.bed_bitmap(iv, chr_len)
            assert w.dtype == np.uint32 and w.size == (chr_len + 31) // 32
            want = bed_rules.bit_array(iv, chr_len)
            assert np.array_equal(bed_rules.bits_from_words(w, chr_len), want)
            assert sum(bin(int(x)).count("1") for x in w) == int(want.sum())          # no bit beyond the contig
    assert not bed.bed_bitmap(None, 100).any() and bed.bed_bitmap([], 0).size == 0
    assert bed.bed_bitmap([[0, 64]], 64).tolist() == [0xFFFFFFFF] * 2
    for bad in ([[5, 5]], [[-1, 3]], [[0, 101]]):
        with pytest.raises(NanoSNPError):
            bed.bed_bitmap(bad, 100)


def test_confident_reach_in_the_restatement():
    """[p - 1, p + max_del + 1): two bits without a deletion - a site just left of an interval passes -, L + 1 bases to the right with one"""
    bits = bed_rules.bit_array([[10, 12]], 40)
    pos = np.arange(1, 41)
    assert np.nonzero(bed_rules.confident_pass(pos, np.zeros(40, int), bits))[0].tolist() == [9, 10, 11]          # positions 10, 11, 12
    assert np.nonzero(bed_rules.confident_pass(pos, np.full(40, 3), bits))[0].tolist() == [6, 7, 8, 9, 10, 11]    # positions 7 .. 12
    assert not bed_rules.confident_pass([41, 100], [60, 0], bits).any()                                          # beyond the contig: 0


@pytest.mark.parametrize("tag,case", CASES)
def test_restated_rules_reproduce_the_reference_fixtures(tag, case):
    """the fixtures and the stated semantics agree before any GPU is involved: sites, windows and depths of the reference's .pd"""
    text, seq, contig, pd, ext, conf = load_case(tag, case)
    pos, col_off, bases = host.mpileup_parse(text)
    eb = None if ext is None else bed_rules.bits_from_words(bed.bed_bitmap(ext, seq.size), seq.size)
    cb = None if conf is None else bed_rules.bits_from_words(bed.bed_bitmap(conf, seq.size), seq.size)
    gx, _, gpos, _ = host.pd_parse(pd)
    rpos, rx, rdepth = bed_rules.reference_sites(pos, col_off, bases, seq, eb, cb)
    assert np.array_equal(rpos, gpos) and np.array_equal(rx, gx)
    assert np.array_equal(rdepth, [int(l.split(b"\t")[2].split(b"-")[0]) for l in pd.splitlines()])
    # every fixture filters something and leaves something
    _, _, npos, _ = host.pd_parse(gzip.open(golden(f"encode_{tag}.pd.gz")).read())
    assert 0 < gpos.size < npos.size and set(gpos.tolist()) < set(npos.tolist())
