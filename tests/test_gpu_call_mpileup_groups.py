"""pipeline.call_mpileup_groups: the file call_mpileup_bed writes, byte for byte, and beside it the stage-4 site groups selected from the
call rows on the device - equal to merge.select_groups on that file.  The thresholds are checked beforehand with the CPU oracle's calls on
the same text: they must leave the yardstick something to find."""
import numpy as np
import pytest

from nanosnp_amd import host, merge
from tests import contig_rules as cr
from tests import group_rules as gr

pytestmark = pytest.mark.gpu

SIZES = (3000, 40, 2500, 3500)
QUALITY, ADJACENT, SUPPORT = 19.0, 5, 14.0


def _oracle_vcf(name, text, seq, weights):
    """the rows the CPU oracle calls on one contig's text, as the writer formats them"""
    from oracle import oracle
    pos, off, bases = host.mpileup_parse(text)
    counts, _, flags = oracle.encode_columns(bases, off, seq[pos - 1])
    centers = oracle.select_sites(pos, flags)
    if not len(centers):
        return ""
    x = oracle.gather_windows(counts, centers)
    gt, zy = oracle.pileup_forward(weights, x, nthreads=8)
    cov = x[:, 16, [0, 1, 2, 3, 9, 10, 11, 12]].astype(np.float32)
    p = pos[centers]
    text, _ = host.vcf_format_batches(host.ContigTable([name]), np.zeros(p.size, np.int32), p, seq[p - 1] & 0xDF, gt.argmax(1).astype(np.uint8),
                                      zy.argmax(1).astype(np.uint8), gt.max(1), zy.max(1), cov)
    return text.decode()


@pytest.fixture(scope="module")
def genome(tmp_path_factory, pileup_weights):
    from nanosnp_amd.pileup_model import LSTMNetwork
    d = tmp_path_factory.mktemp("groups_genome")
    texts, seqs, fasta, fai = {}, {}, b"", ""
    for i, n in enumerate(SIZES):
        name = f"ctg{i}"
        cols = host.synth_columns(20264120 + i, n, coverage=30, het_rate=0.05)
        texts[name], seqs[name] = bytes(cols.mpileup_text_native(name)), cols.ref.copy()
        fasta += b">" + name.encode() + b"\n" + b"\n".join(bytes(seqs[name][a:a + 60]) for a in range(0, n, 60)) + b"\n"
        fai += f"{name}\t{n}\t0\t60\t61\n"
    (d / "ref.fa").write_bytes(fasta)
    whole = b"".join(texts.values())
    assert cr.split_by_contig(whole, [n.encode() for n in texts]) == {n.encode(): t for n, t in texts.items()}
    # the thresholds, judged on the CPU oracle's calls: at least ten groups over at least two contigs
    oracle_groups = merge.select_groups("".join(_oracle_vcf(n, texts[n], seqs[n], pileup_weights) for n in texts), QUALITY, ADJACENT, SUPPORT,
                                        reference_bug=False)
    assert gr.n_groups(oracle_groups) >= 10 and sum(bool(v) for v in oracle_groups.values()) >= 2
    return dict(dir=d, whole=whole, names=list(texts), fasta=str(d / "ref.fa"), fai=fai, model=LSTMNetwork().load_weight_list(pileup_weights))


@pytest.mark.parametrize("chunk_bytes", [1 << 30, 60_000])
def test_the_file_of_call_mpileup_bed_and_the_groups_of_select_groups(genome, chunk_bytes):
    from nanosnp_amd.pipeline import call_mpileup_bed, call_mpileup_groups
    d = genome["dir"]
    args = (genome["model"], genome["whole"], genome["fasta"], genome["fai"])
    st = {}
    want_rows = call_mpileup_bed(*args, str(d / "want.vcf"), contigs=genome["names"], chunk_bytes=chunk_bytes, stats=st)
    assert st["chunks"] == 1 if chunk_bytes > len(genome["whole"]) else st["chunks"] > 5
    rows, groups = call_mpileup_groups(*args, str(d / "got.vcf"), contigs=genome["names"], chunk_bytes=chunk_bytes, quality_threshold=QUALITY,
                                       adjacent_size=ADJACENT, support_quality=SUPPORT)
    vcf = (d / "got.vcf").read_bytes()
    assert rows == want_rows > 300 and vcf == (d / "want.vcf").read_bytes()
    want = merge.select_groups(vcf.decode(), QUALITY, ADJACENT, SUPPORT, reference_bug=False)
    assert gr.n_groups(want) >= 10 and sum(bool(v) for v in want.values()) >= 2
    lists = groups.to_lists()
    assert lists == want and list(lists) == list(want)
    # `rows` count the call rows of the whole run in text order: strictly ascending inside a group, below the sites called
    idx = groups.rows.cpu().numpy()
    assert len(groups) == gr.n_groups(want) and (np.diff(idx, axis=1) > 0).all() and 0 <= idx.min() and idx.max() < st["sites"]
    # the reference's storing bug over the whole list of contigs, not per hand-over
    for nthreads in (1, 2):
        _, bugged = call_mpileup_groups(*args, str(d / "bug.vcf"), contigs=genome["names"], chunk_bytes=chunk_bytes, reference_bug=True, nthreads=nthreads)
        assert bugged.to_lists() == merge.select_groups(vcf.decode(), QUALITY, ADJACENT, SUPPORT, nthreads=nthreads, reference_bug=True)


def test_a_text_without_sites_has_no_groups(genome):
    from nanosnp_amd.pipeline import call_mpileup_groups
    rows, groups = call_mpileup_groups(genome["model"], b"", genome["fasta"], genome["fai"], str(genome["dir"] / "none.vcf"))
    assert rows == 0 and len(groups) == 0 and groups.to_lists() == {} and groups.rows.shape == (0, 11)
