"""BED region filters over a whole-genome text, without a GPU: the bitmap table's layout (bed.table_bitmaps), the reference anchor - the
numpy rules over ONE text of two fixture contigs give exactly the union of the .pd files the reference's programs wrote per contig -, and
the refusals of the two new entry points."""
import numpy as np
import pytest

from nanosnp_amd import _lib, bed, host
from nanosnp_amd._lib import NanoSNPError
from tests import bed_key_rules as bk
from tests import bed_rules
from tests import contig_rules as cr

NAMES = ["a", "zero", "b", "c33", "tiny"]
LENGTHS = [1000, 500, 77, 33, 1]
IV = {"a": [[0, 10], [5, 40], [990, 1000]], "b": [[76, 77], [0, 1]], "c33": [[31, 33]], "tiny": [[0, 1]], "elsewhere": [[0, 10 ** 9]]}


def test_table_layout_word_offsets_and_zero_word_contigs():
    words, off = bed.table_bitmaps(IV, NAMES, LENGTHS)
    assert words.dtype == np.uint32 and off.dtype == np.int64
    # a contig the BED does not mention takes zero words; the others (length + 31) // 32, back to back from 0
    assert off.tolist() == [0, 32, 32, 35, 37, 38] and words.size == 38
    for c, (name, n) in enumerate(zip(NAMES, LENGTHS)):
        w = words[off[c]:off[c + 1]]
        want = bed_rules.bit_array(IV.get(name, []), n)
        assert np.array_equal(bk.words_bits(words, off, LENGTHS)[c], want), name
        if w.size:
            assert np.array_equal(w, bed.bed_bitmap(IV[name], n))
            assert np.array_equal(bed_rules.bits_from_words(w, n), want)
            assert sum(bin(int(x)).count("1") for x in w) == int(want.sum())          # no bit beyond the contig (33 and 77 are no multiples of 32)
    # names outside `names` are ignored, whatever their intervals; an empty interval list is a contig without words
    assert bed.table_bitmaps({"elsewhere": [[5, 2]], "zero": np.zeros((0, 2), np.int64)}, NAMES, LENGTHS)[1].tolist() == [0] * 6
    assert bed.table_bitmaps({}, [], [])[0].size == 0 and bed.table_bitmaps({}, [], [])[1].tolist() == [0]
    # the order of `names` is the order of the table, not the BED's
    w2, o2 = bed.table_bitmaps(IV, NAMES[::-1], LENGTHS[::-1])
    assert o2.tolist() == [0, 1, 3, 6, 6, 38] and np.array_equal(w2[6:], words[:32])
    for bad in ({"a": [[5, 5]]}, {"a": [[-1, 3]]}, {"b": [[0, 78]]}, {"tiny": [[0, 2]]}):
        with pytest.raises(NanoSNPError):
            bed.table_bitmaps(bad, NAMES, LENGTHS)
    with pytest.raises(NanoSNPError):
        bed.table_bitmaps(IV, NAMES, LENGTHS[:-1])


def test_table_from_a_path_is_checked_against_the_whole_index(tmp_path):
    fai = "".join(f"{n}\t{l}\t0\t60\t61\n" for n, l in zip(NAMES + ["other"], LENGTHS + [50]))
    p = tmp_path / "t.bed"
    p.write_bytes(b"# c\nb\t76\t77\na\t0\t10\nother\t0\t50\na\t5\t40\nb\t0\t1\r\na\t990\t1000\nc33\t31\t33\ntiny\t0\t1\n")
    words, off = bed.table_bitmaps(str(p), NAMES, LENGTHS, fai)
    w0, o0 = bed.table_bitmaps(IV, NAMES, LENGTHS)
    assert np.array_equal(words, w0) and np.array_equal(off, o0)
    # `other` is in the index but not wanted: ignored; only part of the names wanted
    w1, o1 = bed.table_bitmaps(str(p), ["b"], [77], fai)
    assert o1.tolist() == [0, 3] and np.array_equal(w1, words[32:35])
    # without an index: checked against the wanted contigs alone, other lines passed over
    assert np.array_equal(bed.table_bitmaps(p, NAMES, LENGTHS)[0], w0)
    # the load_bed errors: an interval beyond its contig, a contig the index lacks, from >= to, too few fields - as the reference asserts
    for line in (b"other\t0\t51\n", b"nowhere\t0\t5\n", b"a\t7\t7\n", b"a\t7\n", b"tiny\t0\t2\n"):
        q = tmp_path / "bad.bed"
        q.write_bytes(p.read_bytes() + line)
        with pytest.raises(NanoSNPError):
            bed.table_bitmaps(str(q), NAMES, LENGTHS, fai)


def test_key_rules_bound_every_test_by_the_keys_own_contig():
    """the restatement the GPU tests lean on: filler and unknown contigs read 0, a reach past the end of a contig is clipped there"""
    bits = bk.contig_bits([[[95, 100]], None, [[0, 4]]], [100, 50, 40])
    k = lambda c, p: (c << bk.KEY_SHIFT) | p
    key = np.array([k(0, 96), k(0, 95), k(0, 100), k(0, 101), k(1, 1), k(2, 1), k(2, 5), k(3, 1), bk.FILLER, k(0, 0)], np.int64)
    assert bk.keep_keys(key, bits).tolist() == [True, False, True, False, False, True, False, False, False, False]
    md = np.zeros(key.size, np.int64)
    assert bk.confident_keys(key, md, bits).tolist() == [True, True, True, False, False, True, False, False, False, False]
    # a deletion of 60 at the last position of contig 1 (no bits) reaches over contig 2's first bits in a single list: not here
    assert not bk.confident_keys(np.array([k(1, 50)]), [60], bits).any()
    assert bk.key_cid_pos(np.array([bk.FILLER]))[0][0] < 0


@pytest.mark.parametrize("case", ["ext", "conf", "both"])
def test_reference_anchor_in_one_text(case):
    """chrS text + lines of an unlisted name + chrC text, the two BED files of the case concatenated: contig_rule + the per-contig rules give
    exactly the union of the two .pd fixtures - sites and windows - and the splitter gives back the two fixture texts"""
    a = bk.anchor(case)
    split = cr.split_by_contig(a["whole"], [n.encode() for n in a["names"]])
    assert {k.decode(): v for k, v in split.items()} == a["texts"]
    assert a["whole"].count(bk.UNLISTED) == 40 and a["whole"].index(bk.UNLISTED) == len(a["texts"]["chrS"])
    fai = {n: int(s.size) for n, s in a["seqs"].items()}
    sites, x = bk.numpy_sites(a["whole"], a["names"], a["seqs"], a["ext"], a["conf"], fai)
    assert sites == a["want"] and len(sites) > 0
    gx = np.concatenate([host.pd_parse(a["pds"][n])[0] for n in a["names"]])
    assert np.array_equal(x, gx)
    assert {c for c, _ in sites} == {"chrS", "chrC"}                    # (both contigs keep sites: neither half is vacuous)
    # the table order may differ from the text order
    sites_r, _ = bk.numpy_sites(a["whole"], a["names"][::-1], a["seqs"], a["ext"], a["conf"], fai)
    assert sites_r == a["want"]
    # every case filters something: without the BEDs the text gives more sites
    plain, _ = bk.numpy_sites(a["whole"], a["names"], a["seqs"], None, None)
    assert len(plain) > len(sites) and set(sites) < set(plain)


def test_bindings_and_entry_points_exist():
    import inspect
    from nanosnp_amd import pipeline
    for name in ("nsnp_pileup_filter_columns_keys", "nsnp_pileup_encode_columns_keys"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    assert hasattr(_lib.Context, "pileup_filter_columns_keys") and hasattr(_lib.Context, "pileup_encode_columns_keys") and hasattr(_lib, "BedTable")
    assert inspect.signature(pipeline._stream_text_dev).parameters["beds"].default is None
    for fn in (pipeline.call_mpileup_bed, pipeline.mpileup_to_bins_bed):
        p = inspect.signature(fn).parameters
        assert p["extended_bed"].default is None and p["confident_bed"].default is None
        assert p["extended_bed"].kind is inspect.Parameter.KEYWORD_ONLY


def _calls(tmp_path):
    import types
    from nanosnp_amd import pipeline
    model = types.SimpleNamespace(ctx=None)                                # (every refusal comes before the model is touched)
    text, fai = b"c\t1\tN\t1\tA\tI\n", "c\t120\t0\t60\t61\n"
    b = {"c": [[0, 5]]}
    return (lambda: pipeline.call_mpileup_bed(model, text, str(tmp_path / "ref.fa"), fai, str(tmp_path / "o.vcf"), extended_bed=b),
            lambda: pipeline.mpileup_to_bins_bed(model, text, str(tmp_path / "ref.fa"), fai, str(tmp_path / "out"), confident_bed=b))


def test_refusals_of_process_groups_and_the_host_tokeniser(tmp_path, monkeypatch):
    import torch.distributed as tdist
    monkeypatch.setenv("NSNP_TOKENISE", "host")
    for call in _calls(tmp_path):
        with pytest.raises(NotImplementedError, match="NSNP_TOKENISE"):
            call()
    monkeypatch.delenv("NSNP_TOKENISE")
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    for call in _calls(tmp_path):
        with pytest.raises(NotImplementedError):
            call()
    assert not (tmp_path / "out").exists() and not (tmp_path / "o.vcf").exists()


def test_refuse_without_a_device_before_touching_anything(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU answers)
    for call in _calls(tmp_path):
        with pytest.raises(NanoSNPError, match="no GPU"):
            call()
    assert not (tmp_path / "out").exists() and not (tmp_path / "o.vcf").exists()
