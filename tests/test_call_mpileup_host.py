"""The host-side pieces of pipeline.call_mpileup that need no device, and the name rule of the reference's splitter
(DNA_ExtractChrPileupData) pinned by its own output: tests/golden/extract_chr.npz holds one small text and the files the reference's
program wrote for it (tests/golden/make_golden_extract_chr.py)."""
import os

import numpy as np
import pytest

from tests.contig_rules import FILLER, KEY_SHIFT, contig_rule, line_name, line_spans, split_by_contig
from tests.helpers import ROOT


def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "extract_chr.npz"))
    files = {str(n)[:-len(".mpileup")].encode(): bytes(g[f"file_{k}"]) for k, n in enumerate(g["files"])}
    return bytes(g["text"]), [str(w).encode() for w in g["wanted"]], files


def test_python_name_rule_equals_the_reference_splitter():
    text, wanted, files = _golden()
    assert len(files) == 5 and sum(map(len, files.values())) > 300
    assert split_by_contig(text, wanted) == files
    # the corner cases are in the text: a space in front of the tab, a leading tab, prefix names, an unlisted name, a name in two runs
    names = [line_name(text[s:e]) for s, e in line_spans(text)]
    assert b"" in names and b"chrUn_unlisted" in names and names.count(b"chrS") == 5
    assert {b"chr1", b"chr10", b"chr1_KI270706v1_random"} <= set(names)
    assert files[b"chr1"].count(b"\n") == 4                # the second run of chr1 replaced the first
    assert files[b"chrS"].count(b"\n") == 5 and b"chrS extra" in files[b"chrS"]


def test_run_table_of_the_rule_gives_the_splitters_files():
    """cid and the run table, as the device reports them, are enough to cut the text as the splitter does: the lines of the LAST run of
    every wanted name"""
    text, wanted, files = _golden()
    spans = line_spans(text)
    pos = [1] * len(spans)
    cid, ref, key, runs = contig_rule(text, wanted, [np.full(100, 65, np.uint8)] * len(wanted), pos)
    assert (key[cid < 0] == FILLER).all() and (key[cid >= 0] >> KEY_SHIFT == cid[cid >= 0]).all()
    last_run = {}
    for i, (first, c) in enumerate(runs.tolist()):
        end = int(runs[i + 1, 0]) if i + 1 < len(runs) else len(spans)
        if c >= 0:
            last_run[wanted[c]] = (first, end)
    for name, (a, b) in last_run.items():
        got = b"".join((text[s:e][:-1] if text[s:e].endswith(b"\r") and e < len(text) else text[s:e]) + b"\n" for s, e in spans[a:b])
        assert got == files[name]


def test_rows_are_cut_by_contig_from_the_keys():
    from nanosnp_amd._lib import NanoSNPError
    from nanosnp_amd.pipeline import cut_rows_by_contig
    k = lambda c, p: (c << KEY_SHIFT) | p
    keys = np.array([k(3, 5), k(3, 9), k(0, 1), k(7, (1 << KEY_SHIFT) - 1), k(7, 1)], np.int64)
    assert cut_rows_by_contig(keys) == [(3, 0, 2), (0, 2, 3), (7, 3, 5)]
    assert cut_rows_by_contig(np.zeros(0, np.int64)) == []
    assert cut_rows_by_contig(np.array([k((1 << 17) - 1, 2)], np.int64)) == [((1 << 17) - 1, 0, 1)]
    with pytest.raises(NanoSNPError, match="two separate pieces"):
        cut_rows_by_contig(np.array([k(1, 5), k(2, 1), k(1, 6)], np.int64))
    # every key is exact in the float64 the call rows carry it in
    big = np.array([k((1 << 17) - 1, (1 << KEY_SHIFT) - 1)], np.int64)
    assert int(big.astype(np.float64)[0]) == int(big[0])


def test_run_tables_of_chunks_detect_a_repeated_contig():
    from nanosnp_amd._lib import NanoSNPError
    from nanosnp_amd.pipeline import ContigRuns
    names = ["a", "b", "c"]
    r = ContigRuns(names)
    # chunk 0: lines [0, 100) own, 16 halo lines behind; a | unknown | b
    assert r.feed(np.array([[0, 0], [40, -1], [60, 1]]), 116, 0, 100) == [0, 1]
    # chunk 1: its first 16 lines are chunk 0's last; b goes on (a run that begins in the halo is not a new one), c starts among its own
    assert r.feed(np.array([[0, 1], [50, 2]]), 200, 16, 200) == [2]
    assert r.order == [0, 1, 2]
    # a run that starts in the halo BEHIND the own lines belongs to the next chunk
    r2 = ContigRuns(names)
    assert r2.feed(np.array([[0, 0], [105, 1]]), 116, 0, 100) == [0]
    assert r2.feed(np.array([[0, 0], [21, 1]]), 80, 16, 80) == [1]
    # A B A: refused, with B unknown too
    for mid in (1, -1):
        r3 = ContigRuns(names)
        with pytest.raises(NanoSNPError, match="two separate runs"):
            r3.feed(np.array([[0, 0], [10, mid], [20, 0]]), 30, 0, 30)
    # ... and across chunks
    r4 = ContigRuns(names)
    r4.feed(np.array([[0, 0], [10, 1]]), 46, 0, 30)
    with pytest.raises(NanoSNPError, match="a: the text holds this contig in two"):
        r4.feed(np.array([[0, 1], [20, 0]]), 60, 16, 60)
    # unknown names may come as often as they like
    r5 = ContigRuns(names)
    assert r5.feed(np.array([[0, -1], [5, 0], [9, -1], [12, -1]]), 20, 0, 20) == [0]


def test_key_limits():
    from nanosnp_amd import _lib
    assert (_lib.KEY_SHIFT, _lib.KEY_FILLER) == (KEY_SHIFT, FILLER)
    _lib.check_key_limits(1 << 17, (1 << 36) - 1)
    with pytest.raises(_lib.NanoSNPError):
        _lib.check_key_limits((1 << 17) + 1, 10)
    with pytest.raises(_lib.NanoSNPError):
        _lib.check_key_limits(3, 1 << 36)
    # the largest key is exact in a float64, and a step from a contig's last position to the next contig's first is never + 1
    top = (((1 << 17) - 1) << KEY_SHIFT) | ((1 << 36) - 1)
    assert top < 1 << 53 and int(float(top)) == top
    assert ((1 << KEY_SHIFT) | 1) - ((0 << KEY_SHIFT) | ((1 << 36) - 1)) != 1
    # (the C entry's own refusal of such a table needs a context: tests/test_gpu_tokenise_contigs.py)


def test_rows_handed_to_the_writer_are_whole_contigs_in_any_table_order():
    """pipeline.complete_rows: every row but the trailing rows of the LAST row's contig - whatever the table indices are (the order of
    contigs= need not be the order of the text)"""
    import torch
    from nanosnp_amd.pipeline import complete_rows, cut_rows_by_contig
    rng = np.random.default_rng(3)
    k = lambda c, n: ((c << KEY_SHIFT) | np.sort(rng.integers(1, 1 << 30, n))).astype(np.int64)
    for order, sizes in (((2, 0, 1, 3), (150, 100, 70, 30)), ((2, 0, 1, 3), (50, 100, 70, 30)), ((0, 1, 2, 3), (5, 5, 5, 5)), ((3, 2, 1, 0), (9, 1, 4, 2)),
                         (((1 << 17) - 1, 0), (3, 4))):
        keys = np.concatenate([k(c, n) for c, n in zip(order, sizes)])
        for dt in (torch.float64, torch.int64):
            assert complete_rows(torch.from_numpy(keys).to(dt)) == sum(sizes[:-1])
            for cut in range(1, len(keys) + 1):          # rows issued so far: the hand-over is always a whole number of contigs
                keep = complete_rows(torch.from_numpy(keys[:cut]).to(dt))
                done = [c for c, a, b in cut_rows_by_contig(keys[:keep])]
                assert keep in np.cumsum((0,) + sizes) and done == list(order[:len(done)]) and (keys[keep:cut] >> KEY_SHIFT == keys[cut - 1] >> KEY_SHIFT).all()
    assert complete_rows(torch.zeros(0, dtype=torch.float64)) == 0


def test_keys_of_the_highest_contig_indices_and_positions_on_the_host():
    """cut_rows_by_contig and complete_rows on the key column as float64 (what the call rows carry) and as int64 (what rows_unpack hands
    back): contig indices 0, 2^17 - 1 and 2^16 in that order - the table order is not the text order -, positions 1 and 2^36 - 1"""
    import torch
    from nanosnp_amd._lib import NanoSNPError
    from nanosnp_amd.pipeline import complete_rows, cut_rows_by_contig
    top_c, top_p = (1 << 17) - 1, (1 << KEY_SHIFT) - 1
    order = (0, top_c, 1 << 16)
    keys = np.array([(c << KEY_SHIFT) | p for c in order for p in (1, 77, top_p)], np.int64)
    assert keys.max() == (1 << 53) - 1 and np.array_equal(keys.astype(np.float64).astype(np.int64), keys)     # the test's own premise
    want = [(c, 3 * i, 3 * i + 3) for i, c in enumerate(order)]
    for col in (keys, keys.astype(np.float64)):
        assert cut_rows_by_contig(col) == want
        t = torch.from_numpy(col)
        assert complete_rows(t) == 6
        for cut in range(1, 10):                           # rows issued so far -> whole contigs handed over
            assert complete_rows(t[:cut]) == 3 * ((cut - 1) // 3)
            assert cut_rows_by_contig(col[:cut]) == [(c, a, min(b, cut)) for c, a, b in want if a < cut]
        # a contig's last position and the next contig's first differ by one in the contig index alone: they are cut apart
        assert cut_rows_by_contig(col[2:4]) == [(0, 0, 1), (top_c, 1, 2)] and complete_rows(t[2:4]) == 1
    two = np.array([(top_c << KEY_SHIFT) | top_p, ((1 << 16) << KEY_SHIFT) | 1, (top_c << KEY_SHIFT) | 1], np.int64)
    for col in (two, two.astype(np.float64)):
        with pytest.raises(NanoSNPError, match="two separate pieces"):
            cut_rows_by_contig(col)


def test_fai_names():
    from nanosnp_amd.pipeline import fai_names
    assert fai_names("chr1\t100\t6\t60\t61\nchr2\t50\t120\t60\t61\n") == ["chr1", "chr2"]


def test_entry_points_refuse_without_a_device(tmp_path):
    import torch
    from nanosnp_amd import _lib
    from nanosnp_amd.pipeline import call_mpileup
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert hasattr(_lib.Context, "mpileup_tokenise_contigs") and hasattr(_lib.Context, "mpileup_tokenise_contigs_into")
    with pytest.raises(_lib.NanoSNPError):
        _lib.Context(0)
    with pytest.raises(_lib.NanoSNPError):
        _lib.ContigTable({"a": np.frombuffer(b"ACGT", np.uint8)})
    with pytest.raises(_lib.NanoSNPError):
        call_mpileup(None, b"a\t1\tN\t1\tA\tI\n", str(tmp_path / "x.fa"), "a\t4\t3\t60\t61\n", str(tmp_path / "o.vcf"))
    assert not (tmp_path / "o.vcf").exists()
    with pytest.raises(NotImplementedError):
        call_mpileup(None, b"", "x.fa", "a\t4\t3\t60\t61\n", str(tmp_path / "o.vcf"), extended_bed={"a": np.zeros((0, 2), np.int64)})
