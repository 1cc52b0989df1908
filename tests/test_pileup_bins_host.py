"""Host side of the stage-1 window-file path: sitefile.PileupBinWriter against write_pileup_bin, and what pipeline.contig_to_bin /
make_pileup_bins refuse before they touch a file (the device side: tests/test_gpu_pileup_bins.py)."""
import os
import types

import numpy as np
import pytest

from nanosnp_amd import _lib, pipeline, sitefile
from tests import records_cases as rc


def _rows(n, seed, wide=False):
    """n sites: matrices, position strings (and their zero-padded rows), alt_info strings (some empty)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-144, 145, (n, 33, 18)).astype(np.int32)
    if wide and n:
        x[n // 2, 7, 3] = 40000
    pos = [f"chr{seed}:{int(p)}:{''.join(rng.choice(list('ACGTN'), 33))}" for p in rng.integers(1, 10 ** 9, n)]
    alts = ["" if i % 7 == 3 else f"{int(rng.integers(6, 99))}-XA {i + 1} IAT{'C' * int(rng.integers(0, 9))} 2" for i in range(n)]
    rowsb = np.zeros((n, sitefile.POSITION_WIDTH), np.uint8)
    for i, p in enumerate(pos):
        rowsb[i, :len(p)] = np.frombuffer(p.encode(), np.uint8)
    return x, pos, rowsb, alts


def _pieces(n, k, seed):
    """k uneven pieces of range(n), empty ones among them"""
    if k == 1:
        return [(0, n)]
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, k - 1))
    b = [0] + [int(c) for c in cuts] + [n]                           # (50 cuts among at most 158 values: some coincide, empty pieces)
    return list(zip(b[:-1], b[1:]))


def _feed(w, x, rowsb, alts, pieces, with_alt, base=0):
    for a, b in pieces:
        if with_alt:
            blob = "".join(alts[a:b]).encode()
            offs = np.zeros(b - a + 1, np.int64)
            np.cumsum([len(s) for s in alts[a:b]], out=offs[1:])
            # (a blob with bytes of other sites around it: only the offsets say what belongs to the piece)
            w.append(x[a:b], rowsb[a:b], np.frombuffer(b"#" * base + blob + b"##", np.uint8), offs + base)
        else:
            w.append(x[a:b], rowsb[a:b])


@pytest.mark.parametrize("n", [0, 1, 157])
@pytest.mark.parametrize("k", [1, 3, 50])
@pytest.mark.parametrize("dtype", ["int16", "int32"])
@pytest.mark.parametrize("with_alt", [True, False])
def test_writer_is_byte_identical_to_write_pileup_bin(tmp_path, n, k, dtype, with_alt):
    x, pos, rowsb, alts = _rows(n, 11 + n)
    want = tmp_path / "want.bin"
    sitefile.write_pileup_bin(want, x, pos, alts if with_alt else None, matrix_dtype=dtype)
    got = tmp_path / "got.bin"
    w = sitefile.PileupBinWriter(str(got), dtype, alt_info=with_alt)
    _feed(w, x, rowsb, alts, _pieces(n, k, 5 * n + k), with_alt, base=k % 3)
    assert not got.exists() and os.path.exists(str(got) + ".tmp")           # the data goes to path + ".tmp" until close()
    assert w.close() == n
    assert got.read_bytes() == want.read_bytes()
    assert not os.path.exists(str(got) + ".tmp")
    a = sitefile.read_arrays(got)
    assert list(a) == (["position_matrix", "position", "alt_info", "alt_info_offsets"] if with_alt else ["position_matrix", "position"])
    assert a["position_matrix"].dtype == np.dtype(dtype)
    if with_alt:
        assert sitefile.read_alt_info(got) == alts


def test_writer_takes_position_strings_and_int16_rows(tmp_path):
    x, pos, rowsb, alts = _rows(40, 3)
    sitefile.write_pileup_bin(tmp_path / "want.bin", x, pos, None)
    with sitefile.PileupBinWriter(str(tmp_path / "got.bin"), alt_info=False) as w:
        w.append(x[:13].astype(np.int16), pos[:13])
        w.append(x[13:], [p.encode() for p in pos[13:]])
    assert (tmp_path / "got.bin").read_bytes() == (tmp_path / "want.bin").read_bytes()


def test_int16_writer_restarts_as_int32(tmp_path):
    """a count outside int16 is refused by an int16 writer; restart('int32') starts the file over and the rows are appended again:
    the file write_pileup_bin writes from such rows (int32, its fallback)"""
    x, pos, rowsb, alts = _rows(90, 4, wide=True)
    want = tmp_path / "want.bin"
    sitefile.write_pileup_bin(want, x, pos, alts)
    assert sitefile.read_arrays(want)["position_matrix"].dtype == np.int32
    w = sitefile.PileupBinWriter(str(tmp_path / "got.bin"))
    pieces = _pieces(90, 3, 1)
    with pytest.raises(sitefile.SiteFileError, match="restart"):
        _feed(w, x, rowsb, alts, pieces, True)
    w.restart("int32")
    _feed(w, x, rowsb, alts, pieces, True)
    assert w.close() == 90
    assert (tmp_path / "got.bin").read_bytes() == want.read_bytes()


def test_abort_leaves_nothing(tmp_path):
    x, pos, rowsb, alts = _rows(20, 6)
    p = str(tmp_path / "a.bin")
    w = sitefile.PileupBinWriter(p)
    _feed(w, x, rowsb, alts, [(0, 20)], True)
    assert os.path.exists(p + ".tmp")
    w.abort()
    assert not os.path.exists(p) and not os.path.exists(p + ".tmp")
    w.abort()                                                            # (idempotent)
    with pytest.raises(sitefile.SiteFileError):
        w.append(x, rowsb, np.empty(0, np.uint8), np.zeros(21, np.int64))
    with pytest.raises(sitefile.SiteFileError):
        w.close()
    # an exception inside a with block aborts
    with pytest.raises(KeyError):
        with sitefile.PileupBinWriter(p) as w2:
            _feed(w2, x, rowsb, alts, [(0, 20)], True)
            raise KeyError("x")
    assert not os.path.exists(p) and not os.path.exists(p + ".tmp")


def test_writer_refuses_malformed_pieces(tmp_path):
    x, pos, rowsb, alts = _rows(5, 8)
    w = sitefile.PileupBinWriter(str(tmp_path / "a.bin"))
    with pytest.raises(sitefile.SiteFileError):
        w.append(x, rowsb)                                               # alt_info promised, none given
    with pytest.raises(sitefile.SiteFileError):
        w.append(x, rowsb[:4], np.empty(0, np.uint8), np.zeros(6, np.int64))
    with pytest.raises(sitefile.SiteFileError):
        w.append(x, rowsb, np.empty(3, np.uint8), np.array([0, 1, 2, 3, 4, 5], np.int64))      # offsets run past the blob
    with pytest.raises(sitefile.SiteFileError):
        w.append(x.astype(np.float32), rowsb, np.empty(0, np.uint8), np.zeros(6, np.int64))
    w.abort()
    with pytest.raises(sitefile.SiteFileError):
        sitefile.PileupBinWriter(str(tmp_path / "b.bin"), "int8")
    assert not os.path.exists(tmp_path / "b.bin.tmp")


def test_entry_points_and_constants_exist():
    assert callable(pipeline.contig_to_bin) and callable(pipeline.make_pileup_bins)
    assert "nsnp_pileup_window_records" in _lib.EXPORTS and "nsnp_pileup_alt_info" in _lib.EXPORTS
    assert _lib.Context.POSITION_WIDTH == sitefile.POSITION_WIDTH == 83
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nanosnp.h")).read()
    assert "#define NSNP_POSITION_WIDTH 83" in header


def test_refuse_without_a_device_before_creating_a_file(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU answers)
    model = types.SimpleNamespace(ctx=None)
    seq = np.frombuffer(b"ACGT" * 30, np.uint8)
    p = tmp_path / "c.pd.bin"
    with pytest.raises(_lib.NanoSNPError):
        pipeline.contig_to_bin(model, b"c\t1\tA\t3\t...\tIII\n", "c", seq, str(p))
    out = tmp_path / "out"
    with pytest.raises(_lib.NanoSNPError):
        pipeline.make_pileup_bins(model, [("c", str(tmp_path / "c.mpileup"))], str(tmp_path / "ref.fa"), "c\t120\t3\t60\t61\n", str(out))
    assert not p.exists() and not os.path.exists(str(p) + ".tmp") and not out.exists()


def test_refusals_of_process_groups_and_the_host_tokeniser(tmp_path, monkeypatch):
    import torch.distributed as tdist
    model = types.SimpleNamespace(ctx=None)
    seq = np.frombuffer(b"ACGT" * 30, np.uint8)
    p = tmp_path / "c.pd.bin"
    call = lambda: pipeline.contig_to_bin(model, b"c\t1\tA\t3\t...\tIII\n", "c", seq, str(p))
    call_many = lambda: pipeline.make_pileup_bins(model, [("c", "nowhere.mpileup")], "nowhere.fa", "c\t120\t3\t60\t61\n", str(tmp_path / "out"))
    monkeypatch.setenv("NSNP_TOKENISE", "host")
    for f in (call, call_many):
        with pytest.raises(NotImplementedError, match="NSNP_TOKENISE"):
            f()
    monkeypatch.delenv("NSNP_TOKENISE")
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    for f in (call, call_many):
        with pytest.raises(NotImplementedError, match="process group"):
            f()
    assert not p.exists() and not os.path.exists(str(p) + ".tmp") and not (tmp_path / "out").exists()


# ---- the builders of tests/records_cases.py: what each text must hold for its GPU test to mean anything (oracle only, no GPU) ---------


def _newline_free_tiles(text):
    a = np.frombuffer(text, np.uint8)
    pad = np.zeros(rc.n_tiles(a.size) * rc.NM_TILE, np.uint8)
    pad[:a.size] = a
    return np.flatnonzero((pad.reshape(-1, rc.NM_TILE) == 10).sum(1) == 0).tolist()


@pytest.mark.parametrize("newline", [True, False])
@pytest.mark.parametrize("rest", [1, 4095, 4096])
@pytest.mark.parametrize("tiles", [1025, 2049])
def test_line_names_texts_hold_what_they_are_built_for(tiles, rest, newline):
    text, name = rc.names_text(tiles, rest, newline)
    per = rc.scan_per(tiles)
    T = rc.NM_TILE
    assert len(text) == (tiles - 1) * T + rest and rc.n_tiles(len(text)) == tiles and per == {1025: 2, 2049: 3}[tiles]
    assert (tiles - 1) // per < 1023                                     # scan threads behind the last owner own nothing
    assert text.endswith(b"\n") == newline
    lines = rc.text_lines(text)
    toks, differ = rc.line_names_rule(text, name)
    assert len(lines) > 80_000 and min(len(l) for l in lines) >= 29 and sorted(len(l) for l in lines)[-3] <= 70
    assert 500 < len(differ) < 1300 and {len(toks[i]) for i in differ} == {1, 3, 4, 5, 15, 37, 40, 45}
    # tiles without a newline: inside the two long lines (the first tiles thread 300 owns, the last tile thread 41 owns and the next)
    empty = _newline_free_tiles(text)
    assert empty[:4] == [per * 41 + per - 1, per * 41 + per, per * 300, per * 300 + 1]
    assert empty[4:] == ([tiles - 1] if rest == 1 and not newline else [])
    starts = np.concatenate([[0], np.cumsum([len(l) + 1 for l in lines])[:-1]])
    tile_of = starts // T
    is_other = np.zeros(len(lines), bool)
    is_other[differ] = True
    marked = rc.names_marked_tiles(tiles)
    assert {0, tiles - 1, tiles - 2, per, 2 * per - 1, ((tiles - 1) // per) * per}.issubset(marked)
    held = 0
    for t in marked:                                                     # first and last line start of every marked tile that holds one
        here = np.flatnonzero(tile_of == t)
        if here.size:
            held += 1
            assert is_other[here[0]] and is_other[here[-1]], t
    assert held >= len(marked) - 3 and is_other[0] and is_other[-1]
    # the anchored lines: where they start, and that token / tabs reach over the tile edge
    by_start = {int(s): i for i, s in enumerate(starts)}
    for off, kind in rc.names_anchors(tiles).items():
        i = by_start[off]
        if kind == "long":
            assert len(lines[i]) == rc.LN_LONG - 1 and not is_other[i] and is_other[i - 1] and is_other[i + 1]
            continue
        assert is_other[i] == kind.endswith("_other"), (off, kind)
        edge = -(-off // T) * T
        if kind.startswith("tok"):
            assert off < edge < off + len(toks[i]) and not lines[i].startswith(b"\t")
        elif kind.startswith("tabs"):
            assert lines[i].startswith(b"\t\t\t\t") and off < edge < off + 4 and (off + 4) // T == off // T + 1
        else:
            assert off % T == 0


def test_site_names_case_alternates_the_contig_name_with_every_length():
    for n in (1, 2, 5, 64, 4097):
        centers, line_idx, names = rc.site_names_case(n, 5000)
        assert np.array_equal(np.diff(centers), np.ones(n - 1, np.int64)) and centers[0] == 16
        e = line_idx[centers + 16]
        lens = np.where(e < 0, 0, names[np.maximum(e, 0), 40:44].copy().view(np.int32)[:, 0])
        assert set(names[:, 40:44].copy().view(np.int32)[:, 0].tolist()) == {1, 2, 36, 37}
        if n >= 64:
            pairs = set(zip(lens[:-1].tolist(), lens[1:].tolist()))
            for l in (1, 2, 36, 37):
                assert (0, l) in pairs and (l, 0) in pairs                # beside the contig's name, on either side
            assert {(37, 1), (1, 36), (36, 2), (2, 37), (37, 2), (2, 1)}.issubset(pairs)    # and two entries of different lengths side by side
        # a row of 83 bytes: three of every four sites start inside a 4-byte word
        assert n < 4 or sum((83 * j) % 4 != 0 for j in range(n)) * 4 >= 3 * (n - n % 4)


@pytest.fixture(scope="module")
def alt_data(tmp_path_factory):
    return rc.alt_case_data(tmp_path_factory.mktemp("alt_host"))


def test_alt_info_cases_reach_the_scan_and_the_second_copy_sweep(alt_data):
    want, sp = alt_data["want"], alt_data["specials"]
    assert len(want) == 4827 and sum(len(v) for v in want.values()) == 131_811 < rc.COPY_SWEEP
    assert [rc.scan_per(n) for n in rc.ALT_SCAN_N] == [1, 1, 1, 2, 2, 3]
    for n in rc.ALT_SCAN_N:
        c = rc.alt_scan_centers(want, n)
        assert c.size == n and all(int(p) + 1 in want for p in c)
        assert n < 1024 or np.unique(c).size < n                         # repeats
    centers, total = rc.alt_sweep_centers(want, sp)
    assert total == sum(len(want[int(c) + 1]) for c in centers)
    assert total > rc.COPY_SWEEP + 16 and total % 16 != 0 and total < 2 * rc.COPY_SWEEP
    big = sp["500 distinct insertions"]
    assert int((centers + 1 == big).sum()) == 1100 and len(want[big]) > 3800
    assert all(int(centers[i]) + 1 == big and len(want[int(centers[i + 1]) + 1]) < 40 for i in range(0, 2200, 2))
    assert (centers.size, total) == (2200, 4_436_141)


@pytest.mark.parametrize("n_other", [600, 1500])
def test_big_chunk_text_is_one_chunk_above_4_mib(tmp_path, n_other):
    text0, seq = rc.synth_text(20261500, 70_000, "ctgE")
    text, which = rc.rename_lines(text0, n_other, 61)
    chunks, sizes = rc.chunk_lines(text, 64 << 20)
    assert len(chunks) == 1 and sizes[0] == len(text) > 4_194_304 and rc.n_tiles(len(text)) > 1024 and rc.scan_per(rc.n_tiles(len(text))) == 2
    toks, differ = rc.line_names_rule(text, b"ctgE")
    assert differ == which.tolist() and (len(differ) > 1024) == (n_other == 1500)
    assert all(1 <= len(toks[i]) <= 37 for i in differ)
    pd, n = rc.oracle_pd(tmp_path, text, seq)
    fields = rc.pd_fields(pd)
    renamed = [(nm, p) for nm, p, _ in fields if nm != b"ctgE"]
    assert n > 3000 and len(renamed) > (20 if n_other == 1500 else 5)
    # a site's name is column 0 of the line at centre + 16 - in another tile than the site's own line for some of them
    starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1])
    assert all(toks[p - 1 + 16] == nm for nm, p in renamed)
    assert sum(starts[p - 1] // 4096 != starts[p - 1 + 16] // 4096 for _, p in renamed) >= 1
    assert (len(text), rc.n_tiles(len(text)), n, len(renamed)) == {600: (5_905_709, 1442, 3693, 25), 1500: (5_918_489, 1445, 3693, 89)}[n_other]


def test_grown_text_has_three_chunks_two_of_them_above_4_mib(tmp_path):
    text0, seq = rc.synth_text(20261501, rc.GROWN_COLS, "ctgF")
    text, which = rc.rename_lines(text0, rc.GROWN_OTHER, 62)
    chunks, sizes = rc.chunk_lines(text, rc.GROWN_CHUNK)
    assert len(chunks) >= 3 and sum(s > 4_194_304 for s in sizes) >= 2
    per_chunk = [int(((which >= lo) & (which < hi)).sum()) for _, _, lo, hi in chunks]
    assert max(per_chunk) > 1024 and min(per_chunk) > 0                  # one chunk's table of 1,024 overflows
    assert len(text) == 15_709_390 and sizes == [1_250_042, 1_875_038, 2_812_500, 4_218_771, 5_553_039] and per_chunk == [270, 382, 536, 778, 1035]


def test_deep_column_leaves_int16_in_the_oracle(tmp_path):
    from nanosnp_amd import host
    from oracle import oracle
    contig, seq, text = rc.deep_text()
    chunks, sizes = rc.chunk_lines(text, rc.DEEP_CHUNK)
    assert len(chunks) >= 2
    pos, off, bases = host.mpileup_parse(text)
    counts, depth, flags = oracle.encode_columns(bases, off, seq[pos - 1])
    assert counts.min() == -(rc.DEEP_READS + 10) and counts.max() == rc.DEEP_READS and int(depth.max()) == rc.DEEP_READS + 10
    assert np.flatnonzero((counts < -32768).any(1) | (counts > 32767).any(1)).tolist() == [299]
    pd, n = rc.oracle_pd(tmp_path, text, seq)
    assert n == 1 and rc.pd_fields(pd)[0][1] == 300
    sitefile.pd_to_bin(pd, tmp_path / "w.bin")
    assert sitefile.read_arrays(tmp_path / "w.bin")["position_matrix"].dtype == np.int32


def test_three_causes_text_holds_all_three(tmp_path):
    contig, seq, text, renamed = rc.three_causes_text()
    chunks, sizes = rc.chunk_lines(text, 64 << 20)
    assert len(chunks) == 1
    toks, differ = rc.line_names_rule(text, contig.encode())
    assert differ == renamed and len(differ) > 1024
    pd, n = rc.oracle_pd(tmp_path, text, seq)
    fields = rc.pd_fields(pd)
    assert [p for _, p, _ in fields] == list(range(50, 250)) + [1000]
    assert sum(len(a) for _, _, a in fields) > 64 * rc.FIRST_ROWS + (1 << 16)        # more than a first slot's blob
    assert sum(nm != contig.encode() for nm, _, _ in fields) > 100
    sitefile.pd_to_bin(pd, tmp_path / "w.bin")
    assert sitefile.read_arrays(tmp_path / "w.bin")["position_matrix"].dtype == np.int32


def test_slot_growth_text_selects_few_sites_three_times_then_many(tmp_path):
    contig, seq, text = rc.slot_growth_text()
    pd, n = rc.oracle_pd(tmp_path, text, seq)
    per_chunk = rc.sites_per_chunk(pd, text, rc.SLOT_CHUNK)
    assert len(per_chunk) == 4 and sum(per_chunk) == n
    assert all(1 <= k < rc.FIRST_ROWS for k in per_chunk[:3]) and per_chunk[3] > rc.FIRST_ROWS + rc.FIRST_ROWS // 4
    from nanosnp_amd.pipeline import _cols_for
    assert _cols_for(rc.SLOT_CHUNK) // 64 < rc.FIRST_ROWS                # a first slot has 1,024 rows at this chunk size
    assert sum(len(a) for _, _, a in rc.pd_fields(pd)) < 64 * per_chunk[3]              # no blob restart: the rows alone outgrow the slot
    assert per_chunk == [4, 5, 176, 2737]
