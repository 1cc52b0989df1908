"""Host side of pipeline.mpileup_to_bins: the by-contig cut of a chunk's records, the staging-then-rename of its window files with a fake
producer in the device's place, and what the entry refuses before it touches anything (the device side: tests/test_gpu_mpileup_bins.py)."""
import os
import types

import numpy as np
import pytest

from nanosnp_amd import _lib, pipeline, sitefile

SHIFT = _lib.KEY_SHIFT


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-144, 145, (n, 33, 18)).astype(np.int16)
    position = np.zeros((n, sitefile.POSITION_WIDTH), np.uint8)
    position[:, :8] = rng.integers(65, 91, (n, 8))
    alts = [b"" if i % 5 == 2 else b"%d-XA %d" % (int(rng.integers(6, 99)), i + 1) for i in range(n)]
    return x, position, alts


def _blob(alts):
    offs = np.zeros(len(alts) + 1, np.int64)
    np.cumsum([len(a) for a in alts], out=offs[1:])
    return np.frombuffer(b"".join(alts) + b"#", np.uint8)[:-1], offs


# ---- the cut ------------------------------------------------------------------------------------------------------------------------------
def test_cut_records_by_contig():
    key = np.array([(4 << SHIFT) | 17, (4 << SHIFT) | 90, (0 << SHIFT) | 3, (2 << SHIFT) | 20, (2 << SHIFT) | 21, (2 << SHIFT) | 5000], np.int64)
    offs = np.array([100, 110, 110, 125, 125, 140, 141], np.int64)        # (any base offset; empty texts among them)
    got = pipeline.cut_records_by_contig(key, offs)
    assert [g[:5] for g in got] == [(4, 0, 2, 100, 110), (0, 2, 3, 110, 125), (2, 3, 6, 125, 141)]
    assert [g[5].tolist() for g in got] == [[0, 10, 10], [0, 15], [0, 0, 15, 16]]
    assert all(g[5].dtype == np.int64 for g in got)
    # without alt_info; one contig alone: it ends exactly at the chunk's last site; no site at all
    assert pipeline.cut_records_by_contig(key) == [(4, 0, 2, 0, 0, None), (0, 2, 3, 0, 0, None), (2, 3, 6, 0, 0, None)]
    one = pipeline.cut_records_by_contig(key[3:], offs[3:])
    assert len(one) == 1 and one[0][:5] == (2, 0, 3, 125, 141) and one[0][5].tolist() == [0, 0, 15, 16]
    assert pipeline.cut_records_by_contig(np.empty(0, np.int64), np.zeros(1, np.int64)) == []
    # a contig in two pieces, offsets that do not match the keys
    with pytest.raises(_lib.NanoSNPError, match="two separate pieces"):
        pipeline.cut_records_by_contig(np.array([(1 << SHIFT) | 5, (0 << SHIFT) | 9, (1 << SHIFT) | 7], np.int64))
    with pytest.raises(_lib.NanoSNPError):
        pipeline.cut_records_by_contig(key, offs[:-1])


def _chunks_of(names, per_contig, chunk_rows, seed=0):
    """sites of the contigs in text order, cut into chunks of chunk_rows sites each: [(site_key, x, position, blob, offsets)] and the rows
    of every contig"""
    rows, keys = {}, []
    for j, (cid, n) in enumerate(per_contig):
        rows[cid] = _rows(n, seed + j)
        keys += [(cid << SHIFT) | (100 + i) for i in range(n)]
    keys = np.array(keys, np.int64)
    x = np.concatenate([rows[c][0] for c, _ in per_contig]); position = np.concatenate([rows[c][1] for c, _ in per_contig])
    alts = sum((rows[c][2] for c, _ in per_contig), [])
    chunks = []
    for a in range(0, len(keys), chunk_rows):
        b = min(a + chunk_rows, len(keys))
        blob, offs = _blob(alts[a:b])
        chunks.append((keys[a:b], x[a:b], position[a:b], blob, offs))
    return chunks, rows


def _feed(staging, chunks, alt_info=True):
    for key, x, position, blob, offs in chunks:
        for cid, a, b, b_lo, b_hi, o in pipeline.cut_records_by_contig(key, offs if alt_info else None):
            staging.append(cid, x[a:b], position[a:b], blob[b_lo:b_hi] if alt_info else None, o)


def _want_file(tmp_path, rows, alt_info=True, dtype="int16"):
    x, position, alts = rows
    sitefile.write_pileup_bin(tmp_path / "want.bin", x, [bytes(r).rstrip(b"\0") for r in position], alts if alt_info else None, matrix_dtype=dtype)
    return (tmp_path / "want.bin").read_bytes()


# ---- staging, rename, clean-up -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alt_info", [True, False])
@pytest.mark.parametrize("chunk_rows", [1, 7, 10, 1000])
def test_staged_files_equal_write_pileup_bin(tmp_path, chunk_rows, alt_info):
    """a fake producer hands over chunks of sites of three contigs (table order other than text order; with 10 rows per chunk the first
    contig ends exactly at a chunk's last site); a fourth contig of the text holds no site and gets its empty file"""
    names = ["c0", "c1", "c2", "c3", "c4"]
    per_contig = [(3, 20), (0, 9), (4, 33)]
    chunks, rows = _chunks_of(names, per_contig, chunk_rows)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    (out_dir / "c0.pd.bin").write_bytes(b"old")
    seen = []

    def run_pass(staging, state):
        _feed(staging, chunks, alt_info)
        seen.append(sorted(os.listdir(out_dir)))
        return False, [3, 1, 0, 4]

    st = {}
    out = pipeline._staged_bins(str(out_dir), names, "int16", alt_info, run_pass, st)
    assert out == {"c3": 20, "c1": 0, "c0": 9, "c4": 33} and list(out) == ["c3", "c1", "c0", "c4"] and "restarts" not in st
    # while the text streamed, the final names were untouched and everything of the call bore a staging name
    assert "c0.pd.bin" in seen[0] and not {"c3.pd.bin", "c4.pd.bin"} & set(seen[0]) and len(seen[0]) >= 2
    assert sorted(os.listdir(out_dir)) == ["c0.pd.bin", "c1.pd.bin", "c3.pd.bin", "c4.pd.bin"]
    for cid in (3, 0, 4):
        assert (out_dir / f"c{cid}.pd.bin").read_bytes() == _want_file(tmp_path, rows[cid], alt_info), cid
    assert (out_dir / "c1.pd.bin").read_bytes() == _want_file(tmp_path, _rows(0, 0), alt_info)


def test_a_restart_drops_the_pass_and_every_file_is_int32(tmp_path):
    names = ["a", "b"]
    chunks, rows = _chunks_of(names, [(1, 12), (0, 5)], 4)
    passes = []

    def run_pass(staging, state):
        passes.append(dict(state))
        _feed(staging, chunks[:2] if len(passes) == 1 else chunks)
        if len(passes) == 1:
            state["elem"] = 4
            return True, None
        return False, [1, 0]

    st = {}
    out = pipeline._staged_bins(str(tmp_path / "new" / "out"), names, "int16", True, run_pass, st)
    assert out == {"b": 12, "a": 5} and st["restarts"] == 1 and [p["elem"] for p in passes] == [2, 4]
    assert sorted(os.listdir(tmp_path / "new" / "out")) == ["a.pd.bin", "b.pd.bin"]
    for cid, n in ((1, "b"), (0, "a")):
        assert sitefile.read_arrays(tmp_path / "new" / "out" / f"{n}.pd.bin")["position_matrix"].dtype == np.int32
        assert (tmp_path / "new" / "out" / f"{n}.pd.bin").read_bytes() == _want_file(tmp_path, rows[cid], dtype="int32")


@pytest.mark.parametrize("when", ["mid_contig", "between_contigs", "contig_twice", "at_commit"])
def test_an_error_leaves_the_directory_as_it_was(tmp_path, when):
    names = ["a", "b", "c"]
    chunks, rows = _chunks_of(names, [(2, 10), (0, 10), (1, 4)], 5)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    (out_dir / "a.pd.bin").write_bytes(b"what was here before")
    (out_dir / "other.txt").write_bytes(b"x")
    before = {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}

    def run_pass(staging, state):
        if when == "mid_contig":
            _feed(staging, chunks[:3])                                     # contig 2 complete, contig 0 half written
            assert sum(f.startswith(staging.tag) for f in os.listdir(staging.out_dir)) == 2      # (a finished staging file and a .tmp)
            raise ValueError("position outside the reference sequence")
        if when == "between_contigs":
            _feed(staging, chunks[:2])
            raise KeyboardInterrupt
        if when == "contig_twice":
            _feed(staging, chunks[:3] + chunks[:1])                        # (sites of a contig that was complete: refused by the staging)
        _feed(staging, chunks)
        return False, [2, 0]                                               # at_commit: sites of a contig the runs do not hold

    exc = {"mid_contig": ValueError, "between_contigs": KeyboardInterrupt}.get(when, _lib.NanoSNPError)
    with pytest.raises(exc):
        pipeline._staged_bins(str(out_dir), names, "int16", True, run_pass, {})
    assert {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)} == before
    # an out_dir the call made itself is gone again
    with pytest.raises(exc):
        pipeline._staged_bins(str(tmp_path / "made" / "here"), names, "int16", True, run_pass, {})
    assert not (tmp_path / "made" / "here").exists()


# ---- the entry ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_and_bindings_exist():
    assert callable(pipeline.mpileup_to_bins) and callable(pipeline.cut_records_by_contig)
    for name in ("pileup_window_records_keys", "pileup_alt_info_keys", "mpileup_line_names_contigs"):
        assert hasattr(_lib.Context, name), name
    for name in ("nsnp_pileup_window_records_keys", "nsnp_pileup_alt_info_keys", "nsnp_mpileup_line_names_contigs"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    import inspect
    sig = inspect.signature(pipeline._stream_text_dev)
    assert sig.parameters["records"].default is None and sig.parameters["indel_min_af"].default is None
    assert "extended_bed" not in inspect.signature(pipeline.mpileup_to_bins).parameters


def _call(tmp_path, **kw):
    model = types.SimpleNamespace(ctx=None)
    return pipeline.mpileup_to_bins(model, b"c\t1\tN\t1\tA\tI\n", str(tmp_path / "ref.fa"), "c\t120\t0\t60\t61\n", str(tmp_path / "out"), **kw)


def test_refuse_without_a_device_before_touching_the_directory(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # (what a machine without a GPU answers)
    with pytest.raises(_lib.NanoSNPError, match="no GPU"):
        _call(tmp_path)
    assert not (tmp_path / "out").exists()
    (tmp_path / "out").mkdir()
    (tmp_path / "out" / "c.pd.bin").write_bytes(b"old")
    with pytest.raises(_lib.NanoSNPError, match="no GPU"):
        _call(tmp_path, contigs=["c"])
    assert os.listdir(tmp_path / "out") == ["c.pd.bin"] and (tmp_path / "out" / "c.pd.bin").read_bytes() == b"old"


def test_refusals_of_process_groups_and_the_host_tokeniser(tmp_path, monkeypatch):
    import torch.distributed as tdist
    monkeypatch.setenv("NSNP_TOKENISE", "host")
    with pytest.raises(NotImplementedError, match="NSNP_TOKENISE"):
        _call(tmp_path)
    monkeypatch.delenv("NSNP_TOKENISE")
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="process group"):
        _call(tmp_path)
    assert not (tmp_path / "out").exists()
