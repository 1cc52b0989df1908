"""Host side of the stage-1 window-file path: sitefile.PileupBinWriter against write_pileup_bin, and what pipeline.contig_to_bin /
make_pileup_bins refuse before they touch a file (the device side: tests/test_gpu_pileup_bins.py)."""
import os
import types

import numpy as np
import pytest

from nanosnp_amd import _lib, pipeline, sitefile


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
