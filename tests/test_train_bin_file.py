"""sitefile.TrainBinWriter / write_train_bin / read_train_bin / td_to_bin: the <chr>.td.bin container (make_bin_train_data.py:101-105's
arrays under the same names).  No GPU."""
import gzip
import os

import numpy as np
import pytest

from nanosnp_amd import sitefile
from tests import label_rules as lr
from tests.helpers import golden


@pytest.fixture(scope="module")
def td():
    return gzip.open(golden("train_g1.td.gz")).read()


def _rows(td):
    x, y, pos, alt = [], [], [], []
    for line in td.split(b"\n"):
        if line.strip():
            f = line.split(b"\t")
            x.append(np.array(f[0].split(), np.int32).reshape(33, 18)); y.append(np.array(f[1].split(), np.int32)); pos.append(f[2]); alt.append(f[3])
    return np.stack(x), np.stack(y), pos, alt


@pytest.mark.parametrize("alt_info", [True, False])
@pytest.mark.parametrize("dtype", ["int16", "int32"])
def test_piecewise_equals_one_call(tmp_path, td, alt_info, dtype):
    x, y, pos, alt = _rows(td)
    n = len(pos)
    want, got = str(tmp_path / "want.bin"), str(tmp_path / "got.bin")
    sitefile.write_train_bin(want, x, pos, y, alt if alt_info else None, matrix_dtype=dtype)
    posb = np.zeros((n, sitefile.POSITION_WIDTH), np.uint8)
    for i, p in enumerate(pos):
        posb[i, :len(p)] = np.frombuffer(p, np.uint8)
    blob = np.frombuffer(b"".join(alt), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(a) for a in alt])]).astype(np.int64)
    w = sitefile.TrainBinWriter(got, "int16", alt_info)
    if dtype == "int32":
        w.append(x[:5], posb[:5], y[:5], *((blob, offs[:6]) if alt_info else ()))
        w.restart("int32")                                   # everything appended so far is dropped, labels included
    for a, b in ((0, 1), (1, 1), (1, 64), (64, n)):          # an empty piece among them
        w.append(x[a:b], posb[a:b] if a else pos[a:b], y[a:b], *((blob, offs[a:b + 1]) if alt_info else ()))
    assert w.close() == n and not os.path.exists(got + ".tmp")
    assert open(got, "rb").read() == open(want, "rb").read()
    a = sitefile.read_arrays(got)
    assert list(a) == ["position_matrix", "position", "label"] + (["alt_info", "alt_info_offsets"] if alt_info else [])
    assert a["label"].dtype == np.int32 and a["label"].shape == (n, 90) and a["position_matrix"].dtype == np.dtype(dtype)
    assert all(off % 64 == 0 for _, _, off, _ in sitefile.array_index(got).values())


def test_td_to_bin_round_trip_and_the_ignored_fifth_column(tmp_path, td):
    x, y, pos, alt = _rows(td)
    path = str(tmp_path / "a.td.bin")
    assert sitefile.td_to_bin(td, path) == len(pos)
    names, p, refb, xm, label = sitefile.read_train_bin(path)
    assert np.array_equal(xm, x) and np.array_equal(label, y) and sitefile.read_alt_info(path) == [a.decode() for a in alt]
    assert names == [q.split(b":")[0].decode() for q in pos] and p.tolist() == [int(q.split(b":")[1]) for q in pos]
    assert np.array_equal(label, lr.parse_td(td.decode())[1]) and label.sum() == 4 * len(pos)
    # the reference appends the truth row to a variant's line: the bytes of the file do not depend on it
    lines = [b"\t".join(line.split(b"\t")[:4]) for line in td.split(b"\n")]
    assert any(len(line.split(b"\t")) > 4 for line in td.split(b"\n"))
    sitefile.td_to_bin(b"\n".join(lines), str(tmp_path / "b.td.bin"))
    assert open(path, "rb").read() == open(tmp_path / "b.td.bin", "rb").read()
    # the same rows through the .pd container: everything but the label is what write_pileup_bin stores
    sitefile.write_pileup_bin(str(tmp_path / "c.pd.bin"), x, pos, alt)
    a, c = sitefile.read_arrays(path), sitefile.read_arrays(str(tmp_path / "c.pd.bin"))
    assert all(np.array_equal(a[k], c[k]) and a[k].dtype == c[k].dtype for k in c)


def test_an_empty_file_and_the_refusals(tmp_path, td):
    path = str(tmp_path / "e.td.bin")
    assert sitefile.td_to_bin(b"", path) == 0
    assert sitefile.TrainBinWriter(str(tmp_path / "f.td.bin")).close() == 0
    assert open(path, "rb").read() == open(tmp_path / "f.td.bin", "rb").read()
    assert sitefile.read_train_bin(path)[4].shape == (0, 90)
    x, y, pos, alt = _rows(td)
    with pytest.raises(sitefile.SiteFileError, match="label"):
        sitefile.write_train_bin(path, x[:2], pos[:2], y[:3], alt[:2])
    with pytest.raises(sitefile.SiteFileError, match="label"):
        sitefile.write_train_bin(path, x[:2], pos[:2], y[:2, :89], alt[:2])
    w = sitefile.TrainBinWriter(str(tmp_path / "g.td.bin"), alt_info=False)
    with pytest.raises(sitefile.SiteFileError, match="label"):
        w.append(x[:2], pos[:2], y[:2].astype(np.float32))
    w.abort()
    assert not os.path.exists(tmp_path / "g.td.bin") and not os.path.exists(str(tmp_path / "g.td.bin") + ".tmp")
    with pytest.raises(sitefile.SiteFileError, match="expected tensor, label"):
        sitefile.td_to_bin(b"1 2 3\tx\ty\n", path)
    with pytest.raises(sitefile.SiteFileError, match="label values"):
        sitefile.td_to_bin(b" ".join([b"0"] * 594) + b"\t1 0\tc:1:A\tx\n", path)
    sitefile.write_pileup_bin(path, x[:2], pos[:2], alt[:2])
    with pytest.raises(sitefile.SiteFileError, match="training"):
        sitefile.read_train_bin(path)
