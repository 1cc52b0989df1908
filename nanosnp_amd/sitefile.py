"""Flat binary containers that stand in for the reference's PyTables/HDF5 ``.bin`` files.

The reference moves sites between stages as HDF5 EArrays:

* ``<chr>.pd.bin``  (``dna_sv_tensor/src/make_bin_data/make_bin_predict_data.py:48-100``): ``position_matrix int32 [N,33,18]``,
  ``position S83 [N,1]`` (``"ctg:pos:ref33"``), ``alt_info S5000 [N,1]``; read by ``PileupModel/dataset.py:118-139``.
* ``haplotype_bins/<ctg>_<s>_<e>.bin`` (``HaplotypeModel/write_to_bins.py:4-64``): eight ``int32 [N,D,L]`` read planes and two
  string arrays; read by ``HaplotypeModel/dataset_dev.py:95-105,135-147``.

PyTables is not part of this stack and a compressed chunked store is the wrong shape for a device pipeline anyway, so the same
arrays (same names, same dtypes, same row order) are kept in one uncompressed file whose arrays start on 64-byte boundaries:
``numpy.memmap`` views go to the GPU with one copy, no parse.  Strings are fixed-width byte rows exactly like the HDF5 atoms
(``alt_info`` is a ragged blob + offsets instead of 5000 bytes per site).

Layout: ``b"NSNPBIN1"``, ``u32 n_arrays``, ``u32 0``; per array a 96-byte record ``name[32] dtype[8] ndim(u32) pad(u32)
shape[4](u64) offset(u64) nbytes(u64)``; then the data.
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"NSNPBIN1"
_REC = struct.Struct("<32s8sII4QQQ")
POSITION_WIDTH = 33 + 50          # make_bin_predict_data.py:94  StringAtom(itemsize = no_of_positions + 50)


class SiteFileError(ValueError):
    pass


def write_arrays(path, arrays: dict):
    """Writes named numpy arrays (<= 4 dimensions) into one flat file."""
    items = []
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.ndim > 4 or len(name.encode()) > 32:
            raise SiteFileError(f"array {name!r}: at most 4 dimensions and 32-byte names")
        items.append((name, a))
    off = len(MAGIC) + 8 + _REC.size * len(items)
    recs = []
    for name, a in items:
        off = (off + 63) & ~63
        shape = list(a.shape) + [0] * (4 - a.ndim)
        recs.append(_REC.pack(name.encode(), a.dtype.str.encode(), a.ndim, 0, *shape, off, a.nbytes))
        off += a.nbytes
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", len(items), 0))
        for r in recs:
            f.write(r)
        for (name, a), r in zip(items, recs):
            o = _REC.unpack(r)[8]
            f.write(b"\0" * (o - f.tell()))
            f.write(a.tobytes())


def create_arrays(path, specs: dict) -> dict:
    """Lays out a site file for arrays that are filled piece by piece (the reference appends to its EArrays chunk by chunk:
    write_to_bins.py:53-63): specs = {name: (dtype, shape)}; returns {name: writable numpy.memmap}.  Flush / delete the maps to finish."""
    items = []
    for name, (dt, shape) in specs.items():
        dt = np.dtype(dt)
        if len(shape) > 4 or len(name.encode()) > 32:
            raise SiteFileError(f"array {name!r}: at most 4 dimensions and 32-byte names")
        items.append((name, dt, tuple(int(v) for v in shape)))
    off = len(MAGIC) + 8 + _REC.size * len(items)
    recs, offs = [], []
    for name, dt, shape in items:
        off = (off + 63) & ~63
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        recs.append(_REC.pack(name.encode(), dt.str.encode(), len(shape), 0, *(list(shape) + [0] * (4 - len(shape))), off, nbytes))
        offs.append(off)
        off += nbytes
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", len(items), 0))
        for r in recs:
            f.write(r)
        f.truncate(max(off, f.tell()))
    return {name: (np.memmap(path, dtype=dt, mode="r+", offset=o, shape=shape) if int(np.prod(shape, dtype=np.int64)) else np.empty(shape, dt))
            for (name, dt, shape), o in zip(items, offs)}


def array_index(path) -> dict:
    """{name: (dtype, shape, byte offset, nbytes)} of a site file, without touching the data (the streamed stage-5 reader preads the
    planes straight into pinned buffers: nanosnp_amd/pipeline.py)."""
    with open(path, "rb") as f:
        head = f.read(len(MAGIC) + 8)
        if len(head) < len(MAGIC) + 8 or head[:8] != MAGIC:
            raise SiteFileError(f"{path}: not an NSNPBIN1 file")
        n, = struct.unpack_from("<I", head, 8)
        recs = [_REC.unpack(f.read(_REC.size)) for _ in range(n)]
    out = {}
    for name, dt, ndim, _, s0, s1, s2, s3, off, nbytes in recs:
        shape = (s0, s1, s2, s3)[:ndim]
        dtype = np.dtype(dt.rstrip(b"\0").decode())
        if int(np.prod(shape, dtype=np.int64)) * dtype.itemsize != nbytes:
            raise SiteFileError(f"{path}: array {name!r} has inconsistent size")
        out[name.rstrip(b"\0").decode()] = (dtype, tuple(int(v) for v in shape), int(off), int(nbytes))
    return out


def read_arrays(path, mmap=True) -> dict:
    """Returns {name: array}; with ``mmap`` the arrays are read-only views of the file."""
    with open(path, "rb") as f:
        head = f.read(len(MAGIC) + 8)
        if len(head) < len(MAGIC) + 8 or head[:8] != MAGIC:
            raise SiteFileError(f"{path}: not an NSNPBIN1 file")
        n, = struct.unpack_from("<I", head, 8)
        recs = [_REC.unpack(f.read(_REC.size)) for _ in range(n)]
    out = {}
    for name, dt, ndim, _, s0, s1, s2, s3, off, nbytes in recs:
        shape = (s0, s1, s2, s3)[:ndim]
        dtype = np.dtype(dt.rstrip(b"\0").decode())
        if int(np.prod(shape, dtype=np.int64)) * dtype.itemsize != nbytes:
            raise SiteFileError(f"{path}: array {name!r} has inconsistent size")
        key = name.rstrip(b"\0").decode()
        if nbytes == 0:
            out[key] = np.empty(shape, dtype)
        elif mmap:
            out[key] = np.memmap(path, dtype=dtype, mode="r", offset=off, shape=shape)
        else:
            out[key] = np.fromfile(path, dtype=dtype, count=int(np.prod(shape)), offset=off).reshape(shape)
    return out


# ---- <chr>.pd.bin ------------------------------------------------------------------------------------------------
def write_pileup_bin(path, position_matrix, position, alt_info=None, matrix_dtype="int16"):
    """position_matrix integer [N,33,18]; position: N strings ``ctg:pos:ref33``; alt_info: N strings or None.
    Row order is the caller's (the reference appends in input order: make_bin_predict_data.py:59-77).
    matrix_dtype "int16" (default): the counts are stored as int16 when every one of them fits (a count is at most the read depth, and
    the column encoder caps the depth at 144 reads: they always do), else as int32, the reference's Int32Atom (make_bin_predict_data.py:
    92) - half the file, half the page-cache bytes the streamed predict loop stages and no narrowing on the way; "int32" keeps int32."""
    x = np.ascontiguousarray(position_matrix)
    if x.dtype.kind not in "iu":
        raise SiteFileError("position_matrix must hold integers")
    if matrix_dtype not in ("int16", "int32"):
        raise SiteFileError("matrix_dtype: 'int16' or 'int32'")
    n = x.shape[0]
    if x.shape[1:] != (33, 18) or len(position) != n:
        raise SiteFileError("position_matrix must be [N,33,18] with one position string per row")
    fits16 = x.dtype.itemsize <= 2 and x.dtype != np.uint16 or (x.size == 0 or (int(x.min()) >= -32768 and int(x.max()) <= 32767))
    x = np.ascontiguousarray(x, dtype=np.int16 if (matrix_dtype == "int16" and fits16) else np.int32)
    pos = np.zeros((n, POSITION_WIDTH), np.uint8)
    for i, p in enumerate(position):
        b = p.encode() if isinstance(p, str) else bytes(p)
        if len(b) > POSITION_WIDTH:
            raise SiteFileError(f"position string longer than {POSITION_WIDTH} bytes: {b[:40]!r}...")
        pos[i, :len(b)] = np.frombuffer(b, np.uint8)
    arrays = {"position_matrix": x, "position": pos}
    if alt_info is not None:
        blobs = [a.encode() if isinstance(a, str) else bytes(a) for a in alt_info]
        if len(blobs) != n:
            raise SiteFileError("alt_info needs one entry per site")
        offs = np.zeros(n + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=offs[1:])
        arrays["alt_info"] = np.frombuffer(b"".join(blobs), np.uint8) if offs[-1] else np.empty(0, np.uint8)
        arrays["alt_info_offsets"] = offs
    write_arrays(path, arrays)


class PileupBinWriter:
    """A <chr>.pd.bin written piece by piece, for a producer that does not know the site count in advance (pipeline.contig_to_bin appends
    every chunk's sites as they come back from the device).  close() leaves a file byte-identical to write_pileup_bin of the same rows in
    one call: same arrays in the same order, same dtypes, 64-byte alignment and header.

    position_matrix is the first array, so its offset follows from the NUMBER of arrays alone: its rows stream into their final place and
    are never held whole in memory.  The small arrays (83 bytes of position string and the alt_info text per site) are held back and
    written behind the matrix at close(), the header last.  Everything goes to path + ".tmp", renamed into place by close(); abort()
    leaves neither file.  matrix_dtype "int16" takes rows of any integer type whose values fit (SiteFileError otherwise: restart("int32")
    starts the file over, and the producer appends its rows again)."""

    def __init__(self, path, matrix_dtype="int16", alt_info=True):
        if matrix_dtype not in ("int16", "int32"):
            raise SiteFileError("matrix_dtype: 'int16' or 'int32'")
        self.path, self.tmp = path, path + ".tmp"
        self.alt_info = bool(alt_info)
        self._f = None
        self._start(matrix_dtype)

    def _start(self, matrix_dtype):
        import os
        self.matrix_dtype = np.dtype(matrix_dtype)
        self.n = 0
        self._positions, self._blobs, self._lens = [], [], []
        n_arrays = 4 if self.alt_info else 2
        self._x_off = (len(MAGIC) + 8 + _REC.size * n_arrays + 63) & ~63
        if self._f is None:
            self._f = open(self.tmp, "wb")
        self._f.seek(0)
        self._f.truncate(0)
        self._f.seek(self._x_off)

    def restart(self, matrix_dtype="int32"):
        """drops everything appended so far and starts the file over with another matrix type"""
        if matrix_dtype not in ("int16", "int32"):
            raise SiteFileError("matrix_dtype: 'int16' or 'int32'")
        if self._f is None:
            raise SiteFileError("restart() of a writer that was closed or aborted")
        self._start(matrix_dtype)

    def append(self, position_matrix_rows, position_rows, alt_blob=None, alt_offsets=None):
        """position_matrix_rows: integer [n,33,18]; position_rows: uint8 [n, POSITION_WIDTH] (zero-padded) or n strings; alt_blob uint8 +
        alt_offsets int64 [n + 1]: text i of this piece is alt_blob[alt_offsets[i]:alt_offsets[i + 1]] (any base offset)."""
        if self._f is None:
            raise SiteFileError("append() to a writer that was closed or aborted")
        x = np.asarray(position_matrix_rows)
        n = x.shape[0]
        if x.dtype.kind not in "iu" or x.shape[1:] != (33, 18):
            raise SiteFileError("position_matrix rows must be integers [n,33,18]")
        if isinstance(position_rows, np.ndarray) and position_rows.dtype == np.uint8:
            pos = position_rows
            if pos.shape != (n, POSITION_WIDTH):
                raise SiteFileError(f"position rows must be uint8 [n,{POSITION_WIDTH}] with one row per site")
        else:
            if len(position_rows) != n:
                raise SiteFileError("one position string per row")
            pos = np.zeros((n, POSITION_WIDTH), np.uint8)
            for i, p in enumerate(position_rows):
                b = p.encode() if isinstance(p, str) else bytes(p)
                if len(b) > POSITION_WIDTH:
                    raise SiteFileError(f"position string longer than {POSITION_WIDTH} bytes: {b[:40]!r}...")
                pos[i, :len(b)] = np.frombuffer(b, np.uint8)
        if self.alt_info:
            if alt_blob is None or alt_offsets is None:
                raise SiteFileError("this writer holds alt_info: every piece needs alt_blob and alt_offsets")
            offs = np.asarray(alt_offsets, np.int64)
            if offs.shape != (n + 1,) or (n and (np.diff(offs) < 0).any()) or (n and int(offs[-1]) > len(alt_blob)) or int(offs[0]) < 0:
                raise SiteFileError("alt_offsets must be n + 1 ascending offsets into alt_blob")
        if n == 0:
            return
        if x.dtype != self.matrix_dtype:
            if self.matrix_dtype == np.int16 and (x.dtype.itemsize > 2 or x.dtype == np.uint16) and (int(x.min()) < -32768 or int(x.max()) > 32767):
                raise SiteFileError("a count outside int16: restart('int32') and append the rows again")
            x = x.astype(self.matrix_dtype)
        self._f.write(memoryview(np.ascontiguousarray(x)).cast("B"))
        self._positions.append(np.array(pos, np.uint8, copy=True))
        if self.alt_info:
            self._blobs.append(np.array(np.asarray(alt_blob, np.uint8)[int(offs[0]):int(offs[-1])], copy=True))
            self._lens.append(np.diff(offs))
        self.n += n

    def close(self):
        """writes the held-back arrays and the header, renames the file into place -> the number of sites"""
        import os
        if self._f is None:
            raise SiteFileError("close() of a writer that was closed or aborted")
        f, n = self._f, self.n
        small = [("position", np.concatenate(self._positions) if self._positions else np.zeros((0, POSITION_WIDTH), np.uint8))]
        if self.alt_info:
            offs = np.zeros(n + 1, np.int64)
            if self._lens:
                np.cumsum(np.concatenate(self._lens), out=offs[1:])
            small.append(("alt_info", np.concatenate(self._blobs) if self._blobs else np.empty(0, np.uint8)))
            small.append(("alt_info_offsets", offs))
        recs = [_REC.pack(b"position_matrix", self.matrix_dtype.str.encode(), 3, 0, n, 33, 18, 0, self._x_off, n * 594 * self.matrix_dtype.itemsize)]
        try:
            off = self._x_off + n * 594 * self.matrix_dtype.itemsize
            if f.tell() != off:
                raise SiteFileError("internal: matrix bytes written do not match the site count")
            for name, a in small:
                o = (off + 63) & ~63
                f.write(b"\0" * (o - off))
                f.write(a.tobytes())
                recs.append(_REC.pack(name.encode(), a.dtype.str.encode(), a.ndim, 0, *(list(a.shape) + [0] * (4 - a.ndim)), o, a.nbytes))
                off = o + a.nbytes
            f.truncate(off)                                # (empty arrays at the end still count their padding, as write_arrays writes it)
            f.seek(0)
            f.write(MAGIC + struct.pack("<II", len(recs), 0))
            for r in recs:
                f.write(r)
            f.close()
            self._f = None
            os.replace(self.tmp, self.path)
        except BaseException:
            self.abort()
            raise
        return n

    def abort(self):
        """drops the file being written: path + '.tmp' is removed and path was never created (idempotent)"""
        import os
        if self._f is not None:
            try:
                self._f.close()
            finally:
                self._f = None
        try:
            os.remove(self.tmp)
        except FileNotFoundError:
            pass

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            self.abort()
        elif self._f is not None:
            self.close()
        return False


def read_pileup_bin(path, mmap=True):
    """-> (contig_names list[str], positions int64[N], reference_bases uint8[N], position_matrix int32[N,33,18]):
    what ``PileupModel/dataset.py:118-139`` extracts (``reference_bases = ord(seq[16])``)."""
    a = read_arrays(path, mmap)
    if "position_matrix" not in a or "position" not in a:
        raise SiteFileError(f"{path}: not a pileup site file")
    names, pos, refb = [], [], []
    for row in np.asarray(a["position"]):
        s = bytes(row).rstrip(b"\0").decode().strip()
        try:
            ctg, p, seq = s.split(":")
            names.append(ctg); pos.append(int(p)); refb.append(ord(seq[16]))
        except (ValueError, IndexError) as e:
            raise SiteFileError(f"{path}: bad position string {s!r}") from e
    x = a["position_matrix"]
    return names, np.asarray(pos, np.int64), np.asarray(refb, np.uint8), (x if x.dtype == np.int32 else np.asarray(x, np.int32))


def read_alt_info(path):
    a = read_arrays(path, mmap=False)
    if "alt_info" not in a:
        return None
    blob, offs = a["alt_info"].tobytes(), a["alt_info_offsets"]
    return [blob[offs[i]:offs[i + 1]].decode() for i in range(len(offs) - 1)]


def pd_to_bin(pd_text: bytes, path, matrix_dtype="int16"):
    """``.pd`` text -> site file: ``transform_one_input`` of make_bin_predict_data.py:48-77 (594 ints, position string,
    alt_info per line).  Lines whose tensor field does not hold 594 integers are rejected, as ``np.array(...).reshape`` would."""
    xs, positions, alts = [], [], []
    for ln, line in enumerate(pd_text.split(b"\n")):
        if not line.strip():
            continue
        fields = line.split(b"\t")
        if len(fields) < 3:
            raise SiteFileError(f".pd line {ln + 1}: expected tensor, position and alt_info fields")
        vals = np.array(fields[0].split(), dtype=np.int64)
        if vals.size != 33 * 18:
            raise SiteFileError(f".pd line {ln + 1}: {vals.size} tensor values, expected 594")
        xs.append(vals.astype(np.int32).reshape(33, 18))
        positions.append(fields[1].strip())
        alts.append(fields[2].strip())
    x = np.stack(xs) if xs else np.empty((0, 33, 18), np.int32)
    write_pileup_bin(path, x, positions, alts, matrix_dtype=matrix_dtype)
    return len(xs)


# ---- <chr>.td.bin ------------------------------------------------------------------------------------------------
LABEL_WIDTH = 90                  # make_bin_train_data.py: label_size = 21 + 3 + 33 + 33 (common/genotype.cpp:264-274)


def _label_rows(label, n):
    y = np.asarray(label)
    if y.dtype.kind not in "iu" or y.shape != (n, LABEL_WIDTH):
        raise SiteFileError(f"label must hold integers [N,{LABEL_WIDTH}] with one row per site")
    return np.ascontiguousarray(y, dtype=np.int32)


def write_train_bin(path, position_matrix, position, label, alt_info=None, matrix_dtype="int16"):
    """The training file the reference's make_bin_train_data.py:101-105 leaves behind, under its array names: position_matrix, position and
    alt_info exactly as write_pileup_bin stores them, and label int32 [N,90] (the reference's Int32Atom) behind position."""
    import os
    tmp = f"{path}.pd.tmp"
    write_pileup_bin(tmp, position_matrix, position, alt_info, matrix_dtype=matrix_dtype)
    try:
        a = read_arrays(tmp, mmap=False)
    finally:
        os.remove(tmp)
    arrays = {"position_matrix": a["position_matrix"], "position": a["position"], "label": _label_rows(label, a["position"].shape[0])}
    arrays.update({k: a[k] for k in ("alt_info", "alt_info_offsets") if k in a})
    write_arrays(path, arrays)


class TrainBinWriter(PileupBinWriter):
    """A <chr>.td.bin written piece by piece (pipeline.mpileup_to_train_bins): PileupBinWriter with one more array, label int32 [N,90], held
    back with the other small arrays and written behind `position`.  close() leaves a file byte-identical to write_train_bin of the same
    rows in one call."""

    def _start(self, matrix_dtype):
        super()._start(matrix_dtype)
        self._labels = []
        n_arrays = 5 if self.alt_info else 3
        self._x_off = (len(MAGIC) + 8 + _REC.size * n_arrays + 63) & ~63
        self._f.seek(self._x_off)

    def append(self, position_matrix_rows, position_rows, label_rows, alt_blob=None, alt_offsets=None):
        """as PileupBinWriter.append, with label_rows: integer [n,90]"""
        y = _label_rows(label_rows, np.asarray(position_matrix_rows).shape[0])
        before = self.n
        super().append(position_matrix_rows, position_rows, alt_blob, alt_offsets)
        if self.n != before:
            self._labels.append(np.array(y, np.int32, copy=True))

    def close(self):
        import os
        if self._f is None:
            raise SiteFileError("close() of a writer that was closed or aborted")
        f, n = self._f, self.n
        # (name, dtype, shape, the pieces held back: written one after another, never joined - the labels are 360 bytes a site)
        small = [("position", np.dtype(np.uint8), (n, POSITION_WIDTH), self._positions), ("label", np.dtype(np.int32), (n, LABEL_WIDTH), self._labels)]
        if self.alt_info:
            offs = np.zeros(n + 1, np.int64)
            if self._lens:
                np.cumsum(np.concatenate(self._lens), out=offs[1:])
            small.append(("alt_info", np.dtype(np.uint8), (int(offs[-1]),), self._blobs))
            small.append(("alt_info_offsets", offs.dtype, offs.shape, [offs]))
        recs = [_REC.pack(b"position_matrix", self.matrix_dtype.str.encode(), 3, 0, n, 33, 18, 0, self._x_off, n * 594 * self.matrix_dtype.itemsize)]
        try:
            off = self._x_off + n * 594 * self.matrix_dtype.itemsize
            if f.tell() != off:
                raise SiteFileError("internal: matrix bytes written do not match the site count")
            for name, dt, shape, pieces in small:
                o = (off + 63) & ~63
                f.write(b"\0" * (o - off))
                nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
                for piece in pieces:
                    f.write(memoryview(np.ascontiguousarray(piece, dt)).cast("B"))
                if f.tell() != o + nbytes:
                    raise SiteFileError(f"internal: {name} bytes written do not match the site count")
                recs.append(_REC.pack(name.encode(), dt.str.encode(), len(shape), 0, *(list(shape) + [0] * (4 - len(shape))), o, nbytes))
                off = o + nbytes
            f.truncate(off)                                # (empty arrays at the end still count their padding, as write_arrays writes it)
            f.seek(0)
            f.write(MAGIC + struct.pack("<II", len(recs), 0))
            for r in recs:
                f.write(r)
            f.close()
            self._f = None
            os.replace(self.tmp, self.path)
        except BaseException:
            self.abort()
            raise
        return n


def read_train_bin(path, mmap=True):
    """-> (contig_names, positions int64 [N], reference_bases uint8 [N], position_matrix int32 [N,33,18], label int32 [N,90]): read_pileup_bin
    plus the labels"""
    a = read_arrays(path, mmap)
    if "label" not in a or tuple(a["label"].shape[1:]) != (LABEL_WIDTH,):
        raise SiteFileError(f"{path}: not a training site file")
    return (*read_pileup_bin(path, mmap), a["label"])


def td_to_bin(td_text: bytes, path, matrix_dtype="int16"):
    """``.td`` text (DNA_CreateTrainData, make_train_data/main.cpp:369-382) -> training site file: ``transform_one_input`` of
    make_bin_train_data.py:61-81 - columns 0-3 of a line are the 594 ints, the 90 label ints, the position string and alt_info; a fifth
    (the truth row the reference appends to a variant's line) is ignored, as there."""
    xs, ys, positions, alts = [], [], [], []
    for ln, line in enumerate(td_text.split(b"\n")):
        line = line.strip()
        if not line:
            continue
        fields = line.split(b"\t")
        if len(fields) < 4:
            raise SiteFileError(f".td line {ln + 1}: expected tensor, label, position and alt_info fields")
        vals, lab = np.array(fields[0].split(), dtype=np.int64), np.array(fields[1].split(), dtype=np.int64)
        if vals.size != 33 * 18 or lab.size != LABEL_WIDTH:
            raise SiteFileError(f".td line {ln + 1}: {vals.size} tensor and {lab.size} label values, expected 594 and {LABEL_WIDTH}")
        xs.append(vals.astype(np.int32).reshape(33, 18))
        ys.append(lab.astype(np.int32))
        positions.append(fields[2].strip())
        alts.append(fields[3].strip())
    x = np.stack(xs) if xs else np.empty((0, 33, 18), np.int32)
    y = np.stack(ys) if ys else np.empty((0, LABEL_WIDTH), np.int32)
    write_train_bin(path, x, positions, y, alts, matrix_dtype=matrix_dtype)
    return len(xs)


# ---- haplotype bins ---------------------------------------------------------------------------------------------------
HAP_PLANES = ("haplotype_sequences", "haplotype_hap", "haplotype_baseq", "haplotype_mapq",
              "pileup_sequences", "pileup_hap", "pileup_baseq", "pileup_mapq")


def _haplotype_arrays(candidate_positions, haplotype_positions, planes, max_haplotype_depth, max_pileup_depth, plane_dtype):
    """-> (the arrays of a haplotype bin in file order, the stable position order they were permuted by)"""
    cand = [c if isinstance(c, str) else bytes(c).decode() for c in candidate_positions]
    n = len(cand)
    order = np.argsort(np.array([int(c.split(":")[1]) for c in cand], np.int64), kind="stable") if n else np.empty(0, np.int64)
    if plane_dtype not in ("int8", "int32"):
        raise SiteFileError("plane_dtype must be 'int8' or 'int32'")
    arrays = {}
    for name in HAP_PLANES:
        a = np.asarray(planes[name])
        if a.ndim != 3 or a.shape[0] != n or a.dtype.kind != "i":
            raise SiteFileError(f"{name}: expected an integer array [N,D,L] with N = {n}")
        cut = max_haplotype_depth if name.startswith("haplotype") else max_pileup_depth
        if cut is not None and cut < a.shape[1]:
            a = a[:, :cut]
        arrays[name] = a[order]
    fits = all(a.size == 0 or (int(a.min()) >= -128 and int(a.max()) <= 127) for a in arrays.values())
    dt = np.int8 if (plane_dtype == "int8" and fits) else np.int32
    arrays = {k: np.ascontiguousarray(a, dtype=dt) for k, a in arrays.items()}
    width_c = max([len(c) for c in cand] + [1])
    cp = np.zeros((n, width_c), np.uint8)
    for i, j in enumerate(order):
        b = cand[j].encode(); cp[i, :len(b)] = np.frombuffer(b, np.uint8)
    arrays["candidate_positions"] = cp
    hp = [[p if isinstance(p, str) else bytes(p).decode() for p in row] for row in haplotype_positions]
    width_h = max([len(p) for row in hp for p in row] + [1])
    L = len(hp[0]) if hp else 0
    hpa = np.zeros((n, L, width_h), np.uint8)
    for i, j in enumerate(order):
        for k, p in enumerate(hp[j]):
            b = p.encode(); hpa[i, k, :len(b)] = np.frombuffer(b, np.uint8)
    arrays["haplotype_positions"] = hpa
    return arrays, order


def write_haplotype_bin(path, candidate_positions, haplotype_positions, planes: dict, max_haplotype_depth=None,
                        max_pileup_depth=None, plane_dtype="int8"):
    """planes: the eight padded integer arrays of write_to_bins.py (``haplotype_*`` [N,Dh,11], ``pileup_*`` [N,Dp,33], padding
    -2).  Sites are sorted by the integer position of ``ctg:pos`` (write_to_bins.py:5-8; stable here) and depth is cut to
    ``max_*_depth`` (:39-42,54-61).
    plane_dtype: "int8" (default) stores the read planes as int8 when EVERY value of all eight fits (base codes -2..4, HP -2..3, base
    qualities <= 93, mapping qualities <= 60 from minimap2: they do; a plane holding e.g. mapq 255 makes the whole file int32) - a
    quarter of the file, of the bytes over PCIe and of the feature kernel's HBM reads, same features bit for bit
    (nsnp_hap_features_i8); "int32" writes the reference's dtype (write_to_bins.py:44-47).  Readers accept both."""
    arrays, _ = _haplotype_arrays(candidate_positions, haplotype_positions, planes, max_haplotype_depth, max_pileup_depth, plane_dtype)
    write_arrays(path, arrays)


def read_haplotype_bin(path, mmap=True):
    """-> (candidate_positions list[str], haplotype_positions list[list[str]], planes dict) as dataset_dev.py:95-105,135-147 reads them."""
    a = read_arrays(path, mmap)
    missing = [k for k in HAP_PLANES + ("candidate_positions", "haplotype_positions") if k not in a]
    if missing:
        raise SiteFileError(f"{path}: not a haplotype bin (missing {missing})")
    dec = lambda row: bytes(row).rstrip(b"\0").decode()
    cand = [dec(r) for r in np.asarray(a["candidate_positions"])]
    hpos = [[dec(p) for p in row] for row in np.asarray(a["haplotype_positions"])]
    return cand, hpos, {k: a[k] for k in HAP_PLANES}


# ---- labelled haplotype bins (HaplotypeModel/make_train_bins.py) -------------------------------------------------------
HAP_LABEL_WIDTH = 3               # make_train_bins.py:123-127,246,258: candidate_labels = {confident, gt21, zygosity} per site


def _hap_label_rows(candidate_labels, n):
    """any integer or float array [N,3] (the reference's is float64, cast by the PyTables Int32Atom) -> int32 [N,3]; a value that is not an
    integer or lies outside int32 is refused instead of truncated"""
    y = np.asarray(candidate_labels)
    if y.dtype.kind not in "iuf" or y.shape != (n, HAP_LABEL_WIDTH):
        raise SiteFileError(f"candidate_labels must hold numbers [N,{HAP_LABEL_WIDTH}] with one row per site")
    if y.dtype.kind == "f":
        if not np.all(np.isfinite(y)) or np.any(y != np.floor(y)):
            raise SiteFileError("candidate_labels holds a value that is not an integer")
    if y.size and (y.min() < np.iinfo(np.int32).min or y.max() > np.iinfo(np.int32).max):
        raise SiteFileError("candidate_labels holds a value outside int32")
    return np.ascontiguousarray(y.astype(np.int32))


def write_haplotype_train_bin(path, candidate_positions, haplotype_positions, planes: dict, candidate_labels, max_haplotype_depth=None,
                              max_pileup_depth=None, plane_dtype="int8"):
    """write_haplotype_bin's arrays plus ``candidate_labels`` int32 [N,3] = {confident, gt21, zygosity} (make_train_bins.py:123-127,246,258),
    permuted by the same stable position order as every other array.  The file stays a valid input of read_haplotype_bin, HapBinSource and
    predict_haplotype_bins, which ignore the extra array."""
    arrays, order = _haplotype_arrays(candidate_positions, haplotype_positions, planes, max_haplotype_depth, max_pileup_depth, plane_dtype)
    arrays["candidate_labels"] = _hap_label_rows(candidate_labels, len(order))[order]
    write_arrays(path, arrays)


def read_haplotype_train_bin(path, mmap=True):
    """-> (candidate_positions, haplotype_positions, planes, candidate_labels int32 [N,3]): read_haplotype_bin plus the labels"""
    a = read_arrays(path, mmap)
    y = a.get("candidate_labels")
    if y is None or y.dtype != np.dtype(np.int32) or y.ndim != 2 or y.shape[1] != HAP_LABEL_WIDTH:
        raise SiteFileError(f"{path}: not a labelled haplotype bin (no candidate_labels int32 [N,{HAP_LABEL_WIDTH}])")
    return (*read_haplotype_bin(path, mmap), y)
