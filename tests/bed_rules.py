"""The two BED rules of DNA_CreateCanSnpTensor restated in numpy (test helper; make_candidate_snp_tensor/main.cpp:158-217,
common/bed_intv_list.cpp), on top of the oracle's per-column results:

    extended BED   a line at 1-based position p exists only when bit p - 1 is set; the kept lines are then an unfiltered text
    confident BED  a column is a candidate only when, besides the usual test, a bit of [p - 1, p + max_del_length + 1) is set

One bitmap per contig: bits outside [0, contig length) read as 0.  max_del_length comes from orc_make_tensor through ctypes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

NCH = 18


class _OrcColumn(C.Structure):
    _fields_ = [("counts", C.c_int32 * NCH), ("depth", C.c_int32), ("max_del_length", C.c_int32), ("af", C.c_double),
                ("pass_af", C.c_uint8), ("pass_snp_af", C.c_uint8), ("pass_indel_af", C.c_uint8)]


def max_del_lengths(bases, col_off, ref):
    """orc_column_t.max_del_length of every column (oracle/pileup_encode_oracle.c orc_make_tensor)"""
    from oracle import oracle
    lib = oracle.lib()
    fn = lib.orc_make_tensor
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_char_p, C.c_int64, C.c_char, C.c_char_p, C.c_int64, C.c_double, C.c_double, C.POINTER(_OrcColumn), C.c_char_p, C.c_size_t]
    raw = np.ascontiguousarray(bases, np.uint8).tobytes()
    out = np.zeros(len(ref), np.int32)
    col = _OrcColumn()
    off = np.asarray(col_off, np.int64)
    for c in range(len(ref)):
        fn(raw[off[c]:off[c + 1]], int(off[c + 1] - off[c]), bytes([int(ref[c])]), None, 0, 0.12, 0.12, C.byref(col), None, 0)
        out[c] = col.max_del_length
    return out


def bit_array(intervals, chr_len):
    """plain loop: one bool per base of the contig"""
    b = np.zeros(int(chr_len), bool)
    for lo, hi in np.asarray(intervals, np.int64).reshape(-1, 2):
        b[int(lo):int(hi)] = True
    return b


def bits_from_words(words, chr_len):
    w = np.asarray(words, np.uint32)
    i = np.arange(int(chr_len))
    return ((w[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def extended_keep(pos, ext_bits):
    """which lines exist: bit pos - 1 set (outside the contig: 0)"""
    i = np.asarray(pos, np.int64) - 1
    ok = (i >= 0) & (i < ext_bits.size)
    keep = np.zeros(i.size, bool)
    keep[ok] = ext_bits[i[ok]]
    return keep


def confident_pass(pos, max_del, conf_bits):
    """any bit of the 0-based range [pos - 1, pos + max_del + 1) set"""
    cs = np.concatenate([[0], np.cumsum(conf_bits.astype(np.int64))])
    n = conf_bits.size
    lo = np.clip(np.asarray(pos, np.int64) - 1, 0, n)
    hi = np.clip(np.asarray(pos, np.int64) + np.asarray(max_del, np.int64) + 1, 0, n)
    return cs[np.maximum(hi, lo)] - cs[lo] > 0


def reference_sites(pos, col_off, bases, seq, ext_bits=None, conf_bits=None, min_af=0.12, min_coverage=6):
    """-> (positions of the emitted sites, their windows int32 [n, 33, 18], their depths): the whole rule on one contig's parsed text"""
    from oracle import oracle
    pos = np.asarray(pos, np.int64)
    col_off = np.asarray(col_off, np.int64)
    bases = np.asarray(bases, np.uint8)
    if ext_bits is not None:
        keep = extended_keep(pos, ext_bits)
        lens = (col_off[1:] - col_off[:-1])[keep]
        bases = np.concatenate([bases[col_off[c]:col_off[c + 1]] for c in np.nonzero(keep)[0]]) if keep.any() else np.zeros(0, np.uint8)
        pos = pos[keep]
        col_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ref = np.asarray(seq, np.uint8)[pos - 1]
    counts, depth, flags = oracle.encode_columns(bases if bases.size else np.zeros(1, np.uint8), col_off, ref, min_af, min_coverage)
    if conf_bits is not None:
        md = max_del_lengths(bases, col_off, ref)
        flags = np.where(confident_pass(pos, md, conf_bits), flags, flags & np.uint8(0xF7)).astype(np.uint8)
    centers = oracle.select_sites(pos, flags)
    return pos[centers], oracle.gather_windows(counts, centers), depth[centers]
