"""BED region files for the candidate selection: the reference's -extended_confident_bed / -confident_bed
(dna_sv_tensor/src/common/bed_intv_list.cpp).

The reference turns a BED file into one bit per reference base - interval [from, to) sets the 0-based bits from .. to - 1 - and asks two
questions of it (make_candidate_snp_tensor/main.cpp:165,194): is bit p - 1 set (extended BED: a line at position p is read at all), and is
any bit of [p - 1, p + max_del_length + 1) set (confident BED: the column may be a candidate).  Here the bits of ONE contig are a uint32
array, bit i = bit (i & 31) of word i >> 5, uploaded once per contig and tested on the device (include/nanosnp.h); bits at or beyond the
contig length read as 0, where the reference - one list over all contigs - reads the first bits of the next contig.
A call over one whole-genome text takes the bitmaps of all its contigs as one TABLE (table_bitmaps; _lib.BedTable puts it on the device).
"""
from __future__ import annotations

import os
import re

import numpy as np

from ._lib import NanoSNPError

_ATOI = re.compile(rb"[ \t\n\v\f\r]*([+-]?[0-9]+)")


def _atoi(tok: bytes) -> int:
    """C atoi: leading white space, an optional sign, digits up to the first other byte; 0 without digits"""
    m = _ATOI.match(tok)
    return int(m.group(1)) if m else 0


def fai_lengths(fai) -> dict:
    """contig lengths from a dict {name: length}, the text of a .fai index (str / bytes: name <tab> length ...) or the path of one"""
    if isinstance(fai, dict):
        return {(k.decode() if isinstance(k, bytes) else str(k)): int(v) for k, v in fai.items()}
    if isinstance(fai, os.PathLike) or (isinstance(fai, str) and "\t" not in fai and "\n" not in fai):
        with open(fai, "rb") as f:
            fai = f.read()
    if isinstance(fai, str):
        fai = fai.encode()
    out = {}
    for line in bytes(fai).splitlines():
        cols = line.split(b"\t")
        if len(cols) >= 2 and cols[0]:
            out[cols[0].decode()] = int(cols[1])
    return out


def load_bed(path_or_bytes, fai, skip_unknown=False) -> dict:
    """A BED file (a path, or its bytes) -> {contig: int64 [n, 2] of (from, to), in file order}.  As BedIntvList's constructor reads it:
    lines beginning with '#' are skipped, fields are runs of non-tab bytes, from / to are read as atoi does; fewer than three fields,
    from >= to, to > the contig length and a contig the index does not hold are errors (the reference asserts): NanoSNPError.
    Overlapping intervals are allowed (bed_bitmap: their union).  skip_unknown: lines of contigs the index does not hold are passed over
    instead (a caller that streams ONE contig and knows only its length)."""
    lengths = fai_lengths(fai)
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data, what = bytes(path_or_bytes), "BED text"
    else:
        what = os.fspath(path_or_bytes)
        with open(what, "rb") as f:
            data = f.read()
    out = {}
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for n, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line[:1] == b"#":
            continue
        cols = [c for c in line.split(b"\t") if c]
        if len(cols) < 3:
            raise NanoSNPError(f"{what}:{n}: a BED line needs three tab-separated fields")
        name = cols[0].decode(errors="replace")
        if name not in lengths:
            if skip_unknown:
                continue
            raise NanoSNPError(f"{what}:{n}: contig {name!r} is not in the reference index")
        lo, hi = _atoi(cols[1]), _atoi(cols[2])
        if not lo < hi:
            raise NanoSNPError(f"{what}:{n}: from ({lo}) must be smaller than to ({hi})")
        if hi > lengths[name]:
            raise NanoSNPError(f"{what}:{n}: to ({hi}) lies beyond the end of {name} ({lengths[name]})")
        if lo < 0:
            raise NanoSNPError(f"{what}:{n}: from ({lo}) is negative")
        out.setdefault(name, []).append((lo, hi))
    return {k: np.asarray(v, np.int64).reshape(-1, 2) for k, v in out.items()}


def bed_bitmap(intervals, chr_len) -> np.ndarray:
    """intervals: int [n, 2] of 0-based half-open (from, to), or None / empty -> uint32 [(chr_len + 31) // 32], bit i of the contig = bit
    (i & 31) of word i >> 5, set when some interval holds i.  Intervals may overlap; one that leaves [0, chr_len] is an error."""
    chr_len = int(chr_len)
    iv = np.zeros((0, 2), np.int64) if intervals is None else np.asarray(intervals, np.int64).reshape(-1, 2)
    if iv.size and (int(iv.min()) < 0 or int(iv[:, 1].max()) > chr_len or bool((iv[:, 0] >= iv[:, 1]).any())):
        raise NanoSNPError("bed_bitmap: an interval must satisfy 0 <= from < to <= contig length")
    n_words = (chr_len + 31) // 32
    words = np.zeros(n_words, np.uint32)
    if not iv.size:
        return words
    # the first and last word of every interval by mask, the whole words between them by a difference array over the words (overlaps:
    # an OR and a count > 0, so the union needs no merge)
    full = np.uint32(0xFFFFFFFF)
    lo, last = iv[:, 0], iv[:, 1] - 1
    w0, w1 = lo >> 5, last >> 5
    m_lo = full << (lo & 31).astype(np.uint32)
    m_hi = full >> (31 - (last & 31)).astype(np.uint32)
    one = w0 == w1
    np.bitwise_or.at(words, w0[one], m_lo[one] & m_hi[one])
    np.bitwise_or.at(words, w0[~one], m_lo[~one])
    np.bitwise_or.at(words, w1[~one], m_hi[~one])
    d = np.zeros(n_words + 1, np.int32)
    np.add.at(d, w0[~one] + 1, 1)
    np.add.at(d, w1[~one], -1)
    words[np.cumsum(d[:n_words]) > 0] = full
    return words


def contig_intervals(bed, contig, chr_len, fai=None):
    """what a pipeline call was given for one contig: bed = None, a path (checked against the index fai - a dict or .fai text - when there
    is one, else against this contig's length alone), or a dict {contig: intervals} -> int64 [n, 2] (empty: the BED holds nothing of this
    contig - every bit 0)"""
    if bed is None:
        return None
    if not isinstance(bed, dict):
        bed = load_bed(bed, fai) if fai is not None else load_bed(bed, {contig: int(chr_len)}, skip_unknown=True)
    iv = bed.get(contig)
    return np.zeros((0, 2), np.int64) if iv is None else np.asarray(iv, np.int64).reshape(-1, 2)


def table_intervals(bed, names, lengths, fai=None):
    """what a whole-genome call was given as one BED -> the intervals of every contig of `names`, in their order: [int64 [n, 2] or None (the
    BED holds nothing of this contig)].  bed: a path - read by load_bed against the whole index fai (a dict, .fai text or path: an interval
    beyond a contig and a contig the index lacks raise, as in the reference), without one against {names: lengths} with other contigs passed
    over - or a dict {contig: intervals}.  Contigs outside `names` are ignored; every interval must lie inside its contig (bed_bitmap's rule)."""
    names, lengths = [str(n) for n in names], [int(n) for n in lengths]
    if len(names) != len(lengths):
        raise NanoSNPError("table_intervals: one length per name")
    if not isinstance(bed, dict):
        bed = load_bed(bed, fai) if fai is not None else load_bed(bed, dict(zip(names, lengths)), skip_unknown=True)
    out = []
    for name, n in zip(names, lengths):
        iv = bed.get(name)
        iv = None if iv is None else np.asarray(iv, np.int64).reshape(-1, 2)
        if iv is not None and not iv.size:
            iv = None
        if iv is not None and (int(iv.min()) < 0 or int(iv[:, 1].max()) > n or bool((iv[:, 0] >= iv[:, 1]).any())):
            raise NanoSNPError(f"{name}: an interval must satisfy 0 <= from < to <= contig length ({n})")
        out.append(iv)
    return out


def table_word_offsets(intervals, lengths):
    """-> int64 [n + 1]: contig c owns words [off[c], off[c + 1]) - (length + 31) // 32 of them, ZERO for a contig without intervals"""
    return np.concatenate([[0], np.cumsum([0 if iv is None else (int(n) + 31) // 32 for iv, n in zip(intervals, lengths)])]).astype(np.int64)


def table_bitmaps(bed, names, lengths, fai=None):
    """The bitmap table of a call over several contigs (include/nanosnp.h) -> (words uint32, off int64 [n + 1]): the bed_bitmap of every contig
    of `names` the BED holds, back to back; contig c owns words [off[c], off[c + 1]) and has min(lengths[c], 32 * its words) bits - a contig
    without intervals takes zero words, every bit of it reads 0.  bed, fai: as table_intervals reads them."""
    iv = table_intervals(bed, names, lengths, fai)
    off = table_word_offsets(iv, lengths)
    parts = [bed_bitmap(v, n) for v, n in zip(iv, lengths) if v is not None]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint32)), off
