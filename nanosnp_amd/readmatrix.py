"""Stage-4 read-matrix builder: haplotagged reads -> per-group read x position matrices -> the padded planes the haplotype
feature kernel consumes.

    read_matrices   create_pileup_haplotype.single_group_pileup_haplotype_feature :22-134   the two pileup passes over the
                    alignment file: coverage filter of the groups, then one row per read name over the union of the groups'
                    positions (base code / HP tag / base quality / mapping quality; 0 = the read does not cover the column)
    group_planes    :137-207 + write_to_bins.py:15-61   per group the 11 support columns and the 33-wide window, reads kept when
                    their centre base is non-zero, ordered by the HP tag at the centre, padded with -2 / cut at D rows -- on the
                    device through nsnp_hap_arrange_reads2 (the planes never visit the host again before the feature kernel);
                    tie_order="numpy1" reproduces the reference's bins row for row

    read_matrices_device   the same two passes on the device (hap_reads.hip: nsnp_hap_read_depths, nsnp_hap_read_matrices) for reads
                    handed over as AlignmentRecords, a struct of arrays of decoded records (``AlignmentRecords.from_alignments(
                    samfile.fetch(...))``); the matrices stay on the device and group_planes takes them as they are

The alignment file of read_matrices is whatever the caller's BAM library hands over: any object with pysam's ``pileup(contig, start, end,
min_base_quality=0, min_mapping_quality=0)`` iteration (columns with ``.pos``, ``.n``, ``.pileups``; pileup reads with
``.alignment.{query_name, has_tag, get_tag, query_sequence, query_qualities, mapping_quality}``, ``.is_del``, ``.is_refskip``,
``.query_position``) -- a ``pysam.AlignmentFile`` works unchanged (htslib is not part of this repository's image; the tests
drive a stand-in with synthetic reads and compare with the reference function run on the same stand-in).
"""
from __future__ import annotations

import numpy as np

BASE_TO_INT = {"A": 1, "C": 2, "G": 3, "T": 4}        # create_pileup_haplotype.py:7


class ReadMatrices:
    """positions: sorted 1-based columns; seq / hap / baseq / mapq: int32 [n_reads, n_positions] in first-seen read order"""

    def __init__(self, contig, positions, names, seq, hap, baseq, mapq, groups):
        self.contig, self.positions, self.names = contig, positions, names
        self.seq, self.hap, self.baseq, self.mapq, self.groups = seq, hap, baseq, mapq, groups
        self._col = {p: i for i, p in enumerate(positions)}

    def columns(self, wanted):
        return np.array([self._col[int(p)] for p in wanted], np.int64)


def read_matrices(samfile, groups, max_coverage, pileup_flanking_size=16):
    """groups: [[(contig, position)] * (2 * adjacent_size + 1)] (or objects with .ctgname / .position as the reference's SNPItem),
    all on one contig.  Returns ReadMatrices, or None when no group survives the coverage filter or a read carries a base
    outside ACGT at a wanted column (the reference's bare `except` then returns nothing for the whole call, :209-214)."""
    def cp(item):
        return (item.ctgname, int(item.position)) if hasattr(item, "position") else (item[0], int(item[1]))
    groups = [[cp(it) for it in g] for g in groups]
    if not groups:
        return None
    ctg = groups[0][0][0]
    assert all(g[0][0] == ctg for g in groups)
    positions = sorted({p for g in groups for _, p in g})
    pset = set(positions)
    failed = set()
    for col in samfile.pileup(ctg, positions[0], positions[-1], min_base_quality=0, min_mapping_quality=0):       # :39-47
        p = col.pos + 1
        if p < positions[0]:
            continue
        if p > positions[-1]:
            break
        if p in pset and col.n > max_coverage:
            failed.add(p)
    if failed:
        groups = [g for g in groups if not any(p in failed for _, p in g)]                                      # :50-60
    if not groups:
        return None
    ext = set()
    for g in groups:                                                                                             # :73-83
        mid = len(g) // 2
        for k, (_, p) in enumerate(g):
            if k == mid:
                ext.update(range(p - pileup_flanking_size, p + pileup_flanking_size + 1))
            else:
                ext.add(p)
    ext = sorted(ext)
    col_of = {p: i for i, p in enumerate(ext)}
    row_of, names = {}, []
    cells = []                                            # (row, col, seq, hap, baseq, mapq)
    for col in samfile.pileup(ctg, ext[0], ext[-1], min_base_quality=0, min_mapping_quality=0):                 # :89-134
        p = col.pos + 1
        if p < ext[0]:
            continue
        if p > ext[-1]:
            break
        i = col_of.get(p)
        if i is None:
            continue
        # The reference asserts here (:98 the coverage of EVERY wanted column - the first pass looked at the group positions only, a
        # window column can still be deeper; :104 the HP tag is 1, 2 or 3) inside its bare try / except (:209-214), which prints and
        # returns its still empty lists: nothing for this chunk of groups.  Same outcome here.
        if col.n > max_coverage:
            return None
        for pr in col.pileups:
            aln = pr.alignment
            tag = aln.get_tag("HP") if aln.has_tag("HP") else 3
            if tag not in (1, 2, 3):
                return None
            r = row_of.get(aln.query_name)
            if r is None:
                r = row_of[aln.query_name] = len(names)
                names.append(aln.query_name)
            if not pr.is_del and not pr.is_refskip:
                code = BASE_TO_INT.get(str.upper(aln.query_sequence[pr.query_position]))
                if code is None:
                    return None
                cells.append((r, i, code, tag, int(aln.query_qualities[pr.query_position]), int(aln.mapping_quality)))
            elif pr.is_del:
                cells.append((r, i, -1, tag, 0, int(aln.mapping_quality)))
    R, P = len(names), len(ext)
    seq = np.zeros((R, P), np.int32); hap = np.zeros((R, P), np.int32)
    bq = np.zeros((R, P), np.int32); mq = np.zeros((R, P), np.int32)
    if cells:
        c = np.array(cells, np.int64)
        seq[c[:, 0], c[:, 1]] = c[:, 2]; hap[c[:, 0], c[:, 1]] = c[:, 3]
        bq[c[:, 0], c[:, 1]] = c[:, 4]; mq[c[:, 0], c[:, 1]] = c[:, 5]
    return ReadMatrices(ctg, ext, names, seq, hap, bq, mq, groups)


# ---- the same matrices from decoded alignment records, on the device (hap_reads.hip) -------------------------------------------------
CIGAR_OPS = "MIDNSHP=X"                                # BAM op codes 0..8
_QUERY_OPS = np.array([1, 1, 0, 0, 1, 0, 0, 1, 1], np.int64)      # M, I, S, =, X consume the query
_SKIP_FLAGS = 0x704                                    # unmapped, secondary, QC-fail, duplicate: pysam's default pileup stepper ("all")


class DeviceRecords:
    """AlignmentRecords.to_device(): the arrays as device tensors (cigar as int32 words, the same bits)"""

    def __init__(self, n, **tensors):
        self.n = n
        self.__dict__.update(tensors)


class AlignmentRecords:
    """The fields of decoded alignment records of ONE contig as a struct of arrays, in file (coordinate) order:

        start      int64 [R]      1-based leftmost reference position (BAM pos + 1), non-decreasing
        mapq       uint8 [R]      mapping quality
        hp         int32 [R]      the HP tag, -1 = no tag (counts as 3, create_pileup_haplotype.py:103)
        cigar      uint32 [sum n_ops]   BAM's own encoding len << 4 | op, ops 0..8 = MIDNSHP=X
        cigar_off  int64 [R+1]    offsets into cigar
        seq, qual  uint8 [sum query_len]   one ASCII byte / one base quality per base, soft clips included, hard clips not
        seq_off    int64 [R+1]    offsets into seq / qual
        names      list [R]       read names, unique (the reference keys a row by the read's name); they stay on the host

    Build with from_arrays (validates) or from_alignments (packs pysam-like AlignedSegments, then validates)."""

    def __init__(self, start, mapq, hp, cigar, cigar_off, seq, qual, seq_off, names, contig=None):
        self.start, self.mapq, self.hp, self.cigar, self.cigar_off = start, mapq, hp, cigar, cigar_off
        self.seq, self.qual, self.seq_off, self.names, self.contig = seq, qual, seq_off, names, contig

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_arrays(cls, start, mapq, hp, cigar, cigar_off, seq, qual, seq_off, names, contig=None):
        """Validates on the host and raises NanoSNPError: nothing out of range ever reaches a kernel."""
        from ._lib import NanoSNPError

        def arr(a, dt, what):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
                raise NanoSNPError(f"AlignmentRecords: {what} must be a vector of integers")
            if a.size and (int(a.min()) < np.iinfo(dt).min or int(a.max()) > np.iinfo(dt).max):
                raise NanoSNPError(f"AlignmentRecords: {what} does not fit {np.dtype(dt).name}")
            a = np.ascontiguousarray(a, dt)
            return a if a.flags.writeable else a.copy()    # (torch.from_numpy wants a writable array)
        if isinstance(seq, (bytes, bytearray, str)):
            seq = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), np.uint8)
        start, mapq, hp = arr(start, np.int64, "start"), arr(mapq, np.uint8, "mapq"), arr(hp, np.int32, "hp")
        cigar, cigar_off = arr(cigar, np.uint32, "cigar"), arr(cigar_off, np.int64, "cigar_off")
        seq, qual, seq_off = arr(seq, np.uint8, "seq"), arr(qual, np.uint8, "qual"), arr(seq_off, np.int64, "seq_off")
        names = list(names)
        R = len(names)
        if not (len(start) == len(mapq) == len(hp) == R):
            raise NanoSNPError("AlignmentRecords: start, mapq, hp and names must have one entry per record")
        if len(set(names)) != R:
            raise NanoSNPError("AlignmentRecords: read names must be unique (the reference keys a row by the read's name; drop "
                               "supplementary alignments, flag 0x800, or rename them)")
        for off, n, what in ((cigar_off, len(cigar), "cigar_off"), (seq_off, len(seq), "seq_off")):
            if len(off) != R + 1 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
                raise NanoSNPError(f"AlignmentRecords: {what} must hold R + 1 monotone offsets from 0 to the array's length")
        if len(qual) != len(seq):
            raise NanoSNPError("AlignmentRecords: seq and qual must have one entry per base")
        ops = cigar & 15
        if (ops > 8).any():
            raise NanoSNPError("AlignmentRecords: CIGAR op code above 8 (MIDNSHP=X are 0..8)")
        qsum = np.concatenate([[0], np.cumsum((cigar >> 4).astype(np.int64) * _QUERY_OPS[ops])])
        bad = np.flatnonzero(qsum[cigar_off[1:]] - qsum[cigar_off[:-1]] != np.diff(seq_off))
        if bad.size:
            raise NanoSNPError(f"AlignmentRecords: record {int(bad[0])} ({names[int(bad[0])]!r}): the lengths of its M, I, S, =, X ops "
                               "do not sum to the length of its sequence")
        if (np.diff(start) < 0).any():
            raise NanoSNPError("AlignmentRecords: starts decrease; the records must come in coordinate order (as an indexed BAM has them)")
        return cls(start, mapq, hp, cigar, cigar_off, seq, qual, seq_off, names, contig)

    @classmethod
    def from_alignments(cls, alignments, contig=None):
        """alignments: any iterable of objects with pysam's AlignedSegment attributes (reference_start, cigartuples, query_sequence,
        query_qualities, mapping_quality, query_name, flag, has_tag / get_tag), e.g. ``samfile.fetch(contig, start, end)``.
        Skips what pysam's default pileup stepper skips: flags 0x704 (unmapped, secondary, QC-fail, duplicate) and paired reads
        that are not properly paired."""
        from ._lib import NanoSNPError
        start, mapq, hp, cigar, cigar_off, seq, qual, seq_off, names = [], [], [], [], [0], [], [], [0], []
        for aln in alignments:
            flag = int(aln.flag)
            if flag & _SKIP_FLAGS or (flag & 0x1 and not flag & 0x2):
                continue
            if aln.cigartuples is None or aln.query_sequence is None or aln.query_qualities is None:
                raise NanoSNPError(f"AlignmentRecords: read {aln.query_name!r} has no CIGAR, sequence or qualities")
            tag = int(aln.get_tag("HP")) if aln.has_tag("HP") else -1
            if aln.has_tag("HP") and not 1 <= tag <= 3:
                tag = 0                                     # any tag outside 1..3 ends the chunk; -1 is kept for "no tag"
            start.append(int(aln.reference_start) + 1); mapq.append(int(aln.mapping_quality)); hp.append(tag)
            cigar.extend((int(n) << 4) | int(op) for op, n in aln.cigartuples)
            cigar_off.append(len(cigar))
            seq.append(aln.query_sequence.encode("ascii"))
            qual.extend(int(q) for q in aln.query_qualities)
            seq_off.append(seq_off[-1] + len(seq[-1]))
            names.append(aln.query_name)
        return cls.from_arrays(np.array(start, np.int64), np.array(mapq, np.int64), np.array(hp, np.int64),
                               np.array(cigar, np.int64), np.array(cigar_off, np.int64), np.frombuffer(b"".join(seq), np.uint8),
                               np.array(qual, np.int64), np.array(seq_off, np.int64), names, contig)

    def to_device(self, device):
        import torch
        t = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
        return DeviceRecords(len(self), start=t(self.start), mapq=t(self.mapq), hp=t(self.hp), cigar=t(self.cigar.view(np.int32)),
                             cigar_off=t(self.cigar_off), seq=t(self.seq), qual=t(self.qual), seq_off=t(self.seq_off))


def read_matrices_device(ctx, records, groups, max_coverage, pileup_flanking_size=16):
    """read_matrices for AlignmentRecords, on the device: the same ReadMatrices (or None in the same cases) with seq / hap / baseq /
    mapq as int32 cuda tensors.  The records go to the device once; the depths of the group positions come back for the group
    filter of :50-60, then the row count and the status word of the fill."""
    import torch
    from ._lib import NanoSNPError

    def cp(item):
        return (item.ctgname, int(item.position)) if hasattr(item, "position") else (item[0], int(item[1]))
    groups = [[cp(it) for it in g] for g in groups]
    if not groups:
        return None
    ctg = groups[0][0][0]
    assert all(g[0][0] == ctg for g in groups)
    if records.contig is not None and records.contig != ctg:
        raise NanoSNPError(f"read_matrices_device: the records are of contig {records.contig!r}, the groups of {ctg!r}")
    dev = torch.device("cuda", ctx.device)
    rec = records.to_device(dev)
    positions = sorted({p for g in groups for _, p in g})
    depth = ctx.hap_read_depths(rec, torch.tensor(positions, dtype=torch.int64, device=dev)).cpu().numpy()
    failed = {p for p, d in zip(positions, depth.tolist()) if d > 0 and d > max_coverage}   # (a pileup yields no empty column)
    if failed:
        groups = [g for g in groups if not any(p in failed for _, p in g)]                                      # :50-60
    if not groups:
        return None
    ext = set()
    for g in groups:                                                                                             # :73-83
        mid = len(g) // 2
        for k, (_, p) in enumerate(g):
            if k == mid:
                ext.update(range(p - pileup_flanking_size, p + pileup_flanking_size + 1))
            else:
                ext.add(p)
    ext = sorted(ext)
    cols = torch.tensor(ext, dtype=torch.int64, device=dev)
    _, rows = ctx.hap_read_depths(rec, cols, want_rows=True)
    seq, hap, bq, mq, row_record, meta = ctx.hap_read_matrices(rec, cols, max_coverage, int(rows.item()))
    n_rows, status = meta[:2].tolist()
    if status != 0:                                        # a column too deep, an HP tag outside 1..3, a base outside ACGTacgt
        return None
    names = [records.names[i] for i in row_record[:n_rows].tolist()]
    return ReadMatrices(ctg, ext, names, seq, hap, bq, mq, groups)


def group_slices(rm, pileup_flanking_size=16):
    """per group the column sets of :141 (its positions) and :178 (the window around its centre) and the position strings"""
    out = []
    for g in rm.groups:
        gpos = [p for _, p in g]
        centre = gpos[len(gpos) // 2]
        wpos = list(range(centre - pileup_flanking_size, centre + pileup_flanking_size + 1))
        out.append(dict(candidate=f"{rm.contig}:{centre}", haplotype_positions=[f"{rm.contig}:{p}" for p in gpos],
                        hap_cols=rm.columns(gpos), pile_cols=rm.columns(wpos)))
    return out


def group_planes(ctx, rm, max_haplotype_depth, max_pileup_depth, pileup_flanking_size=16, tie_order="stable"):
    """-> (candidate_positions, haplotype_positions, (seq, baseq, mapq, hap) int32 cuda [N, D_h, 11], the same [N, D_p, 33],
    depths_h, depths_p): reads filtered on the centre base, HP-sorted, padded with -2 and cut at D, exactly what
    write_to_bins.py stores and nanosnp_amd.predict.predict_haplotype consumes (plus reference rows).
    tie_order (Context.hap_arrange_reads): "numpy1" orders equal HP tags as the reference's NumPy 1.x quicksort does, so the planes
    equal its bins row for row and a cut keeps the reads it keeps; "stable" keeps ties in read order."""
    import torch
    sl = group_slices(rm, pileup_flanking_size)
    dev = torch.device("cuda", ctx.device)
    if isinstance(rm.seq, torch.Tensor):                   # read_matrices_device: the matrices are on the device already
        full = [rm.seq, rm.baseq, rm.mapq, rm.hap]
    else:
        full = [torch.from_numpy(a).to(dev) for a in (rm.seq, rm.baseq, rm.mapq, rm.hap)]
    outs = []
    for key, D in (("hap_cols", max_haplotype_depth), ("pile_cols", max_pileup_depth)):
        idx = torch.from_numpy(np.stack([s[key] for s in sl])).to(dev)                   # [N, L]
        mats = [f[:, idx].permute(1, 0, 2).contiguous() for f in full]                    # [N, R, L] views of the one matrix
        outs.append(ctx.hap_arrange_reads(*mats, int(D), tie_order=tie_order))
    (hs, hb, hm, hh, dh), (ps, pb, pm, ph, dp) = outs
    return ([s["candidate"] for s in sl], [s["haplotype_positions"] for s in sl], (hs, hb, hm, hh), (ps, pb, pm, ph), dh, dp)
