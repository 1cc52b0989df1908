"""Helpers of the alignment-record tests (not a test file): a seeded record generator, a per-base stand-in for the alignment file
that readmatrix.read_matrices iterates, the conversion of tests.helpers reads to records, and a numpy restatement of the rules
by which nanosnp_amd/csrc/hap_reads.hip builds the read matrices (include/nanosnp.h).

A record is a dict {name, a (1-based start), cigar [(op, length)] with ops 0..8 = MIDNSHP=X, seq (str, soft clips included),
quals (one per base), hp (1, 2, None = no tag, or anything else to be refused), mapq, flag}.

The stand-in and the restatement share nothing: RecordSamfile expands every CIGAR base by base into {position: (kind, query
position)} and knows nothing of prefix sums; rules_matrices works on prefix sums and searches and never expands a CIGAR."""
from __future__ import annotations

import numpy as np

from nanosnp_amd import readmatrix

M, I, D, N, S, H, P, EQ, X = range(9)
REF_OPS, QUERY_OPS, MATCH_OPS = (M, D, N, EQ, X), (M, I, S, EQ, X), (M, EQ, X)


# ---- the stand-in: what create_pileup_haplotype.py:39-47,90-134 touches of a pysam.AlignmentFile, from records ----------------------
class _RecAlignment:
    def __init__(self, rd):
        self.rd = rd
        self.query_name, self.query_sequence, self.query_qualities = rd["name"], rd["seq"], list(rd["quals"])
        self.mapping_quality, self.flag = rd["mapq"], rd.get("flag", 0)
        self.reference_start, self.cigartuples = rd["a"] - 1, [tuple(t) for t in rd["cigar"]]
        self.at = {}                                       # 1-based position -> (kind, query position)
        pos, q = rd["a"], 0
        for op, n in rd["cigar"]:
            for _ in range(n):
                if op in MATCH_OPS:
                    self.at[pos] = ("M", q); pos += 1; q += 1
                elif op in (I, S):
                    q += 1
                elif op == D:
                    self.at[pos] = ("D", None); pos += 1
                elif op == N:
                    self.at[pos] = ("N", None); pos += 1
        self.end = pos - 1

    def has_tag(self, t):
        return t == "HP" and self.rd["hp"] is not None

    def get_tag(self, t):
        return self.rd["hp"]


class _RecPileupRead:
    def __init__(self, aln, p):
        kind, q = aln.at[p]
        self.alignment, self.is_del, self.is_refskip, self.query_position = aln, kind == "D", kind == "N", q


class _RecColumn:
    def __init__(self, pos0, prs):
        self.pos, self.pileups, self.n = pos0, prs, len(prs)


class RecordSamfile:
    """pileup() as tests.helpers.FakeSamfile: the columns round the region that at least one read sits in, reads in record order"""

    def __init__(self, records):
        self.alns = [_RecAlignment(rd) for rd in records]

    def pileup(self, contig, start, end, min_base_quality=0, min_mapping_quality=0):
        for p in range(max(start - 3, 1), end + 4):
            prs = [_RecPileupRead(a, p) for a in self.alns if p in a.at]
            if prs:
                yield _RecColumn(p - 1, prs)

    def fetch(self):
        return list(self.alns)


# ---- records ----------------------------------------------------------------------------------------------------------------------------
def from_helper_reads(reads):
    """tests.helpers.synth_reads dicts (one base or 'D' per reference position) -> records in coordinate order"""
    out = []
    for rd in reads:
        cigar = []
        for o in rd["ops"]:
            op = D if o == "D" else M
            if cigar and cigar[-1][0] == op:
                cigar[-1][1] += 1
            else:
                cigar.append([op, 1])
        out.append(dict(name=rd["name"], a=rd["a"], cigar=[tuple(c) for c in cigar], seq="".join(o for o in rd["ops"] if o != "D"),
                        quals=[q for o, q in zip(rd["ops"], rd["quals"]) if o != "D"], hp=rd["hp"], mapq=rd["mapq"], flag=0))
    return sorted(out, key=lambda r: r["a"])


def make_record(rng, name, a, cigar, lower=False, hp="rand", mapq=None):
    qlen = sum(n for op, n in cigar if op in QUERY_OPS)
    seq = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, qlen))
    return dict(name=name, a=int(a), cigar=[(int(op), int(n)) for op, n in cigar], seq=seq.lower() if lower else seq,
                quals=rng.integers(1, 60, qlen).tolist(), hp=[1, 2, None][int(rng.integers(0, 3))] if hp == "rand" else hp,
                mapq=int(rng.integers(0, 61)) if mapq is None else mapq, flag=0)


def _cigar(rng, variant, span):
    """a CIGAR whose reference length is `span`"""
    if variant == "plain":
        out, left = [], span
        while left > 0:
            n = int(min(left, rng.integers(5, 80)))
            out.append((M, n)); left -= n
            if left > 0 and rng.random() < 0.5:
                n = int(min(left, rng.integers(1, 4))); out.append((D, n)); left -= n
        return out
    if variant == "unit":                                  # every op of length 1: as many ops as bases
        out, left = [], span
        while left > 0:
            u = rng.random()
            if u < 0.70:
                out.append((int(rng.choice([M, EQ, X])), 1)); left -= 1
            elif u < 0.80:
                out.append((D, 1)); left -= 1
            elif u < 0.85:
                out.append((N, 1)); left -= 1
            elif u < 0.95:
                out.append((I, 1))
            else:
                out.append((P, 1))
        return out
    out, left = [], span                                   # "mixed": insertions, clips, N, = / X, padding
    if rng.random() < 0.3:
        out.append((H, int(rng.integers(1, 30))))
    if rng.random() < 0.5:
        out.append((S, int(rng.integers(1, 40))))
    while left > 0:
        n = int(min(left, rng.integers(1, 60)))
        out.append((int(rng.choice([M, M, EQ, X])), n)); left -= n
        if left <= 0:
            break
        u = rng.random()
        if u < 0.3:
            out.append((I, int(rng.integers(1, 6))))
        elif u < 0.55:
            n = int(min(left, rng.integers(1, 5))); out.append((D, n)); left -= n
        elif u < 0.7:
            n = int(min(left, rng.integers(5, 60))); out.append((N, n)); left -= n
        elif u < 0.75:
            out.append((P, int(rng.integers(1, 3))))
    if rng.random() < 0.5:
        out.append((S, int(rng.integers(1, 40))))
    if rng.random() < 0.3:
        out.append((H, int(rng.integers(1, 30))))
    return out


def synth_records(seed, variant="plain", n_reads=70, span=(1, 900), lengths=(150, 700)):
    """n_reads records in coordinate order; variant "plain" (M and D), "mixed" (I, S, H, N, =, X, P too), "unit" (every op of
    length 1: a read of 700 bases has more than 700 ops)"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n_reads):
        a = int(rng.integers(span[0], span[1] - 200))
        ln = int(rng.integers(lengths[0], lengths[1]))
        if variant == "unit":
            ln = int(rng.choice([70, 130, 300, 700])) + int(rng.integers(0, 20))
        ln = max(1, min(ln, span[1] - a + 1))
        out.append(make_record(rng, f"r{r}", a, _cigar(rng, variant, ln), lower=rng.random() < 0.1))
    return sorted(out, key=lambda rd: rd["a"])


def to_arrays(records):
    """-> the keyword arguments of AlignmentRecords.from_arrays"""
    cigar = [(n << 4) | op for rd in records for op, n in rd["cigar"]]
    return dict(start=np.array([rd["a"] for rd in records], np.int64), mapq=np.array([rd["mapq"] for rd in records], np.uint8),
                hp=np.array([-1 if rd["hp"] is None else rd["hp"] for rd in records], np.int32), cigar=np.array(cigar, np.uint32),
                cigar_off=np.cumsum([0] + [len(rd["cigar"]) for rd in records]).astype(np.int64),
                seq=np.frombuffer("".join(rd["seq"] for rd in records).encode(), np.uint8),
                qual=np.array([q for rd in records for q in rd["quals"]], np.uint8),
                seq_off=np.cumsum([0] + [len(rd["seq"]) for rd in records]).astype(np.int64), names=[rd["name"] for rd in records])


def to_alignment_records(records):
    return readmatrix.AlignmentRecords.from_arrays(**to_arrays(records))


# ---- the rules, restated on prefix sums ---------------------------------------------------------------------------------------------------
_CODE = np.zeros(256, np.int32)
for _k, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _k + 1


def rules_matrices(ar, groups, max_coverage, pileup_flanking_size=16):
    """ar: readmatrix.AlignmentRecords.  -> (names, ext, seq, hap, baseq, mapq, groups) or None, by the rules of include/nanosnp.h"""
    R = len(ar)
    ops, lens = (ar.cigar & 15).astype(np.int64), (ar.cigar >> 4).astype(np.int64)
    isref, isq = np.isin(ops, REF_OPS), np.isin(ops, QUERY_OPS)
    rcum = np.concatenate([[0], np.cumsum(lens * isref)]); qcum = np.concatenate([[0], np.cumsum(lens * isq)])
    a = ar.start
    b = a + (rcum[ar.cigar_off[1:]] - rcum[ar.cigar_off[:-1]]) - 1

    def depth(cols):
        cols = np.asarray(cols, np.int64)
        return ((a[None, :] <= cols[:, None]) & (cols[:, None] <= b[None, :])).sum(1) if R else np.zeros(len(cols), np.int64)
    groups = [[(c, int(p)) for c, p in g] for g in groups]
    positions = sorted({p for g in groups for _, p in g})
    max_coverage = max(int(max_coverage), 0)               # (an empty column is never seen, whatever the limit)
    failed = {p for p, d in zip(positions, depth(positions)) if d > max_coverage}
    groups = [g for g in groups if not any(p in failed for _, p in g)]
    if not groups:
        return None
    ext = set()
    for g in groups:
        for k, (_, p) in enumerate(g):
            ext.update(range(p - pileup_flanking_size, p + pileup_flanking_size + 1) if k == len(g) // 2 else [p])
    ext = np.array(sorted(ext), np.int64)
    if (depth(ext) > max_coverage).any():
        return None
    lo, hi = np.searchsorted(ext, a, "left"), np.searchsorted(ext, b, "right")
    rows = np.flatnonzero(hi > lo)
    tag = np.where(ar.hp == -1, 3, ar.hp)
    if not np.isin(tag[rows], (1, 2, 3)).all():
        return None
    out = [np.zeros((len(rows), len(ext)), np.int32) for _ in range(4)]
    for row, r in enumerate(rows):
        o0, o1 = int(ar.cigar_off[r]), int(ar.cigar_off[r + 1])
        rinc = rcum[o0 + 1:o1 + 1] - rcum[o0]              # reference bases up to and with each op
        cols = np.arange(lo[r], hi[r])
        off = ext[cols] - a[r]
        k = np.searchsorted(rinc, off, "right")            # the op that holds the column
        op = ops[o0 + k]
        isM, isD = np.isin(op, MATCH_OPS), op == D
        qpos = (qcum[o0 + k] - qcum[o0]) + off - (rinc[k] - lens[o0 + k])
        qi = int(ar.seq_off[r]) + np.where(isM, qpos, 0)
        base = np.where(isM, _CODE[ar.seq[np.minimum(qi, max(len(ar.seq) - 1, 0))]] if len(ar.seq) else 0, 0)
        if (isM & (base == 0)).any():
            return None
        out[0][row, cols] = np.where(isM, base, np.where(isD, -1, 0))
        out[1][row, cols] = np.where(isM | isD, tag[r], 0)
        out[2][row, cols] = np.where(isM, ar.qual[np.minimum(qi, max(len(ar.qual) - 1, 0))] if len(ar.qual) else 0, 0)
        out[3][row, cols] = np.where(isM | isD, ar.mapq[r], 0)
    return [ar.names[r] for r in rows], ext.tolist(), out[0], out[1], out[2], out[3], groups


def same_matrices(got, want):
    """a ReadMatrices (numpy or device matrices) against another, or against rules_matrices' tuple: names, positions, groups, cells"""
    def parts(x):
        if isinstance(x, tuple):
            return x
        mats = [m.cpu().numpy() if hasattr(m, "cpu") else m for m in (x.seq, x.hap, x.baseq, x.mapq)]
        return (x.names, x.positions, *mats, x.groups)
    g, w = parts(got), parts(want)
    assert list(g[0]) == list(w[0]), "read names / row order"
    assert list(g[1]) == list(w[1]), "positions"
    assert [list(map(tuple, x)) for x in g[6]] == [list(map(tuple, x)) for x in w[6]], "groups"
    for name, x, y in zip(("seq", "hap", "baseq", "mapq"), g[2:6], w[2:6]):
        assert x.shape == y.shape and x.dtype == np.int32 and np.array_equal(x, y), name
