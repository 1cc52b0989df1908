"""The truth VCF of a training run, read on the host: what the reference's DNA_SplitVcf (dna_sv_tensor/src/split_vcf/main.cpp:14-126) writes
into <chr>.true_var, and what DNA_CreateTrainData makes of those rows (make_train_data/main.cpp:94-127: load_true_variants,
common/genotype.cpp:179-353: output_labels_from_vcf_columns) - one 90-value label per truth variant, kept here as one packed code.

A code is ``gt21 | zygosity << 8 | length index 1 << 16 | length index 2 << 24`` (include/nanosnp.h: nsnp_pileup_label_sites_keys); the
one-hot label has its ones at gt21, 21 + zygosity, 24 + length index 1 and 57 + length index 2.  The quirks of the reference are kept:
see split_rows and label_code.
"""
from __future__ import annotations

import functools
import gzip
import os
import re

import numpy as np

KEY_SHIFT = 36                                               # _lib.KEY_SHIFT: key = contig index << 36 | position
LABEL_WIDTH = 90                                             # genotype.cpp:264-274: 21 + 3 + 33 + 33
GT21_LABELS = ("AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT", "DelDel", "ADel", "CDel", "GDel", "TDel", "InsIns", "AIns", "CIns",
               "GIns", "TIns", "InsDel")                     # genotype.cpp:12-34
_GT21 = {s: i for i, s in enumerate(GT21_LABELS)}
# VariantLength.min == VariantLength.max == 16 (genotype.cpp:36-43): every length of a truth variant is clamped to 16 and lands on index
# 16 + 16; a reference-labelled site has index 0 + 16 (output_labels_from_reference)
LENGTH_INDEX_TRUTH, LENGTH_INDEX_REFERENCE = 32, 16
REFERENCE_GT21 = {"A": 0, "C": 4, "G": 7, "T": 9}

_ATOI = re.compile(rb"[ \t\n\v\f\r]*([+-]?[0-9]+)")
_POS = re.compile(rb"(?:0|[1-9][0-9]*)\Z")


def _atoi(b):
    m = _ATOI.match(b)
    return int(m.group(1)) if m else 0


def _tokens(b, sep):
    """split_line (common/cpp_aux.cpp:44-59): the non-empty tokens between the delimiters"""
    return [t for t in b.split(sep) if t]


def pack_code(gt21, zygosity, length_1, length_2):
    return int(gt21) | int(zygosity) << 8 | int(length_1) << 16 | int(length_2) << 24


def unpack_codes(codes):
    """uint32 codes -> (gt21, zygosity, length index 1, length index 2) as int64 arrays"""
    c = np.asarray(codes).astype(np.int64)
    return c & 0x1f, (c >> 8) & 3, (c >> 16) & 0x3f, (c >> 24) & 0x3f


def labels_of(codes):
    """uint32 codes [n] -> the one-hot labels int32 [n, 90]"""
    gt, zy, l1, l2 = unpack_codes(codes)
    out = np.zeros((gt.size, LABEL_WIDTH), np.int32)
    rows = np.arange(gt.size)
    for col in (gt, 21 + zy, 24 + l1, 57 + l2):
        out[rows, col] = 1
    return out


def reference_code(base):
    """the code of a site no truth row names, by its upper-cased reference base (output_labels_from_reference)"""
    return pack_code(REFERENCE_GT21[base], 0, LENGTH_INDEX_REFERENCE, LENGTH_INDEX_REFERENCE)


def genotype_of(last_column, row=b""):
    """extract_genotype (split_vcf/main.cpp:14-26): the text of the LAST column in front of its first ':', '/' read as '|' and '.' as '0',
    the two atoi values as (min, max) - so './.' is 0 0.  A text without a separator makes the reference assert: ValueError."""
    gts = last_column.split(b":", 1)[0].replace(b"/", b"|").replace(b".", b"0")
    bar = gts.find(b"|")
    if bar < 0:
        raise ValueError(f"truth VCF: a genotype without '/' or '|' in the last column of {row[:200]!r}")
    t1, t2 = _atoi(gts), _atoi(gts[bar + 1:])
    return min(t1, t2), max(t1, t2)


def fix_alternate(alt, gt1, gt2):
    """fix_alternate (split_vcf/main.cpp:28-49) -> (alt, gt1, gt2), or None for a row the splitter skips: an ALT holding '*' needs
    gt1 + gt2 == 3 and exactly one comma; then the genotype becomes 0 1 and every '*' is removed - the comma STAYS ('G,*' -> 'G,')."""
    if b"*" not in alt:
        return alt, gt1, gt2
    if gt1 + gt2 != 3 or alt.count(b",") != 1:
        return None
    return alt.replace(b"*", b""), 0, 1


def split_rows(vcf_bytes, contigs=None):
    """The rows DNA_SplitVcf writes, in the order of the text: (contig, POS text, REF, ALT, gt1, gt2, the VCF line) - the six columns of
    <contig>.true_var plus the line itself.  Lines that are empty or start with '#' are passed over; contigs (a container of names as
    bytes; None: all): a line of another contig is passed over before anything else of it is read."""
    for line in bytes(vcf_bytes).split(b"\n"):
        if not line or line[:1] == b"#":
            continue
        cols = _tokens(line, b"\t")
        if contigs is not None and (not cols or cols[0] not in contigs):
            continue
        if len(cols) < 5:
            raise ValueError(f"truth VCF: fewer than five columns in {line[:200]!r}")
        gt1, gt2 = genotype_of(cols[-1], line)
        fixed = fix_alternate(cols[4], gt1, gt2)
        if fixed is None:
            continue
        yield (cols[0], cols[1], cols[3], *fixed, line)


def true_var_text(vcf_bytes, contig):
    """<contig>.true_var as the splitter writes it"""
    name = contig.encode() if isinstance(contig, str) else bytes(contig)
    return b"".join(b"%s\t%s\t%s\t%s\t%d\t%d\n" % (c, p, r, a, g1, g2) for c, p, r, a, g1, g2, _ in split_rows(vcf_bytes, (name,)))


def _partial(ref, alt):
    """partial_label_from (genotype.cpp:179-191)"""
    if len(ref) > len(alt):
        return "Del"
    if len(ref) < len(alt):
        return "Ins"
    return alt[:1].decode("latin-1")


def _mix(a, b):
    """mix_two_partial_labels (genotype.cpp:193-227)"""
    if len(a) == 1 and len(b) == 1:
        return a + b if a <= b else b + a
    if len(a) > 1 and len(b) == 1:
        a, b = b, a
    if len(b) > 1 and len(a) == 1:
        return a + b
    if a and b and a == b:
        return a + b
    return "InsDel"


@functools.lru_cache(maxsize=1 << 16)
def label_code(ref, alt, gt1, gt2):
    """output_labels_from_vcf_columns (genotype.cpp:306-353) of one .true_var row, as a packed code.  ALT is cut at its commas (empty
    pieces dropped); a single piece pairs the WHOLE ALT text - a comma left by fix_alternate included - with REF when a genotype is 0 and
    with itself otherwise; more pieces: the first two.  A pair that is no gt21 label aborts the reference: ValueError."""
    arr = _tokens(alt, b",")
    if len(arr) == 1:
        arr = [ref, alt] if (gt1 == 0 or gt2 == 0) else [alt, alt]
    if len(arr) < 2:
        raise ValueError(f"no allele in ALT {alt!r}")
    name = _mix(_partial(ref, arr[0]), _partial(ref, arr[1]))
    if name not in _GT21:
        raise ValueError(f"REF {ref!r} ALT {alt!r} gives {name!r}, which is no gt21 label")
    zygosity = 0 if (gt1 == 0 and gt2 == 0) else 1 if gt1 == gt2 else 2     # (genotype_enum_for_task: 1/2 counts as heterozygous)
    return pack_code(_GT21[name], zygosity, LENGTH_INDEX_TRUTH, LENGTH_INDEX_TRUTH)


def read_vcf(vcf_path_or_bytes):
    if isinstance(vcf_path_or_bytes, (str, os.PathLike)):
        with open(vcf_path_or_bytes, "rb") as f:
            data = f.read()
    else:
        data = bytes(vcf_path_or_bytes)
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


def load_truth(vcf_path_or_bytes, table):
    """The truth table of pipeline.mpileup_to_train_bins.  vcf_path_or_bytes: a path (plain or gzip) or the bytes of a VCF; table: a
    _lib.ContigTable, or the list of its names -> (keys int64 [T] ascending: contig index << 36 | POS, codes uint32 [T] in the same order,
    counts int64 [n_contigs]: the truth variants of every contig - Y.size() of the reference's log).
    A row of a contig outside the table is passed over.  ValueError: a genotype without separator, a pair that is no gt21 label, a POS that
    is not canonical decimal below 2^36, a key that occurs twice (the reference asserts or aborts on each of them)."""
    names = [str(n) for n in getattr(table, "names", table)]
    index = {n.encode(): i for i, n in enumerate(names)}
    keys, codes = [], []
    for contig, pos, ref, alt, gt1, gt2, line in split_rows(read_vcf(vcf_path_or_bytes), index):
        if not _POS.match(pos) or int(pos) >= 1 << KEY_SHIFT:
            raise ValueError(f"truth VCF: POS {pos[:40]!r} is not a canonical decimal number below 2^{KEY_SHIFT} in {line[:200]!r}")
        try:
            code = label_code(ref, alt, gt1, gt2)
        except ValueError as e:
            raise ValueError(f"truth VCF: {e} in {line[:200]!r}") from None
        keys.append(index[contig] << KEY_SHIFT | int(pos))
        codes.append(code)
    keys, codes = np.array(keys, np.int64), np.array(codes, np.uint32)
    order = np.argsort(keys, kind="stable")
    keys, codes = keys[order], codes[order]
    twice = np.flatnonzero(keys[1:] == keys[:-1])
    if twice.size:
        k = int(keys[twice[0]])
        raise ValueError(f"truth VCF: {names[k >> KEY_SHIFT]}:{k & ((1 << KEY_SHIFT) - 1)} occurs twice")
    return keys, codes, np.bincount(keys >> KEY_SHIFT, minlength=len(names)).astype(np.int64)


def keep_thresholds(variants, non_variants, max_non_variant_ratio):
    """calc_non_variant_subsample_ratio (make_train_data/main.cpp:161-164) per contig, as the integer thresholds of
    nsnp_pileup_label_sites_keys: max_nv = int(variants * ratio) with C truncation; a contig is subsampled only when max_nv < non_variants,
    then with thr = (max_nv << 53) // non_variants (a site is kept when hash >> 11 < thr).  -> (thr: list of Python ints - 1 << 53 keeps
    everything -, ratio: list of floats, the reference's subsample_ratio)"""
    thr, ratio = [], []
    for v, nv in zip(variants, non_variants):
        v, nv = int(v), int(nv)
        max_nv = int(v * float(max_non_variant_ratio))
        if max_nv < nv:
            thr.append((max_nv << 53) // nv)
            ratio.append(1.0 * max_nv / nv)
        else:
            thr.append(1 << 53)
            ratio.append(1.0)
    return thr, ratio


# ---- HaplotypeModel: the per-contig truth table of get_truth.py and the label rows of make_train_bins.py ----------------------------
class ContigTruth:
    """One contig of get_truth.get_truth_variants (HaplotypeModel/get_truth.py:258-277), compact: the reference bytes (the non-variant
    gt21 is a function of them), the confident marks as a bitmap (np.packbits, bit n = base index n) and the truth rows that landed on a
    marked base as a sparse map - sorted 0-based indices with their gt21 and zygosity.  The reference keeps float64 [len, 3]."""
    __slots__ = ("ref", "confident", "index", "gt21", "zygosity")

    def __init__(self, ref):
        self.ref = np.frombuffer(bytes(ref), np.uint8)
        self.confident = np.zeros((self.ref.size + 7) // 8, np.uint8)
        self.index, self.gt21, self.zygosity = np.empty(0, np.int64), np.empty(0, np.int32), np.empty(0, np.int32)

    def __len__(self):
        return int(self.ref.size)

    def marked(self, idx):
        idx = np.asarray(idx, np.int64)
        return (self.confident[idx >> 3] >> (7 - (idx & 7)).astype(np.uint8)) & 1


_NONVARIANT_GT21 = np.arange(256, dtype=np.int32)            # get_truth.py:267-270,273: A/a 0, C/c 4, G/g 7, T/t 9, any other byte its code
for _b, _v in ((65, 0), (97, 0), (67, 4), (99, 4), (71, 7), (103, 7), (84, 9), (116, 9)):
    _NONVARIANT_GT21[_b] = _v


def _wrapped(i, n, what, line):
    """index i of a numpy array of n rows as numpy reads it: [-n, -1] wraps round, anything else outside [0, n) raises"""
    from ._lib import NanoSNPError
    if i < -n or i >= n:
        raise NanoSNPError(f"{what}: base index {i} outside a contig of {n} bases in {line[:200]!r}")
    return i + n if i < 0 else i


def haplotype_vcf_labels(columns, line=""):
    """output_labels_from_vcf_columns (get_truth.py:219-239) of the tab-separated columns (str) of a VCF row -> (gt21, zygosity).  The
    genotype is the LAST column in front of its first ':', '/' read as '|': exactly two integers (no '.', unlike the PileupModel's
    splitter).  One ALT pairs with REF when a genotype is 0 and with itself otherwise; of more ALTs the first two count.  zygosity: 0/0 ->
    0, equal -> 1, anything else -> 2 (1/2 counts as heterozygous).  NanoSNPError where the reference raises."""
    from ._lib import NanoSNPError
    try:
        ref, alt = columns[3], columns[4]
        g1, g2 = [int(v) for v in columns[-1].split(":")[0].replace("/", "|").split("|")]
    except (ValueError, IndexError):
        raise NanoSNPError(f"truth VCF: fewer than five columns or a genotype that is not two integers in {line[:200]!r}") from None
    arr = alt.split(",")
    if len(arr) == 1:
        arr = [ref, alt] if (g1 == 0 or g2 == 0) else [alt, alt]
    parts = []
    for a in arr[:2]:
        if len(ref) == len(a) and not a:
            raise NanoSNPError(f"truth VCF: an empty allele in {line[:200]!r}")
        parts.append("Del" if len(ref) > len(a) else "Ins" if len(ref) < len(a) else a[0])
    name = _mix(parts[0], parts[1])
    if name not in _GT21:
        raise NanoSNPError(f"truth VCF: REF {ref!r} ALT {alt!r} gives {name!r}, which is no gt21 label, in {line[:200]!r}")
    return _GT21[name], 0 if (g1 == 0 and g2 == 0) else 1 if g1 == g2 else 2


def _text_lines(path_or_bytes):
    return read_vcf(path_or_bytes).decode("latin-1").split("\n")


def haplotype_truth_table(reference, confident_bed, truth_vcf, contigs=None):
    """get_truth.get_truth_variants (HaplotypeModel/get_truth.py:258-277) -> {contig: ContigTruth}.

    reference: a FASTA path (read as host.load_reference_file does; with a ``.fai`` beside it the contigs and their lengths are the index's,
    get_truth.py:262-271) or a dict {contig: sequence}.  confident_bed, truth_vcf: paths (plain or gzip) or bytes.  contigs: keep only
    these (BED and VCF lines of other contigs are passed over); None: every contig of the reference.

    Quirks kept.  load_confident_bed (:118-126) marks 0-based index i - 1 for i in [start, end): a BED start is read as if it were 1-based,
    and a start of 0 marks index -1, which numpy reads as the contig's LAST base.  load_truth_vcf (:242-255) passes over a row whose base is
    not marked; a row on a marked base overwrites gt21 and zygosity, later rows win.  NanoSNPError with the line where the reference raises:
    a contig absent from the reference, a BED line that is not three tab-separated columns of which the last two are integers, an index
    outside the contig, a genotype that is not two integers, a pair of alleles that is no gt21 label."""
    from . import host
    from ._lib import NanoSNPError
    if isinstance(reference, dict):
        refs = {str(k): (v.encode() if isinstance(v, str) else bytes(v)) for k, v in reference.items()}
    else:
        refs = host.load_reference_file(reference)
        fai = f"{os.fspath(reference)}.fai"
        if os.path.exists(fai):
            with open(fai) as f:
                lens = {ln.strip().split("\t")[0]: int(ln.strip().split("\t")[1]) for ln in f if ln.strip()}
            for c, n in lens.items():
                if c not in refs or len(refs[c]) != n:
                    raise NanoSNPError(f"{fai}: contig {c!r} of {n} bases is not in the FASTA with that length")
            refs = {c: refs[c] for c in lens}
    if contigs is not None:
        want = [c if isinstance(c, str) else bytes(c).decode() for c in contigs]
        missing = [c for c in want if c not in refs]
        if missing:
            raise NanoSNPError(f"contigs {missing[:4]} are not in the reference")
        skip = set(refs) - set(want)
        refs = {c: refs[c] for c in want}
    else:
        skip = set()
    table = {c: ContigTruth(s) for c, s in refs.items()}
    for line in _text_lines(confident_bed):
        if not line:
            continue
        cols = line.strip().split("\t")
        if cols and cols[0] in skip:
            continue
        try:
            ctg, start, end = cols
            start, end = int(start), int(end)
        except ValueError:
            raise NanoSNPError(f"confident BED: not three tab-separated columns with two integers in {line[:200]!r}") from None
        if ctg not in table:
            raise NanoSNPError(f"confident BED: contig {ctg!r} is not in the reference, in {line[:200]!r}")
        t = table[ctg]
        if end > start:
            n = len(t)
            idx = np.arange(start - 1, end - 1, dtype=np.int64)
            if idx[0] < -n or idx[-1] >= n:
                _wrapped(int(idx[0]) if idx[0] < -n else int(idx[-1]), n, "confident BED", line)
            idx = np.where(idx < 0, idx + n, idx)
            np.bitwise_or.at(t.confident, idx >> 3, (np.uint8(128) >> (idx & 7).astype(np.uint8)))
    rows = {c: {} for c in table}
    for line in _text_lines(truth_vcf):
        if line.startswith("#") or not line:
            continue
        fields = line.strip().split("\t")
        if fields[0] in skip:
            continue
        if fields[0] not in table:
            raise NanoSNPError(f"truth VCF: contig {fields[0]!r} is not in the reference, in {line[:200]!r}")
        t = table[fields[0]]
        try:
            pos = int(fields[1])
        except (ValueError, IndexError):
            raise NanoSNPError(f"truth VCF: no integer POS in {line[:200]!r}") from None
        i = _wrapped(pos - 1, len(t), "truth VCF", line)
        if not t.marked(i):
            continue
        rows[fields[0]][i] = haplotype_vcf_labels(fields, line)
    for c, t in table.items():
        if rows[c]:
            t.index = np.array(sorted(rows[c]), np.int64)
            t.gt21 = np.array([rows[c][i][0] for i in t.index.tolist()], np.int32)
            t.zygosity = np.array([rows[c][i][1] for i in t.index.tolist()], np.int32)
    return table


def haplotype_label_rows(table, candidate_positions):
    """The candidate_labels of make_train_bins.py:123-127: per "ctg:pos" the row [pos - 1] of the contig's truth array -> int32 [N,3] =
    {confident, gt21, zygosity}.  A base no truth row overwrote has gt21 0 / 4 / 7 / 9 by its upper- or lower-case reference base, the
    byte's ASCII code otherwise, and zygosity -1.  pos 0 reads index -1, the LAST base, as numpy does there.  table: haplotype_truth_table's
    dict, or one ContigTruth for candidates of one contig (the reference hands one contig's array to its workers)."""
    from ._lib import NanoSNPError
    cand = [c if isinstance(c, str) else bytes(c).rstrip(b"\0").decode() for c in candidate_positions]
    out = np.empty((len(cand), 3), np.int32)
    by_ctg = {}
    for n, c in enumerate(cand):
        try:
            ctg, p = c.split(":")
            p = int(p)
        except ValueError:
            raise NanoSNPError(f"candidate position {c!r} is not 'ctg:pos'") from None
        by_ctg.setdefault(ctg, ([], []))
        by_ctg[ctg][0].append(n); by_ctg[ctg][1].append(p - 1)
    for ctg, (rows, idx) in by_ctg.items():
        if isinstance(table, ContigTruth):
            t = table
        elif ctg in table:
            t = table[ctg]
        else:
            raise NanoSNPError(f"candidate contig {ctg!r} is not in the truth table")
        n = len(t)
        idx = np.array(idx, np.int64)
        bad = np.flatnonzero((idx < -n) | (idx >= n))
        if bad.size:
            _wrapped(int(idx[bad[0]]), n, "candidate position", cand[rows[bad[0]]])
        idx = np.where(idx < 0, idx + n, idx)
        gt = _NONVARIANT_GT21[t.ref[idx]].copy()
        zy = np.full(idx.size, -1, np.int32)
        if t.index.size:
            k = np.minimum(np.searchsorted(t.index, idx), t.index.size - 1)
            hit = t.index[k] == idx
            gt[hit] = t.gt21[k[hit]]; zy[hit] = t.zygosity[k[hit]]
        out[rows, 0] = t.marked(idx); out[rows, 1] = gt; out[rows, 2] = zy
    return out
