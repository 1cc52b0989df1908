"""Final call-set merge (stage s6) and stage-4 group selection, host side.

    merge_calls      scripts/merge.py:15-145   pileup.vcf + haplotype.csv -> final VCF
    select_groups    HaplotypeModel/select_hetesnp_homosnp.py:75-177  low-quality candidates + their
                     5 high-quality heterozygous neighbours each side

Text in, text out, as in the reference (these stages are not accelerable math); written as single
passes over arrays instead of per-row dictionaries.
"""
from __future__ import annotations

import bisect
import math

_CHROMOSOMES = [str(n) for n in range(1, 23)] + ["X", "Y"]
MAJOR_CONTIGS = ["chr" + c for c in _CHROMOSOMES] + _CHROMOSOMES            # UCSC names first, then Ensembl names (select_hetesnp_homosnp.py:14)

_INFO_HEADER = ('##INFO=<ID=P,Number=0,Type=Flag,Description="Result from pileup model">\n'
                '##INFO=<ID=H,Number=0,Type=Flag,Description="Result from haplotype model">\n')
_MIN_CALL_QUAL = 13.0        # scripts/merge.py:68,122: below it neither model's call is written


def haplotype_alleles(ref: str, pair: str):
    """The two genotype letters of a haplotype call (ACGT, D, I) against the site's reference base -> (ALT text, GT text), or None
    when the merged file holds no row for the site.  Decision table of scripts/merge.py:82-111:

        ref among the letters, both equal      -> None (homozygous reference)
        ref among the letters                  -> the other letter, 0/1
        both equal                             -> that letter, 1/1
        two different non-reference letters    -> both, sorted, 1/2
        then an indel letter in ALT ('D' is looked at before 'I'): one ALT allele -> None; two -> the other letter, 0/1"""
    first, second = pair[0], pair[1]
    if ref in pair:
        if first == second:
            return None
        alt, zygosity = pair.replace(ref, ""), "0/1"
    elif first == second:
        alt, zygosity = first, "1/1"
    else:
        alt, zygosity = ",".join(sorted(pair)), "1/2"
    for letter in "DI":
        if letter in alt:
            return (pair.replace(letter, ""), "0/1") if zygosity == "1/2" else None
    return alt, zygosity


def merge_calls(pileup_vcf_text: str, haplotype_csv_text: str, quality_threshold=15.0) -> str:
    """scripts/merge.py:15-145 as one pass with a decision per row.  A pileup row whose QUAL is at most the threshold is REPLACED by
    the haplotype model's call of the same site when that call has QUAL >= 13 (INFO 'H', or no row at all: haplotype_alleles);
    every other row stays as the pileup model wrote it (INFO 'P') provided it is a variant (FILTER != RefCall) whose QUAL is above
    the threshold or at least 13.  Byte-identical to the reference's output (tests/test_next_rows.py)."""
    calls = {}
    for record in haplotype_csv_text.splitlines():
        record = record.strip()
        if record:
            contig, position, letters, score = record.split("\t")
            calls[contig, position] = (letters, score)
    merged, header_pending = [], True
    for raw in pileup_vcf_text.splitlines(keepends=True):
        if raw.startswith("#"):
            merged.append(raw)
            if header_pending:
                merged.append(_INFO_HEADER)
                header_pending = False
            continue
        col = raw.strip().split("\t")
        position, pileup_qual = int(col[1]), float(col[5])
        sample = col[-1].split(":")
        depth, allele_frequency = int(sample[-2]), float(sample[-1])
        variant = col[6] != "RefCall"
        hap = calls.get((col[0], str(position))) if pileup_qual <= quality_threshold else None
        hap_qual = float(hap[1]) if hap is not None else None
        if hap is not None and hap_qual >= _MIN_CALL_QUAL:
            decided = haplotype_alleles(col[3], hap[0])
            if decided is not None:
                alt, zygosity = decided
                merged.append(f"{col[0]}\t{position}\t.\t{col[3]}\t{alt}\t{hap_qual}\tPASS\tH\tGT:GQ:DP:AF\t"
                              f"{zygosity}:{int(hap_qual)}:{depth:d}:{allele_frequency:f}\n")
        elif variant and (pileup_qual > quality_threshold or pileup_qual >= _MIN_CALL_QUAL):
            col[7] = "P"
            merged.append("\t".join(col) + "\n")
    return "".join(merged)


def parse_vcf_for_groups(vcf_text: str, quality_threshold):
    """select_hetesnp_homosnp.py:82-104: {contig: {pos: (genotype, quality)}} without the confident
    homozygous calls"""
    contigs = {}
    for row in vcf_text.splitlines():
        if not row or row[0] == "#":
            continue
        c = row.strip().split()
        genotype = c[9].split(":")[0].replace("|", "/")
        quality = float(c[5])
        if genotype in ("0/0", "1/1") and quality >= quality_threshold:
            continue
        contigs.setdefault(c[0], {})[int(c[1])] = (genotype, quality)
    return contigs


def select_groups(vcf_text: str, quality_threshold=19.0, adjacent_size=5, support_quality=14.0, nthreads=10,
                  reference_bug=True):
    """{contig: [[(pos, genotype, quality)] * (2*adjacent_size+1)]}: every site with quality < threshold
    together with its adjacent_size nearest heterozygous ('0/1') sites of quality >= support_quality on
    each side (select_hetesnp_homosnp.py:180-230; thresholds of scripts/s4...sh:57-65).

    reference_bug=True reproduces find_adjacent_sites storing its result after the contig loop
    (:226, one indentation level too shallow): of every chunk of ceil(n_contigs / nthreads) contigs only
    the LAST contig's groups survive.  With False every contig is kept."""
    contigs = parse_vcf_for_groups(vcf_text, quality_threshold)
    order = MAJOR_CONTIGS + list(contigs.keys())
    names = sorted(contigs.keys(), key=lambda x: order.index(x))
    step = math.ceil(len(names) / nthreads) if names else 1
    chunks = [names[i:i + step] for i in range(0, len(names), step)]
    groups = {}
    for chunk in chunks:
        for ci, contig in enumerate(chunk):
            d = contigs[contig]
            all_pos = sorted(d)
            het_idx = [i for i, p in enumerate(all_pos) if d[p][1] >= support_quality and d[p][0] == "0/1"]
            ctg_groups = []
            for i, p in enumerate(all_pos):
                if not d[p][1] < quality_threshold:
                    continue
                k = bisect.bisect_left(het_idx, i)                    # supports strictly left of i: het_idx[:k]
                left = het_idx[max(0, k - adjacent_size):k]
                k2 = bisect.bisect_right(het_idx, i)
                right = het_idx[k2:k2 + adjacent_size]
                if len(left) != adjacent_size or len(right) != adjacent_size:
                    continue
                ctg_groups.append([(all_pos[j], d[all_pos[j]][0], d[all_pos[j]][1]) for j in left + [i] + right])
            if not reference_bug or ci == len(chunk) - 1:
                groups[contig] = ctg_groups
    return groups


# ---- the same selection from the call rows, on the device (csrc/pileup_groups.hip) ---------------------------------------------------
_ONE_BITS, _INF_BITS, _HALF_BITS = 0x3F800000, 0x7F800000, 0x3F000000


def _f32_of_bits(bits):
    import numpy as np
    return np.array([bits], np.uint32).view(np.float32)[0]


def _first_true(lo, hi, pred):
    """the smallest b in [lo, hi] with pred(b), for a pred that is False up to some b and True from there on; hi + 1 when none"""
    if not pred(hi):
        return hi + 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def group_cuts(quality_threshold=19.0, support_quality=14.0, score_mode=None):
    """The thresholds of select_groups as probabilities, float32 [8] for nsnp_pileup_select_groups: a QUAL is round(score, 2) of a
    monotone function of the float32 probability p, so `QUAL >= T` is `p >= p_cut(T)` for one float32 p_cut - found here by bisection
    over the bit patterns of the non-negative floats with host.calculate_score, the library's own scoring function, which is also
    what writes the QUAL text.  The device then compares bit patterns and needs no logarithm.
        [0] p_cut(quality_threshold)   [1] p_cut(support_quality)      (+inf where no probability reaches the threshold)
        [2] the first and [3] the last probability that has a score (the two modes differ at p == 1: skipped under SCORE_FLOAT32, 3010.3
        under SCORE_FLOAT64)           [4] 1.0 when -0.0 scores as 0.0 does (SCORE_FLOAT64 adds 1e-300 to it), else 0.0      [5:8] 0"""
    import numpy as np
    from . import host
    mode = host.SCORE_FLOAT64 if score_mode is None else int(score_mode)
    score = lambda bits: host.calculate_score(_f32_of_bits(bits), mode)
    has = lambda bits: score(bits)[1]
    if not has(_HALF_BITS):
        raise ValueError("group_cuts: p = 0.5 has no score")
    lo = _first_true(0, _HALF_BITS, has)
    hi = _first_true(_HALF_BITS, _INF_BITS, lambda b: not has(b)) - 1
    out = np.zeros(8, np.uint32)
    for slot, t in enumerate((float(quality_threshold), float(support_quality))):
        cut = _first_true(lo, hi, lambda b: score(b)[0] >= t)
        out[slot] = cut if cut <= hi else _INF_BITS
    out[2], out[3] = lo, hi
    neg_zero = host.calculate_score(np.float32(-0.0), mode)
    if neg_zero[1]:
        if lo != 0 or neg_zero[0] != score(0)[0]:
            raise ValueError("group_cuts: -0.0 has a score of its own")
        out[4] = _ONE_BITS
    return out.view(np.float32)


def _listed_contigs(entered, nthreads, reference_bug):
    """the contigs select_groups reports, in its order, of those that have a dictionary entry (given in text order): sorted as
    MAJOR_CONTIGS lists them, the others behind in text order; with reference_bug only the last of every chunk of
    ceil(n / nthreads) survives"""
    order = MAJOR_CONTIGS + list(entered)
    ordered = sorted(entered, key=order.index)
    step = math.ceil(len(ordered) / nthreads) if ordered else 1
    return [c for i, c in enumerate(ordered) if not reference_bug or (i + 1) % step == 0 or i == len(ordered) - 1]


class DeviceGroups:
    """The groups of select_groups_rows, on the device: `rows` int32 [G, 2A+1] the index of every member among the call rows the
    selection ran over, `keys` int64 [G, 2A+1] their column 0 ((contig index << 36) | position, or a position), groups in row order
    - so every contig's groups are one slice -, with `names` the contig table the keys index.  The device reports every contig;
    `listed` are the contigs select_groups would report, in its order (those with a dictionary entry, after reference_bug / nthreads);
    `contig(name)` slices; `to_lists()` gives select_groups' structure."""

    def __init__(self, rows, keys, names, spans, entered, calls, ref, score_mode, nthreads=10, reference_bug=False):
        self.rows, self.keys, self.names = rows, keys, list(names)
        self.spans = dict(spans)              # contig name -> (first group, end) for every contig that has rows
        self.entered = list(entered)          # the contigs with a dictionary entry, in text order
        self.calls, self.ref = calls, ref     # [G, 2A+1, 4] float64 columns 1..4 and [G, 2A+1] uint8 reference bytes of the members
        self.score_mode, self.nthreads, self.reference_bug = score_mode, nthreads, reference_bug

    def __len__(self):
        return int(self.rows.shape[0])

    @property
    def adjacent_size(self):
        return (int(self.rows.shape[1]) - 1) // 2

    @property
    def listed(self):
        return _listed_contigs(self.entered, self.nthreads, self.reference_bug)

    def contig(self, name):
        """the groups of one contig (none for a contig without rows), listed alone when it has a dictionary entry"""
        a, b = self.spans.get(name, (0, 0))
        return DeviceGroups(self.rows[a:b], self.keys[a:b], self.names, {name: (0, b - a)}, [name] if name in self.entered else [],
                            self.calls[a:b], self.ref[a:b], self.score_mode)

    @staticmethod
    def empty(names, adjacent_size, device, score_mode):
        """no rows, so no groups and no contig with an entry"""
        import torch
        w = 2 * int(adjacent_size) + 1
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        return DeviceGroups(mk((0, w), torch.int32), mk((0, w), torch.int64), names, {}, [], mk((0, w, 4), torch.float64), mk((0, w), torch.uint8),
                            score_mode)

    @staticmethod
    def concat(parts, row_offsets, nthreads=10, reference_bug=False):
        """the groups of consecutive pieces of one list of call rows (piece i begins at row row_offsets[i]; no contig lies in two),
        reference_bug / nthreads applied to the whole list"""
        import torch
        spans, entered, at = {}, [], 0
        for p in parts:
            for n, (a, b) in p.spans.items():
                if n in spans:
                    raise ValueError(f"DeviceGroups.concat: {n} is in two pieces")
                spans[n] = (at + a, at + b)
            entered += p.entered
            at += len(p)
        cat = lambda k: torch.cat([getattr(p, k) for p in parts])
        rows = torch.cat([p.rows + int(o) for p, o in zip(parts, row_offsets)])
        return DeviceGroups(rows, cat("keys"), parts[0].names, spans, entered, cat("calls"), cat("ref"), parts[0].score_mode, nthreads,
                            reference_bug)

    def to_lists(self, rows_host=None):
        """{contig: [[(pos, genotype, quality)] * (2A+1)]} exactly as select_groups returns it for the VCF text of the same rows.
        rows_host (optional): the [N,13] call rows in host memory - their columns 1..4 are then used instead of the copies taken
        at the selection.  Genotype and quality of the selected sites - and of no others - are read from the text the library's row
        writer (host.vcf_format_batches) makes of them."""
        import numpy as np
        from . import host
        from ._lib import NanoSNPError
        w = int(self.rows.shape[1])
        idx = self.rows.cpu().numpy().astype(np.int64).reshape(-1)
        pos = (self.keys.cpu().numpy().reshape(-1) & ((1 << 36) - 1)).tolist()
        ref = self.ref.cpu().numpy().reshape(-1)
        if rows_host is not None:
            calls = np.asarray(rows_host.cpu() if hasattr(rows_host, "cpu") else rows_host, np.float64)[idx, 1:5]
        else:
            calls = self.calls.cpu().numpy().reshape(-1, 4)
        uniq, first, inverse = np.unique(idx, return_index=True, return_inverse=True)
        sites = calls[first]
        n = int(uniq.size)
        pad = np.concatenate([np.arange(n), np.zeros(max(0, 10 - n), np.int64)]) if n else np.zeros(0, np.int64)      # (a batch of ten or more rows: the writer skips none)
        text, written = host.vcf_format_batches(host.ContigTable(["c"]), np.zeros(pad.size, np.int32), np.zeros(pad.size, np.int64),
                                                ref[first][pad] & 0xDF, sites[pad, 0].astype(np.uint8), sites[pad, 1].astype(np.uint8),
                                                sites[pad, 2].astype(np.float32), sites[pad, 3].astype(np.float32),
                                                np.zeros((pad.size, 8), np.float32), batch_size=max(pad.size, 10), score_mode=self.score_mode,
                                                nthreads=1)
        if written != pad.size:
            raise NanoSNPError("DeviceGroups.to_lists: a selected site has no VCF row (the rows are not those the groups were selected from)")
        called = []
        for line in text.decode().splitlines()[:n]:
            c = line.split("\t")
            called.append((c[9].split(":")[0], float(c[5])))
        members = [(pos[j], *called[inverse[j]]) for j in range(idx.size)]
        return {name: [members[g * w:(g + 1) * w] for g in range(*self.spans[name])] for name in self.listed}


def select_groups_rows(ctx, rows, ref_base, names, *, quality_threshold=19.0, adjacent_size=5, support_quality=14.0, batch_size=1000,
                       score_mode=None, nthreads=10, reference_bug=True, stream=None):
    """select_groups without the VCF text: rows float64 cuda [N,13], the call rows of whole contigs in text order (pileup_call_rows:
    column 0 a key (index into `names` << 36) | position, or a bare position of names[0]); ref_base uint8 cuda [N], the reference byte
    of every row.  -> DeviceGroups, equal (to_lists) to select_groups on the text host.vcf_format_batches makes of the same rows with
    the batches of batch_size restarting at every contig.  One launch sequence of nsnp_pileup_select_groups (a second one with the right
    capacity when the groups exceed the first guess) and one host visit for its counts.
    NanoSNPError: a contig in two runs; a column 0 that does not ascend strictly inside a contig (select_groups keeps the last row of a
    repeated position; here it is refused, the row named).  NotImplementedError under a process group of more than one rank."""
    import numpy as np
    import torch
    import torch.distributed as tdist
    from . import host
    from ._lib import KEY_SHIFT, NanoSNPError
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("select_groups_rows: sharding the call rows over ranks")
    mode = host.SCORE_FLOAT64 if score_mode is None else int(score_mode)
    a, n, dev = int(adjacent_size), int(rows.shape[0]), rows.device
    names = list(names)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        rows = rows.contiguous()
        cid = rows[:, 0].to(torch.int64) >> KEY_SHIFT
        edges = torch.nonzero(cid[1:] != cid[:-1]).reshape(-1) + 1 if n else torch.zeros(0, dtype=torch.int64, device=dev)
        run_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), edges, torch.full((1,), n, dtype=torch.int64, device=dev)]) if n \
            else torch.zeros(1, dtype=torch.int64, device=dev)
        run_cid = cid[run_off[:-1]].tolist()
        if len(set(run_cid)) != len(run_cid):
            raise NanoSNPError("select_groups_rows: the rows of one contig come in two separate runs")
        if any(c < 0 or c >= len(names) for c in run_cid):
            raise NanoSNPError("select_groups_rows: a key names a contig outside `names`")
        cuts = torch.from_numpy(group_cuts(quality_threshold, support_quality, mode)).to(dev)
        ref_base = ref_base.contiguous()
        cap = min(n, max(1024, n // 8))
        for _ in range(2):
            g_rows, g_keys, meta, flags = ctx.pileup_select_groups(rows, ref_base, run_off, cuts, adjacent_size=a, batch_size=batch_size,
                                                                   cap_groups=cap, stream=stream)
            found, status, bad_row, _ = meta.tolist()
            if status:
                raise NanoSNPError(f"select_groups_rows: column 0 of row {bad_row} is not above that of the row in front of it in the same contig "
                                   "(positions must ascend strictly)")
            if found <= cap:
                break
            cap = found
        g_rows, g_keys = g_rows[:found], g_keys[:found]
        flat = g_rows.reshape(-1).to(torch.int64)
        calls = rows[flat, 1:5].reshape(found, 2 * a + 1, 4)
        ref = ref_base[flat].reshape(found, 2 * a + 1)
        # per contig: its slice of the groups (they are in row order) and whether any of its rows is in the dictionary
        in_dict = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((flags & ctx.GROUPS_DICT) != 0, 0)])[run_off]
        has_entry = (in_dict[1:] > in_dict[:-1]).tolist() if n else []
        cuts_at = torch.searchsorted(g_rows[:, a].contiguous().to(torch.int64), run_off).tolist() if n else [0]
    spans = {names[c]: (cuts_at[r], cuts_at[r + 1]) for r, c in enumerate(run_cid)}
    entered = [names[c] for r, c in enumerate(run_cid) if has_entry[r]]
    return DeviceGroups(g_rows, g_keys, names, spans, entered, calls, ref, mode, nthreads, reference_bug)
