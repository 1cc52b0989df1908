"""The training-label rules of the reference restated with numpy and plain Python, independent of nanosnp_amd.truth and of the device
code: what DNA_SplitVcf + load_true_variants / output_labels_from_vcf_columns make of a truth VCF (split_vcf/main.cpp:14-126,
common/genotype.cpp:179-353), the label of every candidate site (make_train_data/main.cpp:287-317), the subsample arithmetic
(make_train_data/main.cpp:161-164) and the seeded keep rule of nsnp_pileup_label_sites_keys.  The fixtures' generator checks these rules
against the reference's own programs; the tests check the library against them."""
import numpy as np

KEY_SHIFT = 36
GT21 = "AA AC AG AT CC CG CT GG GT TT DelDel ADel CDel GDel TDel InsIns AIns CIns GIns TIns InsDel".split()
REF_GT21 = {65: 0, 67: 4, 71: 7, 84: 9}                      # A C G T


def c_atoi(s):
    s = s.lstrip(" \t\n\v\f\r")
    n = 0
    if s[:1] in ("+", "-"):
        n = 1
    while n < len(s) and s[n].isdigit() and s[n].isascii():
        n += 1
    try:
        return int(s[:n])
    except ValueError:
        return 0


def true_var_rows(vcf_text):
    """the rows of every <contig>.true_var: [(contig, pos text, ref, alt, gt1, gt2)] in the order of the text"""
    rows = []
    for line in vcf_text.split("\n"):
        if line == "" or line.startswith("#"):
            continue
        cols = [c for c in line.split("\t") if c != ""]
        gts = cols[-1].split(":")[0].replace("/", "|").replace(".", "0")
        assert "|" in gts, line
        g = sorted((c_atoi(gts), c_atoi(gts[gts.index("|") + 1:])))
        alt = cols[4]
        if "*" in alt:
            if sum(g) != 3 or alt.count(",") != 1:
                continue
            g, alt = [0, 1], "".join(ch for ch in alt if ch != "*")
        rows.append((cols[0], cols[1], cols[3], alt, g[0], g[1]))
    return rows


def row_label(ref, alt, gt1, gt2):
    """-> (gt21, zygosity, length index 1, length index 2) of one .true_var row"""
    alleles = [a for a in alt.split(",") if a != ""]
    if len(alleles) == 1:
        alleles = [ref, alt] if 0 in (gt1, gt2) else [alt, alt]
    part = ["Del" if len(ref) > len(a) else "Ins" if len(ref) < len(a) else a[0] for a in alleles[:2]]
    singles = sorted(p for p in part if len(p) == 1)
    longs = [p for p in part if len(p) > 1]
    if len(singles) == 2:
        name = singles[0] + singles[1]
    elif len(singles) == 1:
        name = singles[0] + longs[0]
    else:
        name = longs[0] * 2 if longs[0] == longs[1] else "InsDel"
    zy = 0 if gt1 == 0 and gt2 == 0 else 1 if gt1 == gt2 else 2
    length = [min(max(len(a) - len(ref), 16), 16) + 16 for a in alleles]          # VariantLength.min == max == 16
    return GT21.index(name), zy, sorted(length)[0], sorted(length)[1]


def truth_table(vcf_text, names):
    """-> {key: (gt21, zygosity, l1, l2)} over the contigs of `names`, key = index << 36 | pos"""
    out = {}
    for contig, pos, ref, alt, g1, g2 in true_var_rows(vcf_text):
        if contig in names:
            key = names.index(contig) << KEY_SHIFT | int(pos)
            assert key not in out, (contig, pos)
            out[key] = row_label(ref, alt, g1, g2)
    return out


def one_hot(quads):
    """[(gt21, zy, l1, l2)] -> int32 [n, 90]: column c is 1 where c is one of gt21, 21 + zy, 24 + l1, 57 + l2.  (A truth VCF gives
    gt21 < 21, zy < 3 and lengths < 33; the packed code has room for more, and a column beyond 89 does not exist.)"""
    y = np.zeros((len(quads), 90), np.int32)
    for i, (gt, zy, l1, l2) in enumerate(quads):
        y[i, [c for c in (gt, 21 + zy, 24 + l1, 57 + l2) if c < 90]] = 1
    return y


def site_quads(keys, ref_bases, truth):
    """keys int64 [n], ref_bases uint8 [n] (the FASTA's byte at the site), truth from truth_table -> ([(gt21, zy, l1, l2)], is_truth bool [n])"""
    quads, hit = [], np.zeros(len(keys), bool)
    for i, (k, b) in enumerate(zip(np.asarray(keys).tolist(), np.asarray(ref_bases).tolist())):
        if k in truth:
            quads.append(truth[k]); hit[i] = True
        else:
            quads.append((REF_GT21[b & ~0x20], 0, 16, 16))
    return quads, hit


def key_hash(keys, seed):
    """the splitmix64 finaliser of key + seed * 0x9E3779B97F4A7C15 (mod 2^64), per key"""
    mask = (1 << 64) - 1
    out = []
    for k in np.asarray(keys, np.int64).tolist():
        z = (k + seed * 0x9E3779B97F4A7C15) & mask
        z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & mask
        z ^= z >> 27; z = z * 0x94D049BB133111EB & mask
        z ^= z >> 31
        out.append(z)
    return out


def threshold(variants, non_variants, ratio):
    """-> (thr or None when the contig is not subsampled, the reference's subsample_ratio)"""
    max_nv = int(variants * ratio)                           # (C truncation of a non-negative double)
    if max_nv < non_variants:
        return (max_nv << 53) // non_variants, 1.0 * max_nv / non_variants
    return None, 1.0


def kept_mask(keys, is_truth, thr_of_cid, seed):
    """thr_of_cid: {contig index: thr or None} -> bool [n]: the sites nsnp_pileup_label_sites_keys keeps"""
    keys = np.asarray(keys, np.int64)
    keep = np.array(is_truth, bool).copy()
    for i, (k, h) in enumerate(zip(keys.tolist(), key_hash(keys, seed))):
        thr = thr_of_cid.get(k >> KEY_SHIFT)
        if thr is None or (h >> 11) < thr:
            keep[i] = True
    return keep


def parse_td(td_text):
    """.td text -> (keys text list 'ctg:pos', label int32 [n, 90], has a truth column bool [n])"""
    names, labels, truth = [], [], []
    for line in td_text.split("\n"):
        if not line.strip():
            continue
        cols = line.split("\t")
        labels.append(np.array(cols[1].split(), np.int32))
        names.append(cols[2].rsplit(":", 1)[0])
        truth.append(len(cols) > 4)
    return names, (np.stack(labels) if labels else np.zeros((0, 90), np.int32)), np.array(truth, bool)
