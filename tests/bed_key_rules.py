"""The BED rules over SEVERAL contigs restated in numpy (test helper): a key = (contig index << 36) | position is tested against the bits
of its OWN contig - plain bool arrays built from the intervals by tests/bed_rules.py, never from the table's words - and the whole text of
the reference anchor: the two BED fixture families are different contigs (encode_g1 is chrS, encode_cut is chrC), so chrS text + lines of
an unlisted name + chrC text with the two BED files of a case concatenated is ONE whole-genome input whose expected sites are the union of
the two .pd fixtures the reference's programs wrote."""
from __future__ import annotations

import gzip

import numpy as np

from nanosnp_amd import bed, host
from tests import bed_rules
from tests import contig_rules as cr
from tests.helpers import golden

KEY_SHIFT = cr.KEY_SHIFT
FILLER = cr.FILLER
MASK = (1 << KEY_SHIFT) - 1
FAMILIES = (("g1", "chrS"), ("cut", "chrC"))
UNLISTED = b"chrU_unlisted"


def key_cid_pos(key):
    key = np.asarray(key, np.int64)
    return key >> KEY_SHIFT, key & MASK


def contig_bits(intervals, lengths):
    """[bool array per contig]: intervals = [int [n, 2] or None per contig]"""
    return [bed_rules.bit_array(np.zeros((0, 2), np.int64) if iv is None else iv, n) for iv, n in zip(intervals, lengths)]


def keep_keys(key, bits):
    """the extended rule for keys: cid in [0, n) and bit p - 1 of ITS contig set (outside the contig: 0)"""
    cid, p = key_cid_pos(key)
    keep = np.zeros(cid.size, bool)
    for c, b in enumerate(bits):
        m = cid == c
        keep[m] = bed_rules.extended_keep(p[m], b)
    return keep


def confident_keys(key, max_del, bits):
    """the confident rule for keys: a set bit in [p - 1, p + max_del + 1) of the key's OWN contig, clipped to it; no contig: False"""
    cid, p = key_cid_pos(key)
    ok = np.zeros(cid.size, bool)
    md = np.asarray(max_del, np.int64)
    for c, b in enumerate(bits):
        m = cid == c
        ok[m] = bed_rules.confident_pass(p[m], md[m], b)
    return ok


def words_bits(words, off, lengths):
    """what the table's layout says: [bool array per contig] of min(length, 32 * words) bits read from its own words, False beyond"""
    out = []
    for c, n in enumerate(lengths):
        w = np.asarray(words[int(off[c]):int(off[c + 1])], np.uint32)
        b = np.zeros(int(n), bool)
        k = min(int(n), 32 * w.size)
        if k:
            b[:k] = bed_rules.bits_from_words(w, k)
        out.append(b)
    return out


def _family(tag):
    text = gzip.open(golden(f"encode_{tag}.mpileup.gz")).read()
    fa = gzip.open(golden(f"encode_{tag}.fa.gz")).read()
    return text, np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8).copy()


def anchor(case):
    """case: "ext" / "conf" / "both" -> dict(whole text, texts {name: text}, seqs {name: seq}, names, ext / conf BED bytes or None (the two
    fixture files concatenated), want [(contig, position)] in text order, pds {name: the reference's .pd})"""
    texts, seqs, pds, want = {}, {}, {}, []
    beds = {"ext": b"", "conf": b""}
    for tag, name in FAMILIES:
        texts[name], seqs[name] = _family(tag)
        pds[name] = gzip.open(golden(f"bed_{tag}_{case}.pd.gz")).read()
        _, names, gpos, _ = host.pd_parse(pds[name])
        assert set(names) == {name}
        want += [(name, int(p)) for p in gpos]
        for kind in beds:
            if case in (kind, "both"):
                beds[kind] += open(golden(f"bed_{tag}_{case}.{kind}.bed"), "rb").read()
    s_lines = texts["chrS"].split(b"\n")[100:140]
    unlisted = b"".join(UNLISTED + l[l.index(b"\t"):] + b"\n" for l in s_lines)
    whole = texts["chrS"] + unlisted + texts["chrC"]
    return dict(whole=whole, texts=texts, seqs=seqs, names=[n for _, n in FAMILIES], pds=pds, want=want,
                ext=beds["ext"] or None, conf=beds["conf"] or None)


def numpy_sites(whole, names, seqs, ext_bed, conf_bed, fai=None):
    """the rules in numpy over one whole text: contig_rules.contig_rule finds every line's contig, every contig's lines (one run) go through
    bed_rules.reference_sites with the bits of ITS contig, read back from bed.table_bitmaps' layout -> ([(contig, position)], windows
    int32 [n, 33, 18]) in text order"""
    pos, col_off, bases = host.mpileup_parse(whole)
    lengths = [int(seqs[n].size) for n in names]
    cid, _, _, runs = cr.contig_rule(whole, [n.encode() for n in names], [seqs[n] for n in names], pos)
    tab = {}
    for kind, b in (("ext", ext_bed), ("conf", conf_bed)):
        tab[kind] = None if b is None else words_bits(*bed.table_bitmaps(b, names, lengths, fai), lengths)
    sites, xs = [], []
    ends = [int(r[0]) for r in runs[1:]] + [int(pos.size)]
    for (first, c), end in zip(runs.tolist(), ends):
        if c < 0:
            continue
        a, b = int(col_off[first]), int(col_off[end])
        rpos, rx, _ = bed_rules.reference_sites(pos[first:end], col_off[first:end + 1] - a, bases[a:b], seqs[names[c]],
                                                None if tab["ext"] is None else tab["ext"][c], None if tab["conf"] is None else tab["conf"][c])
        sites += [(names[c], int(p)) for p in rpos]
        xs.append(rx)
    return sites, np.concatenate(xs) if xs else np.zeros((0, 33, 18), np.int32)
