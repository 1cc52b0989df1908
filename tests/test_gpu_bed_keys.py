"""BED region filters over a whole-genome text on the GPU: nsnp_pileup_filter_columns_keys and nsnp_pileup_encode_columns_keys against numpy
(tests/bed_key_rules.py) and against their per-contig neighbours on every contig's slice, and the two entry points call_mpileup_bed /
mpileup_to_bins_bed against the reference's fixtures and against call_variants / make_pileup_bins over the splitter's files.  Nothing is
compared with the keyed code itself; every comparison is exact."""
import gzip
import os

import numpy as np
import pytest

from nanosnp_amd import _lib, bed, host, sitefile
from tests import bed_key_rules as bk
from tests import bed_rules
from tests import contig_rules as cr
from tests import records_cases as rc
from tests.helpers import golden
from tests.test_gpu_mpileup_bins import _chunk_sizes, _space_junk, _write_fasta

pytestmark = pytest.mark.gpu

CAND = 8
SHIFT, MASK, FILLER = bk.KEY_SHIFT, bk.MASK, bk.FILLER
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _pack(bits):
    """bool per base -> uint32 words, (n + 31) // 32 of them"""
    n = bits.size
    return np.packbits(np.concatenate([bits, np.zeros((-n) % 32, bool)]), bitorder="little").view(np.uint32).copy()


def _block_bits(rng, n, density, block=40):
    if density in (0.0, 1.0):
        return np.full(n, bool(density))
    return np.repeat(rng.random(n // block + 1) < density, block)[:n] ^ (rng.random(n) < 0.002)


def _odd_length(n):
    return n + 5 + ((n + 5) % 32 == 0)                        # never a multiple of 32: the last word has bits beyond the contig


def _table_of(bits, garbage=()):
    """bool arrays per contig (None: the BED does not mention it, zero words) -> (words, off); garbage: contigs whose last word gets every
    bit beyond the contig's length set on purpose"""
    parts, off = [], [0]
    for c, b in enumerate(bits):
        w = np.zeros(0, np.uint32) if b is None else _pack(b)
        if c in garbage and w.size and b.size % 32:
            w[-1] |= np.uint32((0xFFFFFFFF << (b.size % 32)) & 0xFFFFFFFF)
        parts.append(w)
        off.append(off[-1] + w.size)
    return np.concatenate(parts), np.asarray(off, np.int64)


# ---- 1. the keyed filter ---------------------------------------------------------------------------------------------------------------
def _filter_case(m, density, cov, edge):
    """Four contigs of unequal length - t0 and t2 with bitmaps of `density`, t1 without words, t3 full - as runs of keyed columns with a
    filler run between them, raw keys at the end (positions beyond their contig - one of them inside the set bits behind t2's length -,
    position 0, contig indices at and beyond the table's size).  edge: the change from t0 to the filler run lies exactly on column 2048,
    the tile's size; every other change lies inside a tile."""
    rng = np.random.default_rng(1000 + m)
    if m < 64:
        seg = [(0, m)]
    else:
        n0 = 2048 if edge else int(m * 0.35) + 3
        n1, n3, n_raw = max(m // 10, 3), min(28, m // 20), 8
        seg = [(0, n0), (-1, 5), (1, n1), (3, n3), (-1, 2), (2, m - n0 - n1 - n3 - 7 - n_raw), ("raw", n_raw)]
        assert all(n > 0 for _, n in seg) and sum(n for _, n in seg) == m
    key, lengths, spans, at = np.empty(m, np.int64), [8, 8, 8, 8], [], 0
    for c, n in seg:
        if c == "raw":
            continue
        if c >= 0:
            p = (np.cumsum(np.where(rng.random(n) < 0.01, 3, 1)) + 2).astype(np.int64)
            lengths[c] = _odd_length(int(p[-1]))
            key[at:at + n] = (c << SHIFT) | p
            spans.append((c, at, at + n))
        else:
            key[at:at + n] = FILLER
        at += n
    if at < m:
        raw = [(0 << SHIFT) | (lengths[0] + 1), (0 << SHIFT) | (lengths[0] + 4000), (2 << SHIFT) | 0, (2 << SHIFT) | (lengths[2] + 1),
               (4 << SHIFT) | 1, (5000 << SHIFT) | 7, (((1 << 17) - 1) << SHIFT) | 1, (2 << SHIFT) | (32 * ((lengths[2] + 31) // 32) + 1)]
        key[at:] = raw
    bits = [_block_bits(rng, lengths[0], density), None, _block_bits(rng, lengths[2], density), np.ones(lengths[3], bool)]
    if cov:
        cols = host.synth_columns(m + 5, m, coverage=cov, het_rate=0.2)
        bases, off = cols.bases, cols.col_off.copy()
        if m > 100:                                            # some columns of zero bytes among them
            lens = off[1:] - off[:-1]
            zero = rng.random(m) < 0.03
            bases = bases[~zero[np.repeat(np.arange(m), lens)]]
            off = np.concatenate([[0], np.cumsum(np.where(zero, 0, lens))]).astype(np.int64)
    else:
        bases, off = np.zeros(1, np.uint8), np.zeros(m + 1, np.int64)
    seqs = {f"t{c}": rng.choice(ACGT, n).astype(np.uint8) for c, n in enumerate(lengths)}
    cid, p = bk.key_cid_pos(key)
    ref = np.full(m, ord("N"), np.uint8)
    for c, a, b in spans:
        ref[a:b] = seqs[f"t{c}"][p[a:b] - 1]
    aux = rng.integers(-1, 1000, m).astype(np.int32)
    return dict(key=key, off=off, bases=bases, ref=ref, aux=aux, seqs=seqs, lengths=lengths, bits=bits, spans=spans)


def _np_filter(key, off, bases, ref, keep):
    lens = (off[1:] - off[:-1])[keep]
    kb = np.concatenate([bases[off[c]:off[c + 1]] for c in np.nonzero(keep)[0]] + [np.zeros(0, np.uint8)])
    return key[keep], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), kb, ref[keep]


@pytest.mark.parametrize("m,density,cov,edge", [(1, 1.0, 30, False), (2047, 0.5, 30, False), (2048, 0.9, 30, False), (2049, 0.1, 30, False),
                                                (4500, 0.3, 30, True), (100_003, 0.5, 30, True), (2049, 0.0, 30, False), (2049, 1.0, 30, False), (5000, 0.5, 0, False),
                                                (70_001, 0.97, 5, False)])
def test_filter_columns_keys_equals_numpy_and_the_per_contig_filter(gpu_ctx, m, density, cov, edge):
    import torch
    t = _filter_case(m, density, cov, edge)
    key, off, bases, ref, aux = t["key"], t["off"], t["bases"], t["ref"], t["aux"]
    table = _lib.ContigTable(t["seqs"])
    words, woff = _table_of(t["bits"], garbage=(0, 2))
    assert woff[2] == woff[1] and (m < 64 or words[woff[3] - 1] >> (t["lengths"][2] % 32))          # t1: zero words; t2: set bits beyond its length
    dbed = _lib.BedTable.upload(table, words, woff)
    clean = [np.zeros(n, bool) if b is None else b for b, n in zip(t["bits"], t["lengths"])]        # (bool per base: the words play no part)
    keep = bk.keep_keys(key, clean)
    wk, wo, wb, wr = _np_filter(key, off, bases, ref, keep)
    K = int(keep.sum())
    if m >= 64:
        assert not keep[-8:].any() and (0 < K < m or density in (0.0, 1.0))
    dk, do, db, dr, da = _dev(key), _dev(off), _dev(bases), _dev(ref), _dev(aux)
    for own_lo, own_hi, pinned, with_aux in ((0, m, False, True), (min(16, m), max(m - 16, 0), True, False), (m // 3, m // 3, False, True),
                                             (m, m, True, True), (m // 2, m - 1, False, False)):
        meta = torch.full((4,), -1, dtype=torch.int64, pin_memory=True) if pinned else None
        ko, oo, bo, ro, ao, meta = gpu_ctx.pileup_filter_columns_keys(dk, do, db, dr, table, dbed, aux=da if with_aux else None, own_lo=own_lo,
                                                                      own_hi=own_hi, meta=meta)
        torch.cuda.synchronize()
        assert meta.tolist() == [K, int(wb.size), int(keep[:own_lo].sum()), int(keep[:own_hi].sum())], (own_lo, own_hi)
        assert np.array_equal(ko.cpu().numpy()[:K], wk) and np.array_equal(ro.cpu().numpy()[:K], wr)
        assert np.array_equal(oo.cpu().numpy()[:K + 1], wo) and np.array_equal(bo.cpu().numpy()[:wb.size], wb)
        # behind the kept columns: empty columns, reference byte N, the filler key, aux -1
        assert (oo.cpu().numpy()[K:] == wb.size).all() and (ro.cpu().numpy()[K:] == ord("N")).all() and (ko.cpu().numpy()[K:] == FILLER).all()
        if with_aux:
            assert np.array_equal(ao.cpu().numpy()[:K], aux[keep]) and (ao.cpu().numpy()[K:] == -1).all()
        else:
            assert ao is None
    # the per-contig filter on every contig's slice, put back together
    got = [np.zeros(0, np.int64)], [np.zeros(0, np.uint8)], [np.zeros(0, np.uint8)]
    for c, a, b in t["spans"]:
        bits_c = t["bits"][c]
        sl = bases[off[a]:off[b]]
        po, oo_, bo_, ro_, meta_c = gpu_ctx.pileup_filter_columns(_dev(key[a:b] & MASK), _dev(off[a:b + 1] - off[a]), _dev(sl if sl.size else np.zeros(1, np.uint8)),
                                                                _dev(ref[a:b]), None if bits_c is None else _dev(_pack(bits_c)),
                                                                0 if bits_c is None else t["lengths"][c])
        torch.cuda.synchronize()
        kc, nbc = int(meta_c[0]), int(meta_c[1])
        got[0].append(po.cpu().numpy()[:kc] | (c << SHIFT)); got[1].append(bo_.cpu().numpy()[:nbc]); got[2].append(ro_.cpu().numpy()[:kc])
    assert np.array_equal(np.concatenate(got[0]), wk) and np.array_equal(np.concatenate(got[1]), wb) and np.array_equal(np.concatenate(got[2]), wr)
    # the tail contract with the keyed encode behind it: nothing is made of the columns behind the K kept ones (K = 0: the front pad)
    conf = _lib.BedTable.upload(table, *_table_of([np.ones(n, bool) for n in t["lengths"]]))
    c, d, f, md = gpu_ctx.pileup_encode_columns_keys(bo, oo, ro, ko, table, conf)
    centers, n = gpu_ctx.pileup_select_sites(ko, f)
    torch.cuda.synchronize()
    assert not (f.cpu().numpy()[K:] & CAND).any() and not c.cpu().numpy()[K:].any()
    c2, d2, f2 = gpu_ctx.pileup_encode_columns(_dev(wb if wb.size else np.zeros(1, np.uint8)), _dev(wo), _dev(wr))
    want, n2 = gpu_ctx.pileup_select_sites(_dev(wk), f2)
    torch.cuda.synchronize()
    assert n == n2 and torch.equal(centers, want) and torch.equal(c[:K], c2) and torch.equal(f[:K], f2)       # (a full confident table changes nothing)
    if density == 0.0:
        assert K == 28                                         # only the columns of the full contig t3 are left
    if density == 1.0 and m >= 64:
        assert K == m - 7 - max(m // 10, 3) - 8                # all but the filler, the contig without words and the raw keys
    if m > 50_000 and cov == 30:
        assert n > 0


def test_nothing_kept_then_the_keyed_encode(gpu_ctx):
    """K = 0 - a BED that mentions no contig of the table, bed_words of no word at all - followed by the keyed encode over the M filled
    columns: nothing selected, no fault (the encode's staging of an all-empty wave reads the 16 bytes in front of the bases: the front pad)"""
    import torch
    t = _filter_case(5000, 0.5, 30, False)
    table = _lib.ContigTable(t["seqs"])
    none = _lib.BedTable.upload(table, np.zeros(0, np.uint32), np.zeros(5, np.int64))
    assert none[0].numel() == 0
    ko, oo, bo, ro, ao, meta = gpu_ctx.pileup_filter_columns_keys(_dev(t["key"]), _dev(t["off"]), _dev(t["bases"]), _dev(t["ref"]), table, none,
                                                                  aux=_dev(t["aux"]), own_lo=16, own_hi=4000)
    for conf in (none, _lib.BedTable.upload(table, *_table_of([np.ones(n, bool) for n in t["lengths"]])), None):
        c, d, f, md = gpu_ctx.pileup_encode_columns_keys(bo, oo, ro, ko, table, conf)
        meta2 = torch.full((4,), -1, dtype=torch.int64, pin_memory=True)
        gpu_ctx.pileup_select_sites_range_dev(ko, f, meta[2:], meta2)
        torch.cuda.synchronize()
        assert meta.tolist() == [0, 0, 0, 0] and meta2.tolist() == [0, 0, 0, 0]
        assert not c.cpu().numpy().any() and not d.cpu().numpy().any() and not (f.cpu().numpy() & CAND).any() and not md.cpu().numpy().any()
    assert (ko.cpu().numpy() == FILLER).all() and (ao.cpu().numpy() == -1).all()


def test_refusals_of_the_keyed_entries(gpu_ctx):
    import ctypes as C
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    t = _filter_case(3000, 0.5, 30, False)
    table = _lib.ContigTable(t["seqs"])
    w, o = _lib.BedTable.upload(table, *_table_of(t["bits"]))
    m = 3000
    k, off, b, r, a = _dev(t["key"]), _dev(t["off"]), _dev(t["bases"]), _dev(t["ref"]), _dev(t["aux"])
    ko = torch.empty(m, dtype=torch.int64).cuda(); oo = torch.empty(m + 1, dtype=torch.int64).cuda(); ao = torch.empty(m, dtype=torch.int32).cuda()
    bo = torch.empty(t["bases"].size + 64, dtype=torch.uint8).cuda()[64:]; ro = torch.empty(m, dtype=torch.uint8).cuda()
    meta = torch.zeros(4, dtype=torch.int64).cuda()
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    d = dict(key=k, aux=a, words=w, boff=o, soff=table.seq_off, n=4, ko=ko, oo=oo, ao=ao, meta=meta)
    def fil(**kw):
        v = {**d, **kw}
        return lib.nsnp_pileup_filter_columns_keys(h, p(v["key"]), p(off), p(b), p(r), p(v["aux"]), m, p(v["words"]), p(v["boff"]), p(v["soff"]), v["n"],
                                                   0, m, p(v["ko"]), p(v["oo"]), p(bo), p(ro), p(v["ao"]), p(v["meta"]), None)
    assert fil(aux=None) == -1 and fil(ao=None) == -1 and fil(ao=a) == -1              # aux without aux_out, the reverse, in place
    assert fil(ko=k) == -1 and fil(key=None) == -1 and fil(meta=None) == -1 and fil(oo=None) == -1 and fil(ko=None) == -1
    assert fil(boff=None) == -1 and fil(soff=None) == -1 and fil(n=-1) == -1
    assert fil() == 0 and fil(aux=None, ao=None) == 0
    torch.cuda.synchronize()
    K = int(meta[0])
    assert fil(n=0, words=None, boff=None, soff=None) == 0                                # a table of no contig: every key is beyond it
    torch.cuda.synchronize()
    assert 0 < K < m and meta.tolist() == [0, 0, 0, 0]
    cnt = torch.empty((m, 18), dtype=torch.int32).cuda(); dep = torch.empty(m, dtype=torch.int32).cuda(); flg = torch.empty(m, dtype=torch.uint8).cuda()
    def enc(**kw):
        v = {**d, **kw}
        return lib.nsnp_pileup_encode_columns_keys(h, p(b), p(off), p(r), p(v["key"]), m, 0.12, 0.12, 6, p(v["words"]), p(v["boff"]), p(v["soff"]), v["n"],
                                                   p(cnt), p(dep), p(flg), None, None)
    assert enc(key=None) == -1 and enc(soff=None) == -1 and enc(boff=None) == -1 and enc(n=-1) == -1      # a table without keys / lengths, words without offsets
    assert enc() == 0 and enc(key=None, words=None, boff=None, soff=None, n=0) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.NanoSNPError):                                 # the bindings check the pair against the table
        gpu_ctx.pileup_filter_columns_keys(k, off, b, r, table, (w, o[:-1]))
    with pytest.raises(_lib.NanoSNPError):
        gpu_ctx.pileup_encode_columns_keys(b, off, r, None, table, (w, o))
    with pytest.raises(_lib.NanoSNPError):
        _lib.BedTable.upload(table, np.zeros(3, np.uint32), np.array([0, 1, 2, 3, 4], np.int64))        # offsets that do not end at the words' end


# ---- 2. the keyed encode -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(gpu_ctx):
    """columns of three contigs with the changes inside 64-column waves - A (1,013 columns: every position of the contig, its last ones
    included), five filler columns, B, C = the encode_cut fixture (deletion lengths 59 / 60 / 61, cut alleles) - and three columns of a contig
    index beyond the table; the confident bits of every contig, A's last word with every bit beyond its length set"""
    rng = np.random.default_rng(17)
    text = gzip.open(golden("encode_cut.mpileup.gz")).read()
    fa = gzip.open(golden("encode_cut.fa.gz")).read()
    seq_c = np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8).copy()
    pos_c, off_c, bases_c = host.mpileup_parse(text)
    parts, key, ref, spans = [], [], [], []
    seqs = {}
    for name, seed, n in (("A", 171, 1013), (None, 172, 5), ("B", 173, 3000), ("C", 0, 0), ("beyond", 174, 3)):
        a = len(key)
        if name == "C":
            seqs["C"], p, cb = seq_c, pos_c, [bases_c[off_c[i]:off_c[i + 1]] for i in range(pos_c.size)]
        elif name not in ("A", "B"):                             # twenty mismatching reads: a candidate wherever only the bases are asked
            p, cb = np.arange(1, n + 1, dtype=np.int64), [np.frombuffer(b"T" * 20, np.uint8)] * n
        else:
            cols = host.synth_columns(seed, n, coverage=30, het_rate=0.2)
            p, cb = np.arange(1, n + 1, dtype=np.int64), [cols.bases[cols.col_off[i]:cols.col_off[i + 1]] for i in range(n)]
            if name in ("A", "B"):
                seqs[name] = cols.ref.copy()
        parts += cb
        if name in seqs:
            c = list(seqs).index(name)
            key += ((c << SHIFT) | p).tolist(); ref += seqs[name][p - 1].tolist(); spans.append((c, a, a + len(p)))
        else:
            key += [FILLER] * n if name is None else ((7 << SHIFT) | p).tolist()
            ref += [ord("A")] * n                                # (a real base: only the key keeps such a column from being a candidate)
    bases = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    lengths = [int(s.size) for s in seqs.values()]
    assert lengths[0] == 1013 and spans[1][1] % 64 != 0 and spans[2][1] % 64 != 0 and lengths[0] % 32
    bits = [_block_bits(rng, lengths[0], 0.5, 7), _block_bits(rng, lengths[1], 0.3, 11), _block_bits(rng, lengths[2], 0.5, 9)]
    bits[1][:40] = True
    table = _lib.ContigTable(seqs)
    return dict(key=np.asarray(key, np.int64), off=off, bases=bases, ref=np.asarray(ref, np.uint8), spans=spans, lengths=lengths, bits=bits, table=table,
                conf=_lib.BedTable.upload(table, *_table_of(bits, garbage=(0, 1, 2))))


def test_encode_columns_keys_against_columns3_on_every_slice(gpu_ctx, three):
    import torch
    t = three
    key, off, bases, ref = t["key"], t["off"], t["bases"], t["ref"]
    db, do, dr, dk = _dev(bases), _dev(off), _dev(ref), _dev(key)
    c3, d3, f3, md3 = (x.cpu().numpy() for x in gpu_ctx.pileup_encode_columns3(db, do, dr))
    c, d, f, md = (x.cpu().numpy() for x in gpu_ctx.pileup_encode_columns_keys(db, do, dr, dk, t["table"], t["conf"]))
    assert np.array_equal(c, c3) and np.array_equal(d, d3) and np.array_equal(md, md3) and np.array_equal(f & 0xF7, f3 & 0xF7)
    assert md3.max() == 60
    # the candidate bit: the numpy rule, bounded by every key's own contig
    ok = bk.confident_keys(key, md3, t["bits"])
    assert np.array_equal(f, np.where(ok, f3, f3 & 0xF7))
    listed = np.zeros(key.size, bool)
    for cid, a, b in t["spans"]:
        listed[a:b] = True
        sl = bases[off[a]:off[b]]
        _, _, fc, _ = gpu_ctx.pileup_encode_columns3(_dev(sl), _dev(off[a:b + 1] - off[a]), _dev(ref[a:b]), _dev(key[a:b] & MASK), _dev(_pack(t["bits"][cid])),
                                                     t["lengths"][cid])
        assert np.array_equal(f[a:b], fc.cpu().numpy()), cid
        assert (f3[a:b] & CAND).any() and ((f3[a:b] & CAND) != (f[a:b] & CAND)).any() and (f[a:b] & CAND).any(), cid
    # filler columns and columns of a contig index beyond the table are never candidates - they would be without the table
    assert (~listed).sum() == 8 and (f3[~listed] & CAND).all() and not (f[~listed] & CAND).any()
    # without max_del; without a table (the plain candidates)
    c, d, f_, none = gpu_ctx.pileup_encode_columns_keys(db, do, dr, dk, t["table"], t["conf"], want_max_del=False)
    assert none is None and np.array_equal(f_.cpu().numpy(), f)
    c, d, f_, md_ = gpu_ctx.pileup_encode_columns_keys(db, do, dr, dk, t["table"], None)
    assert np.array_equal(f_.cpu().numpy(), f3) and np.array_equal(md_.cpu().numpy(), md3)
    torch.cuda.synchronize()


def test_deletion_across_the_end_of_a_contig_never_reads_the_next_contigs_bits(gpu_ctx):
    """deletions at contig A's last positions whose reach [p - 1, p + max_del + 1) passes A's end, A's own bits all 0, the set bits behind
    A's length in its last word and B's first bits - which lie right behind them in bed_words - all 1: no candidate; with A's last bit set
    they are candidates"""
    import torch
    rng = np.random.default_rng(5)
    LA, LB = 100, 90
    seq_a, seq_b = np.full(LA, ord("A"), np.uint8), np.full(LB, ord("A"), np.uint8)
    col = b"".join([b"T-5CCCCC"] * 12)                                    # 12 reads, all mismatching, a deletion of five behind each
    pos_a = np.arange(LA - 3, LA + 1)
    key = np.concatenate([(0 << SHIFT) | pos_a, (1 << SHIFT) | np.arange(1, 4)]).astype(np.int64)
    n = key.size
    bases = np.frombuffer(col * n, np.uint8)
    off = (np.arange(n + 1) * len(col)).astype(np.int64)
    ref = np.full(n, ord("A"), np.uint8)
    table = _lib.ContigTable({"A": seq_a, "B": seq_b})
    db, do, dr, dk = _dev(bases), _dev(off), _dev(ref), _dev(key)
    f_plain = gpu_ctx.pileup_encode_columns(db, do, dr)[2].cpu().numpy()
    assert (f_plain & CAND).all()
    bits = [np.zeros(LA, bool), np.ones(LB, bool)]
    words, woff = _table_of(bits, garbage=(0,))
    assert woff.tolist() == [0, 4, 7] and words[3] == 0xFFFFFFF0 and words[4] == 0xFFFFFFFF
    c, d, f, md = gpu_ctx.pileup_encode_columns_keys(db, do, dr, dk, table, _lib.BedTable.upload(table, words, woff))
    torch.cuda.synchronize()
    assert (md.cpu().numpy() == 5).all()
    assert (f.cpu().numpy() & CAND != 0).tolist() == [False] * 4 + [True] * 3
    # the reference's single list would have let all four pass: bits 100.. of a flat layout are B's
    flat = np.concatenate(bits)
    assert bed_rules.confident_pass(pos_a, np.full(4, 5), flat).all()
    bits[0][LA - 1] = True
    c, d, f, md = gpu_ctx.pileup_encode_columns_keys(db, do, dr, dk, table, _lib.BedTable.upload(table, *_table_of(bits, garbage=(0,))))
    assert (f.cpu().numpy() & CAND != 0).all()
    # the same through the filter: position LA + 1 of contig A (a raw key beyond the contig) sits on a set bit of the last word - dropped
    k2 = np.array([(0 << SHIFT) | LA, (0 << SHIFT) | (LA + 1), (0 << SHIFT) | 129, (1 << SHIFT) | 1], np.int64)
    out = gpu_ctx.pileup_filter_columns_keys(_dev(k2), _dev(off[:5]), _dev(bases[:off[4]]), _dev(ref[:4]), table,
                                             _lib.BedTable.upload(table, *_table_of(bits, garbage=(0,))))
    torch.cuda.synchronize()
    assert out[5].tolist()[0] == 2 and out[0].cpu().numpy()[:2].tolist() == [int(k2[0]), int(k2[3])]


# ---- 3. the reference's fixtures, end to end ---------------------------------------------------------------------------------------------
def _vcf_sites(vcf):
    return [(l.split(b"\t")[0].decode(), int(l.split(b"\t")[1])) for l in bytes(vcf).splitlines() if l and not l.startswith(b"#")]


@pytest.fixture(scope="module")
def weighted(pileup_weights):
    from nanosnp_amd.pileup_model import LSTMNetwork
    return LSTMNetwork().load_weight_list(pileup_weights)


@pytest.mark.parametrize("case", ["ext", "conf", "both"])
def test_reference_fixtures_in_one_text_end_to_end(tmp_path, weighted, case):
    """the whole text of the CPU anchor (chrS + an unlisted contig + chrC, the case's BED files concatenated): the sites the stream selects
    are exactly the fixtures' (contig, position) lists, at three chunk sizes, and the VCF bytes do not depend on the chunk size"""
    from nanosnp_amd import pipeline
    a = bk.anchor(case)
    fasta, fai = _write_fasta(tmp_path, a["seqs"])
    paths = {}
    for kind in ("ext", "conf"):
        paths[kind] = None
        if a[kind] is not None:
            paths[kind] = str(tmp_path / f"{kind}.bed")
            open(paths[kind], "wb").write(a[kind])
    dicts = {k: None if v is None else bed.load_bed(v, fai) for k, v in paths.items()}
    table = _lib.ContigTable(a["seqs"])
    beds = _lib.BedTable(table, paths["ext"], paths["conf"], fai)
    assert (beds.ext is None) == (a["ext"] is None) and (beds.conf is None) == (a["conf"] is None)
    ref_vcf = None
    for cb, how in ((1 << 30, paths), (20_000, dicts), (2_500, paths)):
        keys = []
        st0 = {}
        pipeline._stream_text_dev(weighted, a["whole"], table, cb, 0.12, 6, st0, lambda rows, started: keys.append(rows[:, 0].cpu().numpy()) if rows is not None else None,
                                  beds=beds)
        k = np.concatenate(keys).astype(np.int64) if keys else np.zeros(0, np.int64)
        assert [(a["names"][int(c)], int(p)) for c, p in zip(k >> SHIFT, k & MASK)] == a["want"], cb
        st = {}
        rows = pipeline.call_mpileup_bed(weighted, a["whole"], fasta, fai, str(tmp_path / "o.vcf"), extended_bed=how["ext"], confident_bed=how["conf"],
                                         chunk_bytes=cb, stats=st)
        vcf = (tmp_path / "o.vcf").read_bytes()
        assert st["sites"] == len(a["want"]) and st["chunks"] == st0["chunks"] and (cb > 20_000 or st["chunks"] > 10), cb
        ref_vcf = vcf if ref_vcf is None else ref_vcf
        assert vcf == ref_vcf, cb
    assert set(_vcf_sites(ref_vcf)) <= set(a["want"]) and len(_vcf_sites(ref_vcf)) == rows


# ---- 4. the whole text against the per-contig files --------------------------------------------------------------------------------------
SIZES = (4000, 1, 2500, 40, 6000)


def _random_intervals(rng, n, longest, gap):
    iv, at = [], int(rng.integers(0, 3))
    while at < n:
        k = int(rng.integers(1, longest))
        iv.append((at, min(n, at + k)))
        at += k + int(rng.integers(1, gap))
    return np.asarray(iv, np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def genome(tmp_path_factory, weighted):
    """the five-contig genome of tests/test_gpu_call_mpileup.py (an unlisted contig between ctg2 and ctg3), rebuilt here; random intervals
    per contig for both BEDs, ctg2 absent from the extended and ctg3 from the confident one; what call_variants and make_pileup_bins give
    with the same BEDs over the splitter's files"""
    from nanosnp_amd.pileup_model import LSTMNetwork
    from nanosnp_amd.pipeline import call_variants, make_pileup_bins
    d = tmp_path_factory.mktemp("genome")
    texts, seqs = {}, {}
    for i, n in enumerate(SIZES):
        texts[f"ctg{i}"], seqs[f"ctg{i}"] = rc.synth_text(20261300 + i, n, f"ctg{i}")
        (d / f"ctg{i}.mpileup").write_bytes(texts[f"ctg{i}"])
    fasta, fai = _write_fasta(d, seqs)
    extra = rc.synth_text(20261399, 700, "ctgX_unlisted")[0]
    order = ["ctg0", "ctg1", "ctg2", None, "ctg3", "ctg4"]
    whole = b"".join(extra if n is None else texts[n] for n in order)
    (d / "pileup_data").write_bytes(whole)
    names = [n for n in order if n]
    assert {k.decode(): v for k, v in cr.split_by_contig(whole, [n.encode() for n in names]).items()} == texts
    rng = np.random.default_rng(77)
    ext = {n: _random_intervals(rng, seqs[n].size, 400, 60) for n in names if n != "ctg2"}
    conf = {n: _random_intervals(rng, seqs[n].size, 60, 90) for n in names if n != "ctg3"}
    ext["ctg1"] = np.array([[0, 1]], np.int64)
    for kind, b in (("ext", ext), ("conf", conf)):
        (d / f"{kind}.bed").write_bytes(b"# " + kind.encode() + b"\n" + b"".join(b"%s\t%d\t%d\n" % (n.encode(), lo, hi) for n, iv in b.items() for lo, hi in iv))
    pairs = [(n, str(d / f"{n}.mpileup")) for n in names]
    want = {}
    for tag, kw in (("both", dict(extended_bed=ext, confident_bed=conf)), ("ext", dict(extended_bed=ext)), ("none", {})):
        rows = call_variants(weighted, pairs, fasta, fai, str(d / f"want_{tag}.vcf"), **kw)
        want[tag] = (rows, (d / f"want_{tag}.vcf").read_bytes())
    assert 20 < want["both"][0] < want["ext"][0] < want["none"][0]           # the file has rows, and each BED takes some away
    plain = LSTMNetwork()
    bins = make_pileup_bins(plain, pairs, fasta, fai, str(d / "want_bins"), extended_bed=ext, confident_bed=conf)
    assert bins["ctg2"] == 0 and bins["ctg0"] > 10 and bins["ctg4"] > 10 and sorted(os.listdir(d / "want_bins")) == sorted(f"{n}.pd.bin" for n in names)
    return dict(dir=d, texts=texts, fai=fai, fasta=fasta, whole=whole, names=names, ext=ext, conf=conf, want=want, bins=bins, plain=plain)


def _beds_as(genome, how):
    if how == "dict":
        return dict(extended_bed=genome["ext"], confident_bed=genome["conf"])
    return dict(extended_bed=str(genome["dir"] / "ext.bed"), confident_bed=str(genome["dir"] / "conf.bed"))


@pytest.mark.parametrize("chunks,how", [("one_chunk", "dict"), ("100k", "path"), ("cut_on_boundary", "dict"), ("boundary_in_halo", "path")])
def test_call_mpileup_bed_equals_call_variants_over_the_split_files(weighted, genome, chunks, how):
    from nanosnp_amd.pipeline import call_mpileup_bed
    out = genome["dir"] / f"got_{chunks}.vcf"
    st = {}
    rows = call_mpileup_bed(weighted, str(genome["dir"] / "pileup_data"), genome["fasta"], genome["fai"], str(out), contigs=genome["names"],
                            chunk_bytes=_chunk_sizes(genome)[chunks], stats=st, **_beds_as(genome, how))
    assert (rows, out.read_bytes()) == genome["want"]["both"]
    assert st["vcf_rows"] == rows and (st["chunks"] == 1 if chunks == "one_chunk" else st["chunks"] > 1)
    if chunks == "100k":                                     # one BED alone, and a table order other than the text's
        rows = call_mpileup_bed(weighted, genome["whole"], genome["fasta"], genome["fai"], str(out), contigs=genome["names"][::-1], chunk_bytes=60_000,
                                extended_bed=genome["ext"])
        assert (rows, out.read_bytes()) == genome["want"]["ext"]


@pytest.mark.parametrize("chunks,how", [("one_chunk", "path"), ("100k", "dict"), ("cut_on_boundary", "path"), ("boundary_in_halo", "dict")])
def test_mpileup_to_bins_bed_equals_make_pileup_bins_over_the_split_files(tmp_path, genome, chunks, how):
    from nanosnp_amd.pipeline import mpileup_to_bins_bed
    st = {}
    out = mpileup_to_bins_bed(genome["plain"], str(genome["dir"] / "pileup_data"), genome["fasta"], genome["fai"], str(tmp_path / "b"),
                              contigs=genome["names"], chunk_bytes=_chunk_sizes(genome)[chunks], stats=st, **_beds_as(genome, how))
    assert out == genome["bins"] and list(out) == genome["names"]
    # the same set of files - ctg2, whose lines the extended BED drops altogether, has its empty one - and every file identical
    assert sorted(os.listdir(tmp_path / "b")) == sorted(os.listdir(genome["dir"] / "want_bins"))
    for n in genome["names"]:
        assert (tmp_path / "b" / f"{n}.pd.bin").read_bytes() == (genome["dir"] / "want_bins" / f"{n}.pd.bin").read_bytes(), n
    assert st["sites"] == sum(out.values()) and st.get("restarts", 0) == 0


# ---- 5. names under an extended BED --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [1 << 30, 70_000])
def test_names_of_the_emitting_lines_under_an_extended_bed(tmp_path, genome, chunk_bytes):
    """a line's tab token is not its contig on 600 lines of n1: under the filter the line that emits a site is the 16th KEPT line behind the
    centre, so the name index travels with the columns - the files equal mpileup_to_bins of the text with the dropped lines removed on the host"""
    from nanosnp_amd.pipeline import mpileup_to_bins, mpileup_to_bins_bed
    texts, seqs = {}, {}
    for i, (name, n) in enumerate((("n0", 1500), ("n1", 4000), ("n2", 800))):
        texts[name], seqs[name] = rc.synth_text(20261510 + i, n, name)
    texts["n1"] = _space_junk(texts["n1"], b"n1", 600, 3)
    fasta, fai = _write_fasta(tmp_path, seqs)
    whole = b"".join(texts.values())
    rng = np.random.default_rng(9)
    ext = {"n0": np.array([[0, 1500]]), "n1": _random_intervals(rng, 4000, 300, 50), "n2": _random_intervals(rng, 800, 200, 30)}
    bits = {n: bed_rules.bit_array(iv, seqs[n].size) for n, iv in ext.items()}
    kept = b"".join(l + b"\n" for l in rc.text_lines(whole)
                    if bed_rules.extended_keep([int(l.split(b"\t")[1])], bits[cr.line_name(l).decode()])[0])
    assert 0.5 < len(kept) / len(whole) < 0.95
    want = mpileup_to_bins(genome["plain"], kept, fasta, fai, str(tmp_path / "want"))
    got = mpileup_to_bins_bed(genome["plain"], whole, fasta, fai, str(tmp_path / "got"), extended_bed=ext, chunk_bytes=chunk_bytes)
    assert got == want and list(got) == ["n0", "n1", "n2"] and want["n1"] > 30
    for n in want:
        assert (tmp_path / "got" / f"{n}.pd.bin").read_bytes() == (tmp_path / "want" / f"{n}.pd.bin").read_bytes(), n
    position = np.asarray(sitefile.read_arrays(tmp_path / "got" / "n1.pd.bin")["position"])
    assert sum(bytes(r).startswith(b"n1 ") for r in position) > 3          # (sites emitted by such lines are among them)


# ---- 6. without BEDs ------------------------------------------------------------------------------------------------------------------------
def test_without_beds_the_new_entries_are_the_old_ones(tmp_path, weighted, genome):
    """both BEDs None: the bytes of call_mpileup / mpileup_to_bins and the same kernel launches (nsnp_ctx_enable_timing counts the encode and
    the PileupModel kernels)"""
    from nanosnp_amd.pipeline import call_mpileup, call_mpileup_bed, mpileup_to_bins, mpileup_to_bins_bed
    args = (genome["whole"], genome["fasta"], genome["fai"])
    ctx = weighted.ctx
    ctx.enable_timing(True)
    try:
        ctx.read_timing()
        r0 = call_mpileup(weighted, *args, str(tmp_path / "a.vcf"), contigs=genome["names"], chunk_bytes=100_000)
        t0 = {k: v[1] for k, v in ctx.read_timing().items()}
        st = {}
        r1 = call_mpileup_bed(weighted, *args, str(tmp_path / "b.vcf"), contigs=genome["names"], chunk_bytes=100_000, extended_bed=None, confident_bed=None,
                              stats=st)
        t1 = {k: v[1] for k, v in ctx.read_timing().items()}
        assert (r0, (tmp_path / "a.vcf").read_bytes()) == (r1, (tmp_path / "b.vcf").read_bytes()) == genome["want"]["none"]
        assert t0 == t1 and t0["encode_columns"] == st["chunks"] > 5
        o0 = mpileup_to_bins(weighted, *args, str(tmp_path / "a"), contigs=genome["names"], chunk_bytes=100_000)
        t0 = {k: v[1] for k, v in ctx.read_timing().items()}
        o1 = mpileup_to_bins_bed(weighted, *args, str(tmp_path / "b"), contigs=genome["names"], chunk_bytes=100_000)
        t1 = {k: v[1] for k, v in ctx.read_timing().items()}
        assert o0 == o1 and t0 == t1 and t0["encode_columns"] > 5 and sum(o0.values()) > 100
        for n in genome["names"]:
            assert (tmp_path / "a" / f"{n}.pd.bin").read_bytes() == (tmp_path / "b" / f"{n}.pd.bin").read_bytes(), n
    finally:
        ctx.enable_timing(False)
