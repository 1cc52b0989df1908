"""BED region filters on the GPU: nsnp_pileup_encode_columns3 (max_del_length + the confident test), nsnp_pileup_filter_columns (the
extended-BED compaction), nsnp_pileup_select_sites_range_dev, and the text-to-VCF pipeline with extended_bed / confident_bed - against
the oracle, the numpy restatement of the rules (tests/bed_rules.py) and the fixtures the reference's programs wrote."""
import gzip

import numpy as np
import pytest

from nanosnp_amd import bed, host
from tests import bed_rules
from tests.helpers import golden
from tests.test_bed import CASES, load_case

pytestmark = pytest.mark.gpu

CAND = 8


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _bits(intervals_or_words, n_bits, words=False):
    w = np.asarray(intervals_or_words, np.uint32) if words else bed.bed_bitmap(intervals_or_words, n_bits)
    return _dev(w) if w.size else None


def _columns(cols):
    bases = np.frombuffer(b"".join(cols), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    return (bases if bases.size else np.zeros(1, np.uint8)), off


def _enc3(ctx, bases, off, ref, pos=None, bits=None, n_bits=0, **kw):
    import torch
    out = ctx.pileup_encode_columns3(_dev(bases), _dev(off), _dev(ref), None if pos is None else _dev(pos, np.int64), bits, n_bits, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _check_enc3(ctx, bases, off, ref, seed):
    """max_del against the oracle; without a bitmap everything equals columns2; with one, the candidate bit follows the rule"""
    import torch
    c2, d2, f2 = (t.cpu().numpy() for t in ctx.pileup_encode_columns(_dev(bases), _dev(off), _dev(ref)))
    c, d, f, md = _enc3(ctx, bases, off, ref)
    want_md = bed_rules.max_del_lengths(bases, off, ref)
    assert np.array_equal(md, want_md), np.nonzero(md != want_md)[0][:10]
    assert np.array_equal(c, c2) and np.array_equal(d, d2) and np.array_equal(f, f2)
    rng = np.random.default_rng(seed)
    m = len(ref)
    n_bits = m + 40
    pos = np.arange(1, m + 1, dtype=np.int64) + 5
    conf = rng.random(n_bits) < 0.08
    words = np.packbits(np.concatenate([conf, np.zeros((-n_bits) % 32, bool)]), bitorder="little").view(np.uint32)
    c, d, f, md = _enc3(ctx, bases, off, ref, pos, _bits(words, n_bits, words=True), n_bits)
    ok = bed_rules.confident_pass(pos, want_md, conf)
    assert np.array_equal(f, np.where(ok, f2, f2 & 0xF7)) and np.array_equal(c, c2) and np.array_equal(d, d2) and np.array_equal(md, want_md)
    assert (f2 & CAND).any() and ((f2 & CAND) != (f & CAND)).any() and (f & CAND).any()
    c, d, f, none = _enc3(ctx, bases, off, ref, pos, _bits(words, n_bits, words=True), n_bits, want_max_del=False)
    assert none is None and np.array_equal(f, np.where(ok, f2, f2 & 0xF7))
    torch.cuda.synchronize()


def test_encode_columns3_synthetic_columns_vs_oracle(gpu_ctx):
    cols = host.synth_columns(31, 200_000, coverage=30)
    _check_enc3(gpu_ctx, cols.bases, cols.col_off, cols.ref, 1)


def test_encode_columns3_cut_fixture_and_random_bytes(gpu_ctx):
    """encode_cut: long deletions, deletions the end of the column cuts short (declared length counts), lengths 59 / 60 / 61; random
    printable bytes; opener-dense waves at the variant's smaller entry list (176 entries a segment)"""
    text = gzip.open(golden("encode_cut.mpileup.gz")).read()
    fa = gzip.open(golden("encode_cut.fa.gz")).read()
    seq = np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8)
    pos, off, bases = host.mpileup_parse(text)
    _check_enc3(gpu_ctx, bases, off, seq[pos - 1], 2)
    assert bed_rules.max_del_lengths(bases, off, seq[pos - 1]).max() == 60
    rng = np.random.default_rng(3)
    cols = [bytes(rng.integers(33, 127, int(rng.integers(0, 300)), dtype=np.uint8)) for _ in range(6000)]
    cols += [bytes(rng.choice(np.frombuffer(b"ACGTacgt*#+-^$0123456789", np.uint8), int(rng.integers(0, 400)))) for _ in range(6000)]
    four = b"A+1CA-1GA+1CA-2GT"
    for n4 in (43, 44, 45, 52, 53):                                  # 172 .. 212 openers in a wave of 64 columns
        cols += [four] * n4 + [b"ACGTacgt-3ACG"] * (64 - n4)
    cols += [b"-" * 176 + b"A-7ACGTACG"] + [b"a-12acgtacgtacgt" * 5] * 63 + [b"T" * 1000 + b"-2GG" * 500, b"A-60" + b"C" * 60, b"A-61" + b"C" * 61, b"A-60CC"]
    bases, off = _columns(cols)
    ref = rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), len(cols)).astype(np.uint8)
    _check_enc3(gpu_ctx, bases, off, ref, 4)


def _np_filter(pos, off, bases, ref, keep):
    lens = (off[1:] - off[:-1])[keep]
    kb = np.concatenate([bases[off[c]:off[c + 1]] for c in np.nonzero(keep)[0]] + [np.zeros(0, np.uint8)])
    return pos[keep], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), kb, ref[keep]


def _run_filter(ctx, pos, off, bases, ref, words, n_bits, own_lo, own_hi, pinned_meta=False):
    import torch
    meta = torch.full((4,), -1, dtype=torch.int64, pin_memory=True) if pinned_meta else None
    out = ctx.pileup_filter_columns(_dev(pos), _dev(off), _dev(bases), _dev(ref), _bits(words, n_bits, words=True), n_bits, own_lo, own_hi, meta=meta)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("m,density,cov", [(1, 0.5, 30), (2047, 0.5, 30), (2048, 0.9, 30), (2049, 0.1, 30), (100_003, 0.5, 30), (70_001, 0.97, 5),
                                           (30_000, 0.0, 30), (30_000, 1.0, 30), (5000, 0.5, 0)])
def test_filter_columns_equals_numpy_compaction(gpu_ctx, m, density, cov):
    """random, empty and full bitmaps, M beside the tile size, columns of zero bytes (cov 0: all of them): kept columns in order, bytes
    densely repacked, the tail contract (encode + select over M = over the K kept columns), the images of the own range"""
    import torch
    from oracle import oracle
    rng = np.random.default_rng(m)
    if cov:
        cols = host.synth_columns(m + 5, m, coverage=cov, het_rate=0.2)
        bases, off, ref = cols.bases, cols.col_off.copy(), cols.ref
        if m > 100:                                                                 # some columns of zero bytes among them
            lens = off[1:] - off[:-1]
            zero = rng.random(m) < 0.03
            bases = bases[~zero[np.repeat(np.arange(m), lens)]]
            off = np.concatenate([[0], np.cumsum(np.where(zero, 0, lens))]).astype(np.int64)
    else:
        bases, off, ref = np.zeros(1, np.uint8), np.zeros(m + 1, np.int64), rng.choice(np.frombuffer(b"ACGT", np.uint8), m).astype(np.uint8)
    n_bits = m + 100
    # runs of kept positions long enough for windows, with gaps; positions ascending with a few gaps of their own
    pos = (np.cumsum(np.where(rng.random(m) < 0.01, 3, 1)) + 7).astype(np.int64)
    n_bits = int(pos[-1]) + 50
    if density in (0.0, 1.0):
        bitsb = np.full(n_bits, bool(density))
    else:
        bitsb = np.repeat(rng.random(n_bits // 40 + 1) < density, 40)[:n_bits] ^ (rng.random(n_bits) < 0.002)
    words = np.packbits(np.concatenate([bitsb, np.zeros((-n_bits) % 32, bool)]), bitorder="little").view(np.uint32)
    keep = bed_rules.extended_keep(pos, bitsb)
    wp, wo, wb, wr = _np_filter(pos, off, bases, ref, keep)
    K = int(keep.sum())
    for own_lo, own_hi, pinned in ((0, m, False), (min(16, m), max(m - 16, 0), True), (m // 3, m // 3, False), (m, m, True), (m // 2, m - 1, False)):
        po, oo, bo, ro, meta = _run_filter(gpu_ctx, pos, off, bases, ref, words, n_bits, own_lo, own_hi, pinned)
        assert meta.tolist() == [K, int(wb.size), int(keep[:own_lo].sum()), int(keep[:own_hi].sum())], (own_lo, own_hi)
        assert np.array_equal(po.cpu().numpy()[:K], wp) and np.array_equal(ro.cpu().numpy()[:K], wr)
        assert np.array_equal(oo.cpu().numpy()[:K + 1], wo) and np.array_equal(bo.cpu().numpy()[:wb.size], wb)
        # behind the kept columns: empty columns, reference byte N, positions no step to or from which is + 1
        assert (oo.cpu().numpy()[K:] == wb.size).all() and (ro.cpu().numpy()[K:] == ord("N")).all()
        tail = po.cpu().numpy()[K:]
        assert (tail < -(1 << 61)).all() and (np.diff(tail) != 1).all()
    # the tail contract: the UNCHANGED encode and selection over all M output columns give exactly the sites of the K kept columns
    c, d, f = gpu_ctx.pileup_encode_columns(bo, oo, ro)
    centers, n = gpu_ctx.pileup_select_sites(po, f)
    torch.cuda.synchronize()
    assert not (f.cpu().numpy()[K:] & CAND).any() and not c.cpu().numpy()[K:].any()
    if K == 0:
        assert n == 0
        return
    oc, od, of = oracle.encode_columns(wb if wb.size else np.zeros(1, np.uint8), wo, wr)
    want = oracle.select_sites(wp, of)
    assert n == len(want) and np.array_equal(centers.cpu().numpy(), want)
    assert np.array_equal(c.cpu().numpy()[:K], oc) and np.array_equal(f.cpu().numpy()[:K], of)
    if 0.0 < density < 1.0 and m > 10_000 and cov == 30:
        assert len(want) > 0


def test_filter_encode_select_equal_the_existing_path_on_host_filtered_text(gpu_ctx):
    """whole arrays, NON-MONOTONE positions (repeats and steps back: lines of different runs become neighbours once lines are dropped):
    filter -> encode -> select on the device = the existing encode -> select on the same columns with the dropped lines removed on the host"""
    import torch
    m = 150_000
    rng = np.random.default_rng(99)
    cols = host.synth_columns(20261017, m, coverage=20, het_rate=0.1)
    u = rng.random(m)
    step = np.where(u < 0.004, 0, np.where(u < 0.008, -rng.integers(1, 60, m), np.where(u < 0.012, 2, 1)))
    pos = (np.cumsum(step) + 2000).astype(np.int64)
    assert pos.min() >= 1 and (np.diff(pos) <= 0).sum() > 500
    n_bits = int(pos.max()) + 10
    bitsb = np.repeat(rng.random(n_bits // 25 + 1) < 0.7, 25)[:n_bits]
    words = np.packbits(np.concatenate([bitsb, np.zeros((-n_bits) % 32, bool)]), bitorder="little").view(np.uint32)
    keep = bed_rules.extended_keep(pos, bitsb)
    wp, wo, wb, wr = _np_filter(pos, cols.col_off, cols.bases, cols.ref, keep)
    c0, d0, f0 = gpu_ctx.pileup_encode_columns(_dev(wb), _dev(wo), _dev(wr))
    want, n0 = gpu_ctx.pileup_select_sites(_dev(wp), f0)
    po, oo, bo, ro, meta = _run_filter(gpu_ctx, pos, cols.col_off, cols.bases, cols.ref, words, n_bits, 1000, m - 1000)
    c, d, f = gpu_ctx.pileup_encode_columns(bo, oo, ro)
    meta2 = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    center = gpu_ctx.pileup_select_sites_range_dev(po, f, meta[2:], meta2)
    torch.cuda.synchronize()
    n, c_lo, c_hi, n_ = meta2.tolist()
    assert n == n_ == n0 and n0 > 200 and torch.equal(center[:n], want)
    wn = want.cpu().numpy()
    assert c_lo == int((wn < keep[:1000].sum()).sum()) and c_hi == int((wn < keep[:m - 1000].sum()).sum()) and 0 < c_lo < c_hi < n
    k = int(keep.sum())
    assert torch.equal(c[:k], c0) and torch.equal(d[:k], d0) and torch.equal(f[:k], f0)
    # the same bounds by value and from device memory agree (no BED involved)
    m3 = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    gpu_ctx.pileup_select_sites_range(po, f, int(meta[2]), int(meta[3]), m3)
    torch.cuda.synchronize()
    assert m3.tolist() == meta2.tolist()


@pytest.mark.parametrize("reader", ["device", "host"])
@pytest.mark.parametrize("tag,case", CASES)
def test_reference_bed_fixture_end_to_end(gpu_ctx, tag, case, reader):
    """mpileup text -> tokenise -> filter (extended BED) -> encode3 (confident BED) -> select -> gather == the tensors the reference's
    programs wrote from the same text with the same BED files; both readers, as test_reference_fixture_end_to_end"""
    import torch
    text, seq, contig, pd, ext, conf = load_case(tag, case)
    n_bits = int(seq.size)
    pos, col_off, bases = host.mpileup_parse(text)
    if reader == "device":
        dpos, doff, dbases, dref = gpu_ctx.mpileup_tokenise(_dev(np.frombuffer(text, np.uint8)), _dev(seq))
    else:
        dpos, doff, dbases, dref = _dev(pos), _dev(col_off), _dev(bases), _dev(seq[pos - 1])
    if ext is not None:
        dpos, doff, dbases, dref, meta = gpu_ctx.pileup_filter_columns(dpos, doff, dbases, dref, _bits(ext, n_bits), n_bits)
        assert 0 < int(meta[0]) < pos.size
    if conf is not None:
        c, d, f, md = gpu_ctx.pileup_encode_columns3(dbases, doff, dref, dpos, _bits(conf, n_bits), n_bits)
    else:
        c, d, f = gpu_ctx.pileup_encode_columns(dbases, doff, dref)
    centers, n = gpu_ctx.pileup_select_sites(dpos, f)
    x = gpu_ctx.pileup_gather_windows(c, centers)
    torch.cuda.synchronize()
    gx, names, gpos, gref = host.pd_parse(pd)
    assert n == gx.shape[0] and n > 0
    assert np.array_equal(x.cpu().numpy(), gx)
    assert np.array_equal(dpos.cpu().numpy()[centers.cpu().numpy()], gpos)
    pd_depth = np.array([int(l.split(b"\t")[2].split(b"-")[0]) for l in pd.splitlines()])
    assert np.array_equal(d.cpu().numpy()[centers.cpu().numpy()], pd_depth)


def _vcf_positions(vcf):
    return [int(l.split(b"\t")[1]) for l in bytes(vcf).splitlines() if l and not l.startswith(b"#")]


def test_pipeline_extended_bed_equals_the_host_filtered_text(pileup_weights, tok_mode, tmp_path):
    """call_contig(extended_bed=) writes the bytes call_contig writes for the text with the dropped lines removed on the host, whatever
    the chunk size: chunks of a few dozen lines put the interval edges into the halos.  The BED as a dict and as a path."""
    from nanosnp_amd.pileup_model import LSTMNetwork
    from nanosnp_amd.pipeline import call_contig
    m = LSTMNetwork().load_weight_list(pileup_weights)
    cols = host.synth_columns(20261018, 30_000, coverage=30, het_rate=0.05)
    text = bytes(cols.mpileup_text_native("chrB"))
    seq = cols.ref.copy()
    rng = np.random.default_rng(5)
    iv, at = [], 3
    while at < seq.size:
        n = int(rng.integers(1, 300))
        iv.append((at, min(seq.size, at + n)))
        at += n + int(rng.integers(1, 80))
    iv = np.asarray(iv, np.int64)
    bitsb = bed_rules.bit_array(iv, seq.size)
    lines = text.split(b"\n")[:-1]
    keep = bed_rules.extended_keep(np.array([int(l.split(b"\t")[1]) for l in lines]), bitsb)
    filtered = b"".join(l + b"\n" for l, k in zip(lines, keep) if k)
    want = call_contig(m, filtered, "chrB", seq, chunk_bytes=1 << 30)
    assert want[1] > 100
    plain = call_contig(m, text, "chrB", seq, chunk_bytes=1 << 30)
    assert plain[1] > want[1]
    bed_path = tmp_path / "panel.bed"
    bed_path.write_bytes(b"#panel\n" + b"".join(b"chrB\t%d\t%d\n" % (a, b) for a, b in iv) + b"chrOther\t0\t5\n")
    for cb, how in ((1 << 30, {"chrB": iv}), (200_000, str(bed_path)), (20_000, {"chrB": iv}), (3_000, {"chrB": iv})):
        got = call_contig(m, text, "chrB", seq, chunk_bytes=cb, extended_bed=how)
        assert bytes(got[0]) == bytes(want[0]) and got[1:] == want[1:], cb
    # a BED path checked against a whole index refuses a contig the index does not hold
    from nanosnp_amd._lib import NanoSNPError
    with pytest.raises(NanoSNPError):
        call_contig(m, text, "chrB", seq, extended_bed=str(bed_path), fai={"chrB": int(seq.size)})
    # a BED that holds nothing of the contig: no line is left
    assert call_contig(m, text, "chrB", seq, chunk_bytes=50_000, extended_bed={"chrZ": [[0, 5]]})[1:] == (0, 0)


@pytest.mark.parametrize("tag,case", [("g1", "conf"), ("cut", "conf"), ("g1", "both"), ("cut", "both")])
def test_pipeline_confident_bed_writes_the_fixture_sites(pileup_weights, tok_mode, tag, case):
    """call_contig(confident_bed=) (and both BEDs) calls exactly the sites of the reference's .pd, at every chunk size"""
    from nanosnp_amd.pileup_model import LSTMNetwork
    from nanosnp_amd.pipeline import call_contig, stream_contig
    m = LSTMNetwork().load_weight_list(pileup_weights)
    text, seq, contig, pd, ext, conf = load_case(tag, case)
    _, _, gpos, _ = host.pd_parse(pd)
    kw = dict(confident_bed={contig: conf}, extended_bed=None if ext is None else {contig: ext})
    ref = None
    for cb in (1 << 30, 20_000, 2_500):
        rows = stream_contig(m, text, contig, seq, chunk_bytes=cb, **kw)
        assert np.array_equal(rows[:, 0].cpu().numpy().astype(np.int64), gpos), cb
        vcf, n_sites, n_rows = call_contig(m, text, contig, seq, chunk_bytes=cb, **kw)
        assert n_sites == gpos.size, cb
        ref = bytes(vcf) if ref is None else ref
        assert bytes(vcf) == ref, cb
    assert set(_vcf_positions(ref)) <= set(gpos.tolist()) and len(_vcf_positions(ref)) == n_rows


def test_pipeline_without_beds_is_unchanged(pileup_weights, tok_mode):
    """both BEDs None: the same bytes as a call without the arguments, and the same kernel launches (nsnp_ctx_enable_timing counts the
    encode and the PileupModel kernels; the filter is no part of such a run)"""
    from nanosnp_amd.pileup_model import LSTMNetwork
    from nanosnp_amd.pipeline import call_contig
    m = LSTMNetwork().load_weight_list(pileup_weights)
    cols = host.synth_columns(20261019, 20_000, coverage=30, het_rate=0.05)
    text = bytes(cols.mpileup_text_native("chrN"))
    seq = cols.ref.copy()
    m.ctx.enable_timing(True)
    try:
        m.ctx.read_timing()
        want = call_contig(m, text, "chrN", seq, chunk_bytes=100_000)
        t0 = {k: v[1] for k, v in m.ctx.read_timing().items()}
        st = {}
        got = call_contig(m, text, "chrN", seq, chunk_bytes=100_000, extended_bed=None, confident_bed=None, stats=st)
        t1 = {k: v[1] for k, v in m.ctx.read_timing().items()}
        assert bytes(got[0]) == bytes(want[0]) and got[1:] == want[1:] and want[1] > 100
        assert t0 == t1 and t0["encode_columns"] == st["chunks"] > 5
        # a full BED changes nothing but the launches
        full = {"chrN": [[0, int(seq.size)]]}
        got = call_contig(m, text, "chrN", seq, chunk_bytes=100_000, extended_bed=full, confident_bed=full)
        assert bytes(got[0]) == bytes(want[0]) and got[1:] == want[1:]
    finally:
        m.ctx.enable_timing(False)


def test_refusals_and_short_bitmaps(gpu_ctx):
    """NULL combinations are NSNP_EINVAL; a bitmap shorter than a position reads as 0 there (never out of bounds): the line is dropped /
    the column is no candidate"""
    import ctypes as C
    import torch
    from nanosnp_amd._lib import NanoSNPError
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    cols = host.synth_columns(8, 5000, coverage=30, het_rate=0.3)
    b, o, r = _dev(cols.bases), _dev(cols.col_off), _dev(cols.ref)
    pos = _dev(np.arange(1, 5001, dtype=np.int64))
    m = 5000
    cnt = torch.empty((m, 18), dtype=torch.int32).cuda(); dep = torch.empty(m, dtype=torch.int32).cuda(); flg = torch.empty(m, dtype=torch.uint8).cuda()
    bits = _bits([[0, 64]], 64)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    enc = lambda pos_, bits_, nb: lib.nsnp_pileup_encode_columns3(h, p(b), p(o), p(r), p(pos_), m, 0.12, 0.12, 6, p(bits_), nb, p(cnt), p(dep), p(flg), None, None)
    assert enc(None, bits, 64) == -1                      # a bitmap without positions
    assert enc(pos, bits, 0) == -1 and enc(pos, bits, -5) == -1 and enc(pos, None, 64) == -1
    assert lib.nsnp_pileup_encode_columns3(h, p(b), p(o), p(r), None, m, 0.12, 0.12, 6, None, 0, None, p(dep), p(flg), None, None) == -1
    assert enc(None, None, 0) == 0 and enc(pos, bits, 64) == 0
    torch.cuda.synchronize()
    # 64 bits against 5,000 positions: candidates only where [p - 1, p + max_del + 1) meets [0, 64)
    c2, d2, f2 = gpu_ctx.pileup_encode_columns(b, o, r)
    md = bed_rules.max_del_lengths(cols.bases, cols.col_off, cols.ref)
    ok = bed_rules.confident_pass(np.arange(1, 5001), md, np.ones(64, bool))
    assert np.array_equal(flg.cpu().numpy(), np.where(ok, f2.cpu().numpy(), f2.cpu().numpy() & 0xF7)) and ok.sum() >= 64 and not ok[70:].any()
    po = torch.empty(m, dtype=torch.int64).cuda(); oo = torch.empty(m + 1, dtype=torch.int64).cuda()
    bo = torch.empty(cols.bases.size + 64, dtype=torch.uint8).cuda()[64:]; ro = torch.empty(m, dtype=torch.uint8).cuda()
    meta = torch.zeros(4, dtype=torch.int64).cuda()
    fil = lambda **k: lib.nsnp_pileup_filter_columns(h, p(k.get("pos", pos)), p(o), p(b), p(r), m, p(k.get("bits", bits)), k.get("nb", 64), 0, m,
                                                     p(k.get("po", po)), p(oo), p(bo), p(ro), p(k.get("meta", meta)), None)
    assert fil(bits=None) == -1 and fil(nb=-1) == -1 and fil(meta=None) == -1 and fil(pos=None) == -1 and fil(po=None) == -1
    assert fil(po=pos) == -1                              # not in place
    assert fil() == 0
    torch.cuda.synchronize()
    assert meta.tolist()[0] == 64 and po[:64].tolist() == list(range(1, 65)) and meta.tolist()[2:] == [0, 64]
    assert fil(bits=None, nb=0) == 0                      # a bitmap of no bits: nothing is kept
    torch.cuda.synchronize()
    assert meta.tolist() == [0, 0, 0, 0]
    sel = lambda own: lib.nsnp_pileup_select_sites_range_dev(h, p(pos), p(flg), m, p(own), p(po), m, p(meta), None)
    assert sel(None) == -1 and sel(meta[2:]) == 0
    torch.cuda.synchronize()
    with pytest.raises(NanoSNPError):                     # the binding checks that the words hold n_bits
        gpu_ctx.pileup_filter_columns(pos, o, b, r, bits, 65)
    with pytest.raises(NanoSNPError):
        gpu_ctx.pileup_encode_columns3(b, o, r, pos, bits, 100)
