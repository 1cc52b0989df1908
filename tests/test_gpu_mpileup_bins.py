"""pipeline.mpileup_to_bins: ONE mpileup text holding several contigs -> every <name>.pd.bin, byte for byte what pipeline.contig_to_bin
writes for the files the reference's splitter (DNA_ExtractChrPileupData) would have cut the text into - against the .pd files the
reference's compiled programs wrote (tests/golden), against contig_to_bin at every chunk layout and table order, and the three record
entries underneath it (nsnp_pileup_window_records_keys, nsnp_pileup_alt_info_keys, nsnp_mpileup_line_names_contigs) against their
single-contig neighbours and a Python rule.  Every comparison is exact."""
import gzip
import os

import numpy as np
import pytest

from nanosnp_amd import _lib, host, sitefile
from tests import contig_rules as cr
from tests import records_cases as rc
from tests.helpers import golden

pytestmark = pytest.mark.gpu


def _model():
    from nanosnp_amd.pileup_model import LSTMNetwork
    return LSTMNetwork()                                     # no weights: the stage-1 path needs only the context and the buffer sets


@pytest.fixture(scope="module")
def model():
    return _model()


def _write_fasta(d, seqs):
    """seqs: {name: uint8 sequence} in FASTA order -> (path, fai text)"""
    fasta, fai = b"", ""
    for name, seq in seqs.items():
        seq = np.asarray(seq, np.uint8)
        fasta += b">" + name.encode() + b"\n" + b"\n".join(bytes(seq[a:a + 60]) for a in range(0, seq.size, 60)) + b"\n"
        fai += f"{name}\t{seq.size}\t0\t60\t61\n"
    (d / "ref.fa").write_bytes(fasta)
    return str(d / "ref.fa"), fai


def _listing(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


def _n_cuts_inside(cuts, lo, hi):
    return sum(lo < c < hi for c in cuts)


# ---- 1. the reference's fixtures in one text ------------------------------------------------------------------------------------------
ANCHOR = (("g1", "chrS", 138), ("end", "chrE", 76), ("adv", "chrT", 432), ("cut", "chrC", 1231), ("pos", "chrP", 161))


@pytest.fixture(scope="module")
def anchor(tmp_path_factory):
    d = tmp_path_factory.mktemp("anchor")
    texts, seqs, pds = {}, {}, {}
    for tag, name, _ in ANCHOR:
        text = gzip.open(golden(f"encode_{tag}.mpileup.gz")).read()
        fa = gzip.open(golden(f"encode_{tag}.fa.gz")).read()
        pd = gzip.open(golden(f"encode_{tag}.pd.gz")).read()
        assert pd.split(b"\n")[0].split(b"\t")[1].split(b":")[0].decode() == name and text.endswith(b"\n")
        texts[name], seqs[name], pds[name] = text, np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8), pd
    fasta, fai = _write_fasta(d, seqs)                       # chrE lies in front of chrT: bases follow its end in the resident genome
    return dict(dir=d, texts=texts, pds=pds, fasta=fasta, fai=fai, whole=b"".join(texts.values()))


@pytest.mark.parametrize("chunks", ["one", "many"])
def test_reference_anchor(tmp_path, model, anchor, chunks):
    from nanosnp_amd.pipeline import mpileup_to_bins, ramp_cuts
    whole = anchor["whole"]
    chunk_bytes = 64 << 20 if chunks == "one" else len(whole) // 12
    cuts = ramp_cuts(whole, 0, len(whole), chunk_bytes)
    bounds = np.cumsum([0] + [len(t) for t in anchor["texts"].values()]).tolist()
    if chunks == "many":
        assert len(cuts) - 1 >= 8
        assert any(_n_cuts_inside(cuts, a, b) >= 2 for a, b in zip(bounds[:-1], bounds[1:]))             # a contig spread over several chunks
        assert any(_n_cuts_inside(bounds, a, b) >= 1 for a, b in zip(cuts[:-1], cuts[1:]))               # a chunk holding several contigs
    st = {}
    out = mpileup_to_bins(model, whole, anchor["fasta"], anchor["fai"], str(tmp_path / "bins"), chunk_bytes=chunk_bytes, stats=st)
    assert out == {name: n for _, name, n in ANCHOR} and list(out) == [name for _, name, _ in ANCHOR]
    assert st["chunks"] == len(cuts) - 1 and st["sites"] == sum(out.values()) and st.get("restarts", 0) == 0
    assert sorted(os.listdir(tmp_path / "bins")) == sorted(f"{name}.pd.bin" for _, name, _ in ANCHOR)
    for _, name, n in ANCHOR:
        assert sitefile.pd_to_bin(anchor["pds"][name], tmp_path / "want.bin") == n
        assert (tmp_path / "bins" / f"{name}.pd.bin").read_bytes() == (tmp_path / "want.bin").read_bytes(), name


# ---- 2. against contig_to_bin on the splitter's files -----------------------------------------------------------------------------------
SIZES = (4000, 1, 2500, 40, 6000)


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """five wanted contigs, one unlisted contig whose lines lie between ctg2 and ctg3; what contig_to_bin writes for the splitter's files"""
    from nanosnp_amd.pipeline import contig_to_bin
    d = tmp_path_factory.mktemp("genome")
    texts, seqs = {}, {}
    for i, n in enumerate(SIZES):
        texts[f"ctg{i}"], seqs[f"ctg{i}"] = rc.synth_text(20261300 + i, n, f"ctg{i}")
    fasta, fai = _write_fasta(d, seqs)
    extra = rc.synth_text(20261399, 700, "ctgX_unlisted")[0]
    order = ["ctg0", "ctg1", "ctg2", None, "ctg3", "ctg4"]
    whole = b"".join(extra if n is None else texts[n] for n in order)
    (d / "pileup_data").write_bytes(whole)
    names = [n for n in order if n]
    split = cr.split_by_contig(whole, [n.encode() for n in names])
    assert {k.decode(): v for k, v in split.items()} == texts
    m = _model()
    want = {}
    for tag, kw in (("", {}), ("noalt", dict(alt_info=False)), ("int32", dict(matrix_dtype="int32"))):
        for n in names:
            sites = contig_to_bin(m, split[n.encode()], n, seqs[n], str(d / "want.bin"), **kw)
            want[tag, n] = (sites, (d / "want.bin").read_bytes())
    assert [want["", n][0] for n in ("ctg1", "ctg3")] == [0, 0] and min(want["", n][0] for n in ("ctg0", "ctg2", "ctg4")) > 50
    return dict(dir=d, texts=texts, seqs=seqs, fai=fai, fasta=fasta, whole=whole, extra=extra, names=names, want=want)


def _chunk_sizes(genome):
    """one chunk; 100 000; a cut exactly on the boundary in front of ctg2; that boundary five lines behind a cut (inside its halo)"""
    from nanosnp_amd.pipeline import ramp_cuts
    t, whole = genome["texts"], genome["whole"]
    boundary = len(t["ctg0"]) + len(t["ctg1"])
    back5 = boundary
    for _ in range(5):
        back5 = whole.rfind(b"\n", 0, back5 - 1) + 1
    assert boundary in ramp_cuts(whole, 0, len(whole), boundary) and whole[boundary:boundary + 5] == b"ctg2\t"
    cuts = ramp_cuts(whole, 0, len(whole), back5)
    assert back5 in cuts and boundary not in cuts and whole[back5:boundary].count(b"\n") == 5
    return {"one_chunk": 1 << 30, "100k": 100_000, "cut_on_boundary": boundary, "boundary_in_halo": back5}


def _assert_files(genome, out, out_dir, tag="", names=None):
    names = genome["names"] if names is None else names
    assert list(out) == names and sorted(os.listdir(out_dir)) == sorted(f"{n}.pd.bin" for n in names)
    for n in names:
        sites, data = genome["want"][tag, n]
        assert out[n] == sites and (out_dir / f"{n}.pd.bin").read_bytes() == data, n


@pytest.mark.parametrize("chunks", ["one_chunk", "100k", "cut_on_boundary", "boundary_in_halo"])
def test_whole_text_equals_the_per_contig_files(tmp_path, model, genome, chunks):
    from nanosnp_amd.pipeline import mpileup_to_bins
    st = {}
    out = mpileup_to_bins(model, str(genome["dir"] / "pileup_data"), genome["fasta"], genome["fai"], str(tmp_path / "b"), contigs=genome["names"],
                          chunk_bytes=_chunk_sizes(genome)[chunks], stats=st)
    _assert_files(genome, out, tmp_path / "b")
    assert st["sites"] == sum(out.values()) and st["record_bytes"] > 0 and st.get("restarts", 0) == 0
    assert st["chunks"] == 1 if chunks == "one_chunk" else st["chunks"] > 1


@pytest.mark.parametrize("order", [("ctg1", "ctg3", "ctg0", "ctg4", "ctg2"), ("ctg4", "ctg3", "ctg2", "ctg1", "ctg0")])
def test_table_order_other_than_text_order(tmp_path, model, genome, order):
    from nanosnp_amd.pipeline import mpileup_to_bins
    st = {"time_records": True}
    out = mpileup_to_bins(model, genome["whole"], genome["fasta"], genome["fai"], str(tmp_path / "b"), contigs=list(order), chunk_bytes=60_000, stats=st)
    _assert_files(genome, out, tmp_path / "b")
    assert st["chunks"] >= 15 and st["record_chunks"] >= 10 and st["window_records_s"] > 0 and st["alt_info_s"] > 0


def test_without_alt_info_as_int32_and_a_subset(tmp_path, model, genome):
    from nanosnp_amd.pipeline import mpileup_to_bins
    args = (genome["fasta"], genome["fai"])
    out = mpileup_to_bins(model, genome["whole"], *args, str(tmp_path / "a"), contigs=genome["names"], alt_info=False, chunk_bytes=150_000)
    _assert_files(genome, out, tmp_path / "a", "noalt")
    assert list(sitefile.read_arrays(tmp_path / "a" / "ctg0.pd.bin")) == ["position_matrix", "position"]
    out = mpileup_to_bins(model, np.frombuffer(genome["whole"], np.uint8), *args, str(tmp_path / "b"), matrix_dtype="int32", chunk_bytes=150_000)
    _assert_files(genome, out, tmp_path / "b", "int32")       # contigs=None: every name of the index (the unlisted contig is not in it)
    # a wanted contig the text does not hold gets no file; a text without a wanted line, and an empty one, give none at all
    out = mpileup_to_bins(model, genome["texts"]["ctg3"] + genome["extra"] + genome["texts"]["ctg2"], *args, str(tmp_path / "c"))
    _assert_files(genome, out, tmp_path / "c", names=["ctg3", "ctg2"])
    for text in (genome["extra"], b""):
        assert mpileup_to_bins(model, text, *args, str(tmp_path / "d")) == {} and os.listdir(tmp_path / "d") == []


# ---- 3. names ----------------------------------------------------------------------------------------------------------------------------
def _names_case(tmp_path, names_sizes, seed):
    texts, seqs = {}, {}
    for i, (name, n) in enumerate(names_sizes):
        texts[name], seqs[name] = rc.synth_text(seed + i, n, name)
    fasta, fai = _write_fasta(tmp_path, seqs)
    return texts, seqs, fasta, fai


def _want_bins(tmp_path, texts, seqs, **kw):
    from nanosnp_amd.pipeline import contig_to_bin
    want, m = {}, _model()
    for n, t in texts.items():
        sites = contig_to_bin(m, t, n, seqs[n], str(tmp_path / "want.bin"), **kw)
        want[n] = (sites, (tmp_path / "want.bin").read_bytes())
    return want


def test_names_of_1_and_37_bytes_side_by_side(tmp_path, model):
    """k_position_strings_keys writes 4 bytes per thread across site boundaries (83 is no multiple of 4): a thread's word holds the end of a
    site of one contig and the start of a site of the next, whose names are 1 and 37 bytes long"""
    from nanosnp_amd.pipeline import mpileup_to_bins
    texts, seqs, fasta, fai = _names_case(tmp_path, (("a", 1203), ("b" * 37, 1500), ("c", 900)), 20261500)
    want = _want_bins(tmp_path, texts, seqs)
    assert want["a"][0] % 2 == 1 and want["b" * 37][0] % 2 == 1 and want["a"][0] > 20
    st = {}
    out = mpileup_to_bins(model, b"".join(texts.values()), fasta, fai, str(tmp_path / "b"), stats=st)
    assert st["chunks"] == 1 and out == {n: w[0] for n, w in want.items()}
    for n, (_, data) in want.items():
        assert (tmp_path / "b" / f"{n}.pd.bin").read_bytes() == data, n
    assert bytes(sitefile.read_arrays(tmp_path / "b" / ("b" * 37 + ".pd.bin"))["position"][0]).startswith(b"b" * 37 + b":")


def _space_junk(text, name, n_other, seed):
    """column 0 of n_other seeded lines becomes `name<SPACE>junk`: the splitter still files them under `name` (the bytes in front of the
    first isspace byte), the window program prints the tab token"""
    lines = rc.text_lines(text)
    which = np.sort(np.random.default_rng(seed).choice(len(lines), n_other, replace=False))
    for j, i in enumerate(which):
        lines[i] = name + b" " + rc.OTHER_NAMES[j % 3] + lines[i][lines[i].index(b"\t"):]
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("n_other", [300, 1500])
def test_a_line_whose_tab_token_is_not_its_contig(tmp_path, model, n_other):
    """`name<SPACE>junk<TAB>...`: those sites carry the tab token, as contig_to_bin on the split file gives them; 1,500 such lines in one
    chunk outnumber the first name table (1,024 entries): the text is run once more"""
    from nanosnp_amd.pipeline import mpileup_to_bins
    texts, seqs, fasta, fai = _names_case(tmp_path, (("n0", 1500), ("n1", 4000), ("n2", 800)), 20261510)
    texts["n1"] = _space_junk(texts["n1"], b"n1", n_other, 3)
    whole = b"".join(texts.values())
    assert {k.decode(): v for k, v in cr.split_by_contig(whole, [b"n0", b"n1", b"n2"]).items()} == texts
    want = _want_bins(tmp_path, texts, seqs)
    st = {}
    out = mpileup_to_bins(model, whole, fasta, fai, str(tmp_path / "b"), stats=st)
    assert st.get("restarts", 0) == (1 if n_other > 1024 else 0) and out == {n: w[0] for n, w in want.items()}
    for n, (_, data) in want.items():
        assert (tmp_path / "b" / f"{n}.pd.bin").read_bytes() == data, n
    position = np.asarray(sitefile.read_arrays(tmp_path / "b" / "n1.pd.bin")["position"])
    assert sum(bytes(r).startswith(b"n1 ") for r in position) > 3       # (sites emitted by such lines are among them)


# ---- 4. a deletion declared across the end of a contig that is not the last of the genome -------------------------------------------------
def test_deletion_across_the_end_of_a_contig_with_bases_behind_it(tmp_path, model):
    """the 'D' key of a deletion reaching past the contig's end stops at the contig's OWN end (the NUL the reference meets there), although
    the next contig's bases lie right behind it in the resident genome"""
    from nanosnp_amd.pipeline import mpileup_to_bins
    rng = np.random.default_rng(61)
    L = 400
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), L).astype(np.uint8)
    p_end = L - 16                                                         # the last column a window can be centred on
    o = bytes([b for b in b"CGTA" if b != seq[p_end - 1]][:1])
    special = o * 10 + b"-3ACG" * 2 + b"-20" + b"A" * 20 + b"-40" + b"C" * 40
    lines = [b"dA\t%d\tN\t%d\t%s\tI\n" % (p, len(special), special) if p == p_end else rc._plain_line(b"dA", p, seq) for p in range(1, L + 1)]
    text_a = b"".join(lines)
    text_b, seq_b = rc.synth_text(20261520, 600, "dB")
    pd, n = rc.oracle_pd(tmp_path, text_a, seq, "dA")
    alt = {p: a for _, p, a in rc.pd_fields(pd)}[p_end]
    assert n >= 1 and alt.count(b"D") >= 2 and not alt.endswith(tuple(b"%d" % k for k in range(10)))     # ends inside a key: no count behind it
    assert sitefile.pd_to_bin(pd, tmp_path / "want.bin") == n
    fasta, fai = _write_fasta(tmp_path, {"dA": seq, "dB": seq_b})
    out = mpileup_to_bins(model, text_a + text_b, fasta, fai, str(tmp_path / "b"))
    assert out["dA"] == n and out["dB"] > 5
    assert (tmp_path / "b" / "dA.pd.bin").read_bytes() == (tmp_path / "want.bin").read_bytes()


# ---- 5. the three entries alone ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(gpu_ctx):
    """three contigs of host.synth_columns in one text, tokenised, encoded and selected on the device (computed once, never changed)"""
    import torch
    names = ["k0", "k1_KI270706v1_random", "k2"]
    texts, seqs = {}, {}
    for i, (name, n) in enumerate(zip(names, (901, 700, 1200))):
        texts[name], seqs[name] = rc.synth_text(20261530 + i, n, name)
    table = _lib.ContigTable(seqs)
    whole = b"".join(texts.values())
    d_text = torch.from_numpy(np.frombuffer(whole, np.uint8).copy()).cuda()
    pos, off, bases, ref, cid, key, runs = gpu_ctx.mpileup_tokenise_contigs(d_text, table)
    counts, depth, flags = gpu_ctx.pileup_encode_columns(bases, off, ref)
    centers, n = gpu_ctx.pileup_select_sites(key, flags)
    torch.cuda.synchronize()
    rows = np.cumsum([0] + [t.count(b"\n") for t in texts.values()])
    assert n == centers.shape[0] > 60 and rows[-1] == key.shape[0]
    return dict(names=names, seqs=seqs, table=table, pos=pos, off=off, bases=bases, ref=ref, key=key, counts=counts, depth=depth, centers=centers,
                rows=rows, text=d_text, cid=cid)


def _per_contig(t, centers):
    """[(contig index, its centres as indices into its own rows, first row, end row)] of ascending centres"""
    c = centers.cpu().numpy()
    out = []
    for i in range(len(t["names"])):
        r0, r1 = int(t["rows"][i]), int(t["rows"][i + 1])
        mine = c[(c >= r0) & (c < r1)] - r0
        out.append((i, mine, r0, r1))
    return out


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("n", [0, 1, "odd"])
def test_window_records_keys_against_the_single_contig_entry(gpu_ctx, three, n, elem):
    import torch
    t = three
    n_all = int(t["centers"].shape[0])
    n = (n_all if n_all % 2 else n_all - 1) if n == "odd" else n
    centers = t["centers"][:n].contiguous()
    x, s, sk, meta = gpu_ctx.pileup_window_records_keys(t["counts"], centers, t["key"], t["table"], elem)
    torch.cuda.synchronize()
    assert meta.tolist() == [n, 0, 0, 0] and x.shape == (n, 33, 18) and s.shape == (n, 83)
    assert np.array_equal(sk.cpu().numpy(), t["key"].cpu().numpy()[centers.cpu().numpy()])
    wx, ws, used = [], [], 0
    for i, mine, r0, r1 in _per_contig(t, centers):
        d_seq = torch.from_numpy(t["seqs"][t["names"][i]]).cuda()
        a, b, m1 = gpu_ctx.pileup_window_records(t["counts"][r0:r1].contiguous(), torch.from_numpy(mine).cuda(), t["pos"][r0:r1].contiguous(), d_seq,
                                                 t["names"][i], elem)
        torch.cuda.synchronize()
        assert m1.tolist() == [mine.size, 0, 0, 0]
        wx.append(a.cpu().numpy()); ws.append(b.cpu().numpy()); used += mine.size > 0
    assert used == (3 if n > 1 else n)
    assert np.array_equal(x.cpu().numpy(), np.concatenate(wx)) and np.array_equal(s.cpu().numpy(), np.concatenate(ws))
    # pinned outputs: nothing behind the n sites is touched
    kw = dict(position_matrix=torch.full((max(n, 1) * 594 + 8,), 77, dtype=torch.int16 if elem == 2 else torch.int32).pin_memory(),
              position=torch.full((n + 1, 83), 77, dtype=torch.uint8).pin_memory(), site_key=torch.full((n + 1,), 77, dtype=torch.int64).pin_memory(),
              meta=torch.full((4,), -1, dtype=torch.int64).pin_memory())
    x2, s2, sk2, meta2 = gpu_ctx.pileup_window_records_keys(t["counts"], centers, t["key"], t["table"], elem, **kw)
    torch.cuda.synchronize()
    assert meta2.tolist() == [n, 0, 0, 0] and np.array_equal(x2.numpy(), x.cpu().numpy()) and np.array_equal(s2.numpy(), s.cpu().numpy())
    assert np.array_equal(sk2.numpy(), sk.cpu().numpy())
    assert (kw["position_matrix"][n * 594:] == 77).all() and (kw["position"][n:] == 77).all() and (kw["site_key"][n:] == 77).all()


@pytest.mark.parametrize("n", [0, 1, "odd"])
def test_alt_info_keys_against_the_single_contig_entry(gpu_ctx, three, n):
    import torch
    t = three
    n_all = int(t["centers"].shape[0])
    n = (n_all if n_all % 2 else n_all - 1) if n == "odd" else n
    centers = t["centers"][:n].contiguous()
    blob, offsets, meta = gpu_ctx.pileup_alt_info_keys(t["bases"], t["off"], t["ref"], t["key"], t["depth"], centers, t["table"])
    torch.cuda.synchronize()
    texts = []
    for i, mine, r0, r1 in _per_contig(t, centers):
        d_seq = torch.from_numpy(t["seqs"][t["names"][i]]).cuda()
        # (the whole chunk's bases and offsets: a column's offsets are absolute)
        b1, o1, m1 = gpu_ctx.pileup_alt_info(t["bases"], t["off"], t["ref"], t["pos"], t["depth"], torch.from_numpy(mine + r0).cuda(), d_seq)
        torch.cuda.synchronize()
        b1, o1 = b1.cpu().numpy(), o1.cpu().numpy()
        assert m1.tolist()[1:] == [0, 0, 0]
        texts += [b1[o1[j]:o1[j + 1]].tobytes() for j in range(mine.size)]
    total = sum(map(len, texts))
    assert meta.tolist() == [total, 0, 0, 0] and len(texts) == n
    offsets, blob = offsets.cpu().numpy(), blob.cpu().numpy()
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64))
    assert blob[:total].tobytes() == b"".join(texts) and (n < 2 or total > 10 * n)
    if n > 1:                                                             # a blob one byte too small: ERANGE, right offsets, untouched blob
        small = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        _, o2, m2 = gpu_ctx.pileup_alt_info_keys(t["bases"], t["off"], t["ref"], t["key"], t["depth"], centers, t["table"], cap=total - 1, blob=small[:total - 1])
        torch.cuda.synchronize()
        assert m2.tolist() == [total, gpu_ctx.TOK_ERANGE, 0, 0] and (small.cpu().numpy() == 0xEE).all() and np.array_equal(o2.cpu().numpy(), offsets)


def test_keys_entries_report_what_they_do_not_follow(gpu_ctx, three):
    """a filler key, a contig outside the table, a window outside the site's own contig, a line_idx entry at or above cap_names: status
    words, clamped reads, nothing followed"""
    import torch
    t = three
    centers = t["centers"][:9].contiguous()
    c = centers.cpu().numpy()
    x0, s0, _, _ = gpu_ctx.pileup_window_records_keys(t["counts"], centers, t["key"], t["table"], 2)
    line_idx = torch.full((int(t["key"].shape[0]),), -1, dtype=torch.int32, device="cuda")
    names = torch.from_numpy(np.stack([rc.name_entry(b"other%d" % e) for e in range(8)])).cuda()
    line_idx[int(c[2]) + 16] = 3
    x, s, _, meta = gpu_ctx.pileup_window_records_keys(t["counts"], centers, t["key"], t["table"], 2, line_names=(line_idx, names))
    torch.cuda.synchronize()
    assert meta.tolist() == [9, 0, 0, 0] and bytes(s.cpu().numpy()[2]).startswith(b"other3:")
    assert np.array_equal(np.delete(s.cpu().numpy(), 2, 0), np.delete(s0.cpu().numpy(), 2, 0))
    for bad in (3, 5, rc.NO_ROOM):                                        # at cap_names, above it, the "no room" entry
        line_idx[int(c[2]) + 16] = bad
        x, s, _, meta = gpu_ctx.pileup_window_records_keys(t["counts"], centers, t["key"], t["table"], 2, line_names=(line_idx, names), cap_names=3)
        torch.cuda.synchronize()
        assert meta.tolist()[:2] == [9, 0] and meta[2].item() != 0 and np.array_equal(s.cpu().numpy(), s0.cpu().numpy()), bad
    for bad_key in (cr.FILLER, (len(t["names"]) << cr.KEY_SHIFT) | 50, (1 << cr.KEY_SHIFT) | 3, (1 << cr.KEY_SHIFT) | (700 - 5)):
        key = t["key"].clone()
        key[int(c[4])] = bad_key
        x, s, sk, meta = gpu_ctx.pileup_window_records_keys(t["counts"], centers, key, t["table"], 2)
        torch.cuda.synchronize()
        assert meta[2].item() != 0 and sk.cpu().numpy()[4] == bad_key and np.array_equal(x.cpu().numpy(), x0.cpu().numpy())
        assert np.array_equal(np.delete(s.cpu().numpy(), 4, 0), np.delete(s0.cpu().numpy(), 4, 0))
    for bad_key in (cr.FILLER, (len(t["names"]) << cr.KEY_SHIFT) | 50):     # alt_info: a contig of length 0, said in the status
        key = t["key"].clone()
        key[int(c[4])] = bad_key
        _, o, meta = gpu_ctx.pileup_alt_info_keys(t["bases"], t["off"], t["ref"], key, t["depth"], centers, t["table"])
        torch.cuda.synchronize()
        assert meta[1].item() == gpu_ctx.TOK_EPOS and o.shape[0] == 10


def test_line_names_contigs_against_python(gpu_ctx):
    """the first tab-delimited token of every line against the table name of the line's contig: a text of more than two name tiles with a
    differing token straddling a tile edge, a line longer than a tile, lines of an unlisted contig, `name<SPACE>junk` tokens"""
    import torch
    names = [b"cB", b"cA"]
    seqs = {n.decode(): np.full(400, ord("A"), np.uint8) for n in names}
    table = _lib.ContigTable(seqs)
    rng = np.random.default_rng(9)
    lines, size = [], 0

    def add(name, tok=None, fill=None, length=None):
        """one more line of contig `name` (column 0: tok); length: the line's bytes without its newline, reached by a longer quality field"""
        nonlocal size
        p = sum(1 for l in lines if cr.line_name(l) == name) + 1
        b = b"A" * (int(rng.integers(1, 60)) if fill is None else fill)
        line = (tok if tok is not None else name) + b"\t%d\tN\t%d\t%s\tI" % (p, len(b), b)
        line += b"I" * (len(b) - 1 if length is None else length - len(line))
        assert length is None or len(line) == length
        lines.append(line)
        size += len(line) + 1

    while size < rc.NM_TILE - 400:
        add(b"cA", b"cA x" if rng.random() < 0.1 else None)
    add(b"cA", fill=20, length=rc.NM_TILE - 3 - size - 1)                    # up to three bytes in front of the tile edge ...
    assert size == rc.NM_TILE - 3
    add(b"cA", b"cA straddles")                                            # ... where a differing token starts and ends behind the edge
    add(b"cX", fill=20)
    add(b"cX", b"cX y", fill=20)                                           # an unlisted contig: never an entry, whatever its token
    add(b"cB", fill=rc.NM_TILE + 500, length=rc.NM_TILE + 540)             # a line longer than a tile
    add(b"cB", b"cB\x0bz")                                                 # (a vertical tab is isspace too: the contig is cB, the token is not)
    end = size + 1500
    while size < end:
        add(b"cB", b"cB other" if rng.random() < 0.1 else None)
    for text in (b"\n".join(lines) + b"\n", b"\n".join(lines)):
        assert rc.n_tiles(len(text)) >= 3
        d = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
        cid = gpu_ctx.mpileup_tokenise_contigs(d, table)[4]
        want_cid = [names.index(cr.line_name(l)) if cr.line_name(l) in names else -1 for l in lines]
        assert cid.cpu().numpy().tolist() == want_cid
        toks = [rc.first_token(l) for l in rc.text_lines(text)]
        differ = [i for i, (tk, c_) in enumerate(zip(toks, want_cid)) if c_ >= 0 and tk != names[c_]]
        assert len(differ) > 10 and b"cA straddles" in [toks[i] for i in differ] and b"cX y" not in [toks[i] for i in differ]
        idx, ent, meta = gpu_ctx.mpileup_line_names_contigs(d, cid, table, cap_names=256)
        torch.cuda.synchronize()
        idx, ent = idx.cpu().numpy()[:len(toks)], ent.cpu().numpy()
        assert meta.tolist() == [len(differ), 0, 0, 0]
        assert np.array_equal(np.flatnonzero(idx >= 0), np.array(differ, np.int64)) and (idx[idx < 0] == -1).all()
        assert sorted(idx[differ].tolist()) == list(range(len(differ)))                  # every entry handed out once
        for i in differ:
            assert np.array_equal(ent[idx[i]], rc.name_entry(toks[i])), i
    # a table that is too small: the count needed and the status
    idx, ent, meta = gpu_ctx.mpileup_line_names_contigs(d, cid, table, cap_names=4)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()[:len(toks)]
    assert meta.tolist() == [len(differ), gpu_ctx.TOK_ERANGE, 0, 0]
    assert sorted(idx[differ].tolist()) == [0, 1, 2, 3] + [rc.NO_ROOM] * (len(differ) - 4)


# ---- 6. a count outside int16 ------------------------------------------------------------------------------------------------------------
def test_a_deep_column_makes_every_file_int32(tmp_path, model):
    from nanosnp_amd.pipeline import mpileup_to_bins, ramp_cuts
    texts, seqs = {}, {}
    texts["s0"], seqs["s0"] = rc.synth_text(20261540, 1200, "s0")
    name, seqs["deep"], texts["deep"] = rc.deep_text()
    texts["s1"], seqs["s1"] = rc.synth_text(20261541, 900, "s1")
    fasta, fai = _write_fasta(tmp_path, seqs)
    want = _want_bins(tmp_path, texts, seqs, matrix_dtype="int32")
    st = {}
    whole = b"".join(texts.values())
    n_chunks = len(ramp_cuts(whole, 0, len(whole), 50_000)) - 1
    out = mpileup_to_bins(model, whole, fasta, fai, str(tmp_path / "b"), chunk_bytes=50_000, stats=st)
    assert st["restarts"] == 1 and st["chunks"] > n_chunks > 3 and out == {n: w[0] for n, w in want.items()} and out["deep"] >= 1
    for n, (_, data) in want.items():
        assert sitefile.read_arrays(tmp_path / "b" / f"{n}.pd.bin")["position_matrix"].dtype == np.int32
        assert (tmp_path / "b" / f"{n}.pd.bin").read_bytes() == data, n
    assert int(sitefile.read_arrays(tmp_path / "b" / "deep.pd.bin")["position_matrix"].max()) > 32767
    assert sorted(os.listdir(tmp_path / "b")) == ["deep.pd.bin", "s0.pd.bin", "s1.pd.bin"]


def test_alt_text_outgrowing_its_slot_starts_the_text_over(tmp_path):
    """the text of test_gpu_pileup_bins' test of the same restart (200 neighbouring sites of 120 distinct insertions): the whole text is
    run again with larger blobs, and the file is contig_to_bin's and the oracle's, byte for byte.  A model of its own for either call: the
    slots a model keeps from earlier calls may be large enough already"""
    from nanosnp_amd.pipeline import contig_to_bin, mpileup_to_bins
    name, seq, text = rc.outgrown_blob_text()
    fasta, fai = _write_fasta(tmp_path, {name: seq})
    pd, n = rc.oracle_pd(tmp_path, text, seq, "big")
    assert n == 200 and sitefile.pd_to_bin(pd, tmp_path / "want.bin") == n
    assert contig_to_bin(_model(), text, name, seq, str(tmp_path / "contig.bin")) == n
    st = {}
    out = mpileup_to_bins(_model(), text, fasta, fai, str(tmp_path / "b"), stats=st)
    assert out == {"big": 200} and st["restarts"] == 1
    got = (tmp_path / "b" / "big.pd.bin").read_bytes()
    assert got == (tmp_path / "contig.bin").read_bytes() and got == (tmp_path / "want.bin").read_bytes()
    assert os.listdir(tmp_path / "b") == ["big.pd.bin"]                   # no staging or .tmp name is left


# ---- 7. round trip ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_equals_call_mpileup(tmp_path, genome, pileup_weights):
    from nanosnp_amd.pileup_model import LSTMNetwork
    from nanosnp_amd.pipeline import call_mpileup, mpileup_to_bins, predict_pileup_bins
    m = LSTMNetwork().load_weight_list(pileup_weights)
    out = mpileup_to_bins(m, genome["whole"], genome["fasta"], genome["fai"], str(tmp_path / "b"), chunk_bytes=100_000)
    files = [str(tmp_path / "b" / f"{n}.pd.bin") for n, sites in out.items() if sites]
    assert len(files) == 3
    for bs in (1000, 64):
        rows = call_mpileup(m, genome["whole"], genome["fasta"], genome["fai"], str(tmp_path / "want.vcf"), batch_size=bs, chunk_bytes=100_000)
        assert predict_pileup_bins(m, files, genome["fai"], str(tmp_path / "got.vcf"), batch_size=bs) == rows > 300
        assert (tmp_path / "got.vcf").read_bytes() == (tmp_path / "want.vcf").read_bytes(), bs


# ---- 8. errors and what they leave behind ----------------------------------------------------------------------------------------------
def test_errors_leave_the_directory_as_it_was(tmp_path, model, genome):
    from nanosnp_amd.pipeline import mpileup_to_bins
    t = genome["texts"]
    out_dir = tmp_path / "bins"
    out_dir.mkdir()
    (out_dir / "ctg0.pd.bin").write_bytes(b"what was here before")
    (out_dir / "notes.txt").write_bytes(b"x")
    before = _listing(out_dir)
    args = (genome["fasta"], genome["fai"], str(out_dir))
    twice = t["ctg0"] + t["ctg2"] + t["ctg0"]
    beyond = t["ctg2"] + t["ctg3"] + b"ctg3\t41\tN\t1\tA\tI\n" + t["ctg4"]
    for cb in (1 << 30, 100_000):
        with pytest.raises(_lib.NanoSNPError, match="ctg0: the text holds this contig in two separate runs"):
            mpileup_to_bins(model, twice, *args, chunk_bytes=cb)
        assert _listing(out_dir) == before
        with pytest.raises(ValueError, match="outside the reference"):
            mpileup_to_bins(model, beyond, *args, chunk_bytes=cb)
        assert _listing(out_dir) == before
    for bad in ("c" * 38, "", "a\0b"):
        with pytest.raises(ValueError):
            mpileup_to_bins(model, genome["whole"], *args, contigs=["ctg0", bad])
        assert _listing(out_dir) == before
    with pytest.raises(sitefile.SiteFileError):
        mpileup_to_bins(model, genome["whole"], *args, matrix_dtype="int8")
    with pytest.raises(ValueError):                                       # nothing is created for a call that is refused
        mpileup_to_bins(model, genome["whole"], genome["fasta"], genome["fai"], str(tmp_path / "never"), contigs=["c" * 38])
    assert not (tmp_path / "never").exists()
    # the model still works afterwards, and the file that was there is replaced only now
    out = mpileup_to_bins(model, t["ctg2"] + t["ctg0"], *args, chunk_bytes=100_000)
    assert list(out) == ["ctg2", "ctg0"] and sorted(os.listdir(out_dir)) == ["ctg0.pd.bin", "ctg2.pd.bin", "notes.txt"]
    for n in out:
        assert (out_dir / f"{n}.pd.bin").read_bytes() == genome["want"]["", n][1]
