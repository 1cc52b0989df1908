"""pipeline.mpileup_to_train_bins: one whole-genome mpileup text + a truth VCF -> every <name>.td.bin.  Against the .td files the
reference's compiled programs wrote (tests/golden/train_*: make_golden_train.py), the label entry alone (nsnp_pileup_label_sites_keys)
against the numpy restatement of the rules (tests/label_rules.py), the subsample on a synthetic genome against the same rules applied to
the rows of mpileup_to_bins_bed's .pd.bin, and the restarts and refusals.  Every comparison is exact."""
import gzip
import json
import os

import numpy as np
import pytest

from nanosnp_amd import _lib, sitefile
from tests import label_rules as lr
from tests import records_cases as rc
from tests.helpers import golden

pytestmark = pytest.mark.gpu
KS = 36


def _model():
    from nanosnp_amd.pileup_model import LSTMNetwork
    return LSTMNetwork()                                     # no weights: the data stage needs only the context and the buffer sets


@pytest.fixture(scope="module")
def model():
    return _model()


def _write_fasta(d, seqs):
    fasta, fai = b"", ""
    for name, seq in seqs.items():
        seq = np.asarray(seq, np.uint8)
        fasta += b">" + name.encode() + b"\n" + b"\n".join(bytes(seq[a:a + 60]) for a in range(0, seq.size, 60)) + b"\n"
        fai += f"{name}\t{seq.size}\t0\t60\t61\n"
    (d / "ref.fa").write_bytes(fasta)
    return str(d / "ref.fa"), fai


def _listing(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


# ---- 1. the reference's fixtures in one text -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anchor(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_anchor")
    texts, seqs = {}, {}
    for tag, name in (("g1", "chrS"), ("cut", "chrC")):
        texts[name] = gzip.open(golden(f"encode_{tag}.mpileup.gz")).read()
        fa = gzip.open(golden(f"encode_{tag}.fa.gz")).read()
        seqs[name] = np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8)
    fasta, fai = _write_fasta(d, seqs)
    fix = {c: dict(vcf=open(golden(c + ".vcf"), "rb").read(), td=gzip.open(golden(c + ".td.gz")).read(), counts=json.load(open(golden(c + ".json"))))
           for c in ("train_g1", "train_cut", "train_g1_bed")}
    return dict(dir=d, whole=b"".join(texts.values()), fasta=fasta, fai=fai, fix=fix)


@pytest.mark.parametrize("chunks", ["one", "many"])
@pytest.mark.parametrize("bed", [False, True])
def test_reference_anchor(tmp_path, model, anchor, chunks, bed):
    """ratio None: every <name>.td.bin is byte for byte td_to_bin of the reference's .td (-shuffle_tensors 0, every site kept)"""
    from nanosnp_amd.pipeline import mpileup_to_train_bins, ramp_cuts
    whole, fix = anchor["whole"], anchor["fix"]
    chunk_bytes = 64 << 20 if chunks == "one" else len(whole) // 12
    assert chunks == "one" or len(ramp_cuts(whole, 0, len(whole), chunk_bytes)) - 1 >= 8
    if bed:
        # the BEDs name chrS alone: chrC is held by the text and loses every line - an empty file
        cases, kw = {"chrS": "train_g1_bed"}, dict(extended_bed=golden("bed_g1_both.ext.bed"), confident_bed=golden("bed_g1_both.conf.bed"))
        vcf = fix["train_g1_bed"]["vcf"]
    else:
        cases, kw = {"chrS": "train_g1", "chrC": "train_cut"}, {}
        vcf = fix["train_g1"]["vcf"] + fix["train_cut"]["vcf"]
    st = {}
    out = mpileup_to_train_bins(model, whole, anchor["fasta"], anchor["fai"], vcf, str(tmp_path / "bins"), max_non_variant_ratio=None,
                                chunk_bytes=chunk_bytes, stats=st, **kw)
    assert list(out) == ["chrS", "chrC"] and sorted(os.listdir(tmp_path / "bins")) == ["chrC.td.bin", "chrS.td.bin"] and st.get("restarts", 0) == 0
    for name in out:
        td = fix[cases[name]]["td"] if name in cases else b""
        n = sitefile.td_to_bin(td, str(tmp_path / "want.bin"))
        assert (tmp_path / "bins" / f"{name}.td.bin").read_bytes() == (tmp_path / "want.bin").read_bytes(), name
        if name in cases:
            c = fix[cases[name]]["counts"]["ratio_1000000"]
            got = dict(out[name])
            assert "%g" % got.pop("recall") == c["recall"] and "%g" % got.pop("ratio") == c["ratio"]
            assert got == dict(sites=n, kept=n, variants=c["variants"], non_variants=c["non_variants"], truth=c["truth"])
        else:
            assert out[name]["sites"] == out[name]["kept"] == n == 0
    assert st["sites"] == sum(o["kept"] for o in out.values())


def test_reference_ratio_5_counts(tmp_path, model, anchor):
    """at the reference's default ratio its draw is random, but its counts and its logged ratio are not"""
    from nanosnp_amd.pipeline import mpileup_to_train_bins
    fix = anchor["fix"]
    out = mpileup_to_train_bins(model, anchor["whole"], anchor["fasta"], anchor["fai"], fix["train_g1"]["vcf"] + fix["train_cut"]["vcf"],
                                str(tmp_path / "bins"), chunk_bytes=len(anchor["whole"]) // 5)
    for name, case in (("chrS", "train_g1"), ("chrC", "train_cut")):
        c, o = fix[case]["counts"]["ratio_5"], out[name]
        assert (o["variants"], o["non_variants"], o["truth"], "%g" % o["ratio"], "%g" % o["recall"]) == \
            (c["variants"], c["non_variants"], c["truth"], c["ratio"], c["recall"])
        label = sitefile.read_train_bin(str(tmp_path / "bins" / f"{name}.td.bin"))[4]
        assert c["variants"] <= o["kept"] == label.shape[0] < o["sites"] and int((label[:, 24 + 32] == 1).sum()) == c["variants"]


# ---- 2. the entry alone against the rules ------------------------------------------------------------------------------------------------
N_SITES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 3077)
N_TRUTH = (0, 1, 2, 3, 1000)
PATTERNS = ("all", "none", "alternating", "seeded")


@pytest.fixture(scope="module")
def entry_table():
    """two contigs: c0 = ACGTacgt over and over (a site at every kind of centre base; positions from 3001 on are never sites), c1 seeded"""
    rng = np.random.default_rng(20261019)
    seqs = {"c0": np.tile(np.frombuffer(b"ACGTacgt", np.uint8), 500), "c1": rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 5000).astype(np.uint8)}
    return _lib.ContigTable(contigs=seqs, device=0), seqs


def _site_keys(n):
    """site i lies in contig i % 2 at position i // 2 + 1: every position is a site of BOTH contigs"""
    i = np.arange(n, dtype=np.int64)
    return (i % 2) << KS | (i // 2 + 1)


def _truth_for(keys, t, pattern, rng):
    """t sorted truth keys: the first and the last are sites (with sites below and above them), between them sites and keys no site has;
    'alternating': every second site instead -> (keys, {key: quad})"""
    s = np.unique(keys)
    if pattern == "alternating":
        chosen = keys[::2].tolist()
    elif t == 0 or s.size == 0:
        chosen = []
    else:
        lo, hi = int(s[s.size // 4]), int(s[(3 * s.size) // 4])
        inner = s[(s > lo) & (s < hi)][::3].tolist()
        free = [(0 << KS) | p for p in range(3001, 4001)]                      # c0 beyond every site: above lo's contig position, below c1
        pool = [k for pair in zip(free, inner + free) for k in pair]
        chosen = sorted({lo, hi} if t > 1 else {lo})
        for k in pool:
            if len(set(chosen)) >= t:
                break
            if lo < k < hi or s.size < 4:
                chosen.append(k)
    tk = np.array(sorted(set(chosen)), np.int64)
    quads = [(int(rng.integers(0, 21)), int(rng.integers(0, 3)), int(rng.integers(0, 33)), int(rng.integers(0, 33))) for _ in tk]
    return tk, dict(zip(tk.tolist(), quads))


def _run_entry(ctx, table, keys, centers, tk, quads, thr, seed, pinned=False, m_extra=5, extra_rows=0, codes=None):
    """-> (kept centres, their label rows, meta, the whole label buffer).  extra_rows: rows of a pinned label buffer behind the N the entry
    is told of; codes: the packed codes of tk where they are already an array (a large table)"""
    import torch
    dev = torch.device("cuda", 0)
    key_col = np.concatenate([keys, np.full(m_extra, _lib.KEY_FILLER, np.int64)])
    if codes is None:
        codes = np.array([g | z << 8 | a << 16 | b << 24 for g, z, a, b in (quads[k] for k in tk.tolist())], np.uint32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = {}
    if pinned:
        kw = dict(label=torch.full((max(len(centers), 1) + extra_rows, 90), -7, dtype=torch.int32).pin_memory(),
                  meta=torch.zeros(4, dtype=torch.int64).pin_memory())
    kept, label, meta = ctx.pileup_label_sites_keys(up(key_col), up(np.asarray(centers, np.int64)), table, up(tk), up(codes.view(np.int32)),
                                                    None if thr is None else up(np.array(thr, np.int64)), seed, **kw)
    torch.cuda.synchronize()
    m = meta.cpu().numpy()
    return kept.cpu().numpy()[:m[0]], label.cpu().numpy()[:m[0]], m, kw.get("label", label)


@pytest.mark.parametrize("n", N_SITES)
def test_label_entry_against_the_rules(gpu_ctx, entry_table, n):
    table, seqs = entry_table
    keys = _site_keys(n)
    bases = np.array([seqs[f"c{k >> KS}"][(k & ((1 << KS) - 1)) - 1] for k in keys.tolist()], np.uint8)
    assert n < 16 or set(bases[:16].tolist()) == set(b"ACGTacgt")
    for j, pattern in enumerate(PATTERNS):
        for t in (N_TRUTH if n == 65 and pattern != "alternating" else (N_TRUTH[(j + n) % 5],)):
            rng = np.random.default_rng([n, j, t])
            tk, truth = _truth_for(keys, t, pattern, rng)
            seed = int(rng.integers(0, 1 << 62)) if pattern == "seeded" else 0
            thr = {"all": None, "none": [0, 0], "alternating": [0, 0], "seeded": [1 << 52, 3 << 51]}[pattern]
            quads, hit = lr.site_quads(keys, bases, truth)
            if pattern != "alternating" and t and n >= 8:
                assert tk.size == t and hit.any() and tk[0] in keys and tk[-1] in keys and keys.min() < tk[0] and keys.max() > tk[-1]
            keep = lr.kept_mask(keys, hit, {} if thr is None else {0: thr[0], 1: thr[1]}, seed)
            if pattern == "seeded" and n >= 1023:
                assert 0.4 < keep[~hit & (keys >> KS == 0)].mean() < 0.6 and 0.65 < keep[~hit & (keys >> KS == 1)].mean() < 0.85
            if pattern == "alternating" and n:
                assert np.array_equal(keep, np.arange(n) % 2 == 0)
            kept, label, meta, _ = _run_entry(gpu_ctx, table, keys, np.arange(n), tk, truth, thr, seed, pinned=(j % 2 == 1))
            assert meta.tolist() == [int(keep.sum()), int(hit.sum()), int((~hit).sum()), 0], (n, pattern, t)
            assert np.array_equal(kept, np.flatnonzero(keep)), (n, pattern, t)
            assert np.array_equal(label, lr.one_hot([q for q, k in zip(quads, keep) if k])), (n, pattern, t)


def test_label_entry_centres_in_any_order_and_untouched_rows(gpu_ctx, entry_table):
    """the centres index the key column: any order, repeats; rows behind N' of a pinned label stay as they were"""
    table, seqs = entry_table
    keys = _site_keys(700)
    rng = np.random.default_rng(5)
    centers = rng.integers(0, 700, 333)
    tk, truth = _truth_for(keys, 1000, "all", rng)
    bases = np.array([seqs[f"c{k >> KS}"][(k & ((1 << KS) - 1)) - 1] for k in keys.tolist()], np.uint8)
    quads, hit = lr.site_quads(keys[centers], bases[centers], truth)
    keep = lr.kept_mask(keys[centers], hit, {0: 1 << 51, 1: 1 << 51}, 99)
    kept, label, meta, whole = _run_entry(gpu_ctx, table, keys, centers, tk, truth, [1 << 51, 1 << 51], 99, pinned=True)
    assert 0 < keep.sum() < 333 and meta.tolist() == [int(keep.sum()), int(hit.sum()), int((~hit).sum()), 0]
    assert np.array_equal(kept, centers[keep]) and np.array_equal(label, lr.one_hot([q for q, k in zip(quads, keep) if k]))
    rest = whole.numpy().reshape(-1)[int(keep.sum()) * 90:]
    assert rest.size and (rest == -7).all()


@pytest.mark.parametrize("what", ["filler", "N base", "contig outside the table", "centre outside the columns", "position outside the contig"])
def test_label_entry_status(gpu_ctx, what):
    """what the selection never emits is reported and clamped, never followed"""
    table = _lib.ContigTable(contigs={"a": np.frombuffer(b"ACGTNACGT", np.uint8), "b": np.frombuffer(b"TTTT", np.uint8)}, device=0)
    keys = np.array([1, 2, 3, (1 << KS) | 2], np.int64)
    centers = [0, 1, 2, 3]
    if what == "filler":
        centers = [0, 4, 2]                                  # (column 4 is the first filler _run_entry appends)
    elif what == "N base":
        keys[1] = 5
    elif what == "contig outside the table":
        keys[2] = (2 << KS) | 1
    elif what == "centre outside the columns":
        centers = [0, 1, 10 ** 12, -3]
    else:
        keys[3] = (1 << KS) | 5
    kept, label, meta, _ = _run_entry(gpu_ctx, table, keys, centers, np.zeros(0, np.int64), {}, None, 0)
    assert meta[3] != 0 and meta[0] == len(centers) and label.shape == (len(centers), 90) and (label.sum(axis=1) == 4).all()
    kept, label, meta, _ = _run_entry(gpu_ctx, table, np.array([1, 2, 3, (1 << KS) | 2], np.int64), [0, 1, 2, 3], np.zeros(0, np.int64), {}, None, 0)
    assert meta.tolist() == [4, 0, 4, 0] and np.argmax(label[:, :21], axis=1).tolist() == [0, 4, 7, 9]


def test_label_entry_count_mode(gpu_ctx, entry_table):
    import torch
    table, _ = entry_table
    dev = torch.device("cuda", 0)
    keys = np.concatenate([_site_keys(3077), (np.arange(500, dtype=np.int64) + 2000) | 1 << KS])         # the last blocks hold c1 alone
    rng = np.random.default_rng(11)
    tk, truth = _truth_for(keys, 1000, "all", rng)
    hit = np.isin(keys, tk)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    totals = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    for _ in range(2):                                       # the counts are ADDED
        kept, label, meta = gpu_ctx.pileup_label_sites_keys(up(keys), up(np.arange(keys.size)), table, up(tk), up(np.zeros(tk.size, np.int32)),
                                                            counts=totals, want_label=False)
    assert kept is None and label is None and meta.cpu().tolist() == [keys.size, int(hit.sum()), int((~hit).sum()), 0]
    want = np.bincount((keys >> KS) * 2 + (~hit), minlength=4).reshape(2, 2)
    assert hit.sum() > 100 and np.array_equal(totals.cpu().numpy(), 2 * want)


# ---- 3. with a ratio, on a synthetic genome -------------------------------------------------------------------------------------------------
SIZES = (4000, 1, 2500, 40, 6000)
RATIO = 2.0


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """five contigs as in test_gpu_mpileup_bins.py; what mpileup_to_bins_bed writes for them; a truth VCF at every 7th site of ctg0 and
    ctg2 and at a few positions that are no site - none in ctg4, which therefore keeps nothing under a ratio"""
    from nanosnp_amd.pipeline import mpileup_to_bins_bed
    d = tmp_path_factory.mktemp("train_genome")
    texts, seqs = {}, {}
    for i, n in enumerate(SIZES):
        texts[f"ctg{i}"], seqs[f"ctg{i}"] = rc.synth_text(20261300 + i, n, f"ctg{i}")
    names = list(texts)
    fasta, fai = _write_fasta(d, seqs)
    whole = b"".join(texts.values())
    sites = mpileup_to_bins_bed(_model(), whole, fasta, fai, str(d / "pd"), contigs=names)
    pd = {n: sitefile.read_arrays(str(d / "pd" / f"{n}.pd.bin"), mmap=False) for n in names}
    pos = {n: sitefile.read_pileup_bin(str(d / "pd" / f"{n}.pd.bin"))[1] for n in names}
    assert [sites[n] for n in ("ctg1", "ctg3")] == [0, 0] and min(sites[n] for n in ("ctg0", "ctg2", "ctg4")) > 50
    rows = []
    for n in ("ctg0", "ctg2"):
        at = set(pos[n][::7].tolist()) | ({5, 17, 1999} - set(pos[n].tolist()))
        for k, p in enumerate(sorted(at)):
            ref = chr(int(seqs[n][p - 1]) & ~0x20)
            alt, gt = [("ACGT"["ACGT".index(ref) - 1], "0/1"), (ref + "TT", "1/1"), ("ACGT"["ACGT".index(ref) - 2] + ",*", "2|1")][k % 3]
            rows.append(f"{n}\t{p}\t.\t{ref}\t{alt}\t9\tPASS\t.\tGT\t{gt}\n")
    vcf = ("##fileformat=VCFv4.2\n" + "".join(rows)).encode()
    truth = lr.truth_table(vcf.decode(), names)
    return dict(dir=d, whole=whole, fasta=fasta, fai=fai, names=names, seqs=seqs, pd=pd, pos=pos, vcf=vcf, truth=truth)


def _rule_files(genome, d, ratio, seed):
    """the files and the counts the rules give: the rows of the .pd.bin, their labels, the kept ones"""
    want, counts = {}, {}
    for cid, n in enumerate(genome["names"]):
        a, pos = genome["pd"][n], genome["pos"][n]
        keys = cid << KS | pos
        quads, hit = lr.site_quads(keys, genome["seqs"][n][pos - 1] if pos.size else np.zeros(0, np.uint8), genome["truth"])
        v, nv = int(hit.sum()), int((~hit).sum())
        thr, r = lr.threshold(v, nv, ratio) if ratio is not None else (None, 1.0)
        keep = lr.kept_mask(keys, hit, {cid: thr}, seed)
        offs = a["alt_info_offsets"]
        alts = [bytes(a["alt_info"][offs[i]:offs[i + 1]]) for i in np.flatnonzero(keep)]
        sitefile.write_train_bin(str(d / "rule.bin"), a["position_matrix"][keep], [bytes(p).rstrip(b"\0") for p in a["position"][keep]],
                                 lr.one_hot([q for q, k in zip(quads, keep) if k]), alts)
        want[n] = (d / "rule.bin").read_bytes()
        n_truth = sum(1 for k in genome["truth"] if k >> KS == cid)
        counts[n] = dict(sites=v + nv, variants=v, non_variants=nv, kept=int(keep.sum()), ratio=r, truth=n_truth,
                         recall=v / n_truth if n_truth else float("nan"))
        assert hit[keep].sum() == v                          # every truth site is present
    return want, counts


def _same_counts(got, want):
    return list(got) == list(want) and all({k: v for k, v in got[n].items() if k != "recall"} == {k: v for k, v in want[n].items() if k != "recall"}
                                           and (got[n]["recall"] == want[n]["recall"] or (want[n]["truth"] == 0 and got[n]["recall"] != got[n]["recall"]))
                                           for n in want)


def test_ratio_files_equal_the_rules(tmp_path, model, genome):
    from nanosnp_amd.pipeline import mpileup_to_train_bins
    args = (genome["whole"], genome["fasta"], genome["fai"], genome["vcf"])
    want, counts = _rule_files(genome, tmp_path, RATIO, 7)
    assert counts["ctg0"]["variants"] < counts["ctg0"]["kept"] < counts["ctg0"]["sites"] and counts["ctg4"]["kept"] == 0 < counts["ctg4"]["sites"]
    assert counts["ctg0"]["truth"] > counts["ctg0"]["variants"] > 5
    runs = {}
    for tag, chunk_bytes in (("one", 1 << 30), ("many", 60_000), ("again", 60_000)):
        st = {}
        out = mpileup_to_train_bins(model, *args, str(tmp_path / tag), contigs=genome["names"], max_non_variant_ratio=RATIO, seed=7,
                                    chunk_bytes=chunk_bytes, stats=st)
        assert _same_counts(out, counts), (tag, out)
        assert (st["chunks"] == 1) == (tag == "one") and st["dropped_sites"] == sum(c["sites"] - c["kept"] for c in counts.values())
        runs[tag] = _listing(tmp_path / tag)
        assert runs[tag] == {f"{n}.td.bin": want[n] for n in genome["names"]}, tag
    assert sitefile.read_train_bin(str(tmp_path / "one" / "ctg4.td.bin"))[4].shape == (0, 90)
    other = mpileup_to_train_bins(model, *args, str(tmp_path / "seed8"), contigs=genome["names"], max_non_variant_ratio=RATIO, seed=8, chunk_bytes=60_000)
    want8, counts8 = _rule_files(genome, tmp_path, RATIO, 8)
    assert _same_counts(other, counts8) and _listing(tmp_path / "seed8") == {f"{n}.td.bin": want8[n] for n in genome["names"]}
    assert want8["ctg0"] != want["ctg0"] and want8["ctg2"] != want["ctg2"]


def test_ratio_none_rows_are_those_of_the_pd_bin(tmp_path, model, genome):
    from nanosnp_amd.pipeline import mpileup_to_train_bins
    out = mpileup_to_train_bins(model, genome["whole"], genome["fasta"], genome["fai"], genome["vcf"], str(tmp_path / "b"), contigs=genome["names"],
                                max_non_variant_ratio=None, chunk_bytes=100_000)
    want, counts = _rule_files(genome, tmp_path, None, 0)
    assert _same_counts(out, counts)
    for n in genome["names"]:
        a = sitefile.read_arrays(str(tmp_path / "b" / f"{n}.td.bin"), mmap=False)
        for k, v in genome["pd"][n].items():
            assert np.array_equal(a[k], v) and a[k].dtype == v.dtype, (n, k)
        assert (tmp_path / "b" / f"{n}.td.bin").read_bytes() == want[n]
    # a ratio no contig reaches subsamples nothing: the same files through the count pass
    out = mpileup_to_train_bins(model, genome["whole"], genome["fasta"], genome["fai"], genome["vcf"], str(tmp_path / "c"), contigs=["ctg0", "ctg2"],
                                max_non_variant_ratio=1e6, chunk_bytes=100_000, alt_info=False)
    assert [o["ratio"] for o in out.values()] == [1.0, 1.0] and [o["kept"] for o in out.values()] == [counts[n]["sites"] for n in ("ctg0", "ctg2")]
    assert list(sitefile.read_arrays(str(tmp_path / "c" / "ctg0.td.bin"))) == ["position_matrix", "position", "label"]


# ---- 4. restarts and refusals ----------------------------------------------------------------------------------------------------------------
def test_an_int16_overflow_restart_keeps_the_labels(tmp_path, model):
    from nanosnp_amd.pipeline import mpileup_to_bins, mpileup_to_train_bins
    contig, seq, text = rc.deep_text()
    name = contig if isinstance(contig, str) else contig.decode()
    fasta, fai = _write_fasta(tmp_path, {name: seq})
    assert mpileup_to_bins(_model(), text, fasta, fai, str(tmp_path / "pd"), chunk_bytes=rc.DEEP_CHUNK) == {name: 1}
    pd = sitefile.read_arrays(str(tmp_path / "pd" / f"{name}.pd.bin"), mmap=False)
    ref = chr(int(seq[299]))
    vcf = f"{name}\t300\t.\t{ref}\t{ref}A\t9\tPASS\t.\tGT\t0/1\n".encode()
    for ratio in (None, 5.0):
        st = {}
        out = mpileup_to_train_bins(model, text, fasta, fai, vcf, str(tmp_path / f"td{ratio}"), max_non_variant_ratio=ratio, chunk_bytes=rc.DEEP_CHUNK, stats=st)
        assert st["restarts"] == 1 and out[name] == dict(sites=1, variants=1, non_variants=0, kept=1, ratio=1.0, truth=1, recall=1.0)
        a = sitefile.read_arrays(str(tmp_path / f"td{ratio}" / f"{name}.td.bin"), mmap=False)
        assert a["position_matrix"].dtype == np.int32 and all(np.array_equal(a[k], v) for k, v in pd.items())
        assert np.array_equal(a["label"], lr.one_hot([(lr.GT21.index(ref + "Ins"), 2, 32, 32)]))


def test_a_repeated_position_raises_and_leaves_out_dir(tmp_path, model, genome):
    from nanosnp_amd.pipeline import mpileup_to_train_bins
    text = genome["whole"][:genome["whole"].index(b"ctg1\t")]
    lines = text.split(b"\n")
    p = int(genome["pos"]["ctg0"][40])
    i = next(j for j, l in enumerate(lines) if l.startswith(b"ctg0\t%d\t" % p))
    twice = text + b"\n".join(lines[:i + 20]) + b"\n"      # the contig's first lines once more: one run whose positions step back, sites repeat
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    (out_dir / "ctg0.td.bin").write_bytes(b"old")
    (out_dir / "else.txt").write_bytes(b"x")
    before = _listing(out_dir)
    for ratio in (None, 5.0):
        with pytest.raises(_lib.NanoSNPError, match="strictly ascending"):
            mpileup_to_train_bins(model, twice, genome["fasta"], genome["fai"], genome["vcf"], str(out_dir), contigs=["ctg0"], max_non_variant_ratio=ratio,
                                  chunk_bytes=50_000)
        assert _listing(out_dir) == before
    with pytest.raises(ValueError, match="occurs twice"):
        mpileup_to_train_bins(model, text, genome["fasta"], genome["fai"], genome["vcf"] + genome["vcf"], str(tmp_path / "new"), contigs=["ctg0"])
    assert not (tmp_path / "new").exists()
    assert mpileup_to_train_bins(model, text, genome["fasta"], genome["fai"], genome["vcf"], str(out_dir), contigs=["ctg0"])["ctg0"]["kept"] > 0
    assert (out_dir / "ctg0.td.bin").read_bytes() != b"old" and sorted(os.listdir(out_dir)) == ["ctg0.td.bin", "else.txt"]


def test_refusals_of_process_groups_and_the_host_tokeniser(tmp_path, model, genome, monkeypatch):
    import torch.distributed as tdist
    from nanosnp_amd.pipeline import mpileup_to_train_bins
    call = lambda: mpileup_to_train_bins(model, genome["whole"], genome["fasta"], genome["fai"], genome["vcf"], str(tmp_path / "out"))
    monkeypatch.setenv("NSNP_TOKENISE", "host")
    with pytest.raises(NotImplementedError, match="NSNP_TOKENISE"):
        call()
    monkeypatch.delenv("NSNP_TOKENISE")
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="process group"):
        call()
    assert not (tmp_path / "out").exists()
