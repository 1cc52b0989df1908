"""pipeline.call_mpileup: ONE mpileup text holding several contigs -> pileup.vcf, byte for byte what pipeline.call_variants writes for the
files the reference's splitter (DNA_ExtractChrPileupData) would have cut the text into - at every chunk size, with contig boundaries on a
chunk cut, inside the 16-line halo of one and in the middle of chunks, and with the lines of an unlisted contig in between."""
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (4000, 1, 2500, 40, 6000)


@pytest.fixture(scope="module")
def genome(tmp_path_factory, pileup_weights):
    """five wanted contigs (text, per-contig files, FASTA, index), one unlisted contig whose lines lie between ctg2 and ctg3, the model"""
    from nanosnp_amd import host
    from nanosnp_amd.pileup_model import LSTMNetwork
    d = tmp_path_factory.mktemp("genome")
    texts, fasta, fai = {}, b"", ""
    for i, n in enumerate(SIZES):
        name = f"ctg{i}"
        cols = host.synth_columns(20261300 + i, n, coverage=30, het_rate=0.05)
        texts[name] = bytes(cols.mpileup_text_native(name))
        seq = cols.ref.copy()
        (d / f"{name}.mpileup").write_bytes(texts[name])
        fasta += b">" + name.encode() + b"\n" + b"\n".join(bytes(seq[a:a + 60]) for a in range(0, seq.size, 60)) + b"\n"
        fai += f"{name}\t{seq.size}\t0\t60\t61\n"
    (d / "ref.fa").write_bytes(fasta)
    extra = bytes(host.synth_columns(20261399, 700, coverage=30, het_rate=0.05).mpileup_text_native("ctgX_unlisted"))
    order = ["ctg0", "ctg1", "ctg2", None, "ctg3", "ctg4"]
    whole = b"".join(extra if n is None else texts[n] for n in order)
    (d / "pileup_data").write_bytes(whole)
    return dict(dir=d, texts=texts, fai=fai, whole=whole, extra=extra, names=[n for n in order if n], fasta=str(d / "ref.fa"),
                model=LSTMNetwork().load_weight_list(pileup_weights))


@pytest.fixture(scope="module")
def want(genome):
    """call_variants over the per-contig files, in text order, per batch size: computed once"""
    from nanosnp_amd.pipeline import call_variants
    out = {}
    for bs in (1000, 64):
        p = genome["dir"] / f"want{bs}.vcf"
        rows = call_variants(genome["model"], [(n, str(genome["dir"] / f"{n}.mpileup")) for n in genome["names"]], genome["fasta"], genome["fai"],
                             str(p), batch_size=bs)
        assert rows > 300                                  # (an empty comparison cannot pass)
        out[bs] = (rows, p.read_bytes())
    return out


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


@pytest.mark.parametrize("bs", [1000, 64])
@pytest.mark.parametrize("chunks", ["one_chunk", "100k", "cut_on_boundary", "boundary_in_halo"])
def test_whole_text_equals_the_per_contig_files(genome, want, chunks, bs):
    from nanosnp_amd.pipeline import call_mpileup
    out = genome["dir"] / f"got_{chunks}_{bs}.vcf"
    st = {}
    rows = call_mpileup(genome["model"], str(genome["dir"] / "pileup_data"), genome["fasta"], genome["fai"], str(out), contigs=genome["names"],
                        batch_size=bs, chunk_bytes=_chunk_sizes(genome)[chunks], stats=st)
    assert (rows, out.read_bytes()) == want[bs]
    assert st["vcf_rows"] == rows and st["chunks"] == (1 if chunks == "one_chunk" else st["chunks"]) and st["text_bytes"] >= len(genome["whole"])


def test_subset_of_contigs_and_every_name_of_the_index(genome, want):
    from nanosnp_amd import host
    from nanosnp_amd.pipeline import call_mpileup, call_variants
    d = genome["dir"]
    sub = ["ctg2", "ctg4"]
    rows_w = call_variants(genome["model"], [(n, str(d / f"{n}.mpileup")) for n in sub], genome["fasta"], genome["fai"], str(d / "sub_want.vcf"))
    rows = call_mpileup(genome["model"], genome["whole"], genome["fasta"], genome["fai"], str(d / "sub.vcf"), contigs=sub, chunk_bytes=150_000)
    assert rows == rows_w > 100 and (d / "sub.vcf").read_bytes() == (d / "sub_want.vcf").read_bytes()
    # contigs=None: every name of the index, as -g (the unlisted contig is in neither); the text as a numpy array
    rows = call_mpileup(genome["model"], np.frombuffer(genome["whole"], np.uint8), genome["fasta"], genome["fai"], str(d / "all.vcf"), chunk_bytes=250_000)
    assert (rows, (d / "all.vcf").read_bytes()) == want[1000]
    # a text without any wanted line, and an empty one: the header alone
    for text in (genome["extra"], b""):
        assert call_mpileup(genome["model"], text, genome["fasta"], genome["fai"], str(d / "none.vcf")) == 0
        assert (d / "none.vcf").read_bytes() == host.vcf_header(genome["fai"]).encode()


@pytest.mark.parametrize("bs", [1000, 64])
@pytest.mark.parametrize("order", [("ctg1", "ctg3", "ctg0", "ctg4", "ctg2"), ("ctg4", "ctg3", "ctg2", "ctg1", "ctg0"), ("ctg3", "ctg0", "ctg4", "ctg2", "ctg1")])
def test_table_order_other_than_text_order(genome, want, order, bs):
    """contigs= sorted otherwise than the text (the table index of a contig says nothing about where it lies): the rows are still whole
    contigs in TEXT order - over many chunks, so that every contig is handed to the writer while later ones stream"""
    from nanosnp_amd.pipeline import call_mpileup
    out = genome["dir"] / f"order_{bs}.vcf"
    st = {}
    rows = call_mpileup(genome["model"], str(genome["dir"] / "pileup_data"), genome["fasta"], genome["fai"], str(out), contigs=list(order),
                        batch_size=bs, chunk_bytes=60_000, stats=st)
    assert st["chunks"] >= 15 and (rows, out.read_bytes()) == want[bs]


def _open_state(path):
    with open("/proc/self/maps") as f:
        mapped = str(path) in f.read()
    fds = [os.readlink(f"/proc/self/fd/{x}") for x in os.listdir("/proc/self/fd") if os.path.exists(f"/proc/self/fd/{x}")]
    return mapped, sum(str(path) == p for p in fds)


def test_errors_and_what_they_leave_behind(genome):
    from nanosnp_amd._lib import NanoSNPError
    from nanosnp_amd.pipeline import call_mpileup
    d, t = genome["dir"], genome["texts"]
    args = (genome["fasta"], genome["fai"], str(d / "err.vcf"))
    twice = d / "twice.mpileup"
    twice.write_bytes(t["ctg0"] + t["ctg2"] + t["ctg0"])
    for cb in (1 << 30, 100_000):
        with pytest.raises(NanoSNPError, match="ctg0: the text holds this contig in two separate runs"):
            call_mpileup(genome["model"], str(twice), *args, chunk_bytes=cb)
    gc.collect()
    assert _open_state(twice) == (False, 0) and _open_state(d / "err.vcf")[1] == 0
    beyond = d / "beyond.mpileup"
    beyond.write_bytes(t["ctg2"] + t["ctg3"] + b"ctg3\t41\tN\t1\tA\tI\n" + t["ctg4"])
    with pytest.raises(ValueError, match="outside the reference"):
        call_mpileup(genome["model"], str(beyond), *args, chunk_bytes=100_000)
    gc.collect()
    assert _open_state(beyond) == (False, 0)
    with pytest.raises(NotImplementedError):
        call_mpileup(genome["model"], str(beyond), *args, confident_bed={"ctg2": np.array([[0, 10]])})
    with pytest.raises(NotImplementedError):
        call_mpileup(genome["model"], str(beyond), *args, extended_bed=str(d / "x.bed"))
    # the model still works after the errors
    assert call_mpileup(genome["model"], t["ctg2"] + t["ctg4"], *args, batch_size=64) > 100


# ---- one chunk of more than 16,384 lines -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_genome(tmp_path_factory, genome):
    """three wanted contigs of 9,000 columns each (2.8 MB of text - the names are long ones, about 100 bytes per line -, 27,600 lines with
    the 600 of an unlisted contig between the second and the third): in one chunk the contig tokeniser's scan over blocks of 256 lines leaves its first wave (64 blocks = 16,384 lines).
    -> the text, the per-contig files, FASTA and index, and what call_variants writes for the files (computed once)"""
    from nanosnp_amd import host
    from nanosnp_amd.pipeline import call_variants
    d = tmp_path_factory.mktemp("long_genome")
    texts, fasta, fai = {}, b"", ""
    for i in range(3):
        name = f"long{i}_KI270706v1_random"
        cols = host.synth_columns(20261400 + i, 9000, coverage=30, het_rate=0.05)
        texts[name] = bytes(cols.mpileup_text_native(name))
        seq = cols.ref.copy()
        (d / f"{name}.mpileup").write_bytes(texts[name])
        fasta += b">" + name.encode() + b"\n" + b"\n".join(bytes(seq[a:a + 60]) for a in range(0, seq.size, 60)) + b"\n"
        fai += f"{name}\t{seq.size}\t0\t60\t61\n"
    (d / "ref.fa").write_bytes(fasta)
    extra = bytes(host.synth_columns(20261499, 600, coverage=30, het_rate=0.05).mpileup_text_native("longX_KI270706v1_unlisted"))
    names = list(texts)
    whole = texts[names[0]] + texts[names[1]] + extra + texts[names[2]]
    (d / "pileup_data").write_bytes(whole)
    rows = call_variants(genome["model"], [(n, str(d / f"{n}.mpileup")) for n in names], str(d / "ref.fa"), fai, str(d / "want.vcf"), batch_size=1000)
    assert rows > 300                                      # (an empty comparison cannot pass)
    return dict(dir=d, texts=texts, whole=whole, names=names, fasta=str(d / "ref.fa"), fai=fai, want=(rows, (d / "want.vcf").read_bytes()))


@pytest.mark.parametrize("chunk_bytes", [None, 1_000_000], ids=["default_chunk", "1MB"])
def test_a_chunk_of_more_than_16384_lines(genome, long_genome, chunk_bytes):
    """at the default chunk size the whole text is ONE chunk of 27,600 lines; at 1,000,000 bytes the cuts fall inside contigs, the third
    chunk beginning beyond line 16,384 of the text: the same bytes as call_variants over the per-contig files either way"""
    from nanosnp_amd.pipeline import call_mpileup, ramp_cuts
    g = long_genome
    whole = g["whole"]
    assert whole.count(b"\n") == 27_600 > 256 * 64 and 2_600_000 < len(whole) < 64 << 20
    cuts = ramp_cuts(whole, 0, len(whole), 1_000_000)
    bounds = set(np.cumsum([0] + [len(g["texts"][n]) for n in g["names"][:2]] + [len(whole) - sum(map(len, g["texts"].values()))]).tolist())
    assert len(cuts) == 4 and not bounds & set(cuts[1:-1])             # two cuts, both inside a contig ...
    assert whole[:cuts[2]].count(b"\n") > 256 * 64 and cuts[2] > max(bounds)          # ... the second beyond line 16,384, in the third contig
    out = g["dir"] / f"got_{chunk_bytes}.vcf"
    st = {}
    kw = {} if chunk_bytes is None else dict(chunk_bytes=chunk_bytes)
    rows = call_mpileup(genome["model"], str(g["dir"] / "pileup_data"), g["fasta"], g["fai"], str(out), contigs=g["names"], batch_size=1000, stats=st, **kw)
    assert (rows, out.read_bytes()) == g["want"]
    assert st["vcf_rows"] == rows and (st["chunks"] == 1 if chunk_bytes is None else st["chunks"] == 3)
