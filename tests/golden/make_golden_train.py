#!/usr/bin/env python3
"""Generate the training-data fixtures under tests/golden/ from the reference's own programs.

Runs only where the reference tree is mounted and oracle/_ref holds its compiled programs (make -C oracle ref).  DNA_SplitVcf and
DNA_CreateTrainData are compiled here with g++ into a temporary directory - the flags and the common source list of oracle/Makefile,
plus -lz - and run behind oracle/_ref/DNA_CreateCanSnpTensor on the existing encode_<tag>.mpileup.gz / .fa.gz inputs with a seeded
truth VCF, at -shuffle_tensors 0:

    train_g1       encode_g1
    train_cut      encode_cut
    train_g1_bed   encode_g1 with the BEDs of bed_g1_both

    python tests/golden/make_golden_train.py

Written per case: train_<case>.vcf (the truth VCF), .true_var (what DNA_SplitVcf wrote for the contig), .td.gz (DNA_CreateTrainData at
-maxinum_non_variant_ratio 1000000: every site kept) and .json (the counts of the reference's two log lines in that run and in a second
run at ratio 5: variants, non_variants, the %g ratio, truth, the %g recall).  Before anything is written the run is repeated and must give
the same bytes, every label family the tests are after must occur, and the numpy restatement of the rules (tests/label_rules.py) must
reproduce the reference's rows, labels and counts.
"""
from __future__ import annotations

import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
GOLD = HERE
CASES = (("train_g1", "g1", None), ("train_cut", "cut", None), ("train_g1_bed", "g1", "bed_g1_both"))
REF = os.environ.get("REF", "/root/reference")


def compile_ref(bindir):
    """DNA_SplitVcf and DNA_CreateTrainData with the release flags and the common sources of oracle/Makefile"""
    src = os.path.join(REF, "dna_sv_tensor", "src")
    common = [os.path.join(src, "common", f) for f in ("bed_intv_list.cpp", "cpp_aux.cpp", "genotype.cpp", "line_reader.cpp", "ref_reader.cpp",
                                                       "tensor.cpp")] + [os.path.join(ROOT, "oracle", "_ref", "kstring.o")]
    for prog, main in (("DNA_SplitVcf", "split_vcf"), ("DNA_CreateTrainData", "make_train_data")):
        subprocess.run(["g++", "-pthread", "-O3", "-w", "-std=c++11", "-DNDEBUG", "-mpopcnt", "-o", os.path.join(bindir, prog),
                        os.path.join(src, main, "main.cpp"), *common, "-lm", "-lz"], check=True)


def run_tensor(workdir, contig, fasta, mpileup_bytes, ext_bed=None, conf_bed=None):
    """DNA_CreateCanSnpTensor with the flags of make_train_data.sh:238-250 -> the rows of <contig>.tensor: [(name, pos, ref33)]"""
    refdir = os.path.join(ROOT, "oracle", "_ref")
    pile = os.path.join(workdir, "pile"); os.makedirs(pile, exist_ok=True)
    with open(os.path.join(pile, contig + ".mpileup"), "wb") as f:
        f.write(mpileup_bytes)
    beds = []
    for flag, path in (("-extended_confident_bed", ext_bed), ("-confident_bed", conf_bed)):
        if path is not None:
            beds += [flag, path]
    subprocess.run([os.path.join(refdir, "DNA_CreateCanSnpTensor"), "-reference", fasta, "-chr_pileup_dir", pile,
                    "-output_dir", os.path.join(workdir, "tensor"), *beds, "-min_af", "0.12", "-snp_min_af", "0.12", "-indel_min_af", "0.12",
                    "-min_coverage", "6", "-flanking_base", "16", "-num_threads", "1", contig], check=True, capture_output=True)
    with open(os.path.join(workdir, "tensor", contig + ".tensor"), "rb") as f:
        return [tuple(line.split(b"\t")[:3]) for line in f.read().split(b"\n") if line]


LOG = re.compile(r"variants / non_variants / subsample_ratio : (\d+) / (\d+) / (\S+)\s+True variants / recall / recall_ratio : (\d+) / (\d+) / (\S+)")


def run_train(bindir, workdir, contig, fasta, vcf_bytes, ratio, conf_bed=None, tag=""):
    """DNA_SplitVcf + DNA_CreateTrainData (make_train_data.sh:222,266-275) -> (.true_var bytes, .td bytes, the counts of the log)"""
    vcf = os.path.join(workdir, "truth.vcf")
    with open(vcf, "wb") as f:
        f.write(vcf_bytes)
    tv, td = os.path.join(workdir, f"tv_{ratio}{tag}"), os.path.join(workdir, f"td_{ratio}{tag}")
    os.makedirs(tv, exist_ok=True)
    subprocess.run([os.path.join(bindir, "DNA_SplitVcf"), vcf, tv], check=True, capture_output=True)
    bed = ["-confident_bed", conf_bed] if conf_bed is not None else []
    r = subprocess.run([os.path.join(bindir, "DNA_CreateTrainData"), "-chr_tensor_dir", os.path.join(workdir, "tensor"), "-chr_true_var_dir", tv,
                        "-reference", fasta, *bed, "-output_dir", td, "-shuffle_tensors", "0", "-maxinum_non_variant_ratio", str(ratio),
                        "-num_threads", "1", contig], check=True, capture_output=True)
    m = LOG.search(r.stderr.decode())
    assert m and m.group(1) == m.group(5), r.stderr
    counts = dict(variants=int(m.group(1)), non_variants=int(m.group(2)), ratio=m.group(3), truth=int(m.group(4)), recall=m.group(6))
    return open(os.path.join(tv, contig + ".true_var"), "rb").read(), open(os.path.join(td, contig + ".td"), "rb").read(), counts


def truth_vcf(case, contig, seq, sites, lost_to_bed):
    """The seeded truth VCF of one case.  sites: the candidate positions of the run; lost_to_bed: candidates of the unfiltered run the BEDs
    remove (empty without BEDs).  REF is the contig's own upper-cased base(s), as a real truth set has it."""
    rng = np.random.default_rng([20261019, [c[0] for c in CASES].index(case)])
    up = lambda p, n=1: bytes(seq[p - 1:p - 1 + n]).upper().decode()
    other = lambda b: "ACGT"[("ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4] if b in "ACGT" else "A"
    at_site = [int(p) for p in rng.permutation(sites)[:12]]
    free = [p for p in range(40, len(seq) - 40) if p not in set(sites) and p not in set(lost_to_bed) and up(p) in "ACGT"]
    off_site = int(free[int(rng.integers(0, len(free)))])
    rows = {}                                                # pos -> (REF, ALT, the FORMAT columns)
    a = iter(at_site)
    p = next(a); rows[p] = (up(p), other(up(p)), "GT\t0/1")                                       # het SNP
    p = next(a); rows[p] = (up(p), other(up(p)), "GT\t1/1")                                       # hom SNP
    p = next(a); b = up(p); two = [c for c in "ACGT" if c != b][:2]
    rows[p] = (b, ",".join(two[::-1]), "GT\t1|2")                                                 # two ALT alleles
    p = next(a); rows[p] = (up(p), up(p) + "GA", "GT\t0/1")                                       # insertion
    p = next(a); rows[p] = (up(p, 3), up(p), "GT\t1/1")                                           # deletion, homozygous
    p = next(a); rows[p] = (up(p), "G,*", "GT\t1/2")                                              # '*' behind: 'G,' -> an insertion of one allele
    p = next(a); rows[p] = (up(p), "*,G", "GT\t2|1")                                              # '*' in front: ',G'
    p = next(a); rows[p] = (up(p), other(up(p)), "GT\t./.")                                       # becomes 0 0 and IS a truth entry
    p = next(a); rows[p] = (up(p), other(up(p)), "GT:DP:AD:PS\t1|0:35:12,23:1001")                # phased, extra FORMAT fields
    p = next(a); rows[p] = (up(p, 2), up(p) + "TTT," + up(p), "GT\t1/2")                          # insertion + deletion
    p = next(a); rows[p] = (up(p), "*", "GT\t0/1")                                                # '*' without a comma: the splitter skips it
    rows[off_site] = (up(off_site), other(up(off_site)), "GT\t0/1")                               # a truth variant at no candidate site
    for p in lost_to_bed[:1]:
        rows[int(p)] = (up(p), other(up(p)), "GT\t1/1")                                           # a truth variant only the BED removes
    head = b"##fileformat=VCFv4.2\n##source=tests/golden/make_golden_train.py\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    body = "".join(f"{contig}\t{p}\t.\t{r}\t{alt}\t50\tPASS\t.\t{fmt}\n" for p, (r, alt, fmt) in sorted(rows.items()))
    body += f"chrOther\t{at_site[0]}\t.\tA\tC\t50\tPASS\t.\tGT\t0/1\n"                            # a contig the run does not hold
    return head + body.encode()


def check_case(case, contig, seq, vcf, true_var, td, tensor_rows, counts, counts5):
    """a fixture must prove something, and the restated rules must reproduce it: see the asserts"""
    from tests import label_rules as lr
    rows = lr.true_var_rows(vcf.decode())
    mine = "".join("%s\t%s\t%s\t%s\t%d\t%d\n" % r for r in rows if r[0] == contig)
    assert mine.encode() == true_var, (case, "the restated splitter differs from DNA_SplitVcf")
    truth = lr.truth_table(vcf.decode(), [contig])
    names, labels, has_truth = lr.parse_td(td.decode())
    assert names == [f"{n.decode()}:{p.decode()}" for n, p, _ in tensor_rows], (case, "the .td rows are not the tensor's, in its order")
    keys = np.array([int(n.split(":")[1]) for n in names], np.int64)
    quads, hit = lr.site_quads(keys, seq[keys - 1], truth)
    assert np.array_equal(lr.one_hot(quads), labels) and np.array_equal(hit, has_truth), (case, "the restated labels differ from the reference's")
    assert (counts["variants"], counts["non_variants"], counts["truth"]) == (int(hit.sum()), int((~hit).sum()), len(truth)), (case, counts)
    assert counts["ratio"] == "1" and counts["recall"] == "%g" % (hit.sum() / len(truth)), (case, counts)
    thr, ratio = lr.threshold(counts5["variants"], counts5["non_variants"], 5.0)
    assert (thr is not None or counts5["non_variants"] <= 5 * counts5["variants"]) and counts5["ratio"] == "%g" % ratio and {k: counts5[k] for k in ("variants", "non_variants", "truth", "recall")} == \
        {k: counts[k] for k in ("variants", "non_variants", "truth", "recall")}, (case, counts5)
    # every label family occurs
    gt = {lr.GT21[int(np.argmax(y[:21]))] for y in labels[hit]}
    assert {"AIns", "CIns", "GIns", "TIns"} & gt and {"ADel", "CDel", "GDel", "TDel", "DelDel"} & gt and "InsDel" in gt, (case, gt)
    assert any(len(g) == 2 and g[0] != g[1] for g in gt) and any(len(g) == 2 and g[0] == g[1] for g in gt), (case, gt)
    assert {int(np.argmax(y[21:24])) for y in labels[hit]} == {0, 1, 2}, (case, "zygosity")
    assert all(y[24 + 32] == 1 and y[57 + 32] == 1 for y in labels[hit]) and all(y[24 + 16] == 1 and y[57 + 16] == 1 for y in labels[~hit])
    assert {int(np.argmax(y[:21])) for y in labels[~hit]} == {0, 4, 7, 9} and bool((seq[keys[~hit] - 1] >= 97).any()), (case, "reference labels")
    star = {r[3]: r for r in rows if r[0] == contig and r[3] in ("G,", ",G")}
    assert set(star) == {"G,", ",G"} and all(r[4:] == (0, 1) for r in star.values()), (case, "both '*' orders")
    for alt in star:
        y = labels[names.index(f"{contig}:{star[alt][1]}")]
        assert lr.GT21[int(np.argmax(y[:21]))] == star[alt][2] + "Ins", (case, "'G,' counts as one allele of length 2")
    assert len(truth) > int(hit.sum()), (case, "no truth variant lies at no candidate site")
    return int(hit.sum()), len(names)


def main():
    from nanosnp_amd import host
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "DNA_CreateCanSnpTensor")):
        sys.exit("oracle/_ref/DNA_CreateCanSnpTensor is missing: the fixtures can only be generated where the reference tree is (make -C oracle ref)")
    limit = max(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if not f.startswith("train_"))
    with tempfile.TemporaryDirectory() as bindir:
        compile_ref(bindir)
        for case, tag, bed in CASES:
            text = gzip.open(os.path.join(GOLD, f"encode_{tag}.mpileup.gz")).read()
            fa = gzip.open(os.path.join(GOLD, f"encode_{tag}.fa.gz")).read()
            contig = fa.split(b"\n")[0][1:].split()[0].decode()
            seq = np.frombuffer(b"".join(fa.split(b"\n")[1:]), np.uint8)
            ext = conf = None
            if bed is not None:
                ext, conf = os.path.join(GOLD, f"{bed}.ext.bed"), os.path.join(GOLD, f"{bed}.conf.bed")
            with tempfile.TemporaryDirectory() as d:
                fasta = os.path.join(d, "ref.fa")
                host.write_fasta(fasta, contig, seq)
                lost = []
                if bed is not None:
                    all_sites = {int(p) for _, p, _ in run_tensor(os.path.join(d, "nobed"), contig, fasta, text)}
                tensor_rows = run_tensor(d, contig, fasta, text, ext, conf)
                sites = [int(p) for _, p, _ in tensor_rows]
                if bed is not None:
                    lost = sorted(all_sites - set(sites))
                    assert lost, (case, "the BEDs remove no candidate")
                vcf = truth_vcf(case, contig, seq, sites, lost)
                true_var, td, counts = run_train(bindir, d, contig, fasta, vcf, 1000000, conf)
                _, td_again, _ = run_train(bindir, d, contig, fasta, vcf, 1000000, conf, tag="_again")
                assert td_again == td, (case, "two runs of the reference differ")
                _, _, counts5 = run_train(bindir, d, contig, fasta, vcf, 5, conf)
            n_var, n = check_case(case, contig, seq, vcf, true_var, td, tensor_rows, counts, counts5)
            if bed is not None:
                assert any(f"{contig}\t{p}\t".encode() in vcf for p in lost[:1]), case
            out = {".vcf": vcf, ".true_var": true_var, ".td.gz": gzip.compress(td, 9, mtime=0),
                   ".json": (json.dumps({"ratio_1000000": counts, "ratio_5": counts5}, indent=1, sort_keys=True) + "\n").encode()}
            for suffix, data in out.items():
                assert len(data) <= limit, (case, suffix, len(data), "larger than the largest fixture already there")
                with open(os.path.join(GOLD, case + suffix), "wb") as f:
                    f.write(data)
            print(f"{case}: {n} sites, {n_var} of them truth variants; ratio 5 -> {counts5['ratio']}; .td.gz {len(out['.td.gz'])} bytes")


if __name__ == "__main__":
    main()
