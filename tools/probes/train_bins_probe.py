#!/usr/bin/env python3
"""Development probe: pipeline.mpileup_to_train_bins (ONE whole-genome mpileup text + a truth VCF -> every <chr>.td.bin) at
max_non_variant_ratio None (B: one pass, every site kept) and 5.0 (C: a count pass, then the write pass with the subsample) against
pipeline.mpileup_to_bins_bed on the same text and the same two BEDs (A: the yardstick - the entry this one is built on, unchanged by it),
in one process, alternating A / B / C / A / B / C; the text in the page cache, outputs on tmpfs when /dev/shm is there.

    python tools/probes/train_bins_probe.py [contigs=3] [columns per contig=2000000] [steps=5]

The truth VCF names every 10th candidate site of run A (heterozygous SNPs) and as many positions that are no candidate.  Two warm-up
rounds, then the median wall time of each with the spread of the repeats, the time of reading the truth VCF on the host, and the
stages of the write passes."""
import json, os, shutil, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from nanosnp_amd import host, sitefile, truth
from nanosnp_amd.pileup_model import LSTMNetwork
from nanosnp_amd.pipeline import mpileup_to_bins_bed, mpileup_to_train_bins

n_ctg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
steps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
bare = LSTMNetwork(device=0)                                # no entry here needs weights
d = tempfile.mkdtemp(prefix="nsnp_train_bins_")
out_dir = tempfile.mkdtemp(prefix="nsnp_train_bins_out_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
names, fai, total, seqs = [f"chr{i + 1}s" for i in range(n_ctg)], "", 0, {}
whole, fasta = os.path.join(d, "pileup_data"), os.path.join(d, "ref.fa")
conf_bed, ext_bed = os.path.join(d, "conf.bed"), os.path.join(d, "ext.bed")
with open(fasta, "wb") as fa, open(whole, "wb") as w, open(conf_bed, "w") as cb, open(ext_bed, "w") as eb:
    for i, name in enumerate(names):
        cols = host.synth_columns(20261800 + i, n_cols, coverage=30.0, het_rate=0.03)
        text = memoryview(cols.mpileup_text_native(name))
        w.write(text)
        total += len(text)
        seqs[name] = np.array(cols.ref)
        seq = bytes(cols.ref)
        fa.write(b">" + name.encode() + b"\n" + b"\n".join(seq[a:a + 60] for a in range(0, len(seq), 60)) + b"\n")
        fai += f"{name}\t{len(seq)}\t0\t60\t61\n"
        for lo in range(0, len(seq), 10_000):               # 85 % of every 10 kb confident, the extended BED 50 bases wider
            cb.write(f"{name}\t{lo + 700}\t{min(lo + 9200, len(seq))}\n")
            eb.write(f"{name}\t{lo + 650}\t{min(lo + 9250, len(seq))}\n")
        del cols, text
beds = dict(extended_bed=ext_bed, confident_bed=conf_bed)


def run_a(st=None):
    t0 = time.perf_counter()
    sites = mpileup_to_bins_bed(bare, whole, fasta, fai, os.path.join(out_dir, "a"), contigs=names, stats=st, **beds)
    return time.perf_counter() - t0, sites


def run_train(tag, ratio, st=None):
    t0 = time.perf_counter()
    out = mpileup_to_train_bins(bare, whole, fasta, fai, vcf_path, os.path.join(out_dir, tag), contigs=names, max_non_variant_ratio=ratio, seed=1,
                                stats=st, **beds)
    return time.perf_counter() - t0, out


_, sites_a = run_a()
vcf_path, rows = os.path.join(d, "truth.vcf"), []
for name in names:
    pos = sitefile.read_pileup_bin(os.path.join(out_dir, "a", f"{name}.pd.bin"))[1]
    at = set(pos[::10].tolist())
    at |= {int(p) + 1 for p in pos[5::10].tolist() if int(p) + 1 <= seqs[name].size} - set(pos.tolist())
    for p in sorted(at):
        ref = chr(int(seqs[name][p - 1]) & ~0x20)
        rows.append(f"{name}\t{p}\t.\t{ref}\t{'ACGT'['ACGT'.index(ref) - 1]}\t50\tPASS\t.\tGT\t0/1\n")
with open(vcf_path, "w") as f:
    f.write("##fileformat=VCFv4.2\n" + "".join(rows))
t0 = time.perf_counter()
n_truth = truth.load_truth(vcf_path, names)[0].size
t_truth = time.perf_counter() - t0

for _ in range(2):                                         # warm-up: buffer sets, pinned memory, the page cache
    run_a(); run_train("b", None); run_train("c", 5.0)
ta, tb, tc, sa, sb, sc = [], [], [], {}, {}, {}
for _ in range(steps):
    t, sites_a = run_a(sa); ta.append(t)
    t, out_b = run_train("b", None, sb); tb.append(t)
    t, out_c = run_train("c", 5.0, sc); tc.append(t)
assert {n: o["kept"] for n, o in out_b.items()} == sites_a, "ratio None wrote other site counts than mpileup_to_bins_bed"
for n in names:
    a, b = sitefile.read_arrays(os.path.join(out_dir, "a", f"{n}.pd.bin")), sitefile.read_arrays(os.path.join(out_dir, "b", f"{n}.td.bin"))
    assert all(np.array_equal(a[k], b[k]) for k in a), f"{n}: the rows of the .td.bin differ from the .pd.bin's"
cols_all = n_ctg * n_cols
med = statistics.median
stages = ("setup_s", "issue_s", "wait_counts_s", "wait_parse_s", "drain_s", "gpu_s", "tok_s", "h2d_s", "count_pass_s", "wait_labels_s")
rate = lambda ts: dict(median_s=round(med(ts), 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4), Mcols_per_s=round(cols_all / med(ts) / 1e6, 2))
res = dict(probe="train_bins", gpu=torch.cuda.get_device_name(0), contigs=n_ctg, columns=cols_all, text_MB=round(total / 1e6, 1), steps=steps,
           sites=sum(sites_a.values()), truth_rows=n_truth, load_truth_s=round(t_truth, 3),
           variants=sum(o["variants"] for o in out_c.values()), non_variants=sum(o["non_variants"] for o in out_c.values()),
           kept_at_ratio_5=sum(o["kept"] for o in out_c.values()), rows_identical_to_pd_bin=True,
           A_mpileup_to_bins_bed=rate(ta), B_train_ratio_none=rate(tb), C_train_ratio_5=rate(tc),
           B_over_A=round(med(tb) / med(ta), 3), C_over_A=round(med(tc) / med(ta), 3),
           record_bytes_per_step=dict(A=int(sa["record_bytes"] / steps), B=int(sb["record_bytes"] / steps), C=int(sc["record_bytes"] / steps)),
           restarts=dict(A=sa.get("restarts", 0), B=sb.get("restarts", 0), C=sc.get("restarts", 0)),
           A_stages_s_per_step={k: round(sa.get(k, 0.0) / steps, 4) for k in stages},
           B_stages_s_per_step={k: round(sb.get(k, 0.0) / steps, 4) for k in stages},
           C_stages_s_per_step={k: round(sc.get(k, 0.0) / steps, 4) for k in stages})
print(json.dumps(res))
shutil.rmtree(d); shutil.rmtree(out_dir)
