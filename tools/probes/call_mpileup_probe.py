#!/usr/bin/env python3
"""Development probe: pipeline.call_mpileup (B: one whole-genome mpileup text, contigs found on the device) against pipeline.call_variants
over the pre-split per-contig files (A: the yardstick), in one process, alternating A / B / A / B on files in the page cache.

    python tools/probes/call_mpileup_probe.py [contigs=3] [columns per contig=6000000] [steps=5]

Prints the median rate of both in columns / s with the spread of the repeats, the HIP-event time of the tokeniser launches per chunk
(nsnp_mpileup_tokenise against nsnp_mpileup_tokenise_contigs: the difference is what the five added launches cost), and asserts that
the two outputs are equal."""
import json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from nanosnp_amd import host
from nanosnp_amd.fixtures import load_pileup_weights
from nanosnp_amd.pileup_model import LSTMNetwork
from nanosnp_amd.pipeline import call_mpileup, call_variants

n_ctg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 6_000_000
steps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
model = LSTMNetwork(device=0).load_weight_list(load_pileup_weights())
d = tempfile.mkdtemp(prefix="nsnp_call_mpileup_")
names, fai, total = [f"chr{i + 1}s" for i in range(n_ctg)], "", 0
with open(os.path.join(d, "pileup_data"), "wb") as whole, open(os.path.join(d, "ref.fa"), "wb") as fa:
    for i, name in enumerate(names):
        cols = host.synth_columns(20261000 + i, n_cols, coverage=30.0, het_rate=0.03)
        text = memoryview(cols.mpileup_text_native(name))
        with open(os.path.join(d, f"{name}.mpileup"), "wb") as f:
            f.write(text)
        whole.write(text); total += len(text)
        seq = bytes(cols.ref)
        fa.write(b">" + name.encode() + b"\n" + b"\n".join(seq[a:a + 60] for a in range(0, len(seq), 60)) + b"\n")
        fai += f"{name}\t{len(seq)}\t0\t60\t61\n"
        del cols, text
items = [(n, os.path.join(d, f"{n}.mpileup")) for n in names]
fasta, out_a, out_b = os.path.join(d, "ref.fa"), os.path.join(d, "a.vcf"), os.path.join(d, "b.vcf")


def run_a(st=None):
    t0 = time.perf_counter()
    rows = call_variants(model, items, fasta, fai, out_a, stats=st)
    return time.perf_counter() - t0, rows


def run_b(st=None):
    t0 = time.perf_counter()
    rows = call_mpileup(model, os.path.join(d, "pileup_data"), fasta, fai, out_b, stats=st)
    return time.perf_counter() - t0, rows


for _ in range(2):                                         # warm-up: buffer sets, pinned memory, the page cache
    run_a(); run_b()
ta, tb, sa, sb = [], [], {}, {}
for _ in range(steps):
    t, rows_a = run_a(sa); ta.append(t)
    t, rows_b = run_b(sb); tb.append(t)
assert rows_a == rows_b and open(out_a, "rb").read() == open(out_b, "rb").read(), "call_mpileup differs from call_variants"
cols_all = n_ctg * n_cols
med = lambda v: statistics.median(v)
res = dict(probe="call_mpileup", gpu=torch.cuda.get_device_name(0), contigs=n_ctg, columns=cols_all, text_MB=round(total / 1e6, 1), steps=steps, rows=rows_a,
           A_call_variants=dict(median_s=round(med(ta), 4), min_s=round(min(ta), 4), max_s=round(max(ta), 4), Mcols_per_s=round(cols_all / med(ta) / 1e6, 2)),
           B_call_mpileup=dict(median_s=round(med(tb), 4), min_s=round(min(tb), 4), max_s=round(max(tb), 4), Mcols_per_s=round(cols_all / med(tb) / 1e6, 2)),
           tokenise_ms_per_chunk=dict(A=round(1e3 * sa["tok_s"] / sa["chunks"], 3), B=round(1e3 * sb["tok_s"] / sb["chunks"], 3), chunks_A=int(sa["chunks"] / steps),
                                      chunks_B=int(sb["chunks"] / steps)),
           B_stages_s_per_step={k: round(sb[k] / steps, 4) for k in ("setup_s", "issue_s", "wait_counts_s", "wait_parse_s", "drain_s", "vcf_s", "gpu_s", "h2d_s")},
           A_stages_s_per_step={k: round(sa.get(k, 0.0) / steps, 4) for k in ("setup_s", "issue_s", "wait_counts_s", "wait_parse_s", "drain_s", "vcf_s", "gpu_s", "h2d_s")})
print(json.dumps(res))
for f in os.listdir(d):
    os.remove(os.path.join(d, f))
os.rmdir(d)
