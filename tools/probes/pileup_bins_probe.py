#!/usr/bin/env python3
"""Development probe: pipeline.make_pileup_bins (B: stage s1 alone, <chr>.mpileup -> <chr>.pd.bin) against pipeline.call_variants on the
same texts (A: the fused text -> VCF path, the yardstick), in one process, alternating A / B / A / B; texts in the page cache, outputs on
tmpfs when /dev/shm is there.

    python tools/probes/pileup_bins_probe.py [contigs=3] [columns per contig=6000000] [steps=5]

Two warm-up passes each, then the median wall time of both with the spread of the repeats; for B the HIP-event time of the two record
kernels per chunk (nsnp_pileup_window_records, nsnp_pileup_alt_info), the bytes per site that cross PCIe towards the host (1,188 + 83 +
alt_info + 8 of offsets) and the main thread's waits, which say what bounds the run."""
import json, os, shutil, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from nanosnp_amd import host
from nanosnp_amd.fixtures import load_pileup_weights
from nanosnp_amd.pileup_model import LSTMNetwork
from nanosnp_amd.pipeline import call_variants, make_pileup_bins

n_ctg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 6_000_000
steps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
model = LSTMNetwork(device=0).load_weight_list(load_pileup_weights())
bare = LSTMNetwork(device=0)                                # make_pileup_bins needs no weights
d = tempfile.mkdtemp(prefix="nsnp_pileup_bins_")
out_dir = tempfile.mkdtemp(prefix="nsnp_pileup_bins_out_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
names, fai, total = [f"chr{i + 1}s" for i in range(n_ctg)], "", 0
with open(os.path.join(d, "ref.fa"), "wb") as fa:
    for i, name in enumerate(names):
        cols = host.synth_columns(20261000 + i, n_cols, coverage=30.0, het_rate=0.03)
        text = memoryview(cols.mpileup_text_native(name))
        with open(os.path.join(d, f"{name}.mpileup"), "wb") as f:
            f.write(text)
        total += len(text)
        seq = bytes(cols.ref)
        fa.write(b">" + name.encode() + b"\n" + b"\n".join(seq[a:a + 60] for a in range(0, len(seq), 60)) + b"\n")
        fai += f"{name}\t{len(seq)}\t0\t60\t61\n"
        del cols, text
items = [(n, os.path.join(d, f"{n}.mpileup")) for n in names]
fasta, out_a = os.path.join(d, "ref.fa"), os.path.join(out_dir, "a.vcf")


def run_a(st=None):
    t0 = time.perf_counter()
    rows = call_variants(model, items, fasta, fai, out_a, stats=st)
    return time.perf_counter() - t0, rows


def run_b(st=None):
    t0 = time.perf_counter()
    sites = make_pileup_bins(bare, items, fasta, fai, os.path.join(out_dir, "bins"), stats=st)
    return time.perf_counter() - t0, sum(sites.values())


for _ in range(2):                                         # warm-up: buffer sets, pinned memory, the page cache
    run_a(); run_b()
ta, tb, sa, sb = [], [], {}, {"time_records": True}
for _ in range(steps):
    t, rows_a = run_a(sa); ta.append(t)
    t, sites_b = run_b(sb); tb.append(t)
assert sites_b == sa["sites"] // steps, "make_pileup_bins wrote another number of sites than call_variants called"
cols_all = n_ctg * n_cols
med = statistics.median
file_bytes = sum(os.path.getsize(os.path.join(out_dir, "bins", f)) for f in os.listdir(os.path.join(out_dir, "bins")))
stages = ("setup_s", "issue_s", "wait_counts_s", "wait_parse_s", "drain_s", "gpu_s", "h2d_s")
res = dict(probe="pileup_bins", gpu=torch.cuda.get_device_name(0), contigs=n_ctg, columns=cols_all, text_MB=round(total / 1e6, 1), steps=steps, sites=sites_b,
           A_call_variants=dict(median_s=round(med(ta), 4), min_s=round(min(ta), 4), max_s=round(max(ta), 4), Mcols_per_s=round(cols_all / med(ta) / 1e6, 2)),
           B_make_pileup_bins=dict(median_s=round(med(tb), 4), min_s=round(min(tb), 4), max_s=round(max(tb), 4), Mcols_per_s=round(cols_all / med(tb) / 1e6, 2)),
           B_record_kernels_ms_per_chunk=dict(window_records=round(1e3 * sb["window_records_s"] / sb["record_chunks"], 3),
                                              alt_info=round(1e3 * sb["alt_info_s"] / sb["record_chunks"], 3), chunks=int(sb["record_chunks"] / steps)),
           B_d2h_bytes_per_site=round(sb["record_bytes"] / steps / max(sites_b, 1), 1), B_file_MB=round(file_bytes / 1e6, 1), B_restarts=sb.get("restarts", 0),
           B_stages_s_per_step={k: round(sb.get(k, 0.0) / steps, 4) for k in stages},
           A_stages_s_per_step={k: round(sa.get(k, 0.0) / steps, 4) for k in stages + ("vcf_s",)})
print(json.dumps(res))
shutil.rmtree(d); shutil.rmtree(out_dir)
