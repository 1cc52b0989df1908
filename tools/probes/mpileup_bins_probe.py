#!/usr/bin/env python3
"""Development probe: pipeline.mpileup_to_bins (B: ONE whole-genome mpileup text -> every <chr>.pd.bin) against pipeline.make_pileup_bins
over the pre-split <chr>.mpileup files of the same text (A: the yardstick, which leaves the splitter's pass out), in one process,
alternating A / B / A / B; texts in the page cache, outputs on tmpfs when /dev/shm is there.

    python tools/probes/mpileup_bins_probe.py [contigs=3] [columns per contig=6000000] [steps=5]

Two warm-up passes each, then the median wall time of both with the spread of the repeats; the HIP-event time per chunk of the record
kernels of either path on the same sites (nsnp_pileup_window_records / nsnp_pileup_alt_info against their _keys siblings); and what the
pass A leaves out would have cost on the host: one thread reading the whole text and writing the per-contig files, timed here as a
line-wise copy (the reference's DNA_ExtractChrPileupData does the same work through a line reader)."""
import json, os, shutil, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from nanosnp_amd import host
from nanosnp_amd.pileup_model import LSTMNetwork
from nanosnp_amd.pipeline import make_pileup_bins, mpileup_to_bins

n_ctg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 6_000_000
steps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
bare = LSTMNetwork(device=0)                                # neither entry needs weights
d = tempfile.mkdtemp(prefix="nsnp_mpileup_bins_")
out_dir = tempfile.mkdtemp(prefix="nsnp_mpileup_bins_out_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
names, fai, total = [f"chr{i + 1}s" for i in range(n_ctg)], "", 0
whole = os.path.join(d, "pileup_data")
with open(os.path.join(d, "ref.fa"), "wb") as fa, open(whole, "wb") as w:
    for i, name in enumerate(names):
        cols = host.synth_columns(20261000 + i, n_cols, coverage=30.0, het_rate=0.03)
        text = memoryview(cols.mpileup_text_native(name))
        with open(os.path.join(d, f"{name}.mpileup"), "wb") as f:
            f.write(text)
        w.write(text)
        total += len(text)
        seq = bytes(cols.ref)
        fa.write(b">" + name.encode() + b"\n" + b"\n".join(seq[a:a + 60] for a in range(0, len(seq), 60)) + b"\n")
        fai += f"{name}\t{len(seq)}\t0\t60\t61\n"
        del cols, text
items = [(n, os.path.join(d, f"{n}.mpileup")) for n in names]
fasta = os.path.join(d, "ref.fa")


def run_a(st=None):
    t0 = time.perf_counter()
    sites = make_pileup_bins(bare, items, fasta, fai, os.path.join(out_dir, "a"), stats=st)
    return time.perf_counter() - t0, sites


def run_b(st=None):
    t0 = time.perf_counter()
    sites = mpileup_to_bins(bare, whole, fasta, fai, os.path.join(out_dir, "b"), contigs=names, stats=st)
    return time.perf_counter() - t0, sites


def split_pass():
    """the host pass A presupposes: every line of the whole text read and written to its contig's file by one thread"""
    t0 = time.perf_counter()
    outs, last, out = {}, None, None
    with open(whole, "rb") as f:
        for line in f:
            name = line.split(None, 1)[0]
            if name != last:
                last = name
                out = outs[name] = open(os.path.join(out_dir, name.decode() + ".split"), "wb")
            out.write(line)
    for o in outs.values():
        o.close()
    return time.perf_counter() - t0


for _ in range(2):                                         # warm-up: buffer sets, pinned memory, the page cache
    run_a(); run_b()
ta, tb, sa, sb = [], [], {"time_records": True}, {"time_records": True}
for _ in range(steps):
    t, sites_a = run_a(sa); ta.append(t)
    t, sites_b = run_b(sb); tb.append(t)
assert sites_a == sites_b, "mpileup_to_bins wrote other site counts than make_pileup_bins"
for n in names:
    with open(os.path.join(out_dir, "a", f"{n}.pd.bin"), "rb") as fa_, open(os.path.join(out_dir, "b", f"{n}.pd.bin"), "rb") as fb_:
        assert fa_.read() == fb_.read(), f"{n}.pd.bin differs between the two paths"
t_split = split_pass()
cols_all = n_ctg * n_cols
med = statistics.median
stages = ("setup_s", "issue_s", "wait_counts_s", "wait_parse_s", "drain_s", "gpu_s", "tok_s", "h2d_s")
per_chunk = lambda st: dict(window_records=round(1e3 * st["window_records_s"] / st["record_chunks"], 3),
                            alt_info=round(1e3 * st["alt_info_s"] / st["record_chunks"], 3), chunks=int(st["record_chunks"] / steps))
rate = lambda ts: dict(median_s=round(med(ts), 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4), Mcols_per_s=round(cols_all / med(ts) / 1e6, 2))
res = dict(probe="mpileup_bins", gpu=torch.cuda.get_device_name(0), contigs=n_ctg, columns=cols_all, text_MB=round(total / 1e6, 1), steps=steps,
           sites=sum(sites_b.values()), files_identical=True,
           A_make_pileup_bins=rate(ta), B_mpileup_to_bins=rate(tb),
           A_record_kernels_ms_per_chunk=per_chunk(sa), B_keys_record_kernels_ms_per_chunk=per_chunk(sb),
           A_record_kernels_s_per_step=dict(window_records=round(sa["window_records_s"] / steps, 5), alt_info=round(sa["alt_info_s"] / steps, 5)),
           B_keys_record_kernels_s_per_step=dict(window_records=round(sb["window_records_s"] / steps, 5), alt_info=round(sb["alt_info_s"] / steps, 5)),
           B_restarts=sb.get("restarts", 0), host_split_pass_s=round(t_split, 3),
           A_stages_s_per_step={k: round(sa.get(k, 0.0) / steps, 4) for k in stages},
           B_stages_s_per_step={k: round(sb.get(k, 0.0) / steps, 4) for k in stages})
print(json.dumps(res))
shutil.rmtree(d); shutil.rmtree(out_dir)
