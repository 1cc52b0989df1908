#!/usr/bin/env python3
"""Development probe of the BED region filters (docs/rounds/r08.md):

  filter   nsnp_pileup_filter_columns alone on the columns of synthetic 30x text (default 6 M columns) with a BED keeping about half of
           them in runs: HIP-event time per call, the bytes it moves (positions, offsets, reference bytes and column bytes read; the kept
           ones written) as a rate and as a fraction of HBM, beside a device-to-device hipMemcpyAsync of the same number of bytes in the
           same process
  e2e      pipeline.call_contig, text to VCF rows, on the same contig without BEDs and with extended + confident BEDs covering about
           100 %, 10 % and 1 % of it: wall time per contig (median of the steps)

    python tools/probes/bed_probe.py [columns] [steps] [filter]        ("filter": the first part alone, e.g. under rocprofv3 --kernel-trace --stats)
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from nanosnp_amd import _lib, bed, host
from nanosnp_amd.fixtures import load_pileup_weights
from nanosnp_amd.pileup_model import LSTMNetwork
from nanosnp_amd.pipeline import call_contig

n_cols = int(sys.argv[1]) if len(sys.argv) > 1 else 6_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
HBM = 8000e9
cols = host.synth_columns(20261020, n_cols, coverage=30.0, het_rate=0.03)
seq = cols.ref.copy()
chr_len = int(seq.size)
rng = np.random.default_rng(1)


def panel(fraction, mean_len=300):
    """intervals of about mean_len bases covering about `fraction` of the contig"""
    if fraction >= 1.0:
        return np.array([[0, chr_len]], np.int64)
    n = max(1, int(chr_len * fraction / mean_len))
    lo = np.sort(rng.integers(0, chr_len - 2 * mean_len, n))
    return np.stack([lo, np.minimum(chr_len, lo + rng.integers(mean_len // 2, mean_len * 3 // 2, n))], 1)


dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
ctx = _lib.Context(0)
pos, off, bases, ref = dev(np.arange(1, n_cols + 1, dtype=np.int64)), dev(cols.col_off), dev(cols.bases), dev(cols.ref)
iv = panel(0.5)
words = bed.bed_bitmap(iv, chr_len)
bits = dev(words.view(np.int32))
kept = np.nonzero((words[(np.arange(n_cols) >> 5)] >> (np.arange(n_cols) & 31).astype(np.uint32)) & 1)[0]
kept_bytes = int((cols.col_off[kept + 1] - cols.col_off[kept]).sum())
out = None
for _ in range(3):
    po, oo, bo, ro, meta = ctx.pileup_filter_columns(pos, off, bases, ref, bits, chr_len, out=out)
    out = (po, oo, bo, ro)
torch.cuda.synchronize()
assert meta.tolist()[:2] == [kept.size, kept_bytes], (meta.tolist(), kept.size, kept_bytes)
reps = 30
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    ctx.pileup_filter_columns(pos, off, bases, ref, bits, chr_len, out=out, meta=meta)
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / reps
# bytes: the count pass reads positions and offsets, the scatter pass reads them again with the kept reference and column bytes, and
# writes 17 B per column (kept or filler) and the kept bytes
moved = n_cols * 16 + n_cols * 16 + kept.size + kept_bytes + n_cols * 17 + kept_bytes
src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
for _ in range(3):
    dst.copy_(src)
torch.cuda.synchronize()
e0.record()
for _ in range(reps):
    dst.copy_(src)                                   # hipMemcpyAsync device to device: moved / 2 read + moved / 2 written
e1.record(); torch.cuda.synchronize()
ms_cp = e0.elapsed_time(e1) / reps
print(f"filter: {n_cols} columns, {int(cols.col_off[-1]) / 1e6:.0f} MB of column bytes, {kept.size} kept ({kept_bytes / 1e6:.0f} MB): {ms * 1e3:.0f} us per call, "
      f"{moved / 1e6:.0f} MB moved = {moved / ms / 1e6:.0f} GB/s ({moved / (ms * 1e-3) / HBM:.3f} of HBM); "
      f"hipMemcpyAsync D2D of the same bytes: {ms_cp * 1e3:.0f} us = {moved / ms_cp / 1e6:.0f} GB/s ({moved / (ms_cp * 1e-3) / HBM:.3f} of HBM)")

if len(sys.argv) > 3 and sys.argv[3] == "filter":
    sys.exit(0)
model = LSTMNetwork().load_weight_list(load_pileup_weights())
text = cols.mpileup_text_native("chrP")
runs = [("no BED", {})]
for frac in (1.0, 0.1, 0.01):
    iv = panel(frac)
    cov = bed.bed_bitmap(iv, chr_len)
    runs.append((f"BEDs over {100.0 * sum(bin(int(x)).count('1') for x in cov[::97]) * 97 / chr_len:.1f} %", dict(extended_bed={"chrP": iv}, confident_bed={"chrP": iv})))
for name, kw in runs:
    times, res = [], None
    for s in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call_contig(model, text, "chrP", seq, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = np.sort(times[2:])
    print(f"e2e {name}: {np.median(t) * 1e3:.1f} ms per contig (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f}; {steps} steps), {res[1]} sites, {res[2]} rows")
