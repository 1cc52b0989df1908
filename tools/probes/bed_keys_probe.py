#!/usr/bin/env python3
"""Development probe: the keyed BED kernels against their `pos` neighbours, and pipeline.call_mpileup_bed against pipeline.call_variants with
the same BEDs over the pre-split per-contig files.

    python tools/probes/bed_keys_probe.py [contigs=3] [columns per contig=2000000] [steps=5] [kernel columns=760000]

1. nsnp_pileup_filter_columns / nsnp_pileup_filter_columns_keys and nsnp_pileup_encode_columns3 / nsnp_pileup_encode_columns_keys on the same
   single-contig columns (the keyed ones see them as contig 1 of a three-contig table), HIP events around every call, A / B / A / B;
   asserts that the outputs are equal.
2. A: call_variants(extended_bed=, confident_bed=) over the per-contig files, B: call_mpileup_bed over the one text, alternating, files
   in the page cache; asserts that the two VCFs are equal.
Prints medians with the spread of the repeats and one JSON line."""
import json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from nanosnp_amd import _lib, bed, host
from nanosnp_amd.fixtures import load_pileup_weights
from nanosnp_amd.pileup_model import LSTMNetwork
from nanosnp_amd.pipeline import call_mpileup_bed, call_variants

n_ctg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
steps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
m_k = int(sys.argv[4]) if len(sys.argv) > 4 else 760_000
model = LSTMNetwork(device=0).load_weight_list(load_pileup_weights())
ctx = model.ctx
dev = torch.device("cuda", 0)
med = lambda v: statistics.median(v)
spread = lambda v: (max(v) - min(v)) / med(v)
result = {}


def intervals(rng, n, longest, gap):
    iv, at = [], 0
    while at < n:
        k = int(rng.integers(1, longest))
        iv.append((at, min(n, at + k)))
        at += k + int(rng.integers(1, gap))
    return np.asarray(iv, np.int64)


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(1)
cols = host.synth_columns(20261700, m_k, coverage=30.0, het_rate=0.03)
seq = cols.ref.copy()
side = rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000).astype(np.uint8)
table = _lib.ContigTable({"left": side, "mid": seq, "right": side}, device=0)
iv_ext, iv_conf = intervals(rng, m_k, 3000, 400), intervals(rng, m_k, 300, 300)
w_ext, w_conf = bed.bed_bitmap(iv_ext, m_k), bed.bed_bitmap(iv_conf, m_k)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
pos = np.arange(1, m_k + 1, dtype=np.int64)
d_pos, d_key = up(pos), up(pos | (1 << _lib.KEY_SHIFT))
d_off, d_bases, d_ref = up(cols.col_off), up(cols.bases), up(cols.ref)
t_ext = _lib.BedTable.upload(table, *bed.table_bitmaps({"mid": iv_ext}, table.names, table.lengths))
t_conf = _lib.BedTable.upload(table, *bed.table_bitmaps({"mid": iv_conf, "right": [[0, 5000]]}, table.names, table.lengths))
b_ext, b_conf = up(w_ext), up(w_conf)
aux = torch.arange(m_k, dtype=torch.int32, device=dev)
out_p = out_k = out_a = None


def fil_pos():
    global out_p
    out_p = ctx.pileup_filter_columns(d_pos, d_off, d_bases, d_ref, b_ext, m_k, out=None if out_p is None else out_p[:4])
def fil_key():
    global out_k
    out_k = ctx.pileup_filter_columns_keys(d_key, d_off, d_bases, d_ref, table, t_ext, out=None if out_k is None else out_k[:4])
def fil_key_aux():
    global out_a
    out_a = ctx.pileup_filter_columns_keys(d_key, d_off, d_bases, d_ref, table, t_ext, aux=aux, out=None if out_a is None else out_a[:5])
enc = {}
def enc_pos():
    enc["p"] = ctx.pileup_encode_columns3(d_bases, d_off, d_ref, d_pos, b_conf, m_k, want_max_del=False)
def enc_key():
    enc["k"] = ctx.pileup_encode_columns_keys(d_bases, d_off, d_ref, d_key, table, t_conf, want_max_del=False)
def enc_plain():
    enc["0"] = ctx.pileup_encode_columns(d_bases, d_off, d_ref)


def timed(fns, reps=20):
    for f in fns:
        f(); f()
    torch.cuda.synchronize()
    ms = {f.__name__: [] for f in fns}
    for _ in range(reps):
        for f in fns:                                      # A / B / A / B
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); e1.synchronize()
            ms[f.__name__].append(e0.elapsed_time(e1))
    return ms

for group in ((fil_pos, fil_key, fil_key_aux), (enc_plain, enc_pos, enc_key)):
    for name, v in timed(group).items():
        result[name + "_us"] = round(med(v) * 1e3, 1)
        print(f"{name:12s} {med(v) * 1e3:9.1f} us  (spread {spread(v):.2f}, {m_k} columns, {int(cols.col_off[-1])} bytes)")
torch.cuda.synchronize()
K = int(out_p[4][0])
assert out_p[4].tolist() == out_k[5].tolist() == out_a[5].tolist() and 0 < K < m_k
assert torch.equal(out_p[0][:K] | (1 << _lib.KEY_SHIFT), out_k[0][:K]) and torch.equal(out_p[2][:int(out_p[4][1])], out_k[2][:int(out_p[4][1])])
assert torch.equal(out_p[1][:K + 1], out_k[1][:K + 1]) and torch.equal(out_p[3][:K], out_k[3][:K]) and torch.equal(out_a[4][:K], aux[out_p[0][:K] - 1])
assert all(torch.equal(a, b) for a, b in zip(enc["p"][:3], enc["k"][:3])) and not torch.equal(enc["p"][2], enc["0"][2])
result.update(kernel_columns=m_k, kernel_kept=K)
del cols, d_bases, out_p, out_k, out_a, enc

# ---- 2. the pipelines -------------------------------------------------------------------------------------------------------------------
d = tempfile.mkdtemp(prefix="nsnp_bed_keys_")
names, fai, ext, conf = [f"chr{i + 1}s" for i in range(n_ctg)], "", {}, {}
with open(os.path.join(d, "pileup_data"), "wb") as whole, open(os.path.join(d, "ref.fa"), "wb") as fa:
    for i, name in enumerate(names):
        c = host.synth_columns(20261000 + i, n_cols, coverage=30.0, het_rate=0.03)
        text = memoryview(c.mpileup_text_native(name))
        with open(os.path.join(d, f"{name}.mpileup"), "wb") as f:
            f.write(text)
        whole.write(text)
        s = bytes(c.ref)
        fa.write(b">" + name.encode() + b"\n" + b"\n".join(s[a:a + 60] for a in range(0, len(s), 60)) + b"\n")
        fai += f"{name}\t{len(s)}\t0\t60\t61\n"
        ext[name], conf[name] = intervals(rng, n_cols, 3000, 400), intervals(rng, n_cols, 300, 300)
        del c, text
items = [(n, os.path.join(d, f"{n}.mpileup")) for n in names]
fasta, va, vb = os.path.join(d, "ref.fa"), os.path.join(d, "a.vcf"), os.path.join(d, "b.vcf")


def run_a(st=None):
    t0 = time.perf_counter()
    rows = call_variants(model, items, fasta, fai, va, stats=st, extended_bed=ext, confident_bed=conf)
    return time.perf_counter() - t0, rows


def run_b(st=None):
    t0 = time.perf_counter()
    rows = call_mpileup_bed(model, os.path.join(d, "pileup_data"), fasta, fai, vb, stats=st, extended_bed=ext, confident_bed=conf)
    return time.perf_counter() - t0, rows


for _ in range(2):                                         # warm-up: buffer sets, pinned memory, the page cache
    run_a(); run_b()
ta, tb, sa, sb = [], [], {}, {}
for _ in range(steps):
    t, rows_a = run_a(sa); ta.append(t)
    t, rows_b = run_b(sb); tb.append(t)
assert rows_a == rows_b > 0 and open(va, "rb").read() == open(vb, "rb").read(), "call_mpileup_bed differs from call_variants"
total = n_ctg * n_cols
print(f"call_variants + BEDs    {total / med(ta) / 1e6:7.2f} M columns/s  median {med(ta) * 1e3:8.1f} ms (spread {spread(ta):.2f})  gpu_s/run {sa['gpu_s'] / steps:.4f}")
print(f"call_mpileup_bed        {total / med(tb) / 1e6:7.2f} M columns/s  median {med(tb) * 1e3:8.1f} ms (spread {spread(tb):.2f})  gpu_s/run {sb['gpu_s'] / steps:.4f}")
result.update(contigs=n_ctg, columns=total, rows=rows_a, call_variants_bed_ms=round(med(ta) * 1e3, 1), call_mpileup_bed_ms=round(med(tb) * 1e3, 1),
              call_variants_bed_spread=round(spread(ta), 3), call_mpileup_bed_spread=round(spread(tb), 3),
              call_variants_bed_gpu_ms=round(sa["gpu_s"] / steps * 1e3, 1), call_mpileup_bed_gpu_ms=round(sb["gpu_s"] / steps * 1e3, 1))
print(json.dumps(result))
for f in os.listdir(d):
    os.remove(os.path.join(d, f))
os.rmdir(d)
