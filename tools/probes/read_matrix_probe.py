#!/usr/bin/env python3
"""readmatrix.read_matrices_device (hap_reads.hip) against readmatrix.read_matrices on the same synthetic records, A/B/A/B.

    python tools/probes/read_matrix_probe.py [--reads 600] [--length 3000] [--groups 40] [--reps 2] [--timed 20]

What the ratio is and is not: the host side runs readmatrix.read_matrices through a Python stand-in for the alignment file (columns
served from a per-position index built beforehand, outside the timed region), so the host time is the cost of the per-column,
per-read Python loop of readmatrix.py alone.  It is NOT pysam's C pileup engine, which would add its own time in front of that loop;
nothing here reads a BAM.  The device time is the whole call: the upload of the records, three entry points, two small read-backs.

Also printed: HIP-event times of the two entry points with the records already on the device (median of --timed back-to-back calls
each) and the bytes they move (the four output matrices written once, the CIGAR words read by the span and the fill kernels, the
record scalars) against the 8 TB/s HBM peak.  At probe size the outputs are far below the size at which a bandwidth fraction means
anything: the figure is recorded, not judged.  One JSON line; no threshold is asserted."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

M, I, D, N, S = 0, 1, 2, 3, 4


def make_records(rng, n_reads, length, span):
    """nanopore-like records in coordinate order: M runs of ~12 bases between short I / D, a soft clip at either end, rare N"""
    recs = []
    for r in range(n_reads):
        a = int(rng.integers(1, span - length))
        ln = int(rng.integers(length // 2, length * 3 // 2))
        cigar, left = [(S, int(rng.integers(1, 40)))], ln
        while left > 0:
            n = int(min(left, rng.geometric(1 / 12.0))); cigar.append((M, n)); left -= n
            if left <= 0:
                break
            u = rng.random()
            if u < 0.45:
                cigar.append((I, int(rng.geometric(0.6))))
            elif u < 0.98:
                n = int(min(left, rng.geometric(0.6))); cigar.append((D, n)); left -= n
            else:
                n = int(min(left, rng.integers(20, 200))); cigar.append((N, n)); left -= n
        cigar.append((S, int(rng.integers(1, 40))))
        qlen = sum(n for op, n in cigar if op in (M, I, S))
        recs.append(dict(name=f"r{r}", a=a, cigar=cigar, seq="".join("ACGT"[k] for k in rng.integers(0, 4, qlen)),
                         quals=rng.integers(1, 60, qlen).astype(np.uint8), hp=int(rng.integers(1, 4)), mapq=int(rng.integers(0, 61))))
    recs.sort(key=lambda rd: rd["a"])
    return recs


class _Aln:
    def __init__(self, rd):
        self.query_name, self.query_sequence, self.query_qualities, self.mapping_quality = rd["name"], rd["seq"], rd["quals"], rd["mapq"]
        self.hp = rd["hp"]

    def has_tag(self, t):
        return t == "HP" and self.hp != 3

    def get_tag(self, t):
        return self.hp


class _Read:
    __slots__ = ("alignment", "is_del", "is_refskip", "query_position")

    def __init__(self, aln, kind, q):
        self.alignment, self.is_del, self.is_refskip, self.query_position = aln, kind == D, kind == N, q


class _Column:
    __slots__ = ("pos", "pileups", "n")

    def __init__(self, pos0, prs):
        self.pos, self.pileups, self.n = pos0, prs, len(prs)


class IndexedSamfile:
    """the columns of every position, built once from the CIGARs (untimed); pileup() only looks them up"""

    def __init__(self, recs):
        self.cols = {}
        for rd in recs:
            aln, pos, q = _Aln(rd), rd["a"], 0
            for op, n in rd["cigar"]:
                if op == M:
                    for k in range(n):
                        self.cols.setdefault(pos + k, []).append(_Read(aln, M, q + k))
                    pos += n; q += n
                elif op in (I, S):
                    q += n
                else:
                    for k in range(n):
                        self.cols.setdefault(pos + k, []).append(_Read(aln, op, None))
                    pos += n

    def pileup(self, contig, start, end, min_base_quality=0, min_mapping_quality=0):
        for p in range(max(start - 3, 1), end + 4):
            prs = self.cols.get(p)
            if prs:
                yield _Column(p - 1, prs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=600)
    ap.add_argument("--length", type=int, default=3000)
    ap.add_argument("--groups", type=int, default=40)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timed", type=int, default=20)
    a = ap.parse_args()
    import torch
    from nanosnp_amd import _lib, readmatrix
    rng = np.random.default_rng(39)
    span = max(a.reads * a.length // 30, 4 * a.length)                     # about 30x
    recs = make_records(rng, a.reads, a.length, span)
    centres = np.sort(rng.choice(np.arange(a.length, span - a.length), a.groups, replace=False))
    groups = []
    for c in centres.tolist():
        left = sorted(rng.choice(np.arange(c - 400, c - 2), 5, replace=False).tolist())
        right = sorted(rng.choice(np.arange(c + 2, c + 400), 5, replace=False).tolist())
        groups.append([("c", int(p)) for p in left + [c] + right])
    ar = readmatrix.AlignmentRecords.from_arrays(
        start=[rd["a"] for rd in recs], mapq=[rd["mapq"] for rd in recs], hp=[-1 if rd["hp"] == 3 else rd["hp"] for rd in recs],
        cigar=[(n << 4) | op for rd in recs for op, n in rd["cigar"]], cigar_off=np.cumsum([0] + [len(rd["cigar"]) for rd in recs]),
        seq="".join(rd["seq"] for rd in recs), qual=np.concatenate([rd["quals"] for rd in recs]),
        seq_off=np.cumsum([0] + [len(rd["seq"]) for rd in recs]), names=[rd["name"] for rd in recs], contig="c")
    sam = IndexedSamfile(recs)
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    readmatrix.read_matrices_device(ctx, ar, groups, 10000)                 # warm-up: allocator, first launches
    torch.cuda.synchronize()
    host_s, dev_s, rm_h, rm_d = [], [], None, None
    for _ in range(a.reps):                                                 # A/B/A/B
        t0 = time.perf_counter(); rm_h = readmatrix.read_matrices(sam, groups, 10000); host_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); rm_d = readmatrix.read_matrices_device(ctx, ar, groups, 10000); torch.cuda.synchronize()
        dev_s.append(time.perf_counter() - t0)
    equal = rm_h is not None and rm_d is not None and rm_h.names == rm_d.names and rm_h.positions == rm_d.positions and all(
        np.array_equal(x, y.cpu().numpy()) for x, y in zip((rm_h.seq, rm_h.hap, rm_h.baseq, rm_h.mapq), (rm_d.seq, rm_d.hap, rm_d.baseq, rm_d.mapq)))
    # ---- the entry points alone, records on the device ----
    rec = ar.to_device(dev)
    cols = torch.tensor(rm_d.positions, dtype=torch.int64, device=dev)
    rows, P = len(rm_d.names), len(rm_d.positions)

    def events(fn):
        for _ in range(3):
            fn()
        out = []
        for _ in range(a.timed):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return sorted(out)[len(out) // 2]
    depths_us = events(lambda: ctx.hap_read_depths(rec, cols, want_rows=True))
    matrices_us = events(lambda: ctx.hap_read_matrices(rec, cols, 10000, rows))
    n_ops, R = int(ar.cigar.size), len(ar)
    bytes_depths = 4 * n_ops + R * (8 + 16 + 12) + 3 * 4 * (R + P) + 4 * P
    bytes_matrices = bytes_depths - 4 * P + 16 * rows * P + 4 * n_ops + R * (8 + 1 + 4 + 32 + 12)     # (+ at most 2 bytes per filled cell)
    print(json.dumps({
        "reads": R, "cigar_ops": n_ops, "max_ops_per_read": int(np.diff(ar.cigar_off).max()), "bases": int(ar.seq.size), "groups": len(groups),
        "rows": rows, "columns": P, "equal": bool(equal),
        "host_python_loop_s": [round(x, 4) for x in host_s], "device_call_s": [round(x, 5) for x in dev_s],
        "ratio_host_over_device": round(min(host_s) / min(dev_s), 1),
        "hap_read_depths_us": round(depths_us, 1), "hap_read_matrices_us": round(matrices_us, 1),
        "bytes_depths": bytes_depths, "bytes_matrices": bytes_matrices,
        "hbm_fraction_depths": round(bytes_depths / (depths_us * 1e-6) / 8e12, 5),
        "hbm_fraction_matrices": round(bytes_matrices / (matrices_us * 1e-6) / 8e12, 5),
        "note": "host = the Python per-cell loop over a pre-built column index, not pysam's pileup engine; event times include launch gaps "
                "(9 and 12 launches) and, for hap_read_matrices, one stream wait"}), flush=True)
    ctx.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
