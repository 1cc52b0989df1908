#!/usr/bin/env python3
"""Times the two tie orders of the stage-4 read arrangement on the same inputs (nsnp_hap_arrange_reads2: NSNP_TIE_STABLE =
k_hap_arrange, NSNP_TIE_NUMPY1 = k_hap_arrange_numpy1), with HIP events around back-to-back launches, the modes interleaved.

    python tools/probes/arrange_probe.py [--sites 16384] [--reps 5] [--timed 20]

Two inputs:
  30x   tools/hap_bench.py's arrange shape: 16,384 sites, L = 33, R = 64 rows, D_out = 90, about 30 reads per site, some with no
        base at the centre column
  deep  120-150 kept reads per site, R = 160, D_out = 90: every site is cut, so the tie order decides which reads survive
Prints one JSON line per input: microseconds per launch of each mode (median of --reps interleaved passes) and their ratio."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def make_inputs(torch, dev, n, R, L, lo, hi, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    n_reads = torch.randint(lo, hi + 1, (n,), generator=g, device=dev, dtype=torch.int32).clamp_(max=R)
    live = torch.arange(R, device=dev)[None, :] < n_reads[:, None]
    seq = torch.randint(1, 5, (n, R, L), generator=g, device=dev, dtype=torch.int32)
    seq[:, :, L // 2] *= (torch.rand((n, R), generator=g, device=dev) > 0.05).int()      # reads with no base at the centre
    hp = torch.randint(1, 4, (n, R, 1), generator=g, device=dev, dtype=torch.int32).expand(n, R, L)
    bq = torch.randint(0, 60, (n, R, L), generator=g, device=dev, dtype=torch.int32)
    mq = torch.randint(0, 61, (n, R, L), generator=g, device=dev, dtype=torch.int32)
    mats = [(m * live[:, :, None].int()).contiguous() for m in (seq, bq, mq, hp)]
    return mats, n_reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    import torch
    from nanosnp_amd import _lib
    ctx = _lib.Context(0)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    L, D = 33, 90
    for name, R, lo, hi in (("30x", 64, 22, 38), ("deep", 160, 126, 158)):
        n = a.sites
        mats, n_reads = make_inputs(torch, dev, n, R, L, lo, hi, 11)
        outs = {m: [torch.empty((n, D, L), dtype=torch.int32, device=dev) for _ in range(4)] for m in (0, 1)}
        deps = {m: torch.empty(n, dtype=torch.int32, device=dev) for m in (0, 1)}
        P = lambda t: C.c_void_p(t.data_ptr())

        def launch(mode):
            rc = lib.nsnp_hap_arrange_reads2(ctx.handle, *[P(t) for t in mats], P(n_reads), n, R, L, D, mode,
                                             *[P(o) for o in outs[mode]], P(deps[mode]), C.c_void_p(stream.cuda_stream))
            _lib.check(rc, ctx.handle, "nsnp_hap_arrange_reads2")

        def timed(mode):
            for _ in range(a.warm):
                launch(mode)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.timed):
                launch(mode)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.timed

        us = {0: [], 1: []}
        for _ in range(a.reps):
            for mode in (0, 1):
                us[mode].append(timed(mode))
        torch.cuda.synchronize()
        # sanity: the same depth, the kept rows in non-decreasing centre HP, the same rows as a set per site
        hp0, hp1 = outs[0][3][:, :, L // 2], outs[1][3][:, :, L // 2]
        kept = torch.arange(D, device=dev)[None, :] < deps[1][:, None]
        ok = bool(torch.equal(deps[0], deps[1])) and bool(((hp1[:, 1:] >= hp1[:, :-1]) | ~kept[:, 1:]).all())
        ok = ok and bool(torch.equal(hp0.sort(1).values, hp1.sort(1).values))
        diff = float((outs[0][1] != outs[1][1]).any(2).any(1).float().mean())
        med = {m: sorted(v)[len(v) // 2] for m, v in us.items()}
        print(json.dumps({"input": name, "sites": n, "R": R, "L": L, "D_out": D,
                          "mean_reads_in": round(float(n_reads.float().mean()), 2), "mean_depth_out": round(float(deps[1].float().mean()), 2),
                          "stable_us": round(med[0], 2), "numpy1_us": round(med[1], 2), "ratio": round(med[1] / med[0], 3),
                          "stable_us_all": [round(x, 2) for x in us[0]], "numpy1_us_all": [round(x, 2) for x in us[1]],
                          "sites_with_a_different_order": round(diff, 4), "sanity_ok": ok}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
