#!/usr/bin/env python3
"""merge.select_groups_rows (pileup_groups.hip) on device call rows against merge.select_groups on the VCF text of the same rows, A/B/A/B.

    python tools/probes/groups_probe.py [N ...] [--reps 2] [--timed 20] [--contigs 24]

Default sizes: 6,161 rows (the largest case of tests/test_gpu_select_groups.py) and 1,500,000 (the stage-2 sites of BASELINE configs[3]).
The rows are those of tests/group_rules.make_case, cut into --contigs runs.  What is timed: on the host merge.select_groups over the text
(the text itself is made beforehand by host.vcf_format_batches, untimed - in a run it already exists, the writer thread made it); on the
device merge.select_groups_rows with the rows and reference bytes resident (run table, cut table, the launches, the read-back of the
counts, the gathers for to_lists), and to_lists() apart, which goes back through the host writer for the selected sites.  Also the
HIP-event time of nsnp_pileup_select_groups alone (median of --timed calls, twelve launches and one memset).  One JSON line per size;
nothing is asserted but the equality of the two results."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", type=int, nargs="*", default=[3 * 2048 + 17, 1_500_000])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--contigs", type=int, default=24)
    a = ap.parse_args()
    import torch
    from nanosnp_amd import _lib, merge
    from tests import group_rules as gr
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    ok = True
    for n in a.sizes:
        lengths = [n // a.contigs + (r < n % a.contigs) for r in range(a.contigs)] if n >= 10 * a.contigs else [n]
        case = gr.make_case(41, lengths)
        text = gr.vcf_text(case)
        rows, ref = torch.from_numpy(case["rows"]).to(dev), torch.from_numpy(case["ref"]).to(dev)
        merge.select_groups_rows(ctx, rows, ref, case["names"], reference_bug=False)          # warm-up: allocator, first launches
        torch.cuda.synchronize()
        host_s, dev_s, lists_s, want, got, lists = [], [], [], None, None, None
        for _ in range(a.reps):                                                               # A/B/A/B
            t0 = time.perf_counter(); want = merge.select_groups(text, reference_bug=False); host_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); got = merge.select_groups_rows(ctx, rows, ref, case["names"], reference_bug=False); torch.cuda.synchronize()
            dev_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); lists = got.to_lists(); lists_s.append(time.perf_counter() - t0)
        equal = lists == want and list(lists) == list(want)
        ok = ok and equal
        run_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
        cuts = torch.from_numpy(merge.group_cuts()).to(dev)
        entry = lambda: ctx.pileup_select_groups(rows, ref, run_off, cuts, cap_groups=len(got))
        for _ in range(3):
            entry()
        times = []
        for _ in range(a.timed):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); entry(); e1.record(); e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        print(json.dumps({
            "rows": n, "contigs": len(lengths), "vcf_rows": text.count("\n"), "groups": len(got), "equal": bool(equal),
            "host_select_groups_s": [round(x, 4) for x in host_s], "device_select_groups_rows_s": [round(x, 5) for x in dev_s],
            "to_lists_s": [round(x, 4) for x in lists_s], "ratio_host_over_device": round(min(host_s) / min(dev_s), 1),
            "nsnp_pileup_select_groups_us": round(sorted(times)[len(times) // 2], 1),
            "bytes_read_per_row": 13 * 8 + 1, "note": "host = select_groups over text that already exists; device = rows already resident; "
            "the event time includes the launch gaps of twelve launches and the allocation of the outputs and the scratch"}), flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
