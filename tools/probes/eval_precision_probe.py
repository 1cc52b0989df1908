#!/usr/bin/env python3
"""What scoring costs in each arithmetic, beside calling in the same arithmetic (docs/rounds/r36.md).

  A/B/A/B   per round and per arithmetic p in 0 (fp32) / 2 (bf16x3) / 1 (f16x3): evaluate.evaluate_train_bins(precision=p,
            variants_only=False) and pipeline.predict_pileup_bins with pileup_precision = p on the SAME windows (one <chr>.td.bin of
            seeded windows with random one-hot labels, as eval_probe.py makes it), rounds alternating, wall time of each call.  Every round
            starts with evaluate_train_bins(precision=None), the fp32-only entry of the parent commit: the yardstick of the ratios.
  heads     the heads kernel alone from nsnp_ctx_read_timing (one event pair per launch): the scoring heads kernel of each arithmetic with
            and without the logit store, beside the probability heads kernel of the same arithmetic, at N = 4096 and 131072.

    python tools/probes/eval_precision_probe.py [sites=131072] [rounds=4]

Read the numbers per the measurement rules of DESIGN.md section 6: same process, alternating, the first round of each is the warm-up and is
printed but not averaged."""
from __future__ import annotations

import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NAMES = {0: "fp32", 2: "bf16x3", 1: "f16x3"}


def main():
    import torch
    from eval_probe import windows
    from nanosnp_amd import evaluate, pileup_model, sitefile
    from nanosnp_amd.pipeline import predict_pileup_bins
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    rng = np.random.default_rng(1)
    x = windows(n)
    label = np.zeros((n, 90), np.int32)
    for r0, c in ((0, 21), (21, 3), (24, 33), (57, 33)):
        label[np.arange(n), r0 + rng.integers(0, c, n)] = 1
    position = [f"chr1:{p + 1}:{'N' * 16}A{'N' * 16}" for p in range(n)]
    fai = f"chr1\t{n + 100}\t6\t60\t61\n"
    model = pileup_model.LSTMNetwork.from_npz(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"))
    ctx = model.ctx

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "chr1.td.bin")
        sitefile.write_train_bin(path, x, position, label)
        t = {k: [] for k in ["parent"] + [f"{w}{p}" for p in NAMES for w in ("eval", "predict")]}
        for r in range(rounds):
            ctx.set_option("pileup_precision", 0)
            dt, res = timed(lambda: evaluate.evaluate_train_bins(model, [path], variants_only=False))
            t["parent"].append(dt)
            line = [f"round {r}: fp32 entry of the parent {1e3 * dt:7.1f} ms ({n / dt / 1e6:.2f} M sites/s), sites {res['sites']}"]
            for p, name in NAMES.items():
                ctx.set_option("pileup_precision", p)
                de, res = timed(lambda: evaluate.evaluate_train_bins(model, [path], variants_only=False, precision=p))
                dp, _ = timed(lambda: predict_pileup_bins(model, [path], fai, os.path.join(d, "out.vcf")))
                t[f"eval{p}"].append(de); t[f"predict{p}"].append(dp)
                line.append(f"{name}: evaluate {1e3 * de:7.1f} ms ({n / de / 1e6:.2f} M sites/s) predict {1e3 * dp:7.1f} ms ({n / dp / 1e6:.2f} M sites/s)")
            print("   ".join(line))
        if rounds > 1:
            med = {k: float(np.median(v[1:])) for k, v in t.items()}
            print(f"median of rounds 1..: fp32 entry of the parent {1e3 * med['parent']:.1f} ms ({n / med['parent'] / 1e6:.2f} M sites/s)")
            for p, name in NAMES.items():
                e, q = med[f"eval{p}"], med[f"predict{p}"]
                print(f"  {name}: evaluate {1e3 * e:.1f} ms ({n / e / 1e6:.2f} M sites/s), {med['parent'] / e:.3f} x the parent's fp32 scoring rate; "
                      f"predict {1e3 * q:.1f} ms ({n / q / 1e6:.2f} M sites/s); evaluate / predict time {e / q:.3f}")
    ctx.enable_timing(True)
    for m in (4096, 131072):
        xd = torch.from_numpy(windows(m, seed=m).astype(np.int32)).cuda()
        cls = torch.from_numpy(np.stack([rng.integers(0, c, m) for c in (21, 3, 33, 33)], axis=1).astype(np.uint8)).cuda()
        counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
        for p, name in NAMES.items():
            ctx.set_option("pileup_precision", p)
            out = {}
            for what, run in (("predict heads", lambda: ctx.pileup_forward(xd)),
                              ("scoring heads", lambda: ctx.pileup_eval_windows(xd, None, cls, counters, precision=p)),
                              ("scoring heads + logits", lambda: ctx.pileup_eval_windows(xd, None, cls, counters, want_logits=True, precision=p)),
                              ("predict heads again", lambda: ctx.pileup_forward(xd))):
                run(); torch.cuda.synchronize(); ctx.read_timing()
                for _ in range(10):
                    run()
                torch.cuda.synchronize()
                ms, k = ctx.read_timing()["pileup_head"]
                out[what] = ms / 10
            print(f"N = {m}, {name}: heads kernel per forward " + ", ".join(f"{k} {1e3 * v:.1f} us" for k, v in out.items()))
    ctx.set_option("pileup_precision", 0)
    ctx.enable_timing(False)


if __name__ == "__main__":
    main()
