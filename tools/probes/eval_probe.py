#!/usr/bin/env python3
"""What scoring costs beside calling (docs/rounds/r20.md).

  A/B/A/B   evaluate.evaluate_train_bins(variants_only=False) against pipeline.predict_pileup_bins on the SAME windows (one <chr>.td.bin
            of seeded windows with random one-hot labels: predict_pileup_bins reads its position_matrix and position arrays and ignores
            the labels), rounds alternating, wall time of each call.
  heads     the heads kernel alone from nsnp_ctx_read_timing (one event pair per launch): k_pileup_head_eval with loss and counts, with and
            without the logit store, beside k_pileup_head_rs, at N = 4096 and 131072.

    python tools/probes/eval_probe.py [sites=131072] [rounds=4]

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


def windows(n, seed=20261020):
    """plausible windows: small counts, a dominant reference channel per position (negative as the encoder writes it)"""
    rng = np.random.default_rng(seed)
    x = rng.poisson(0.3, (n, 33, 18)).astype(np.int16)
    ref = rng.integers(0, 4, (n, 33))
    depth = rng.integers(8, 40, (n, 33)).astype(np.int16)
    np.put_along_axis(x, ref[..., None], -depth[..., None], axis=2)
    np.put_along_axis(x, (ref + 9)[..., None], -(depth // 2)[..., None], axis=2)
    return x


def main():
    import torch
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
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "chr1.td.bin")
        sitefile.write_train_bin(path, x, position, label)
        t_eval, t_pred = [], []
        for r in range(rounds):
            t0 = time.perf_counter()
            res = evaluate.evaluate_train_bins(model, [path], variants_only=False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            predict_pileup_bins(model, [path], fai, os.path.join(d, "out.vcf"))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_eval.append(t1 - t0); t_pred.append(t2 - t1)
            print(f"round {r}: evaluate {1e3 * (t1 - t0):8.1f} ms ({n / (t1 - t0) / 1e6:.2f} M sites/s)   predict {1e3 * (t2 - t1):8.1f} ms "
                  f"({n / (t2 - t1) / 1e6:.2f} M sites/s)   sites {res['sites']}")
        if rounds > 1:
            e, p = np.median(t_eval[1:]), np.median(t_pred[1:])
            print(f"median of rounds 1..: evaluate {1e3 * e:.1f} ms, predict {1e3 * p:.1f} ms, ratio {e / p:.3f}")
    ctx = model.ctx
    ctx.enable_timing(True)
    for m in (4096, 131072):
        xd = torch.from_numpy(windows(m, seed=m).astype(np.int32)).cuda()
        cls = torch.from_numpy(np.stack([rng.integers(0, c, m) for c in (21, 3, 33, 33)], axis=1).astype(np.uint8)).cuda()
        counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
        out = {}
        for name, run in (("head_rs", lambda: ctx.pileup_forward(xd)), ("head_eval", lambda: ctx.pileup_eval_windows(xd, None, cls, counters)),
                          ("head_eval+logits", lambda: ctx.pileup_eval_windows(xd, None, cls, counters, want_logits=True)),
                          ("head_rs again", lambda: ctx.pileup_forward(xd))):
            run(); torch.cuda.synchronize(); ctx.read_timing()
            for _ in range(10):
                run()
            torch.cuda.synchronize()
            ms, k = ctx.read_timing()["pileup_head"]
            out[name] = ms / 10
        print(f"N = {m}: heads kernel per forward " + ", ".join(f"{k} {1e3 * v:.1f} us" for k, v in out.items()))
    ctx.enable_timing(False)


if __name__ == "__main__":
    main()
