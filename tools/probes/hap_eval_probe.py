#!/usr/bin/env python3
"""What scoring a HaplotypeModel checkpoint costs beside calling with it (docs/rounds/r22.md).

  A/B/A/B   evaluate.evaluate_haplotype_bins against hap_pipeline.predict_haplotype_bins on the SAME labelled site files, every row kept
            (predict_haplotype_bins ignores the labels), rounds alternating, wall time of each call.
  heads     the heads launch alone from nsnp_ctx_read_timing (one event pair per pass): k_hap_head_eval with loss and counts, with and
            without the logit store, beside k_hap_heads, per pass of 16,384 sites.

    python tools/probes/hap_eval_probe.py [sites per file=16384] [files=2] [rounds=4]

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


def main():
    import torch
    from nanosnp_amd import evaluate, host, sitefile
    from nanosnp_amd.fixtures import seeded_hap_weights
    from nanosnp_amd.hap_pipeline import DeviceReference, predict_haplotype_bins
    from nanosnp_amd.haplotype_model import LSTMNetwork
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    n_files = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    rng = np.random.default_rng(1)
    model = LSTMNetwork(None).load_weight_list(seeded_hap_weights(13, H=256, ih_scale=0.03, head_scale=120.0))
    ref_len = 4 * n + 100
    refs = {"chr1": rng.choice(list(b"ACGT"), ref_len).astype(np.uint8)}
    reference = DeviceReference(refs, 0)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for f in range(n_files):
            pp = host.synth_hap_planes(100 + f, n, 30, 90, 33); ph = host.synth_hap_planes(200 + f, n, 30, 90, 11)
            posn = np.sort(rng.choice(np.arange(40, ref_len - 40), n, replace=False))
            cands = [f"chr1:{p}" for p in posn]
            hpos = [[f"chr1:{p + 3 * (k - 5)}" for k in range(11)] for p in posn]
            planes = dict(zip(sitefile.HAP_PLANES, (ph[0], ph[3], ph[1], ph[2], pp[0], pp[3], pp[1], pp[2])))
            labels = np.stack([np.ones(n), rng.integers(0, 10, n), rng.choice([-1, 1, 2], n)], axis=1)          # every row is kept
            paths.append(os.path.join(d, f"chr1_{f}_{f}.bin"))
            sitefile.write_haplotype_train_bin(paths[-1], cands, hpos, planes, labels)
        total = n * n_files
        t_eval, t_pred = [], []
        for r in range(rounds):
            st = {}
            t0 = time.perf_counter()
            res = evaluate.evaluate_haplotype_bins(model, paths, reference, stats=st)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            predict_haplotype_bins(model.ctx, paths, reference, os.path.join(d, "out.csv"))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_eval.append(t1 - t0); t_pred.append(t2 - t1)
            print(f"round {r}: evaluate {1e3 * (t1 - t0):8.1f} ms ({total / (t1 - t0) / 1e3:.1f} k sites/s)   predict {1e3 * (t2 - t1):8.1f} ms "
                  f"({total / (t2 - t1) / 1e3:.1f} k sites/s)   sites {res['sites']}  passes {st['passes']}", flush=True)
        if rounds > 1:
            e, p = np.median(t_eval[1:]), np.median(t_pred[1:])
            print(f"median of rounds 1..: evaluate {1e3 * e:.1f} ms, predict {1e3 * p:.1f} ms, evaluate / predict rate {p / e:.3f}")
        print(evaluate.format_haplotype_report(res))
    ctx = model.ctx
    ctx.enable_timing(True)
    m = 16384
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    xp = torch.randn((m, 105, 33), generator=g, device="cuda") * 30
    xh = torch.randn((m, 105, 11), generator=g, device="cuda") * 30
    cls = torch.from_numpy(np.stack([rng.integers(0, 10, m), rng.integers(0, 3, m)], axis=1).astype(np.uint8)).cuda()
    counters = ctx.hap_eval_counters()
    out = {}
    for name, run in (("k_hap_heads", lambda: ctx.hap_forward(xp, xh)), ("k_hap_head_eval", lambda: ctx.hap_eval(xp, xh, cls, counters)),
                      ("k_hap_head_eval+logits", lambda: ctx.hap_eval(xp, xh, cls, counters, want_logits=True)),
                      ("k_hap_heads again", lambda: ctx.hap_forward(xp, xh))):
        run(); torch.cuda.synchronize(); ctx.read_timing()
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        tim = ctx.read_timing()
        out[name] = (tim["hap_head"][0] / 5, tim["hap_lstm_chain"][0] / 5)
    print(f"N = {m}: heads launch per pass " + ", ".join(f"{k} {1e3 * v[0]:.1f} us (LSTM chain {v[1]:.1f} ms)" for k, v in out.items()))
    ctx.enable_timing(False)


if __name__ == "__main__":
    main()
