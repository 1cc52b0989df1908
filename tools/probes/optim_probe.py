#!/usr/bin/env python3
"""What the tail of a training step costs: the fused step (nsnp_optim_step through train.DeviceOptimizer, two launches) beside torch's
clip_grad_norm_ + a foreach Adam + a Python Lookahead on the same 24 tensors of the PileupModel (docs/rounds/r27.md).

    python tools/probes/optim_probe.py [N=2000] [step_repeats=2000] [batch_repeats=20]

The driver never touches the GPU.  It starts four child processes one after the other - fused, torch, fused, torch (A/B/A/B) - each under
its own time limit; a child warms up, times between two HIP events and prints one JSON line.  A child that ends with a Python error ends
that step and nothing else; a child that is killed by a signal or by its time limit ends the probe (nothing more is started on a device
that may be in trouble).

Per child, on a PileupTrainer with the shipped weights and gradients left by one nsnp_pileup_loss_grad call:
  step_us    `step_repeats` optimiser steps back to back (clip at 20, LookaheadAdam lr 1e-4, alpha 0.5, k 6), per step: host enqueue and
             device work together, whichever is longer - what a training loop sees
  batch_ms   `batch_repeats` iterations of what train_train_bins does per batch of N sites: the keep mask (p = 0.3), loss_and_grad, the step,
             the accuracy count
  grad_ms    the same iterations without the step
The share of a batch is step_us / batch_ms; batch_ms - grad_ms is the same thing measured in place."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 240
MAX_NORM = 20.0


class TorchLookahead:
    """lookahead.py:34-58 on foreach ops"""

    def __init__(self, base, params, alpha=0.5, k=6):
        self.base, self.params, self.alpha, self.k, self.n, self.slow = base, [p.detach() for p in params], alpha, k, 0, None

    def step(self):
        import torch
        self.base.step()
        self.n += 1
        if self.n % self.k == 0:
            if self.slow is None:
                self.slow = [p.clone() for p in self.params]
            torch._foreach_add_(self.slow, torch._foreach_sub(self.params, self.slow), alpha=self.alpha)
            torch._foreach_copy_(self.params, self.slow)


def side(which, n, step_repeats, batch_repeats):
    import torch
    from grad_probe import inputs, timed
    from nanosnp_amd import train
    tr = train.PileupTrainer.from_npz(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"), chunk_sites=n)
    x, cls = inputs(n)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cls).cuda()
    params = tr.parameters()
    if which == "fused":
        opt = train.DeviceOptimizer(tr, kind="LookaheadAdam", lr=1e-4)
        step = lambda: opt.step(MAX_NORM)
    else:
        opt = TorchLookahead(torch.optim.Adam(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, foreach=True), params)

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            opt.step()
    gen = torch.Generator(device="cuda").manual_seed(27)
    correct = torch.zeros(2, dtype=torch.int64, device="cuda")

    def batch(with_step):
        mask = (torch.rand((n, 33, 128), generator=gen, device="cuda") >= 0.3).to(torch.uint8)
        loss, pred = tr._loss_and_grad_cls(xd, None, cd, n, mask, 0.3)
        if with_step:
            step()
        correct.add_((pred == cd[:, :2]).sum(0))
        return loss
    for _ in range(3):
        batch(True)
    for _ in range(24):
        step()
    torch.cuda.synchronize()
    out = {"side": which, "n": n, "step_us": [], "batch_ms": [], "grad_ms": []}
    for _ in range(3):                                   # three windows each, interleaved: the spread is part of the result
        out["step_us"].append(1e3 * timed(step, step_repeats))
        out["batch_ms"].append(timed(lambda: batch(True), batch_repeats))
        out["grad_ms"].append(timed(lambda: batch(False), batch_repeats))
    out["clock_mhz"] = tr.ctx.shader_clock_mhz()
    out["finite"] = all(bool(torch.isfinite(p).all()) for p in params)
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--fused", "--torch"):
        print("RESULT " + json.dumps(side(sys.argv[1][2:], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))), flush=True)
        return 0
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    step_repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    batch_repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    results = []
    for which in ("--fused", "--torch", "--fused", "--torch"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), which, str(n), str(step_repeats), str(batch_repeats)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{which}: no result within {STEP_LIMIT_S} s - the probe ends here")
            return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            print(f"{which}: ended with status {r.returncode} - the probe ends here\n{r.stderr[-2000:]}")
            return 1
        if r.returncode or not line:
            print(f"{which}: step failed with status {r.returncode}, skipped\n{r.stderr[-2000:]}")
            continue
        results.append(json.loads(line[0][7:]))
        print(json.dumps(results[-1]), flush=True)
    print(f"\nN = {n} sites per batch; {step_repeats} steps and {batch_repeats} batches per window, three windows per process")
    print(f"{'variant':8s} {'step us':>24s} {'batch ms':>24s} {'batch w/o step ms':>24s} {'share of a batch':>17s}")
    med = {}
    for which in ("fused", "torch"):
        rs = [r for r in results if r["side"] == which]
        if not rs:
            continue
        cat = lambda k: [v for r in rs for v in r[k]]
        s, b, g = cat("step_us"), cat("batch_ms"), cat("grad_ms")
        med[which] = (float(np.median(s)), float(np.median(b)), float(np.median(g)))
        rng = lambda v: f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
        print(f"{which:8s} {rng(s):>24s} {rng(b):>24s} {rng(g):>24s} {100 * np.median(s) / (1e3 * np.median(b)):16.2f}%")
    if len(med) == 2:
        print(f"step: fused / torch {med['fused'][0] / med['torch'][0]:.3f}; batch: fused / torch {med['fused'][1] / med['torch'][1]:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
