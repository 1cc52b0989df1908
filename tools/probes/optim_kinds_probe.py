#!/usr/bin/env python3
"""What the optimiser step costs for the kinds of nsnp_optim_step_kind: the fused step (train.DeviceOptimizer, two launches) beside the
matching torch optimiser stepping the same tensors, on the 24 tensors of the PileupModel (198,040 floats) and the 58 of the HaplotypeModel
(docs/rounds/r34.md).

    python tools/probes/optim_kinds_probe.py [step_repeats=1000]

The driver never touches the GPU.  It starts four child processes one after the other - fused, torch, fused, torch (A/B/A/B) - each under
its own time limit; a child warms up, times between two HIP events and prints one JSON line.  A child that ends with a Python error ends
that step and nothing else; a child that is killed by a signal or by its time limit ends the probe (nothing more is started on a device
that may be in trouble).

Per child, per model and per kind, on device tensors of the model's shapes with random parameters and gradients (clip at 20):
  adam       the yardstick: LookaheadAdam as docs/rounds/r27.md measured it - fused nsnp_optim_step; torch clip_grad_norm_ + foreach Adam +
             a foreach Lookahead
  novograd   LookaheadNovograd - fused; torch clip_grad_norm_ + a per-tensor loop written to the rule of novograd.py:197-221 (the
             reference's file is not imported) + the foreach Lookahead
  sgd        momentum 0.9, nesterov, weight decay 1e-4 - fused; torch clip_grad_norm_ + foreach SGD
  adadelta   lr 1, weight decay 1e-4 - fused; torch clip_grad_norm_ + foreach Adadelta
step_us: `step_repeats` steps back to back, per step: host enqueue and device work together, whichever is longer - what a training loop
sees.  Three windows per process."""
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
KINDS = ("adam", "novograd", "sgd", "adadelta")
FUSED = {"adam": dict(kind="LookaheadAdam", lr=1e-4), "novograd": dict(kind="LookaheadNovograd", lr=1e-3),
         "sgd": dict(kind="sgd", lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4), "adadelta": dict(kind="adadelta", lr=1.0, weight_decay=1e-4)}


class TorchNovograd:
    """novograd.py:197-221 as a plain per-tensor loop (amsgrad and grad_averaging off); the gradient is divided in place, as there"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        import torch
        self.params, self.lr, self.betas, self.eps, self.wd = params, lr, betas, eps, weight_decay
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros((), device=p.device) for p in params]
        self.first = True

    def step(self):
        import torch
        b1, b2 = self.betas
        for p, m, v in zip(self.params, self.m, self.v):
            g = p.grad
            n = torch.sum(torch.pow(g, 2))
            if self.first:                               # (the reference asks `exp_avg_sq == 0` of the device at every step: a host wait
                v.copy_(n)                               # per tensor, which this loop spares the torch side)
            else:
                v.mul_(b2).add_(n, alpha=1 - b2)
            g.div_(v.sqrt().add_(self.eps))
            if self.wd != 0:
                g.add_(p.detach(), alpha=self.wd)
            m.mul_(b1).add_(g)
            p.detach().add_(m, alpha=-self.lr)
        self.first = False


def side(which, step_repeats):
    import torch
    from grad_probe import timed
    from optim_probe import TorchLookahead
    from nanosnp_amd import _lib, train
    ctx = _lib.Context(0)
    out = {"side": which, "step_us": {}, "finite": True}
    for model, shapes in (("pileup", _lib.Context.TRAIN_SHAPES), ("haplotype", _lib.Context.hap_train_shapes())):
        gen = torch.Generator(device="cuda").manual_seed(34)
        for kind in KINDS:
            params = [torch.nn.Parameter(torch.randn(s, generator=gen, device="cuda") * 0.1) for s in shapes]
            grads = [torch.randn(s, generator=gen, device="cuda") * 0.05 for s in shapes]
            for p, g in zip(params, grads):
                p.grad = g.clone()
            if which == "fused":
                opt = train.DeviceOptimizer(params, ctx=ctx, **FUSED[kind])
                step = lambda opt=opt: opt.step(MAX_NORM)
            else:
                if kind == "adam":
                    opt = TorchLookahead(torch.optim.Adam(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, foreach=True), params)
                elif kind == "novograd":
                    opt = TorchLookahead(TorchNovograd(params, lr=1e-3), params)
                elif kind == "sgd":
                    opt = torch.optim.SGD(params, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4, foreach=True)
                else:
                    opt = torch.optim.Adadelta(params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=1e-4, foreach=True)

                def step(opt=opt, params=params, grads=grads, restore=kind == "novograd"):
                    if restore:                          # the loop divides the gradients in place: give it the gradients of a batch again
                        torch._foreach_copy_([p.grad for p in params], grads)
                    torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
                    opt.step()
            for _ in range(24):
                step()
            torch.cuda.synchronize()
            out["step_us"][f"{model}.{kind}"] = [1e3 * timed(step, step_repeats) for _ in range(3)]
            out["finite"] = out["finite"] and all(bool(torch.isfinite(p).all()) for p in params)
    out["floats"] = {"pileup": int(sum(np.prod(s) for s in _lib.Context.TRAIN_SHAPES)),
                     "haplotype": int(sum(np.prod(s) for s in _lib.Context.hap_train_shapes()))}
    out["clock_mhz"] = ctx.shader_clock_mhz()
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--fused", "--torch"):
        print("RESULT " + json.dumps(side(sys.argv[1][2:], int(sys.argv[2]))), flush=True)
        return 0
    step_repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    results = []
    for which in ("--fused", "--torch", "--fused", "--torch"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), which, str(step_repeats)], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S)
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
    print(f"\n{step_repeats} steps per window, three windows per process, two processes per side; step us: median (min .. max)")
    print(f"{'tensors.kind':20s} {'fused':>26s} {'torch':>26s} {'fused / torch':>14s} {'fused / fused adam':>19s}")
    med = {}
    for key in [f"{m}.{k}" for m in ("pileup", "haplotype") for k in KINDS]:
        cells = []
        for which in ("fused", "torch"):
            v = [x for r in results if r["side"] == which for x in r["step_us"].get(key, [])]
            med[which, key] = float(np.median(v)) if v else float("nan")
            cells.append(f"{np.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})" if v else "-")
        yard = med.get(("fused", key.split(".")[0] + ".adam"), float("nan"))
        print(f"{key:20s} {cells[0]:>26s} {cells[1]:>26s} {med['fused', key] / med['torch', key]:14.3f} {med['fused', key] / yard:19.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
