#!/usr/bin/env python3
"""What a training step's gradients cost: nsnp_pileup_loss_grad beside PyTorch-ROCm autograd of the same network on the same GPU
(docs/rounds/r23.md).

    python tools/probes/grad_probe.py N [repeats=20]

The driver never touches the GPU.  It starts four child processes one after the other - hip, torch, hip, torch (A/B/A/B) - each under its
own time limit; a child warms up, then times `repeats` calls between two HIP events and prints one JSON line.  A child that ends with a
Python error ends that step and nothing else; a child that is killed by a signal or by its time limit ends the probe (nothing more is
started on a device that may be in trouble).

  hip     one Context with a reservation of N sites; per call nsnp_pileup_loss_grad on N seeded windows with a keep mask at p = 0.3; the three
          phases (forward with loss, backward, weight gradients) from nsnp_ctx_read_timing in a second timed loop (one event pair per phase)
  torch   torch.nn.LSTM(18, 64, 2, batch_first=True, bidirectional=True, dropout=0.3) + output_proj, dense, the two heads, fp32, train():
          forward over all 33 positions as the reference runs it, the label-smoothed loss, loss.backward()

FLOPs are the matrix products the kernels execute (2 M N K each, sites padded to 16, the reduced schedule), over the measured time, against
the 157.3 TFLOP/s fp32 MFMA peak of the MI355X."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK_TFLOPS = 157.3
STEP_LIMIT_S = 240


def flops_per_site():
    """matrix-product FLOPs of one site in the three phases of pileup_train.hip"""
    heads = 2 * (128 * 128 + 256 * 128 + 24 * 256)
    l0_ih, l0_hh = 2 * 33 * 2 * 256 * 18, 2 * 32 * 2 * 256 * 64
    l1_ih, l1_hh = 2 * 17 * 2 * 256 * 128, 2 * 16 * 2 * 256 * 64
    return {"train_forward": l0_ih + l0_hh + l1_ih + l1_hh + heads,
            "train_backward": heads + l1_hh + l1_ih + l0_hh,          # W^T products; layer 0 needs no dx
            "train_wgrad": l0_ih + l0_hh + l1_ih + l1_hh + heads}


def inputs(n):
    """plausible windows (small counts, a dominant negative reference channel per position, as eval_probe.py builds them) and random classes"""
    rng = np.random.default_rng(23)
    x = rng.poisson(0.3, (n, 33, 18)).astype(np.int32)
    ref = rng.integers(0, 4, (n, 33))
    depth = rng.integers(8, 40, (n, 33)).astype(np.int32)
    np.put_along_axis(x, ref[..., None], -depth[..., None], axis=2)
    np.put_along_axis(x, (ref + 9)[..., None], -(depth // 2)[..., None], axis=2)
    cls = np.stack([rng.integers(0, c, n) for c in (21, 3, 33, 33)], axis=1).astype(np.uint8)
    return x, cls


def timed(run, repeats):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def side_hip(n, repeats):
    import torch
    from nanosnp_amd import train
    tr = train.PileupTrainer.from_npz(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"), chunk_sites=n)
    x, cls = inputs(n)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cls).cuda()
    mask = (torch.rand((n, 33, 128), device="cuda") >= 0.3).to(torch.uint8)
    params, grads = tr.parameters(), tr._grads
    site_loss = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    pred = torch.empty((n, 2), dtype=torch.uint8, device="cuda")
    run = lambda: tr.ctx.pileup_loss_grad(params, xd, None, cd, grads, mask, 1.0 / 0.7, site_loss=site_loss, pred=pred)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = timed(run, repeats)
    tr.ctx.enable_timing(True)
    run(); torch.cuda.synchronize(); tr.ctx.read_timing()
    for _ in range(repeats):
        run()
    torch.cuda.synchronize()
    t = tr.ctx.read_timing()
    tr.ctx.enable_timing(False)
    np16 = -(-n // 16) * 16
    phases = {k: t[k][0] / max(t[k][1], 1) for k in ("train_forward", "train_backward", "train_wgrad")}
    fl = {k: v * np16 for k, v in flops_per_site().items()}
    return {"side": "hip", "n": n, "ms": ms, "clock_mhz": tr.ctx.shader_clock_mhz(), "phase_ms": phases, "gflop": {k: v / 1e9 for k, v in fl.items()},
            "tflops": sum(fl.values()) / (ms * 1e-3) / 1e12, "loss": float(site_loss.double().sum() / n)}


def side_torch(n, repeats):
    import torch
    import torch.nn as nn
    z = np.load(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"))
    lstm = nn.LSTM(18, 64, 2, batch_first=True, bidirectional=True, dropout=0.3)
    proj, dense, gt, zy = nn.Linear(128, 128), nn.Linear(128, 256), nn.Linear(256, 21), nn.Linear(256, 3)
    lstm.load_state_dict({k[len("encoder.lstm."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("encoder.lstm.")})
    for m, k in ((proj, "encoder.output_proj"), (dense, "forward_layer.dense"), (gt, "forward_layer.genotype_layer"), (zy, "forward_layer.zygosity_layer")):
        m.load_state_dict({"weight": torch.from_numpy(z[k + ".weight"]), "bias": torch.from_numpy(z[k + ".bias"])})
    mods = nn.ModuleList([lstm, proj, dense, gt, zy]).cuda().train()
    x, cls = inputs(n)
    xd = torch.from_numpy(x).cuda().float()
    t = [torch.from_numpy(cls[:, h].astype(np.int64)).cuda() for h in range(2)]

    def smooth(logits, target, c):
        lp = torch.log_softmax(logits, dim=-1)
        td = torch.full_like(lp, 0.1 / (c - 1)).scatter_(1, target[:, None], 0.9)
        return (-td * lp).sum(-1).mean()

    def run():
        for p in mods.parameters():
            p.grad = None
        out, _ = lstm(xd)
        mid = torch.tanh(dense(proj(out)))[:, 16]
        loss = smooth(gt(mid), t[0], 21) + smooth(zy(mid), t[1], 3)
        loss.backward()
        return loss
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = timed(run, repeats)
    return {"side": "torch", "n": n, "ms": ms, "loss": float(run().detach())}


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--hip", "--torch"):
        n, repeats = int(sys.argv[2]), int(sys.argv[3])
        print("RESULT " + json.dumps((side_hip if sys.argv[1] == "--hip" else side_torch)(n, repeats)), flush=True)
        return 0
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    results = []
    for side in ("--hip", "--torch", "--hip", "--torch"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), side, str(n), str(repeats)], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{side}: no result within {STEP_LIMIT_S} s - the probe ends here")
            return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            print(f"{side}: ended with status {r.returncode} - the probe ends here\n{r.stderr[-2000:]}")
            return 1
        if r.returncode or not line:
            print(f"{side}: step failed with status {r.returncode}, skipped\n{r.stderr[-2000:]}")
            continue
        results.append(json.loads(line[0][7:]))
        print(json.dumps(results[-1]), flush=True)
    hip = [r for r in results if r["side"] == "hip"]
    tor = [r for r in results if r["side"] == "torch"]
    if hip:
        h = hip[-1]
        print(f"\nN = {n}, {repeats} calls per step; nsnp_pileup_loss_grad {np.mean([r['ms'] for r in hip]):.3f} ms per call "
              f"({', '.join('%.3f' % r['ms'] for r in hip)}), {h['tflops']:.2f} TFLOP/s = {100 * h['tflops'] / PEAK_TFLOPS:.1f} % of the fp32 MFMA peak")
        print(f"{'phase':16s} {'ms':>9s} {'GFLOP':>9s} {'TFLOP/s':>9s} {'% peak':>7s}")
        for k, ms in h["phase_ms"].items():
            tf = h["gflop"][k] / ms if ms else 0.0               # GFLOP per ms = TFLOP/s
            print(f"{k:16s} {ms:9.3f} {h['gflop'][k]:9.2f} {tf:9.2f} {100 * tf / PEAK_TFLOPS:7.1f}")
    if tor:
        print(f"torch autograd (nn.LSTM + linear layers, fp32) {np.mean([r['ms'] for r in tor]):.3f} ms per call "
              f"({', '.join('%.3f' % r['ms'] for r in tor)})")
    if hip and tor:
        print(f"ratio hip / torch {np.mean([r['ms'] for r in hip]) / np.mean([r['ms'] for r in tor]):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
