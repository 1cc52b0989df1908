#!/usr/bin/env python3
"""What a HaplotypeModel training step's gradients cost: nsnp_hap_loss_grad beside PyTorch-ROCm autograd of the same network on the same GPU
(docs/rounds/r29.md).

    python tools/probes/hap_grad_probe.py [N=512] [repeats=10]

The driver never touches the GPU.  It starts four child processes one after the other - hip, torch, hip, torch (A/B/A/B) - each under its
own time limit; a child warms up, then times `repeats` calls between two HIP events and prints one JSON line.  A child that ends with a
Python error ends that step and nothing else; a child that is killed by a signal or by its time limit ends the probe (nothing more is
started on a device that may be in trouble).

  hip     one Context with a reservation of N sites; per call nsnp_hap_loss_grad on N seeded sites with four keep masks at p = 0.1; the three
          phases (forward with loss, backward, weight gradients) from nsnp_ctx_read_timing in a second timed loop (one event pair per phase)
  torch   two torch.nn.LSTM(105, 256, 3, batch_first=True, bidirectional=True, dropout=0.1) + output_proj, dense, the two heads, fp32,
          train(): forward over every position as the reference runs it, the label-smoothed loss, loss.backward()

FLOPs are the matrix products the kernels execute (2 M N K each, the reduced schedule), over the measured time, against the 157.3 TFLOP/s
fp32 MFMA peak of the MI355X.  The weight-gradient phase is big GEMMs only (K = sites x steps); the forward and backward phases mix the
per-step products (W_hh h, W_hh^T dgates: M x K = 1024 x 256, N sites) with the whole-layer products (W_ih x, W_ih^T dgates): their FLOPs
are listed side by side, their times are not separated (one event pair per phase)."""
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
F, N_GT, N_ZY = 105, 10, 3


def flops_per_site():
    """matrix-product FLOPs of one site in the three phases of hap_train.hip, split into per-step products and whole-layer products"""
    heads = 2 * (2 * 256 * 512 + 256 * 512 + (N_GT + N_ZY) * 256)
    ih = hh = dx = 0
    for L, Tc in ((33, 17), (11, 6)):
        ih += 2 * 2 * 1024 * (L * F + L * 512 + Tc * 512)
        hh += 2 * 2 * 1024 * 256 * ((L - 1) * 2 + Tc - 1)
        dx += 2 * 2 * 512 * 1024 * (L + Tc)
    return {"hap_train_forward": {"step": hh, "layer": ih + heads}, "hap_train_backward": {"step": hh, "layer": dx + heads},
            "hap_train_wgrad": {"step": 0, "layer": ih + hh + heads}}


def inputs(n):
    rng = np.random.default_rng(29)
    xp = rng.random((n, F, 33), dtype=np.float32)
    xh = rng.random((n, F, 11), dtype=np.float32)
    cls = np.stack([rng.integers(0, N_GT, n), rng.integers(0, N_ZY, n)], axis=1).astype(np.uint8)
    return xp, xh, cls


def weights():
    from nanosnp_amd.haplotype_model import state_dict_keys
    from tests.helpers import seeded_hap_weights
    return dict(zip(state_dict_keys(), seeded_hap_weights(12, H=256)))


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
    tr = train.HaplotypeTrainer(weights(), chunk_sites=n)
    xp, xh, cls = [torch.from_numpy(a).cuda() for a in inputs(n)]
    masks = [(torch.rand((n, L, 512), device="cuda") >= 0.1).to(torch.uint8) for L in (33, 33, 11, 11)]
    params, grads = tr.parameters(), tr._grads
    site_loss = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    pred = torch.empty((n, 2), dtype=torch.uint8, device="cuda")
    run = lambda: tr.ctx.hap_loss_grad(params, xp, xh, cls, grads, masks, 1.0 / 0.9, site_loss=site_loss, pred=pred)
    for _ in range(2):
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
    fl = flops_per_site()
    phases = {k: t[k][0] / max(t[k][1], 1) for k in fl}
    gflop = {k: {q: v * n / 1e9 for q, v in d.items()} for k, d in fl.items()}
    total = sum(sum(d.values()) for d in fl.values()) * n
    return {"side": "hip", "n": n, "ms": ms, "clock_mhz": tr.ctx.shader_clock_mhz(), "phase_ms": phases, "gflop": gflop,
            "tflops": total / (ms * 1e-3) / 1e12, "loss": float(site_loss.double().sum() / n)}


def side_torch(n, repeats):
    import torch
    import torch.nn as nn
    w = {k: torch.from_numpy(np.array(v)) for k, v in weights().items()}
    encs = []
    for name in ("pileup_encoder", "haplotype_encoder"):
        lstm, proj = nn.LSTM(F, 256, 3, batch_first=True, bidirectional=True, dropout=0.1), nn.Linear(512, 256)
        lstm.load_state_dict({k[len(name) + 6:]: v for k, v in w.items() if k.startswith(name + ".lstm.")})
        proj.load_state_dict({"weight": w[name + ".output_proj.weight"], "bias": w[name + ".output_proj.bias"]})
        encs += [lstm, proj]
    dense, gt, zy = nn.Linear(512, 256), nn.Linear(256, N_GT), nn.Linear(256, N_ZY)
    for m, k in ((dense, "forward_layer.dense"), (gt, "forward_layer.genotype_layer"), (zy, "forward_layer.zygosity_layer")):
        m.load_state_dict({"weight": w[k + ".weight"], "bias": w[k + ".bias"]})
    mods = nn.ModuleList(encs + [dense, gt, zy]).cuda().train()
    xp, xh, cls = inputs(n)
    xpd, xhd = torch.from_numpy(xp).cuda().permute(0, 2, 1), torch.from_numpy(xh).cuda().permute(0, 2, 1)
    t = [torch.from_numpy(cls[:, h].astype(np.int64)).cuda() for h in range(2)]

    def smooth(logits, target, c):
        lp = torch.log_softmax(logits, dim=-1)
        td = torch.full_like(lp, 0.1 / (c - 1)).scatter_(1, target[:, None], 0.9)
        return (-td * lp).sum(-1).mean()

    def run():
        for p in mods.parameters():
            p.grad = None
        ep = encs[1](encs[0](xpd)[0])[:, 16]
        eh = encs[3](encs[2](xhd)[0])[:, 5]
        mid = torch.tanh(dense(torch.cat((ep, eh), 1)))
        loss = smooth(gt(mid), t[0], N_GT) + smooth(zy(mid), t[1], N_ZY)
        loss.backward()
        return loss
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = timed(run, repeats)
    return {"side": "torch", "n": n, "ms": ms, "loss": float(run().detach())}


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--hip", "--torch"):
        n, repeats = int(sys.argv[2]), int(sys.argv[3])
        print("RESULT " + json.dumps((side_hip if sys.argv[1] == "--hip" else side_torch)(n, repeats)), flush=True)
        return 0
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
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
        print(f"\nN = {n}, {repeats} calls per step; nsnp_hap_loss_grad {np.mean([r['ms'] for r in hip]):.3f} ms per call "
              f"({', '.join('%.3f' % r['ms'] for r in hip)}), {h['tflops']:.2f} TFLOP/s = {100 * h['tflops'] / PEAK_TFLOPS:.1f} % of the fp32 MFMA peak")
        print(f"{'phase':20s} {'ms':>9s} {'GFLOP step':>11s} {'GFLOP layer':>12s} {'TFLOP/s':>9s} {'% peak':>7s}")
        for k, ms in h["phase_ms"].items():
            g = h["gflop"][k]
            tf = (g["step"] + g["layer"]) / ms if ms else 0.0     # GFLOP per ms = TFLOP/s
            print(f"{k:20s} {ms:9.3f} {g['step']:11.2f} {g['layer']:12.2f} {tf:9.2f} {100 * tf / PEAK_TFLOPS:7.1f}")
    if tor:
        print(f"torch autograd (2 x nn.LSTM + linear layers, fp32) {np.mean([r['ms'] for r in tor]):.3f} ms per call "
              f"({', '.join('%.3f' % r['ms'] for r in tor)})")
    if hip and tor:
        print(f"ratio hip / torch {np.mean([r['ms'] for r in hip]) / np.mean([r['ms'] for r in tor]):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
