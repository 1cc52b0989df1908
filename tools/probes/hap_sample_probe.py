#!/usr/bin/env python3
"""What the training sample list of a HaplotypeModel pass costs (docs/rounds/r32.md).

  A   ctx.hap_train_samples (nsnp_hap_train_samples: flags, scan, lists, one wait for the counts, placement) on the cls the label pass
      left on the device: HIP events around the call and the wall time of the call (the entry waits for the stream once).
  B   the host formulation it replaces: numpy on the host's copy of the classes by the same rules (flatnonzero twice, per block of 1,000
      refcalls one Generator.integers draw, concatenate), then the upload of the int64 list; wall time, the upload awaited.
  A/B/A/B in one process, the first round of each printed and not averaged, at 16,384 kept rows (a default pass) and 1,048,576 (a whole
  file as one pass, the reference's scope), refcalls : variants = 10 : 1, pn_value 0.7.
  step   nsnp_hap_loss_grad on 512 sites (a training batch without the optimiser), HIP events: the list's share of a pass is
         A / (ceil(M / 512) x step).

    python tools/probes/hap_sample_probe.py [rounds=6] [kept sizes=16384,1048576] [gradient steps=3, 0: skip]

Read the numbers per the measurement rules of DESIGN.md section 6."""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PN, SEED = 0.7, (7 << 32) | 2021


def host_list(cls, pn, rng):
    """TrainingDataset.__init__'s list without its in-block shuffle, in numpy"""
    refs, var = np.flatnonzero(cls[:, 1] == 0), np.flatnonzero(cls[:, 1] != 0)
    out = []
    for i in range(0, refs.size, 1000):
        blk = refs[i:i + 1000]
        out.append(blk)
        q = int(blk.size * pn) if var.size else 0
        if q:
            out.append(var[rng.integers(0, var.size, q)])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def main():
    import torch
    from nanosnp_amd import _lib, train
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [16384, 1048576]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ctx = _lib.Context(0)
    step_ms = None
    if steps > 0:
        from nanosnp_amd.fixtures import seeded_hap_weights
        from nanosnp_amd.haplotype_model import state_dict_keys
        rng = np.random.default_rng(29)
        tr = train.HaplotypeTrainer(dict(zip(state_dict_keys(), seeded_hap_weights(12, H=256))), chunk_sites=512)
        xp = torch.from_numpy(rng.random((512, 105, 33), dtype=np.float32)).cuda()
        xh = torch.from_numpy(rng.random((512, 105, 11), dtype=np.float32)).cuda()
        gt, zy = torch.from_numpy(rng.integers(0, 10, 512)).cuda(), torch.from_numpy(rng.integers(0, 3, 512)).cuda()
        tr.loss_and_grad(xp, xh, gt, zy)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            tr.loss_and_grad(xp, xh, gt, zy)
        b.record()
        torch.cuda.synchronize()
        step_ms = a.elapsed_time(b) / steps
        print(f"nsnp_hap_loss_grad, 512 sites: {step_ms:.3f} ms per step ({steps} steps)")
        tr.ctx.close()
    for kept in sizes:
        rng = np.random.default_rng(kept)
        cls_h = np.zeros((kept, 2), np.uint8)
        cls_h[:, 0] = rng.integers(0, 10, kept)
        cls_h[rng.permutation(kept)[:kept // 11], 1] = rng.integers(1, 3, kept // 11)
        n_var = int((cls_h[:, 1] != 0).sum())
        M = train.pn_sample_count(kept - n_var, n_var, PN)
        cls_d = torch.from_numpy(cls_h).cuda()
        samples = torch.empty(M, dtype=torch.int64, device="cuda")
        meta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
        pinned = torch.empty(M, dtype=torch.int64, pin_memory=True)
        host_rng = np.random.default_rng(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev, wall_a, wall_b = [], [], []
        for r in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            ctx.hap_train_samples(cls_d, kept, PN, SEED, draw=r, samples=samples, meta=meta)
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert int(meta[0]) == M
            lst = host_list(cls_h, PN, host_rng)
            pinned.numpy()[:] = lst
            up = pinned.to("cuda", non_blocking=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert lst.size == M and up.numel() == M
            ev.append(a.elapsed_time(b)); wall_a.append((t1 - t0) * 1e3); wall_b.append((t2 - t1) * 1e3)
        mean = lambda v: float(np.mean(v[1:])) if len(v) > 1 else float(v[0])
        print(f"kept {kept}: {kept - n_var} refcalls, {n_var} variants, M {M}")
        print("  A device, HIP events ms  " + " ".join(f"{v:.3f}" for v in ev) + f"   mean {mean(ev):.3f}")
        print("  A device, wall ms        " + " ".join(f"{v:.3f}" for v in wall_a) + f"   mean {mean(wall_a):.3f}")
        print("  B numpy + upload, wall ms " + " ".join(f"{v:.3f}" for v in wall_b) + f"   mean {mean(wall_b):.3f}")
        if step_ms:
            batches = -(-M // 512)
            print(f"  share of a pass: {batches} batches x {step_ms:.3f} ms = {batches * step_ms:.1f} ms of gradient work; "
                  f"A {100 * mean(wall_a) / (batches * step_ms):.4f} %, B {100 * mean(wall_b) / (batches * step_ms):.4f} %")
    ctx.close()


if __name__ == "__main__":
    main()
