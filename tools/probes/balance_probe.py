#!/usr/bin/env python3
"""What the balanced training sample list of a PileupModel pass costs (docs/rounds/r35.md).

  A   ctx.pileup_balance_samples (nsnp_pileup_balance_samples: count, scan, lists, one wait for M, placement) on the cls the label pass
      left on the device: HIP events around the call and the wall time of the call (the entry waits for the stream once).
  B   the host formulation it replaces: numpy on the host's copy of the classes by the same rules (a stable argsort by category and a
      bincount, per category below the largest one Generator.integers draw, the concatenated balanced list as the reference builds it, one
      draw of M slots), then the upload of the int64 list; wall time, the upload awaited.
  A/B/A/B in one process, the first round of each printed and not averaged, at 65,536 rows (a default pass) and 1,048,576 (a whole file as
  one pass, the reference's scope); four large categories (30 / 27 / 22 / 18 % of the rows) and twelve small ones (3 % together).
  step   nsnp_pileup_loss_grad on 2,000 sites with a keep mask (a training batch without the optimiser), measured as grad_probe.py
         measures it (its inputs, its timing loop): the list's share of a pass is A / (ceil(M / 2000) x step).

    python tools/probes/balance_probe.py [rounds=6] [row counts=65536,1048576] [gradient steps=10, 0: skip]

Read the numbers per the measurement rules of DESIGN.md section 6."""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SEED = (7 << 32) | 2022
LARGE, SMALL = (0, 15, 27, 36), (1, 2, 4, 5, 13, 16, 17, 28, 29, 37, 38, 44)
BATCH = 2000


def host_list(cls, rng):
    """balance_dataset's list (dataset.py:32-66) without its shuffle, in numpy -> the M drawn rows (None when U == 0)"""
    cat = 3 * cls[:, 0].astype(np.int64) + cls[:, 1]
    by_cat = np.argsort(cat, kind="stable")
    sizes = np.bincount(cat, minlength=63)
    off = np.cumsum(sizes) - sizes
    mx = int(sizes.max())
    total, under = [], 0
    for c in np.flatnonzero(sizes):
        rows = by_cat[off[c]:off[c] + sizes[c]]
        total.append(rows)
        if sizes[c] < mx:
            total.append(rows[rng.integers(0, sizes[c], mx - sizes[c])])
            under += 1
    if not under:
        return None
    total = np.concatenate(total)
    return total[rng.integers(0, total.size, total.size // under)]


def main():
    import torch
    from nanosnp_amd import _lib, train
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [65536, 1048576]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    ctx = _lib.Context(0)
    step_ms = None
    if steps > 0:
        import grad_probe
        tr = train.PileupTrainer.from_npz(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"), chunk_sites=BATCH)
        x, cls = grad_probe.inputs(BATCH)
        xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cls).cuda()
        mask = (torch.rand((BATCH, 33, 128), device="cuda") >= 0.3).to(torch.uint8)
        site_loss = torch.empty((BATCH, 2), dtype=torch.float32, device="cuda")
        pred = torch.empty((BATCH, 2), dtype=torch.uint8, device="cuda")
        run = lambda: tr.ctx.pileup_loss_grad(tr.parameters(), xd, None, cd, tr._grads, mask, 1.0 / 0.7, site_loss=site_loss, pred=pred)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        step_ms = grad_probe.timed(run, steps)
        print(f"nsnp_pileup_loss_grad, {BATCH} sites: {step_ms:.3f} ms per step ({steps} steps)")
        tr.ctx.close()
    for n in sizes:
        rng = np.random.default_rng(n)
        p = np.concatenate([[0.30, 0.27, 0.22, 0.18], np.full(len(SMALL), 0.03 / len(SMALL))])
        cat = np.asarray(LARGE + SMALL)[rng.choice(len(p), n, p=p / p.sum())]
        cls_h = np.zeros((n, 4), np.uint8)
        cls_h[:, 0], cls_h[:, 1] = cat // 3, cat % 3
        M, K, U, mx = train.balance_sample_count(np.bincount(cat, minlength=63))
        cls_d = torch.from_numpy(cls_h).cuda()
        samples = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        meta = torch.zeros(8, dtype=torch.int64).pin_memory()
        pinned = torch.empty(M, dtype=torch.int64).pin_memory()
        host_rng = np.random.default_rng(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev, wall_a, wall_b = [], [], []
        for r in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            ctx.pileup_balance_samples(cls_d, n, SEED, draw=r, samples=samples, sizes=False, meta=meta)
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert int(meta[0]) == M and int(meta[5]) == 0
            lst = host_list(cls_h, host_rng)
            pinned.numpy()[:] = lst
            up = pinned.to("cuda", non_blocking=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert lst.size == M and up.numel() == M
            ev.append(a.elapsed_time(b)); wall_a.append((t1 - t0) * 1e3); wall_b.append((t2 - t1) * 1e3)
        mean = lambda v: float(np.mean(v[1:])) if len(v) > 1 else float(v[0])
        print(f"rows {n}: K {K}, U {U}, max {mx}, M {M}")
        print("  A device, HIP events ms  " + " ".join(f"{v:.3f}" for v in ev) + f"   mean {mean(ev):.3f}")
        print("  A device, wall ms        " + " ".join(f"{v:.3f}" for v in wall_a) + f"   mean {mean(wall_a):.3f}")
        print("  B numpy + upload, wall ms " + " ".join(f"{v:.3f}" for v in wall_b) + f"   mean {mean(wall_b):.3f}")
        if step_ms:
            batches = -(-M // BATCH)
            print(f"  share of a pass: {batches} batches x {step_ms:.3f} ms = {batches * step_ms:.1f} ms of gradient work; "
                  f"A {100 * mean(wall_a) / (batches * step_ms):.4f} %, B {100 * mean(wall_b) / (batches * step_ms):.4f} %")
    ctx.close()


if __name__ == "__main__":
    main()
