#!/usr/bin/env python3
"""Generate tests/golden/pileup_optim.npz from the reference's own optimisers: what clip_grad_norm_ and optimizer.step() of its training step
(PileupModel/train.py:61-62) leave in the parameters, with PileupModel/lookahead.py (LookaheadAdam, LookaheadRadam), PileupModel/radam.py and
torch.optim.Adam, fp32 on the CPU.

Runs only where the reference tree is mounted (REF, as make_golden_eval.py finds it).  The cases, tensors, step count and recorded steps are
tests/optim_rules.py's (CASES, SHAPES, STEPS, RECORD).

    p0, grad_base             the starting tensors (shared) and the base gradients [STEPS, TOTAL]: multiples of 2^-10 in (-1, 1), so that a
                              case's gradients, base times a power of two per step (<case>_grad_scale), are exact in fp32
    <case>_p                  the parameters after every step of RECORD, [len(RECORD), TOTAL]
    <case>_m, _v, _slow       exp_avg, exp_avg_sq and the Lookahead slow buffers after the last step (no _slow for plain Adam)
    <case>_norm               what clip_grad_norm_ returned at every step (plain Adam: clip_grad_norm_(.., inf), which scales by 1)
    <case>_ref_abs_max  [4]   the largest distance of the reference's fp32 p, m, v, slow from the float64 restatement optim_rules.run
    <case>_ref_norm_rel       the largest relative distance of its norms from the float64 norms

The scales are drawn so that every clipped case holds steps with a norm above max_norm and steps below it; that, and the restatement
reproducing every stored number within 4 x max(ref_abs_max, 2^-23 max |value|), is asserted before anything is written.  fp32 arrays are
stored as byte planes (optim_rules.pack).

    python tests/golden/make_golden_optim.py
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
LIMIT = 512 * 1024


def reference_optimizer(params, cfg):
    import torch
    from make_golden_eval import REF
    pm = os.path.join(REF, "PileupModel")
    if pm not in sys.path:
        sys.path.insert(0, pm)
    import lookahead                                      # (imports radam and novograd from the same directory)
    kw = dict(lr=cfg["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=cfg["weight_decay"])
    if cfg["kind"] == "LookaheadAdam":
        return lookahead.LookaheadAdam(params, cfg["alpha"], cfg["k"], **kw)
    if cfg["kind"] == "LookaheadRadam":
        return lookahead.LookaheadRadam(params, cfg["alpha"], cfg["k"], **kw)
    assert cfg["kind"] == "Adam"
    return torch.optim.Adam(params, **kw)


def main():
    import torch
    from tests import optim_rules as orl
    warnings.filterwarnings("ignore", message=".*add_.*deprecated.*")
    warnings.filterwarnings("ignore", message=".*addcmul_.*deprecated.*")
    warnings.filterwarnings("ignore", message=".*addcdiv_.*deprecated.*")
    rng = np.random.default_rng(2027)
    p0 = (rng.standard_normal(orl.TOTAL) * 0.1).astype(np.float32)
    base = (rng.integers(-1023, 1024, (orl.STEPS, orl.TOTAL)) / 1024.0).astype(np.float32)
    base_norm = np.sqrt((base.astype(np.float64) ** 2).sum(1))
    out = {"p0": orl.pack(p0), "grad_base": orl.pack(base), "record": np.array(orl.RECORD), "sizes": np.array(orl.SIZES)}
    for ci, (name, cfg) in enumerate(orl.CASES.items()):
        # per step a power of two that puts the norm within a factor of four on either side of max_norm (plain Adam: around 20)
        target = cfg["max_norm"] or 20.0
        expo = np.floor(np.log2(target / base_norm)) + np.random.default_rng([7, ci]).integers(-1, 3, orl.STEPS)
        scale = (2.0 ** expo).astype(np.float32)
        grads = orl.case_grads(base, scale)
        assert np.array_equal(grads.astype(np.float64), base.astype(np.float64) * scale.astype(np.float64)[:, None])
        params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in orl.split(p0)]
        opt = reference_optimizer(params, cfg)
        rec, norms = [], []
        for s in range(1, orl.STEPS + 1):
            for p, g in zip(params, orl.split(grads[s - 1])):
                p.grad = torch.from_numpy(g.copy())
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, cfg["max_norm"] if cfg["max_norm"] else float("inf"))))
            opt.step()
            if s in orl.RECORD:
                rec.append(orl.join([p.detach().numpy() for p in params]).copy())
        norms = np.array(norms, np.float32)
        if cfg["max_norm"]:
            above, below = int((norms > cfg["max_norm"]).sum()), int((norms < cfg["max_norm"]).sum())
            assert above >= 3 and below >= 3, (name, norms, "a clipped case needs steps on both sides of max_norm")
        base_opt = opt.base_optimizer if hasattr(opt, "base_optimizer") else opt
        m = orl.join([base_opt.state[p]["exp_avg"].numpy() for p in params])
        v = orl.join([base_opt.state[p]["exp_avg_sq"].numpy() for p in params])
        slow = orl.join([opt.state[p]["slow_buffer"].numpy() for p in params]) if hasattr(opt, "base_optimizer") else None
        f64 = orl.run(name, p0, grads)
        ps = np.stack(rec)
        ram = np.array([max(np.abs(ps[j] - f64["p"][s]).max() for j, s in enumerate(orl.RECORD)), np.abs(m - f64["m"]).max(),
                        np.abs(v - f64["v"]).max(), np.abs(slow - f64["slow"]).max() if slow is not None else 0.0])
        rel = float(np.abs(norms.astype(np.float64) / f64["norm"] - 1.0).max())
        # the restatement reproduces every stored number within the bound the tests use
        for j, s in enumerate(orl.RECORD):
            assert np.abs(ps[j] - f64["p"][s]).max() <= orl.bound(ram[0], ps[j]), (name, s)
        # the first sync changes nothing: up to the step before the second sync the Lookahead-free restatement gives the same numbers
        if slow is not None:
            free = orl.run(name, p0, grads, lookahead=False)
            for j, s in enumerate(orl.RECORD):
                if s < 2 * cfg["k"]:
                    assert np.abs(ps[j] - free["p"][s]).max() <= orl.bound(ram[0], ps[j]), (name, s, "the first sync moved the parameters")
            assert np.abs(ps[-1] - free["p"][orl.STEPS]).max() > 100 * orl.bound(ram[0], ps[-1]), (name, "the second sync moved nothing")
        out[f"{name}_grad_scale"] = scale
        out[f"{name}_p"], out[f"{name}_m"], out[f"{name}_v"] = orl.pack(ps), orl.pack(m), orl.pack(v)
        if slow is not None:
            out[f"{name}_slow"] = orl.pack(slow)
        out[f"{name}_norm"], out[f"{name}_ref_abs_max"], out[f"{name}_ref_norm_rel"] = norms, ram, np.float64(rel)
        print(f"{name}: norms {norms.min():.3g} .. {norms.max():.3g} (max_norm {cfg['max_norm']}), ref_abs_max p {ram[0]:.2e} m {ram[1]:.2e} "
              f"v {ram[2]:.2e} slow {ram[3]:.2e}, norm rel {rel:.2e}; |p14 - p0| max {np.abs(ps[-1] - p0).max():.2e}")
    path = os.path.join(HERE, "pileup_optim.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, (os.path.getsize(path), "the fixture must stay under 512 KB")
    fx = orl.load_fixture(path)                           # (and it reads back)
    assert np.array_equal(fx["p0"], p0) and np.array_equal(fx["base"], base)
    print(f"pileup_optim.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
