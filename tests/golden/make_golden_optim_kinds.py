#!/usr/bin/env python3
"""Generate tests/golden/pileup_optim_kinds.npz from the reference's own optimisers: what clip_grad_norm_ and optimizer.step() of its training
step (PileupModel/train.py:61-62) leave in the parameters with PileupModel/novograd.py (Novograd), PileupModel/lookahead.py
(LookaheadNovograd), torch.optim.SGD and torch.optim.Adadelta as PileupModel/optim.py:42-104 builds them, fp32 on the CPU.

Runs only where the reference tree is mounted (REF, as make_golden_eval.py finds it).  Built as make_golden_optim.py builds pileup_optim.npz:
the tensors, step count and recorded steps are tests/optim_rules.py's, the cases tests/optim_kinds_rules.py's (CASES).

    shared_crc                the starting tensors p0 and the base gradients [STEPS, TOTAL] are those of pileup_optim.npz and are stored there
                              only (multiples of 2^-10 in (-1, 1), so that a case's gradients, base times a power of two per step
                              (<case>_grad_scale), are exact in fp32); this is the CRC-32 of their bytes.  In the Novograd cases the 21-float
                              tensor's gradients are then zeroed at steps 1 and 2 (optim_kinds_rules.zero_the_tensor)
    <case>_p                  the parameters after every step of RECORD, [len(RECORD), TOTAL]
    <case>_a, _b, _slow       the per-element states after the last step in the order of optim_kinds_rules.STATES (exp_avg; momentum_buffer;
                              square_avg, acc_delta) and the Lookahead slow buffers; only what the case has
    <case>_v, _v2, _v3        Novograd: the per-tensor exp_avg_sq after the last step, after step 2 and after step 3, [8]
    <case>_norm               what clip_grad_norm_ returned at every step (sgd_plain: clip_grad_norm_(.., inf), which scales by 1)
    <case>_ref_abs_max  [4]   the largest distance of the reference's fp32 p, a, b, slow from the float64 restatement optim_kinds_rules.run
    <case>_ref_v_rel          Novograd: the largest relative distance of its per-tensor v (last step, steps 2 and 3) from the float64 ones
    <case>_ref_norm_rel       the largest relative distance of its norms from the float64 norms

Asserted before anything is written: every clipped case holds at least 3 steps with a norm above max_norm and 3 below; the restatement
reproduces every stored number within 4 x max(ref_abs_max, 2^-23 max |value|); the first Lookahead sync moves nothing and the second does;
the zeroed tensor's v is exactly 0 after step 2 and equals its n_t after step 3 while its neighbours average.

    python tests/golden/make_golden_optim_kinds.py
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
    from tests import optim_kinds_rules as okr
    pm = os.path.join(REF, "PileupModel")
    if pm not in sys.path:
        sys.path.insert(0, pm)
    import lookahead                                      # (imports radam and novograd from the same directory)
    import novograd
    kw = dict(lr=cfg["lr"], betas=okr.BETAS, eps=okr.NOVOGRAD_EPS, weight_decay=cfg["weight_decay"])
    if cfg["kind"] == "LookaheadNovograd":
        return lookahead.LookaheadNovograd(params, cfg["alpha"], cfg["k"], **kw)
    if cfg["kind"] == "Novograd":
        return novograd.Novograd(params, **kw)
    if cfg["kind"] == "sgd":
        return torch.optim.SGD(params, lr=cfg["lr"], momentum=cfg["momentum"], nesterov=cfg["nesterov"], weight_decay=cfg["weight_decay"])
    assert cfg["kind"] == "adadelta"
    return torch.optim.Adadelta(params, lr=cfg["lr"], rho=okr.RHO, eps=okr.ADADELTA_EPS, weight_decay=cfg["weight_decay"])


def main():
    import torch
    from tests import optim_kinds_rules as okr
    from tests import optim_rules as orl
    warnings.filterwarnings("ignore", message=".*add_.*deprecated.*")
    warnings.filterwarnings("ignore", message=".*addcmul_.*deprecated.*")
    warnings.filterwarnings("ignore", message=".*addcdiv_.*deprecated.*")
    top = lambda a: float(np.abs(a).max())
    shared = orl.load_fixture()                           # p0 and the base gradients are pileup_optim.npz's: stored once
    p0, base = shared["p0"], shared["base"]
    assert np.array_equal(base * 1024.0, np.round(base * 1024.0)) and top(base) < 1.0
    out = {"shared_crc": np.array(okr.shared_crc(p0, base), np.int64), "record": np.array(orl.RECORD), "sizes": np.array(orl.SIZES)}
    for ci, (name, cfg) in enumerate(okr.CASES.items()):
        novo = okr.RULE[cfg["kind"]] == "novograd"
        # per step a power of two that puts the norm within a factor of four on either side of max_norm (sgd_plain: around 20)
        target = cfg["max_norm"] or 20.0
        shaped = okr.zero_the_tensor(base) if novo else base
        base_norm = np.sqrt((shaped.astype(np.float64) ** 2).sum(1))
        # (the first draw of the stream [34, case, 0], [34, case, 1], ... that leaves at least 3 norms on each side of max_norm)
        for draw in range(16):
            expo = np.floor(np.log2(target / base_norm)) + np.random.default_rng([34, ci, draw]).integers(-1, 3, orl.STEPS)
            sides = base_norm * 2.0 ** expo
            if not cfg["max_norm"] or min((sides > cfg["max_norm"]).sum(), (sides < cfg["max_norm"]).sum()) >= 3:
                break
        scale = (2.0 ** expo).astype(np.float32)
        grads = orl.case_grads(base, scale)
        assert np.array_equal(grads.astype(np.float64), base.astype(np.float64) * scale.astype(np.float64)[:, None])
        if novo:
            grads = okr.zero_the_tensor(grads)
        params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in orl.split(p0)]
        opt = reference_optimizer(params, cfg)
        base_opt = opt.base_optimizer if hasattr(opt, "base_optimizer") else opt
        rec, norms, v_at = [], [], {}
        for s in range(1, orl.STEPS + 1):
            for p, g in zip(params, orl.split(grads[s - 1])):
                p.grad = torch.from_numpy(g.copy())                  # (a copy: novograd.py:214 divides the gradient in place)
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, cfg["max_norm"] if cfg["max_norm"] else float("inf"))))
            opt.step()
            if novo:
                v_at[s] = np.array([float(base_opt.state[p]["exp_avg_sq"]) for p in params], np.float32)
            if s in orl.RECORD:
                rec.append(orl.join([p.detach().numpy() for p in params]).copy())
        norms = np.array(norms, np.float32)
        if cfg["max_norm"]:
            above, below = int((norms > cfg["max_norm"]).sum()), int((norms < cfg["max_norm"]).sum())
            assert above >= 3 and below >= 3, (name, norms, "a clipped case needs at least 3 steps on each side of max_norm")
        names = okr.STATES[okr.RULE[cfg["kind"]]] if cfg.get("momentum", 1.0) != 0 else ()
        states = [orl.join([base_opt.state[p][q].numpy() for p in params]) for q in names]
        slow = orl.join([opt.state[p]["slow_buffer"].numpy() for p in params]) if hasattr(opt, "base_optimizer") else None
        f64 = okr.run(name, p0, grads)
        ps = np.stack(rec)
        ram = np.zeros(4)
        ram[0] = max(top(ps[j] - f64["p"][s]) for j, s in enumerate(orl.RECORD))
        for j, (st, key) in enumerate(zip(states, ("a", "b"))):
            ram[1 + j] = top(st - f64[key])
            assert ram[1 + j] <= orl.bound(ram[1 + j], st) and top(st) > 0
        ram[3] = top(slow - f64["slow"]) if slow is not None else 0.0
        rel = float(np.abs(norms.astype(np.float64) / f64["norm"] - 1.0).max())
        # the restatement reproduces every stored number within the bound the tests use
        for j, s in enumerate(orl.RECORD):
            assert top(ps[j] - f64["p"][s]) <= orl.bound(ram[0], ps[j]), (name, s)
        v_rel = 0.0
        if novo:
            z = okr.ZERO_TENSOR
            assert v_at[2][z] == 0.0 and f64["v_at"][2][z] == 0.0 and (np.delete(v_at[2], z) > 0).all(), (name, "the zeroed tensor's v after step 2")
            n3 = float((orl.split(grads[2])[z].astype(np.float64) ** 2).sum()) * min(1.0, cfg["max_norm"] / (f64["norm"][2] + 1e-6)) ** 2
            assert n3 > 0 and abs(f64["v_at"][3][z] / n3 - 1.0) < 1e-12 and abs(v_at[3][z] / n3 - 1.0) < 1e-5, (name, "the copy branch at step 3")
            for i in (z - 1, z + 1):                                     # (its neighbours average)
                ni = float((orl.split(grads[2])[i].astype(np.float64) ** 2).sum()) * min(1.0, cfg["max_norm"] / (f64["norm"][2] + 1e-6)) ** 2
                mix = okr.BETAS[1] * f64["v_at"][2][i] + (1 - okr.BETAS[1]) * ni
                assert abs(f64["v_at"][3][i] / mix - 1.0) < 1e-12 and abs(v_at[3][i] / mix - 1.0) < 1e-5, (name, i)
            for s in (2, 3, orl.STEPS):
                want = f64["v_at"][s]
                nz = want != 0
                assert np.array_equal(v_at[s] != 0, nz)
                v_rel = max(v_rel, float(np.abs(v_at[s][nz] / want[nz] - 1.0).max()))
            out[f"{name}_v"], out[f"{name}_v2"], out[f"{name}_v3"] = v_at[orl.STEPS], v_at[2], v_at[3]
            out[f"{name}_ref_v_rel"] = np.float64(v_rel)
        # the first sync changes nothing: up to the step before the second sync the Lookahead-free restatement gives the same numbers
        if slow is not None:
            free = okr.run(name, p0, grads, lookahead=False)
            for j, s in enumerate(orl.RECORD):
                if s < 2 * cfg["k"]:
                    assert top(ps[j] - free["p"][s]) <= orl.bound(ram[0], ps[j]), (name, s, "the first sync moved the parameters")
            assert top(ps[-1] - free["p"][orl.STEPS]) > 100 * orl.bound(ram[0], ps[-1]), (name, "the second sync moved nothing")
            assert top(slow - f64["slow"]) <= orl.bound(ram[3], slow)
            out[f"{name}_slow"] = orl.pack(slow)
        out[f"{name}_grad_scale"], out[f"{name}_p"] = scale, orl.pack(ps)
        for st, key in zip(states, ("a", "b")):
            out[f"{name}_{key}"] = orl.pack(st)
        out[f"{name}_norm"], out[f"{name}_ref_abs_max"], out[f"{name}_ref_norm_rel"] = norms, ram, np.float64(rel)
        print(f"{name}: norms {norms.min():.3g} .. {norms.max():.3g} (max_norm {cfg['max_norm']}), ref_abs_max p {ram[0]:.2e} a {ram[1]:.2e} "
              f"b {ram[2]:.2e} slow {ram[3]:.2e}, v rel {v_rel:.2e}, norm rel {rel:.2e}; |p14 - p0| max {top(ps[-1] - p0):.2e}")
    path = os.path.join(HERE, "pileup_optim_kinds.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, (os.path.getsize(path), "the fixture must stay under 512 KB")
    fx = okr.load_fixture(path)                           # (and it reads back)
    assert np.array_equal(fx["p0"], p0) and np.array_equal(fx["base"], base)
    for name in okr.CASES:
        assert set(fx["cases"][name]["p"]) == set(orl.RECORD)
    print(f"pileup_optim_kinds.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
