#!/usr/bin/env python3
"""Generate tests/golden/pileup_grad.npz from the reference's own model code: what loss.backward() of its training step
(PileupModel/train.py:56-59) leaves in param.grad, with ont_pileup.chkpt, dropout 0, model.train(), fp32 on the CPU.

Runs only where the reference tree is mounted.  Inputs are the seeded batches eval_rules.synthetic_windows(train_cut windows, N).

    N = 17                     all 24 gradients in full (198,040 floats), the loss
    N = 1, 33, 257, 2000       the loss; per tensor its sum, L2 norm and 64 seeded entries (grad_rules.sample_index)
    every batch                dist_<N> [24]: max |g32 - g64| / max |g64| per tensor, the reference's own fp32 distance from the float64
                               restatement tests/grad_rules.py
    ref_rel_max                the largest of those distances

The four indel tensors must have grad None.  Before anything is written grad_rules must reproduce every stored number within ref_rel_max.

    python tests/golden/make_golden_grad.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
FULL, SAMPLED = 17, (1, 33, 257, 2000)


def main():
    import torch
    from make_golden_eval import reference_model
    from tests import eval_rules as er
    from tests import grad_rules as gr
    from nanosnp_amd.pileup_model import ENCODER_KEYS, FORWARD_KEYS, INDEL_KEYS
    torch.manual_seed(0)
    model, ck = reference_model()
    model.encoder.lstm.dropout = 0.0                   # config.model.dropout = 0: nothing random between the layers
    model.train()
    npf = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)
    weights = [npf(ck["encoder"][k]) for k in ENCODER_KEYS] + [npf(ck["forward_layer"][k]) for k in FORWARD_KEYS]
    params = [model.encoder.state_dict(keep_vars=True)[k] for k in ENCODER_KEYS] + [model.forward_layer.state_dict(keep_vars=True)[k] for k in FORWARD_KEYS]
    indel = [model.forward_layer.state_dict(keep_vars=True)[k] for k in INDEL_KEYS]
    with tempfile.TemporaryDirectory() as d:
        _, base, _ = er.fixture_rows("train_cut", d)
    out, ref_rel_max = {}, 0.0
    for n in (FULL,) + SAMPLED:
        x, cls = er.synthetic_windows(base, n)
        model.zero_grad(set_to_none=True)
        t = [torch.from_numpy(cls[:, h].astype(np.int64)) for h in range(4)]
        loss, *_ = model(torch.from_numpy(x.astype(np.float32)), *t)
        loss.backward()
        assert all(p.grad is None for p in indel), "the indel heads received a gradient"
        g32 = [npf(p.grad) for p in params]
        mine = gr.loss_and_grad(weights, x, cls)
        dist = np.array([gr.rel_dist(a, b) for a, b in zip(g32, mine["grads"])])
        ref_rel_max = max(ref_rel_max, float(dist.max()))
        out[f"dist_{n}"] = dist
        out[f"loss_{n}"] = np.float32(loss.item())
        if n == FULL:
            for i, g in enumerate(g32):
                out[f"g{n}_{i:02d}"] = g
        else:
            out[f"sum_{n}"] = np.array([g.astype(np.float64).sum() for g in g32])
            out[f"l2_{n}"] = np.array([np.sqrt((g.astype(np.float64) ** 2).sum()) for g in g32])
            out[f"val_{n}"] = np.stack([g.reshape(-1)[gr.sample_index(i, g.shape)] for i, g in enumerate(g32)])
        print(f"N = {n}: loss {loss.item():.6f}, |g32 - g64| / max |g64| per tensor: {dist.min():.2e} .. {dist.max():.2e}")
    out["ref_rel_max"] = np.float64(ref_rel_max)
    # the restatement reproduces every stored number within ref_rel_max (sums and norms: relative to the tensor's largest entry times its size)
    for n in (FULL,) + SAMPLED:
        x, cls = er.synthetic_windows(base, n)
        mine = gr.loss_and_grad(weights, x, cls)
        assert abs(mine["loss"] - float(out[f"loss_{n}"])) <= 1e-4, n
        for i, g in enumerate(mine["grads"]):
            top = np.abs(g).max()
            if n == FULL:
                assert np.abs(out[f"g{n}_{i:02d}"] - g).max() <= ref_rel_max * top, (n, i)
            else:
                assert np.abs(out[f"val_{n}"][i] - g.reshape(-1)[gr.sample_index(i, g.shape)]).max() <= ref_rel_max * top, (n, i)
                assert abs(out[f"sum_{n}"][i] - g.sum()) <= ref_rel_max * top * g.size, (n, i)
                assert abs(out[f"l2_{n}"][i] - np.sqrt((g ** 2).sum())) <= ref_rel_max * top * np.sqrt(g.size), (n, i)
    path = os.path.join(HERE, "pileup_grad.npz")
    np.savez_compressed(path, **out)
    limit = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "pileup_grad.npz")
    assert os.path.getsize(path) <= limit, (os.path.getsize(path), "larger than the largest fixture already there")
    print(f"pileup_grad.npz: {os.path.getsize(path)} bytes; ref_rel_max {ref_rel_max:.3e}")


if __name__ == "__main__":
    main()
