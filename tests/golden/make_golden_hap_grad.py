#!/usr/bin/env python3
"""Generate tests/golden/hap_grad.npz from the reference's own model code: what loss.backward() of its HaplotypeModel training step
(HaplotypeModel/train_dev.py:58-59) leaves in param.grad, with seeded_hap_weights(12, H=256), dropout 0, model.train(), fp32 on the CPU.

Runs only where the reference tree is mounted.  model_dev.LSTMNetwork is imported with the stubs make_golden_hap_eval.py uses; nothing of it
is copied.  Inputs: the first N sites of the `main` case of hap_eval.npz for N in {1, 17, 96} (tests.test_hap_eval_rules.eval_case refuses
other input bytes), and one batch of 257 sites built by the same recipe from new seeds (tests.test_hap_grad_rules), whose CRC-32s and targets
are recorded here.

    every batch   the loss; per tensor its sum, L2 norm and 64 seeded entries (hap_grad_rules.sample_index) - the full gradient is
                  8,192,013 floats and is not stored;
                  dist_<N> [58]: max |g32 - g64| / max |g64| per tensor, the reference's own fp32 distance from the float64 restatement
                  tests/hap_grad_rules.py;  near_<N>: the sites within hap_eval_rules.MARGIN of an argmax tie in float64
    ref_rel_max   the largest of those distances

Before anything is written the restatement must reproduce every stored number within ref_rel_max, and at most MARGIN_SHARE of a batch's
sites may lie within the margin (another seed otherwise).

    python tests/golden/make_golden_hap_grad.py
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def main():
    import torch
    from make_golden_hap_eval import _stubs, reference_model
    _stubs()
    from nanosnp_amd import host
    from oracle import oracle
    from tests import hap_eval_rules as hr
    from tests import hap_grad_rules as gr
    from tests import test_hap_grad_rules as tg
    from tests.test_hap_eval_rules import eval_case, seeded_targets
    torch.manual_seed(0)
    weights = list(tg.weights())
    model = reference_model(105, 10, 3, weights)
    model.pileup_encoder.lstm.dropout = 0.0            # config.model.dropout = 0: nothing random between the layers
    model.haplotype_encoder.lstm.dropout = 0.0
    model.train()
    from nanosnp_amd.haplotype_model import state_dict_keys
    sd = model.state_dict(keep_vars=True)
    params = [sd[k] for k in state_dict_keys()]
    npf = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)
    assert all(np.array_equal(npf(p), w) for p, w in zip(params, weights))
    main_case = eval_case("main")
    big = [oracle.hap_features_batch(*host.synth_hap_planes(sd_ + tg.SEED_BIG, tg.N_BIG, 30, 90, L), nthreads=4) for sd_, L in ((540, 33), (640, 11))]
    big_cls = seeded_targets(tg.SEED_BIG, tg.N_BIG, 10, 3)
    out = {"big_input_crc32": np.array([zlib.crc32(big[0].tobytes()), zlib.crc32(big[1].tobytes())], np.int64), "big_cls": big_cls}
    ref_rel_max, results = 0.0, {}
    for n in tg.MAIN_SIZES + (tg.N_BIG,):
        xp, xh, cls = (big[0], big[1], big_cls) if n == tg.N_BIG else (main_case["xp"][:n], main_case["xh"][:n], main_case["cls"][:n])
        model.zero_grad(set_to_none=True)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        loss, *_ = model(t(xp), t(xh), t(cls[:, 0].astype(np.int64)), t(cls[:, 1].astype(np.int64)))
        loss.backward()
        g32 = [npf(p.grad) for p in params]
        mine = gr.loss_and_grad(weights, xp, xh, cls)
        results[n] = mine
        near = (hr.margins(mine["logits"], 10) < hr.MARGIN).any(1)
        assert near.mean() <= hr.MARGIN_SHARE, (n, int(near.sum()), "too many sites within the argmax margin: another seed")
        dist = np.array([gr.rel_dist(a, b) for a, b in zip(g32, mine["grads"])])
        ref_rel_max = max(ref_rel_max, float(dist.max()))
        out[f"dist_{n}"] = dist
        out[f"near_{n}"] = np.int64(near.sum())
        out[f"loss_{n}"] = np.float32(loss.item())
        out[f"sum_{n}"] = np.array([g.astype(np.float64).sum() for g in g32])
        out[f"l2_{n}"] = np.array([np.sqrt((g.astype(np.float64) ** 2).sum()) for g in g32])
        out[f"val_{n}"] = np.stack([g.reshape(-1)[gr.sample_index(i, g.shape)] for i, g in enumerate(g32)])
        print(f"N = {n}: loss {loss.item():.6f}, |g32 - g64| / max |g64| per tensor: {dist.min():.2e} .. {dist.max():.2e}, "
              f"smallest max |g| {min(np.abs(g).max() for g in mine['grads']):.2e}, {int(near.sum())} sites within the margin")
    out["ref_rel_max"] = np.float64(ref_rel_max)
    # the restatement reproduces every stored number within ref_rel_max (sums and norms: relative to the tensor's largest entry times its size)
    for n, mine in results.items():
        assert abs(mine["loss"] - float(out[f"loss_{n}"])) <= 1e-4, n
        for i, g in enumerate(mine["grads"]):
            top = np.abs(g).max()
            assert top > 0, (n, i)
            assert np.abs(out[f"val_{n}"][i] - g.reshape(-1)[gr.sample_index(i, g.shape)]).max() <= ref_rel_max * top, (n, i)
            assert abs(out[f"sum_{n}"][i] - g.sum()) <= ref_rel_max * top * g.size, (n, i)
            assert abs(out[f"l2_{n}"][i] - np.sqrt((g ** 2).sum())) <= ref_rel_max * top * np.sqrt(g.size), (n, i)
    path = os.path.join(HERE, "hap_grad.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 827160, (os.path.getsize(path), "larger than the largest fixture already there")
    print(f"hap_grad.npz: {os.path.getsize(path)} bytes; ref_rel_max {ref_rel_max:.3e}")


if __name__ == "__main__":
    main()
