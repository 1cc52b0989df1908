#!/usr/bin/env python3
"""Generate tests/golden/pileup_eval.npz from the reference's own model code: what its eval() (PileupModel/train.py:93-150) computes on the
windows and labels of train_g1.td.gz and train_cut.td.gz with ont_pileup.chkpt.

Runs only where the reference tree is mounted.  The reference's model.LSTMNetwork is imported with the stubs of SURVEY appendix C, the
checkpoint loaded, and per set

    model(x, ...) over ALL rows in one batch                      -> logits fp32 [N,90] (gt | zy | indel1 | indel2)
    model(x, ...) over the variant rows in batches of 4, in order -> the per-batch losses, as the loop of train.py:103-136 sees them
    its LabelSmoothingLoss on single rows                         -> site_loss fp32 [variants,4]

and over both files in the order g1, cut: total_loss, avg_loss (train.py:122,136), the argmax-derived accuracies and confusion matrices.
Before anything is written the float64 restatement (tests/eval_rules.py) must reproduce every number, and the distance between the
reference's fp32 logits and the restatement is recorded (dist_f64_<set>): an input is admissible for a 1e-4 test only below 2.5e-5.  The same
distance is measured for the seeded synthetic windows of eval_rules.synthetic_windows (synth_dist_f64).

    python tests/golden/make_golden_eval.py
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("REF", "/root/reference")
SETS = (("g1", "train_g1"), ("cut", "train_cut"))
BATCH = 4
ADMISSIBLE = 2.5e-5


def reference_model():
    import torch
    import yaml
    for name, attrs in (("ranger", {"Ranger": object}), ("ranger21", {"Ranger21": object}), ("tables", {"Filters": lambda **k: None}), ("pysam", {})):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules.setdefault(name, m)
    pm = os.path.join(REF, "PileupModel")
    sys.path.insert(0, pm)
    from model import LSTMNetwork
    from utils import AttrDict
    cfg = AttrDict(yaml.load(open(os.path.join(pm, "config", "ont_pileup.yaml")), Loader=yaml.FullLoader))
    model = LSTMNetwork(cfg.model)
    ck = torch.load(os.path.join(pm, "models", "ont_pileup.chkpt"), map_location="cpu", weights_only=False)
    model.encoder.load_state_dict(ck["encoder"]); model.forward_layer.load_state_dict(ck["forward_layer"]); model.eval()
    return model, ck


def run(model, x, cls):
    import torch
    t = [torch.from_numpy(cls[:, h].astype(np.int64)) for h in range(4)]
    with torch.no_grad():
        loss, *logits = model(torch.from_numpy(x.astype(np.float32)), *t)
    return float(loss.item()), np.concatenate([z.numpy() for z in logits], axis=1)


def main():
    import torch
    from tests import eval_rules as er
    from nanosnp_amd.pileup_model import ENCODER_KEYS, FORWARD_KEYS
    torch.manual_seed(0)
    model, ck = reference_model()
    npf = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)
    weights = [npf(ck["encoder"][k]) for k in ENCODER_KEYS] + [npf(ck["forward_layer"][k]) for k in FORWARD_KEYS]
    indel = [npf(ck["forward_layer"][k]) for k in ("indel1_layer.weight", "indel1_layer.bias", "indel2_layer.weight", "indel2_layer.bias")]
    crits = (model.gt_crit, model.zy_crit, model.indel1_crit, model.indel2_crit)
    out = {"indel1_weight": indel[0], "indel1_bias": indel[1], "indel2_weight": indel[2], "indel2_bias": indel[3], "batch_size": np.int64(BATCH)}
    total_loss, total_sites, parts, files = 0.0, 0, [], []
    with tempfile.TemporaryDirectory() as d:
        for tag, case in SETS:
            _, x, label = er.fixture_rows(case, d)
            files.append((x, label))
            cls_all, bad = er.decode_labels(label)
            assert not bad.any(), (case, "the reference wrote a row that is not one-hot")
            _, logits = run(model, x, cls_all)
            z64 = er.forward_logits_f64(weights, indel, x)
            dist = float(np.abs(logits.astype(np.float64) - z64).max())
            assert dist <= ADMISSIBLE, (case, dist, "not admissible: the reference's own fp32 result is too far from float64")
            k = er.keep_rows(cls_all)
            assert k.size % BATCH, (case, "no short last batch")
            xv, cv = x[k], cls_all[k]
            batch_loss, vz = [], []
            for a in range(0, k.size, BATCH):
                l, z = run(model, xv[a:a + BATCH], cv[a:a + BATCH])
                batch_loss.append(l); vz.append(z)
                total_loss += l; total_sites += z.shape[0]
            vz = np.concatenate(vz)
            assert np.abs(vz - logits[k]).max() <= 1e-5, case        # (the batch a row sits in moves its logits by rounding only)
            site_loss = np.zeros((k.size, 4), np.float32)
            with torch.no_grad():
                for h, ((r0, c, _), crit) in enumerate(zip(er.HEADS, crits)):
                    for i in range(k.size):
                        site_loss[i, h] = float(crit(torch.from_numpy(vz[i:i + 1, r0:r0 + c]), torch.from_numpy(cv[i:i + 1, h].astype(np.int64))))
            pred = np.stack([torch.from_numpy(vz[:, r0:r0 + c]).argmax(1).numpy() for r0, c, _ in er.HEADS], axis=1).astype(np.uint8)
            parts.append((site_loss, cv, pred))
            out.update({f"logits_{tag}": logits, f"batch_loss_{tag}": np.array(batch_loss, np.float64), f"site_loss_{tag}": site_loss,
                        f"pred_{tag}": pred, f"dist_f64_{tag}": np.float64(dist), f"variants_{tag}": k.astype(np.int64)})
            # the restatement reproduces the set
            mine = er.smoothed_loss(z64[k], cv)
            assert np.abs(mine - site_loss).max() <= 1e-4 and np.array_equal(er.predictions(z64[k]), pred), case
            bm = er.batch_means(mine, BATCH)
            assert np.abs(bm[:, 0] + bm[:, 1] - np.array(batch_loss)).max() <= 1e-4, case
            print(f"{case}: {x.shape[0]} rows, {k.size} variants, |fp32 - f64| = {dist:.3e}")
        # the synthetic windows of the GPU tests: admissible too?
        xs, cs = er.synthetic_windows(files[1][0], er.SYNTH_MAX)
        sd = 0.0
        for a in range(0, er.SYNTH_MAX, 4096):
            _, z = run(model, xs[a:a + 4096], cs[a:a + 4096])
            sd = max(sd, float(np.abs(z.astype(np.float64) - er.forward_logits_f64(weights, indel, xs[a:a + 4096])).max()))
        assert sd <= ADMISSIBLE, (sd, "the synthetic windows are not admissible: another seed")
        out["synth_dist_f64"] = np.float64(sd)
        print(f"synthetic: {er.SYNTH_MAX} rows, |fp32 - f64| = {sd:.3e}")
    ref = er.result_from(parts, BATCH)
    conf = er.confusion(np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    out.update({"total_loss": np.float64(total_loss), "avg_loss": np.float64(total_loss / total_sites), "sites": np.int64(total_sites),
                "gt_accuracy": np.float64(ref["gt_accuracy"]), "zy_accuracy": np.float64(ref["zy_accuracy"]), "confusion": conf})
    mine = er.evaluate(weights, indel, files, BATCH)
    assert mine["sites"] == total_sites and abs(mine["avg_loss"] - out["avg_loss"]) <= 1e-4 and np.array_equal(mine["gt_confusion"], ref["gt_confusion"])
    path = os.path.join(HERE, "pileup_eval.npz")
    np.savez_compressed(path, **out)
    limit = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "pileup_eval.npz")
    assert os.path.getsize(path) <= limit, (os.path.getsize(path), "larger than the largest fixture already there")
    print(f"pileup_eval.npz: {os.path.getsize(path)} bytes; avg_loss {out['avg_loss']:.6f} over {total_sites} sites")


if __name__ == "__main__":
    main()
