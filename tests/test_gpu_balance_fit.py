"""train.train_train_bins(use_balance=True) and train.fit(use_balance=True): an epoch over balance_dataset's sample lists
(nsnp_pileup_balance_samples on the device) against a float64 replay that builds each pass's list with tests/balance_rules.py and the same
pass_order, on the fixture files and helpers of tests/test_gpu_train.py.

Passes of 615 rows: train_g1 is one pass of 138 rows (14 categories, M = 39), train_cut three of 615, 615 and 1 rows (M = 200, M = 181, and
a tail of one row: one category, status 1, trained as it is).  Bound: that test's ATOL (1e-4, the project's bound for this replay) on
mean_loss, the accuracies and all 24 tensors; sites, samples_drawn, rows and passes_unbalanced exact."""
from __future__ import annotations

import numpy as np
import pytest

from tests import balance_rules as br
from tests import eval_rules as er
from tests import grad_rules as gr
from tests.test_gpu_train import ATOL, DATA_NPZ, sets, weights  # noqa: F401

pytestmark = pytest.mark.gpu

B, P, LR, SEED = 64, 615, 0.005, 7
CASES = ("train_g1", "train_cut")


def _params(tr):
    return [p.detach().cpu().numpy().copy() for p in tr.parameters()]


def test_one_balanced_epoch_follows_the_float64_replay(weights, sets):
    import torch
    from nanosnp_amd import train
    paths = [sets[c][0] for c in CASES]
    tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
    stats = {}
    res = train.train_train_bins(tr, paths, optimizer=torch.optim.SGD(tr.parameters(), lr=LR), batch_size=B, dropout=0.0, max_grad_norm=None,
                                 seed=SEED, pass_sites=P, stats=stats, use_balance=True)
    # the replay
    gen = torch.Generator().manual_seed(SEED)
    w = [np.asarray(t, np.float64) for t in weights]
    losses, correct, sites, rows_read, drawn, unbalanced, pass_no, counts = [], np.zeros(2), 0, 0, 0, 0, 0, []
    for c in CASES:
        _, x, label = sets[c]
        cls_all, _ = er.decode_labels(label)
        for a in range(0, x.shape[0], P):
            b = min(x.shape[0], a + P)
            samples, _, meta = br.balance_samples(cls_all[a:b], SEED, pass_no)
            pass_no, rows_read = pass_no + 1, rows_read + (b - a)
            if meta[5] == 0:
                order = samples[train.pass_order(gen, samples.size).numpy()] + a
                drawn += samples.size
            else:
                order = train.pass_order(gen, b - a).numpy() + a
                unbalanced += 1
            counts.append(order.size)
            for o in range(0, order.size, B):
                rows = order[o:o + B]
                r = gr.loss_and_grad(w, x[rows], cls_all[rows])
                w = [u - LR * g for u, g in zip(w, r["grads"])]
                losses.append(r["loss"])
                correct += (r["pred"] == cls_all[rows][:, :2]).sum(0)
                sites += rows.size
    dist = [float(np.abs(p - u).max()) for p, u in zip(_params(tr), w)]
    print("device", res, "float64 mean_loss", np.mean(losses), "accuracies", correct / sites, "per pass", counts, "stats", stats,
          "max |p - f64| per tensor", " ".join(f"{d:.1e}" for d in dist))
    assert counts == [39, 200, 181, 1]                                    # (three balanced passes and the tail of one row)
    assert res["sites"] == sites == 421 and res["samples_drawn"] == drawn == 420 and res["rows"] == rows_read == 138 + 1231
    assert res["passes_unbalanced"] == unbalanced == 1 and res["batches"] == len(losses) and stats["passes"] == 4 and stats["rows"] == 1369
    assert abs(res["mean_loss"] - np.mean(losses)) <= ATOL
    assert abs(res["gt_accuracy"] - correct[0] / sites) <= ATOL and abs(res["zy_accuracy"] - correct[1] / sites) <= ATOL
    assert len(dist) == 24 and max(dist) <= ATOL


def test_use_balance_false_is_the_call_without_the_keyword(sets):
    import torch
    from nanosnp_amd import train
    paths = [sets[c][0] for c in CASES]
    out = []
    for kw in ({}, {"use_balance": False}):
        tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
        res = train.train_train_bins(tr, paths, optimizer=torch.optim.SGD(tr.parameters(), lr=LR), batch_size=B, dropout=0.25, max_grad_norm=5.0,
                                     seed=SEED, pass_sites=P, **kw)
        out.append((res, _params(tr)))
    assert out[0][0] == out[1][0] and set(out[0][0]) == {"sites", "batches", "mean_loss", "gt_accuracy", "zy_accuracy"}
    assert out[0][0]["sites"] == 1369
    for u, v in zip(out[0][1], out[1][1]):
        assert np.array_equal(u, v)


def test_fit_two_balanced_epochs_with_a_checkpoint(sets, tmp_path):
    import torch
    from nanosnp_amd import train
    paths = [sets[c][0] for c in CASES]
    cls = [er.decode_labels(sets[c][2])[0] for c in CASES]
    tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
    opt = train.DeviceOptimizer(tr, kind="sgd", lr=LR)
    before = _params(tr)
    out = train.fit(tr, paths, epochs=2, optimizer=opt, batch_size=B, dropout=0.0, max_grad_norm=None, seed=SEED, pass_sites=P,
                    save_prefix=str(tmp_path / "bal"), use_balance=True)
    assert [r["epoch"] for r in out] == [0, 1]
    lists = []
    for e, r in enumerate(out):
        # the lists of epoch e are drawn under seed + e: the counts are the labels' alone, the rows are not
        want = [br.balance_samples(c[a:a + P], SEED + e, k) for k, (c, a) in enumerate([(cls[0], 0), (cls[1], 0), (cls[1], P), (cls[1], 2 * P)])]
        assert r["samples_drawn"] == sum(int(m[0]) for _, _, m in want) == 420 and r["sites"] == 421 and r["rows"] == 1369
        assert r["passes_unbalanced"] == 1 and np.isfinite(r["mean_loss"]) and r["batches"] == 1 + 4 + 3 + 1
        lists.append(np.concatenate([s for s, _, _ in want]))
    assert not np.array_equal(lists[0], lists[1])
    assert out[0]["mean_loss"] != out[1]["mean_loss"]
    ck = torch.load(out[1]["checkpoint"], map_location="cpu", weights_only=False)
    assert ck["epoch"] == 2 and ck["step"] == opt.global_step == 1 + 2 * 9
    back = train.PileupTrainer.from_checkpoint(out[1]["checkpoint"], chunk_sites=64)
    for u, v, w0 in zip(_params(back), _params(tr), before):
        assert np.array_equal(u, v)
    assert any(not np.array_equal(v, w0) for v, w0 in zip(_params(tr), before))
    # the device's lists of epoch e come from seed + e: two single epochs by hand under SEED and SEED + 1 repeat fit's bits (mean loss
    # and every parameter), and a second epoch under SEED again - what a fit that handed every epoch the same seed would run - does not
    by_hand = {}
    for second in (SEED + 1, SEED):
        t = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
        o = train.DeviceOptimizer(t, kind="sgd", lr=LR)
        res = [train.train_train_bins(t, paths, optimizer=o, batch_size=B, dropout=0.0, max_grad_norm=None, seed=s, pass_sites=P,
                                      use_balance=True) for s in (SEED, second)]
        by_hand[second] = (res, _params(t))
    res, params = by_hand[SEED + 1]
    assert [r["mean_loss"] for r in res] == [r["mean_loss"] for r in out]
    assert all(np.array_equal(u, v) for u, v in zip(params, _params(tr)))
    res, params = by_hand[SEED]
    assert res[0]["mean_loss"] == out[0]["mean_loss"] and res[1]["mean_loss"] != out[1]["mean_loss"]
    assert any(not np.array_equal(u, v) for u, v in zip(params, _params(tr)))
    # the keyword off: fit runs the plain epoch
    tr2 = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
    plain = train.fit(tr2, paths, epochs=1, optimizer=train.DeviceOptimizer(tr2, kind="sgd", lr=LR), batch_size=B, dropout=0.0,
                      max_grad_norm=None, seed=SEED, pass_sites=P)
    assert plain[0]["sites"] == 1369 and "samples_drawn" not in plain[0]
