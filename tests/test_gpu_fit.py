"""Training with the fused step: train_train_bins with a DeviceOptimizer against the same loop on torch's own pieces, resuming from a
checkpoint, and the epoch loop ``fit`` (nanosnp_amd.train).

Data: tests/golden/train_g1.td.gz (138 rows); batches of 10 give 14 batches per epoch, so with Lookahead's k = 6 an epoch holds the no-op
first sync (step 6) and the first real one (step 12).  Weights: nanosnp_amd/data/ont_pileup_weights.npz.  Dropout 0 throughout: nothing random.

The displacement cap of 1e-3 is a cap, not a measurement: fp32 rounding of a parameter is about 1e-5 of a 14-step displacement at lr 1e-4,
while a wrong beta, bias correction, clip or sync moves it by percents.  Measured on an MI355X (docs/rounds/r27.md): 2e-6 .. 1.1e-4 per
tensor.  The shipped weights reach 1.3 - 1.7 in the LSTM matrices, not 0.1, so ONE rounding of such a parameter (1.5e-7 - 2e-7) is 1e-4 of a
14-step displacement of 1.4e-3; in roundings (2^-23) of the tensor's largest parameter every distance is 0.77 or less, which the test
prints beside the ratios."""
import os

import numpy as np
import pytest

from tests import eval_rules as er
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu
DATA_NPZ = os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz")
B, LR, MAX_NORM, SEED = 10, 1e-4, 20.0, 7


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return er.fixture_rows("train_g1", str(tmp_path_factory.mktemp("gpu_fit")))          # (path, windows, labels)


def _trainer():
    from nanosnp_amd import train
    return train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)


def _host(tr):
    return [p.detach().cpu().numpy().copy() for p in tr.parameters()]


class _Lookahead:
    """PileupModel/lookahead.py:34-58 in six lines: the slow copy is made at the first sync"""

    def __init__(self, base, params, alpha=0.5, k=6):
        self.base, self.params, self.alpha, self.k, self.n, self.slow = base, params, alpha, k, 0, None

    def step(self):
        self.base.step()
        self.n += 1
        if self.n % self.k == 0:
            self.slow = self.slow if self.slow is not None else [p.detach().clone() for p in self.params]
            for p, s in zip(self.params, self.slow):
                s.add_(p.detach() - s, alpha=self.alpha)
                p.data.copy_(s)


def test_epoch_equals_torch_adam_clip_and_lookahead(rows):
    import torch
    from nanosnp_amd import train
    path = rows[0]
    kw = dict(batch_size=B, dropout=0.0, max_grad_norm=MAX_NORM, seed=SEED)
    a = _trainer()
    start = _host(a)
    res_a = train.train_train_bins(a, path, optimizer=train.DeviceOptimizer(a, kind="LookaheadAdam", lr=LR), **kw)
    b = _trainer()
    res_b = train.train_train_bins(b, path, optimizer=_Lookahead(torch.optim.Adam(b.parameters(), lr=LR, betas=(0.9, 0.999), eps=1e-8), b.parameters()),
                                   **kw)
    assert res_a["batches"] == res_b["batches"] == 14 >= 13 and res_a["sites"] == 138
    ratios, ulps = [], []
    for name, s, pa, pb in zip(train.PARAM_NAMES, start, _host(a), _host(b)):
        da, db = pa - s, pb - s
        top = float(np.abs(db).max())
        diff = float(np.abs(da - db).max())
        ratios.append(diff / top if top > 0 else 0.0)
        ulps.append(diff / (2.0 ** -23 * float(np.abs(s).max())))
        assert top > 0 and diff <= 1e-3 * top, (name, diff, top)
    print("displacement distance / largest displacement per tensor: " + " ".join(f"{r:.1e}" for r in ratios) + f"; worst {max(ratios):.2e}; "
          "the same distances in roundings (2^-23) of the tensor's largest parameter: " + " ".join(f"{u:.2f}" for u in ulps) +
          f"; mean_loss {res_a['mean_loss']:.7f} against {res_b['mean_loss']:.7f}")
    assert abs(res_a["mean_loss"] - res_b["mean_loss"]) <= 1e-4
    assert res_a["gt_accuracy"] == res_b["gt_accuracy"] and res_a["zy_accuracy"] == res_b["zy_accuracy"]


def _steps(tr, opt, x, cls, first, last):
    """batches first .. last - 1 of 9 rows each: loss_and_grad and the fused step"""
    for s in range(first, last):
        r = slice(9 * s, 9 * s + 9)
        tr.loss_and_grad(x[r], cls[r, 0], cls[r, 1])
        opt.step(MAX_NORM)


@pytest.mark.parametrize("kind, cut", [("LookaheadAdam", 7), ("LookaheadRadam", 5)])
def test_resume_is_bit_exact(rows, tmp_path, kind, cut):
    """14 straight steps = `cut` steps, save_checkpoint(optimizer=...), a fresh trainer from the file plus load_state_dict, the other steps.
    LookaheadAdam, 7: the checkpoint is cut between the first sync (step 6, which fills the slow buffers) and the second (step 12, which
    reads them).  LookaheadRadam, 5: it is written while N_sma < 5 and before any sync - the file holds no slow buffers - and the first
    resumed step is both the first form = 0 step of RAdam and the first Lookahead sync."""
    import torch
    from nanosnp_amd import train
    _, x, label = rows
    xd = torch.from_numpy(x).cuda()
    cls = torch.from_numpy(er.decode_labels(label)[0].astype(np.int64)).cuda()
    a = _trainer()
    oa = train.DeviceOptimizer(a, kind=kind, lr=LR, weight_decay=1e-4)
    _steps(a, oa, xd, cls, 0, 14)
    b = _trainer()
    ob = train.DeviceOptimizer(b, kind=kind, lr=LR, weight_decay=1e-4)
    ob.epoch()
    _steps(b, ob, xd, cls, 0, cut)
    path = str(tmp_path / "mid.chkpt")
    b.save_checkpoint(path, optimizer=ob)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["step"] == cut + 1 and sorted(ck["optimizer"]) == ["param_groups", "slow_state", "state"]
    assert sorted(ck["optimizer"]["state"]) == list(range(24)) and sorted(ck["optimizer"]["slow_state"]) == (list(range(24)) if cut >= 6 else [])
    assert sorted(ck["optimizer"]["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and not ck["optimizer"]["state"][0]["exp_avg"].is_cuda
    if kind == "LookaheadRadam":
        assert [train.step_scalars(True, t, LR, 0.9, 0.999, 1e-4)["form"] for t in (cut, cut + 1)] == [1, 0] and cut + 1 == ob.k
    c = train.PileupTrainer.from_checkpoint(path, chunk_sites=64)
    oc = train.DeviceOptimizer(c, kind=kind, lr=3.0, weight_decay=0.5, alpha=0.1, k=3)               # (every setting comes from the file)
    oc.load_state_dict(ck["optimizer"], ck["step"], ck["epoch"])
    assert (oc.lr, oc.weight_decay, oc.alpha, oc.k, oc.global_step, oc.current_epoch, oc.step_count) == (LR, 1e-4, 0.5, 6, cut + 1, 1, cut)
    assert oc.slow_ready == (cut >= 6) and oc.lookahead_step == cut
    _steps(c, oc, xd, cls, cut, 14)
    torch.cuda.synchronize()
    for pa, pc in zip(_host(a), _host(c)):
        assert np.array_equal(pa, pc)
    for ta, tc in zip(oa.exp_avg + oa.exp_avg_sq + oa.slow, oc.exp_avg + oc.exp_avg_sq + oc.slow):
        assert torch.equal(ta, tc)
    assert oa.global_step == oc.global_step == 15
    if kind != "LookaheadAdam":
        return
    # a reference checkpoint's optimizer entry: torch's state plus a slow_state keyed by id() - the moments load, the slow buffers restart
    theirs = {"state": {i: {"step": torch.tensor(7.0), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]} for i, st in ck["optimizer"]["state"].items()},
              "slow_state": {140000000000000 + 64 * i: v for i, v in ck["optimizer"]["slow_state"].items()},
              "param_groups": [dict(ck["optimizer"]["param_groups"][0], amsgrad=False, maximize=False)]}
    od = train.DeviceOptimizer(_trainer(), kind="LookaheadAdam")
    od.load_state_dict(theirs)
    assert od.step_count == 7 and od.lookahead_step == 7 and not od.slow_ready and od.state_dict()["slow_state"] == {}
    assert all(torch.equal(t.cpu(), ck["optimizer"]["state"][i]["exp_avg"]) for i, t in enumerate(od.exp_avg))


def test_fit_three_epochs(rows, tmp_path):
    import torch
    from nanosnp_amd import train
    from nanosnp_amd.pileup_model import LSTMNetwork
    path = rows[0]
    tr = _trainer()
    opt = train.DeviceOptimizer(tr, kind="LookaheadAdam", lr=LR)
    prefix = str(tmp_path / "run")
    out = train.fit(tr, path, validating_paths=path, epochs=3, optimizer=opt, batch_size=B, dropout=0.0, max_grad_norm=MAX_NORM, decay_ratio=0.98,
                    begin_to_adjust_lr=1, seed=SEED, save_prefix=prefix)
    assert [r["epoch"] for r in out] == [0, 1, 2] and [r["batches"] for r in out] == [14, 14, 14]
    assert [r["lr"] for r in out] == [LR, LR, LR * 0.98] and opt.lr == LR * 0.98 * 0.98          # decay after epochs 1 and 2, not after epoch 0
    assert opt.global_step == 1 + 3 * 14 and opt.current_epoch == 3 and [r["global_step"] for r in out] == [15, 29, 43]
    assert out[0]["mean_loss"] != out[1]["mean_loss"]                                             # (another order and other weights)
    xs = torch.from_numpy(rows[1][:8]).cuda()
    for e, r in enumerate(out):
        assert r["checkpoint"] == f"{prefix}.epoch{e}.chkpt" and r["eval"]["sites"] > 0 and np.isfinite(r["eval"]["avg_loss"])
        ck = torch.load(r["checkpoint"], map_location="cpu", weights_only=False)
        assert ck["epoch"] == e + 1 and ck["step"] == 1 + 14 * (e + 1) and ck["optimizer"]["param_groups"][0]["lr"] == r["lr"]
        model = LSTMNetwork.from_checkpoint(r["checkpoint"])
        assert all(bool(torch.isfinite(t).all()) for t in model.predict(xs))
    last = LSTMNetwork.from_checkpoint(out[2]["checkpoint"])
    now = tr.to_model()
    for u, v in zip(last.predict(xs), now.predict(xs)):
        assert torch.equal(u, v)
    # the default optimiser is the shipped configuration
    quick = train.fit(_trainer(), path, epochs=1, batch_size=69, dropout=0.0)
    assert len(quick) == 1 and quick[0]["batches"] == 2 and quick[0]["lr"] == 1e-4 and quick[0]["global_step"] == 3 and quick[0]["checkpoint"] is None
