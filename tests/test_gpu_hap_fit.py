"""train.train_haplotype_bins(pn_value=...) and train.fit_haplotype on the device, on the labelled files, weights and float64 epoch of
tests/test_gpu_hap_train_bins.py.

The upsampled epoch is held to the float64 restatement (tests/hap_grad_rules.py) fed the restated sample order: per pass the list of
tests/hap_sample_rules.py at draw = the pass's number, permuted by pass_order of its length.  Bounds: those of
test_gpu_hap_train_bins.py::test_one_epoch_follows_the_restatement - mean loss within 1e-4, every tensor plain SGD leaves within PARITY of
the float64 one, at the same rate 1e-6 (that file's docstring says why the rule carries over at that rate; the upsampled epoch has fewer
batches than the plain one, so no tensor moves further)."""
from __future__ import annotations

import shutil

import numpy as np
import pytest

from tests import hap_eval_rules as hr
from tests import hap_grad_rules as gr
from tests import hap_sample_rules as sr
from tests.test_gpu_hap_train_bins import B, LR, PARITY, PASS, _float64_epoch, _params, _run_epoch, _state, epoch_files  # noqa: F401
from tests.test_hap_eval_rules import file_features

pytestmark = pytest.mark.gpu
PN = 0.7


def _float64_pn_epoch(files, weights, seed, pn):
    """_float64_epoch of test_gpu_hap_train_bins.py with the sample list between the label pass and the order"""
    import torch
    from nanosnp_amd import train
    gen = torch.Generator().manual_seed(seed)
    w = [np.asarray(a, np.float64).copy() for a in weights]
    losses, counts, per_pass, pass_no = [], np.zeros(2, np.int64), [], 0
    for f in files:
        xp, xh = file_features(f)
        rows, cls, _ = hr.label_filter(f["labels"])
        for a in range(0, len(f["labels"]), PASS):
            draw, pass_no = pass_no, pass_no + 1
            sel = np.flatnonzero((rows >= a) & (rows < a + PASS))
            samples, meta = sr.train_samples(cls[sel], pn, seed, draw)
            per_pass.append((int(meta[1]), int(meta[2])))
            if not samples.size:
                continue
            counts += (meta[1], meta[0] - meta[1])
            s_all = sel[samples[train.pass_order(gen, samples.size).numpy()]]
            for o in range(0, s_all.size, B):
                s = s_all[o:o + B]
                r = gr.loss_and_grad(w, xp[rows[s]], xh[rows[s]], cls[s])
                losses.append(r["loss"])
                w = [p - LR * g for p, g in zip(w, r["grads"])]
    return dict(w=w, mean_loss=float(np.mean(losses)), batches=len(losses), counts=counts, per_pass=per_pass)


def _run_pn_epoch(ef, pn, seed=2022):
    import torch
    from nanosnp_amd import train
    tr = train.HaplotypeTrainer(_state(ef["weights"]), chunk_sites=32)
    opt = torch.optim.SGD(tr.parameters(), lr=LR)
    res = train.train_haplotype_bins(tr, ef["paths"], ef["reference"], optimizer=opt, batch_size=B, dropout=0.0, max_grad_norm=None, seed=seed,
                                     pass_sites=PASS, pn_value=pn)
    p = _params(tr)
    tr.ctx.close()
    return res, p


def test_one_upsampled_epoch_follows_the_restatement(epoch_files):
    from nanosnp_amd import train
    ef = epoch_files
    want = _float64_pn_epoch(ef["files"], ef["weights"], 2022, PN)
    res, p = _run_pn_epoch(ef, PN)
    live = [c for c in want["per_pass"] if c[0]]
    assert len(live) >= 2 and sum(1 for c in live if c[1]) >= 2           # several passes draw, so the draw counter advances
    # counts: sites are samples, a variant counts as often as it was drawn
    assert res["sites"] == sum(train.pn_sample_count(r, v, PN) for r, v in want["per_pass"]) == int(want["counts"].sum())
    assert (res["samples_refcall"], res["samples_variant"]) == tuple(int(v) for v in want["counts"])
    assert res["samples_refcall"] == res["refcalls"] and res["samples_variant"] == sum(int(r * PN) for r, v in want["per_pass"] if v)
    assert res["samples_variant"] != res["variants"] and res["batches"] == want["batches"] >= 3
    print(f"upsampled epoch: {res['samples_refcall']} refcalls + {res['samples_variant']} draws of {res['variants']} variants; mean_loss "
          f"{res['mean_loss']:.6f} against {want['mean_loss']:.6f}; parameters (bound {PARITY:.2e}) "
          + " ".join(f"{gr.rel_dist(a, b):.1e}" for a, b in zip(p, want["w"])))
    moved = max(gr.rel_dist(a, b) for a, b in zip(want["w"], ef["weights"]))
    assert 100 * PARITY < moved <= 1.0                                    # (the premise of the bound, as in the plain epoch's test)
    assert abs(res["mean_loss"] - want["mean_loss"]) <= 1e-4
    assert max(gr.rel_dist(a, b) for a, b in zip(p, want["w"])) <= PARITY
    res2, p2 = _run_pn_epoch(ef, PN)                                      # the same seed gives the same bits
    assert res2 == res and all(np.array_equal(a, b) for a, b in zip(p, p2))


def test_without_pn_value_the_epoch_is_the_plain_one(epoch_files):
    ef = epoch_files
    res, p = _run_pn_epoch(ef, None)
    res0, p0 = _run_epoch(ef, 0.0)                                        # the call test_one_epoch_follows_the_restatement makes
    assert res == res0 and all(np.array_equal(a, b) for a, b in zip(p, p0))
    want = _float64_epoch(ef["files"], ef["weights"], 2022)
    assert res["sites"] == int(want["meta"][0]) == res["samples_refcall"] + res["samples_variant"]
    assert (res["samples_refcall"], res["samples_variant"]) == (res["refcalls"], res["variants"])
    assert abs(res["mean_loss"] - want["mean_loss"]) <= 1e-4
    assert max(gr.rel_dist(a, b) for a, b in zip(p, want["w"])) <= PARITY


def _fit(ef, prefix, trainer=None, **kw):
    from nanosnp_amd import train
    tr = trainer if trainer is not None else train.HaplotypeTrainer(_state(ef["weights"]), chunk_sites=32)
    args = dict(validating_paths=ef["paths"], epochs=3, batch_size=B, dropout=0.0, begin_to_adjust_lr=1, seed=5, save_prefix=prefix,
                pass_sites=PASS)
    args.update(kw)
    out = train.fit_haplotype(tr, ef["paths"], ef["reference"], **args)
    tr.ctx.close()
    return out


def test_fit_three_epochs_checkpoints_and_resume(epoch_files, tmp_path):
    import torch
    from nanosnp_amd import haplotype_model, train
    ef, prefix = epoch_files, str(tmp_path / "hap")
    out = _fit(ef, prefix)
    assert [r["epoch"] for r in out] == [0, 1, 2] and not any(r["stopped"] for r in out)
    assert [r["lr"] for r in out] == [1e-5, 1e-5, 1e-5 * 0.98]            # the rate each epoch ran with: the decay starts behind epoch 1
    assert out[0]["global_step"] == 1 + out[0]["batches"] and out[2]["global_step"] == 1 + sum(r["batches"] for r in out)
    assert all(r["sites"] == r["samples_refcall"] + r["samples_variant"] and r["samples_variant"] > 0 for r in out)        # pn_value 0.7
    f1 = [r["eval"]["gt_f1"] for r in out]
    best, best_epoch = 0.0, None
    for e, v in enumerate(f1):
        if v >= best:                                                     # the reference's >=: the last of tied epochs
            best, best_epoch = v, e
    assert best_epoch is not None
    assert [r["best_checkpoint"] is not None for r in out] == [v >= max([0.0] + f1[:e]) for e, v in enumerate(f1)]
    sds = [torch.load(f"{prefix}.epoch{e}.chkpt") for e in range(3)]
    for e, sd in enumerate(sds):
        assert out[e]["checkpoint"] == f"{prefix}.epoch{e}.chkpt" and list(sd) == haplotype_model.state_dict_keys()
        haplotype_model.LSTMNetwork().load_state_dict(sd)
    assert any(not torch.equal(sds[0][k], sds[2][k]) for k in sds[0])
    top = torch.load(f"{prefix}.chkpt")
    assert all(torch.equal(top[k], sds[best_epoch][k]) for k in top)
    # the default optimiser is the shipped file's; the state beside an epoch holds the rate the next one runs with
    ck = [torch.load(f"{prefix}.epoch{e}.optim") for e in range(3)]
    assert [c["optimizer"]["param_groups"][0]["lr"] for c in ck] == [1e-5, 1e-5 * 0.98, 1e-5 * 0.98 * 0.98]
    assert all(c["optimizer"]["param_groups"][0]["weight_decay"] == 1e-4 and "lookahead_k" in c["optimizer"]["param_groups"][0] for c in ck)
    assert [c["step"] for c in ck] == [r["global_step"] for r in out] and [c["epoch"] for c in ck] == [1, 2, 3]
    assert ck[2]["best_gt_f1"] == best
    # resume behind epoch 1: the third epoch again, from the files alone
    prefix2 = str(tmp_path / "again")
    shutil.copy(f"{prefix}.epoch1.optim", f"{prefix2}.epoch1.optim")
    tr = train.HaplotypeTrainer.from_checkpoint(f"{prefix}.epoch1.chkpt", chunk_sites=32)
    opt = train.DeviceOptimizer(tr, kind="LookaheadAdam")
    opt.load_state_dict(ck[1]["optimizer"], ck[1]["step"], ck[1]["epoch"])
    again = _fit(ef, prefix2, trainer=tr, optimizer=opt, start_epoch=2)
    assert len(again) == 1 and again[0]["epoch"] == 2
    assert (again[0]["lr"], again[0]["global_step"]) == (out[2]["lr"], out[2]["global_step"])
    assert again[0]["mean_loss"] == out[2]["mean_loss"] and again[0]["eval"]["gt_f1"] == f1[2]
    sd = torch.load(f"{prefix2}.epoch2.chkpt")
    assert all(sd[k].numpy().tobytes() == sds[2][k].numpy().tobytes() for k in sds[2])
    assert (again[0]["best_checkpoint"] is not None) == (f1[2] >= max(f1[:2]))                       # the best so far came with the state


def test_fit_finetune_rate_the_stop_and_refusals(epoch_files, tmp_path, monkeypatch):
    """the loop's bookkeeping alone: on the file that keeps no row an epoch has no batch"""
    import torch
    import torch.distributed as tdist
    from nanosnp_amd import train
    ef = epoch_files
    empty = dict(ef, paths=[ef["paths"][2]])
    out = _fit(empty, None, validating_paths=None, epochs=1, finetune=True)
    assert len(out) == 1 and out[0]["lr"] == 1e-5 * 0.1 and out[0]["batches"] == 0 and out[0]["eval"] is None and out[0]["checkpoint"] is None
    # min_lr just above the first decayed rate: the loop ends behind the epoch that decayed
    prefix = str(tmp_path / "stop")
    out = _fit(empty, prefix, validating_paths=None, epochs=5, begin_to_adjust_lr=1, min_lr=1e-5 * 0.98 * (1 + 1e-9))
    assert [r["stopped"] for r in out] == [False, True] and [r["lr"] for r in out] == [1e-5, 1e-5]
    assert torch.load(f"{prefix}.epoch1.optim")["optimizer"]["param_groups"][0]["lr"] == 1e-5 * 0.98
    tr = train.HaplotypeTrainer(_state(ef["weights"]), chunk_sites=8)
    with pytest.raises(ValueError, match="finetune"):
        train.fit_haplotype(tr, empty["paths"], ef["reference"], optimizer=train.DeviceOptimizer(tr), finetune=True)
    with pytest.raises(ValueError, match="pn_value"):
        train.train_haplotype_bins(tr, empty["paths"], ef["reference"], pn_value=-0.1)
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="process group"):
        train.fit_haplotype(tr, ef["paths"], ef["reference"])
    tr.ctx.close()
