"""Score a checkpoint on training window files (<chr>.td.bin): the reference's ``eval()`` (PileupModel/train.py:93-150) on the device.

``evaluate_train_bins`` reads the files pipeline.mpileup_to_train_bins / sitefile.td_to_bin write, keeps the variant sites as
``TrainDataset(for_evaluate=True)`` does (dataset.py:98-104), runs the forward with all four heads and the label-smoothed loss
(model.py:97-112, optim.py:137-144) and returns what eval() accumulates: the loss, the accuracies and the confusion matrices of genotype
and zygosity - plus those of the two indel heads, which eval() computes logits for and then ignores.  Training itself is out of scope
(DESIGN.md section 9): this is inference with labels attached.  fp32 only.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, host, sitefile

HEAD_NAMES = ("gt", "zy", "id1", "id2")


class _PassSet:
    """buffers of one pass in flight: windows (bytes: int16 or int32 per file) and label rows; pinned on the host, plain on the device"""
    def __init__(self, P, dev=None):
        import torch
        kw = dict(pin_memory=True) if dev is None else dict(device=dev)
        self.x = torch.empty(P * 594 * 4, dtype=torch.uint8, **kw)
        self.y = torch.empty((P, _lib.Context.LABEL_WIDTH), dtype=torch.int32, **kw)
        if dev is None:
            self.meta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
            self.h2d_done = None
        else:
            self.x32 = torch.empty((P * 33, 18), dtype=torch.int32, device=dev)     # the pass flattened: centre of window n at row 33 n + 16
            self.cls = torch.empty((P, 4), dtype=torch.uint8, device=dev)
            self.centers = torch.empty(P, dtype=torch.int64, device=dev)
            self.free = None


def evaluate_train_bins(model, validating_paths, batch_size=1000, variants_only=True, pass_sites=65536, keep_sites=False, stats=None):
    """``eval(epoch, config, model, validating_paths, batch_size, ...)`` of PileupModel/train.py:93-150 over ``.td.bin`` files -> dict

        sites                 kept sites (variants_only: rows whose zygosity class is > 0, dataset.py:99; else every row)
        avg_loss              train.py:122,136 - the sum over batches of the batch MEAN of gt + zy, divided by the number of SITES (the
                              reference's own quantity, quirk kept: it shrinks with batch_size)
        mean_loss             the mean over sites of gt + zy (= gt_loss + zy_loss)
        gt_loss, zy_loss, id1_loss, id2_loss     per-head means over sites
        gt_accuracy, zy_accuracy                 torchmetrics.Accuracy of train.py:97-98,137-138
        gt_confusion [21,21], zy_confusion [3,3], id1_confusion [33,33], id2_confusion [33,33]     int64 [target][predicted] (train.py:101-102)
        malformed_labels      rows (of all rows read) that are not one-hot in some family
        files                 with keep_sites: per file {path, rows int64 [k], cls uint8 [k,4], pred uint8 [k,4], site_loss fp32 [k,4]}

    validating_paths: a list of paths or a directory (its ``*.bin`` files in os.listdir order).  Batches restart with every file, as the
    reference's DataLoader per file does.  Host loop: a file is read in passes of `pass_sites` rows through three pinned sets, sent on the
    package's copy stream (int16 windows widened on the device) with the label rows beside them; the label pass of pass k + 1
    (nsnp_pileup_label_classes) is issued before the host reads the kept count of pass k from pinned memory, so the one host wait per pass
    is for work issued a pass earlier.  Losses, predictions, classes and rows of a file stay on the device until the run ends; the per-batch
    sums are float64 (nsnp_pileup_batch_loss)."""
    import torch
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("evaluate_train_bins under a process group of more than one rank (validation is not sharded)")
    if not getattr(model, "_loaded", False):
        raise _lib.NanoSNPError("weights not loaded")
    if not getattr(model, "_indel_loaded", False):
        raise _lib.NanoSNPError("indel heads not loaded: the forward_layer state dict had no indel1_layer / indel2_layer tensors")
    B = int(batch_size)
    if B < 1:
        raise ValueError("batch_size >= 1")
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    st = stats if stats is not None else {}
    for k in ("passes", "rows", "bytes_h2d"):
        st.setdefault(k, 0)
    if isinstance(validating_paths, (str, os.PathLike)):
        d = str(validating_paths)
        paths = [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".bin")] if os.path.isdir(d) else [d]
    else:
        paths = [str(p) for p in validating_paths]
    files = []
    for p in paths:                                        # every header is checked before anything runs
        idx = sitefile.array_index(p)
        if ("position_matrix" not in idx or idx["position_matrix"][0] not in (np.dtype(np.int32), np.dtype(np.int16))
                or idx["position_matrix"][1][1:] != (33, 18)):
            raise sitefile.SiteFileError(f"{p}: not a window file (position_matrix int16 / int32 [N,33,18])")
        n = int(idx["position_matrix"][1][0])
        if "label" not in idx or idx["label"][0] != np.dtype(np.int32) or idx["label"][1] != (n, _lib.Context.LABEL_WIDTH):
            raise sitefile.SiteFileError(f"{p}: not a training window file (no label int32 [N,{_lib.Context.LABEL_WIDTH}] beside the windows)")
        a = sitefile.read_arrays(p, mmap=True)
        files.append(dict(path=p, n=n, x=a["position_matrix"], y=a["label"], elem=idx["position_matrix"][0].itemsize))
    P = int(max(1, pass_sites))
    passes = [(fi, a, min(f["n"], a + P)) for fi, f in enumerate(files) for a in range(0, f["n"], P)]
    last_pass_of = {fi: k for k, (fi, _, _) in enumerate(passes)}
    counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device=dev)
    per_file = [None] * len(files)
    malformed = 0
    if passes:
        sets = getattr(model, "_eval_sets", None)
        if not sets or sets[0] < P:
            sets = model._eval_sets = (P, [_PassSet(P) for _ in range(3)], [_PassSet(P, dev) for _ in range(3)])
        hsets, dsets = sets[1], sets[2]
        copy_stream = host.copy_stream(dev)
        main = torch.cuda.current_stream(dev)
        for s_ in hsets:
            s_.h2d_done = None
        for s_ in dsets:
            s_.free = None
        copy_stream.wait_stream(main)
        labelled = [None] * len(passes)                    # the event behind the label pass of pass k (blocking: the host sleeps on it)
        fill = {}                                          # file -> kept sites so far

        def issue(k):
            """stage pass k, send it, widen it, run its label pass"""
            fi, a, b = passes[k]
            f, m = files[fi], b - a
            hs, ds = hsets[k % 3], dsets[k % 3]
            if hs.h2d_done is not None:
                hs.h2d_done.synchronize()                  # (pass k - 3 has left this pinned set)
            nb = m * 594 * f["elem"]
            hs.x.numpy()[:nb].view(np.int16 if f["elem"] == 2 else np.int32)[:] = np.asarray(f["x"][a:b]).reshape(-1)
            hs.y.numpy()[:m] = f["y"][a:b]
            if ds.free is not None:
                copy_stream.wait_event(ds.free)            # (pass k - 3 has been scored out of this device set)
            with torch.cuda.stream(copy_stream):
                ds.x[:nb].copy_(hs.x[:nb], non_blocking=True)
                ds.y[:m].copy_(hs.y[:m], non_blocking=True)
                hs.h2d_done = torch.cuda.Event(blocking=True); hs.h2d_done.record(copy_stream)
            main.wait_event(hs.h2d_done)
            ds.x32[:m * 33].view(-1).copy_(ds.x[:nb].view(torch.int16 if f["elem"] == 2 else torch.int32))
            ctx.pileup_label_classes(ds.y[:m], variants_only, cls=ds.cls, center_idx=ds.centers, meta=hs.meta)
            labelled[k] = torch.cuda.Event(blocking=True); labelled[k].record(main)
            st["passes"] += 1; st["rows"] += m; st["bytes_h2d"] += nb + m * 360

        def score(k):
            """the kept sites of pass k (its count is on the host by now) through forward, loss and counts"""
            nonlocal malformed
            fi, a, b = passes[k]
            f, m = files[fi], b - a
            hs, ds = hsets[k % 3], dsets[k % 3]
            labelled[k].synchronize()
            kept, bad = int(hs.meta[0]), int(hs.meta[1])
            malformed += bad
            if per_file[fi] is None:
                mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
                per_file[fi] = dict(loss=mk((f["n"], 4), torch.float32), pred=mk((f["n"], 4), torch.uint8), cls=mk((f["n"], 4), torch.uint8),
                                    rows=mk(f["n"], torch.int64))
                fill[fi] = 0
            o, r = fill[fi], per_file[fi]
            if kept:
                ctx.pileup_eval_windows(ds.x32[:m * 33], ds.centers[:kept], ds.cls, counters, n=kept, site_loss=r["loss"][o:o + kept],
                                        pred=r["pred"][o:o + kept])
                r["cls"][o:o + kept].copy_(ds.cls[:kept])
                r["rows"][o:o + kept].copy_(torch.div(ds.centers[:kept] - 16, 33, rounding_mode="floor") + a)
            fill[fi] = o + kept
            ds.free = torch.cuda.Event(); ds.free.record(main)
            if last_pass_of[fi] == k:
                r["kept"] = fill[fi]
                r["batch_sum"] = ctx.pileup_batch_loss(r["loss"], B, n=r["kept"])

        for k in range(len(passes) + 1):
            if k < len(passes):
                issue(k)
            if k >= 1:
                score(k - 1)
    # everything of the run comes to the host here, once
    conf = counters.cpu().numpy()
    sites, total, head_sum = 0, 0.0, np.zeros(4)
    out_files = []
    for fi, f in enumerate(files):
        r = per_file[fi]
        kept = r["kept"] if r else 0
        if kept:
            bs = r["batch_sum"].cpu().numpy()                                  # float64 [batches, 4]: sums
            sizes = np.minimum(B, kept - B * np.arange(bs.shape[0])).astype(np.float64)
            total += float(((bs[:, 0] + bs[:, 1]) / sizes).sum())              # train.py:122: the batch's mean, batches restart per file
            head_sum += bs.sum(0)
            sites += kept
        if keep_sites:
            get = lambda key, dt, shape: r[key][:kept].cpu().numpy() if kept else np.zeros(shape, dt)
            out_files.append(dict(path=f["path"], rows=get("rows", np.int64, (0,)), cls=get("cls", np.uint8, (0, 4)),
                                  pred=get("pred", np.uint8, (0, 4)), site_loss=get("loss", np.float32, (0, 4))))
    div = max(sites, 1)
    res = {"sites": sites, "avg_loss": total / div, "mean_loss": float(head_sum[0] + head_sum[1]) / div, "malformed_labels": malformed}
    for h, (name, (_, c, o)) in enumerate(zip(HEAD_NAMES, ctx.EVAL_HEADS)):
        res[f"{name}_loss"] = float(head_sum[h]) / div
        res[f"{name}_confusion"] = conf[o:o + c * c].reshape(c, c).copy()
    res["gt_accuracy"] = float(np.trace(res["gt_confusion"])) / div
    res["zy_accuracy"] = float(np.trace(res["zy_confusion"])) / div
    if keep_sites:
        res["files"] = out_files
    return res


def format_report(result, epoch):
    """the line of train.py:147.  The reference prints torchmetrics' F1Score beside the accuracy: with its defaults that is the MICRO
    average, and micro-F1 of a single-label multi-class problem equals the accuracy (every false positive of one class is a false negative
    of another, so micro precision = micro recall = accuracy) - the accuracy is printed in both places."""
    return ('-Validating-Epoch:%d, | Zygosity Accuracy:%.5f F1-Score:%.5f | Genotype Accuracy:%.5f F1-Score:%.5f' %
            (epoch, result["zy_accuracy"], result["zy_accuracy"], result["gt_accuracy"], result["gt_accuracy"]))
