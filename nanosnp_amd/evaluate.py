"""Score a checkpoint on training window files (<chr>.td.bin): the reference's ``eval()`` (PileupModel/train.py:93-150) on the device.

``evaluate_train_bins`` reads the files pipeline.mpileup_to_train_bins / sitefile.td_to_bin write, keeps the variant sites as
``TrainDataset(for_evaluate=True)`` does (dataset.py:98-104), runs the forward with all four heads and the label-smoothed loss
(model.py:97-112, optim.py:137-144) and returns what eval() accumulates: the loss, the accuracies and the confusion matrices of genotype
and zygosity - plus those of the two indel heads, which eval() computes logits for and then ignores.  Training is nanosnp_amd.train's:
this is inference with labels attached.  The arithmetic is the ``precision`` argument (fp32, f16x3 or bf16x3); ``compare_precisions``
scores the same files under several and reports what differs.

``evaluate_haplotype_bins`` is the HaplotypeModel's counterpart, ``eval()`` of HaplotypeModel/evaluate_dev.py:16-86 over labelled haplotype
site files (sitefile.write_haplotype_train_bin), under every ``hap_precision``.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, hap_pipeline, host, sitefile

HEAD_NAMES = ("gt", "zy", "id1", "id2")


def _paths(paths, suffix):
    """a list of paths as given; a directory: its files whose names end with `suffix`, in os.listdir order; anything else: that one path"""
    if isinstance(paths, (str, os.PathLike)):
        d = str(paths)
        return [os.path.join(d, f) for f in os.listdir(d) if f.endswith(suffix)] if os.path.isdir(d) else [d]
    return [str(p) for p in paths]


def _open_window_files(paths):
    """the ``.td.bin`` files of a run, memory-mapped; every header is checked before anything runs"""
    files = []
    for p in paths:
        idx = sitefile.array_index(p)
        if ("position_matrix" not in idx or idx["position_matrix"][0] not in (np.dtype(np.int32), np.dtype(np.int16))
                or idx["position_matrix"][1][1:] != (33, 18)):
            raise sitefile.SiteFileError(f"{p}: not a window file (position_matrix int16 / int32 [N,33,18])")
        n = int(idx["position_matrix"][1][0])
        if "label" not in idx or idx["label"][0] != np.dtype(np.int32) or idx["label"][1] != (n, _lib.Context.LABEL_WIDTH):
            raise sitefile.SiteFileError(f"{p}: not a training window file (no label int32 [N,{_lib.Context.LABEL_WIDTH}] beside the windows)")
        a = sitefile.read_arrays(p, mmap=True)
        files.append(dict(path=p, n=n, x=a["position_matrix"], y=a["label"], elem=idx["position_matrix"][0].itemsize))
    return files


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


def evaluate_train_bins(model, validating_paths, batch_size=1000, variants_only=True, pass_sites=65536, keep_sites=False, stats=None,
                        precision=None):
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
        precision             with a `precision` argument: that argument, 0 / 1 / 2 or "context"

    precision: None scores in fp32 through the fp32-only entry (refused while the context's pileup_precision is 1 or 2); 0 (fp32), 1 (f16x3),
    2 (bf16x3) or "context" (the context's pileup_precision) name the arithmetic of the forward - an argument, no option is set.
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
    prec = ctx.eval_precision_arg(precision)              # (refused here, before anything is read; the calls below take the keyword itself)
    dev = torch.device("cuda", ctx.device)
    st = stats if stats is not None else {}
    for k in ("passes", "rows", "bytes_h2d"):
        st.setdefault(k, 0)
    files = _open_window_files(_paths(validating_paths, ".bin"))
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
                                        pred=r["pred"][o:o + kept], precision=precision)
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
    if prec is not None:
        res["precision"] = "context" if prec == -1 else prec
    return res


def precision_differences(base, other):
    """two evaluate_train_bins(keep_sites=True) results over the same files -> what differs between them:
        differing_sites       kept sites whose genotype, zygosity or either indel prediction differs
        max_site_loss_diff    the largest |site_loss| difference over sites and heads
        avg_loss_diff         other's avg_loss minus base's"""
    if len(base["files"]) != len(other["files"]):
        raise ValueError("results over different files")
    differing, worst = 0, 0.0
    for fb, fo in zip(base["files"], other["files"]):
        if fb["path"] != fo["path"] or not np.array_equal(fb["rows"], fo["rows"]):
            raise ValueError(f"results over different sites ({fb['path']}, {fo['path']})")
        differing += int((fb["pred"] != fo["pred"]).any(axis=1).sum())
        if fb["site_loss"].size:
            worst = max(worst, float(np.abs(fo["site_loss"].astype(np.float64) - fb["site_loss"].astype(np.float64)).max()))
    return {"differing_sites": differing, "max_site_loss_diff": worst, "avg_loss_diff": float(other["avg_loss"] - base["avg_loss"])}


def compare_precisions(model, validating_paths, precisions=(0, 2, 1), **kw):
    """what the arithmetic does to a checkpoint's calls on labelled data: one ``evaluate_train_bins(keep_sites=True, precision=p)`` per entry
    of `precisions` (each named once) -> {p: {"result": that result, **precision_differences(result of precisions[0], result)}}, in the order
    given.  Nothing is set on the context and so nothing is restored: the arithmetic is an argument."""
    kw = dict(kw, keep_sites=True)
    out, base = {}, None
    names = [None if p is None else _lib.Context.eval_precision_arg(p) for p in precisions]
    if None in names or len(set(names)) != len(names):
        raise ValueError('precisions: 0, 1, 2 or "context", each once')
    for p in precisions:
        res = evaluate_train_bins(model, validating_paths, precision=p, **kw)
        base = res if base is None else base
        out[res["precision"]] = dict(result=res, **precision_differences(base, res))
    return out


# ---- HaplotypeModel: HaplotypeModel/evaluate_dev.py:16-86 ----------------------------------------------------------------------------
class _HapPassSet:
    """buffers of one pass in flight: hap_pipeline's set of read planes and position arrays with the pass's label rows beside them"""
    def __init__(self, P, Dp, Dh, elem, dev=None):
        import torch
        self.planes = hap_pipeline._Set(P, Dp, Dh, elem, dev)
        kw = dict(pin_memory=True) if dev is None else dict(device=dev)
        self.y = torch.empty((P, sitefile.HAP_LABEL_WIDTH), dtype=torch.int32, **kw)
        if dev is None:
            self.meta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
            self.h2d_done = None
        else:
            self.cls = torch.empty((P, 2), dtype=torch.uint8, device=dev)
            self.rows = torch.empty(P, dtype=torch.int64, device=dev)
            self.xp = self.xh = None                                     # the features of every row of the pass, until it is scored
            self.free = None


def _macro_prf(cm):
    """evaluate_dev.py:67-79 on a confusion matrix [target][predicted] -> (recall, precision, f1), macro means with its 1e-6 terms"""
    cm = cm.astype(np.float64)
    tp = np.diag(cm)
    fp, fn = cm.sum(0) - tp, cm.sum(1) - tp
    recall, precision = tp / (tp + fn + 1e-6), tp / (tp + fp + 1e-6)
    f1 = 2 * (precision * recall) / (precision + recall + 1e-6)
    return float(recall.mean()), float(precision.mean()), float(f1.mean())


def _open_hap_files(paths, narrow):
    """the labelled haplotype bins of a run, open (the caller closes every f["src"]); every header is checked before anything runs.
    e_out: the bytes per plane element a pass is staged with - 1 (int8) under `narrow` until a value does not fit"""
    files = []
    try:
        for p in paths:
            src = hap_pipeline.HapBinSource(p)
            files.append(dict(path=p, src=src, n=src.n, e_out=1 if (narrow or src.elem == 1) else src.elem))
            y = src.idx.get("candidate_labels")
            if y is None or y[0] != np.dtype(np.int32) or y[1] != (src.n, sitefile.HAP_LABEL_WIDTH):
                raise sitefile.SiteFileError(f"{p}: not a labelled haplotype bin (no candidate_labels int32 [N,{sitefile.HAP_LABEL_WIDTH}] "
                                             "beside the read planes)")
            files[-1]["y"] = sitefile.read_arrays(p, mmap=True)["candidate_labels"]
    except BaseException:
        for f in files:
            f["src"].close()
        raise
    return files


def _fill_hap_pass(f, a, b, hs, reference):
    """rows [a, b) of file f into the pinned set hs: the eight planes, narrowed to int8 while that fits, the parsed positions (contigs the
    reference's table does not know yet are added to it) and the label rows; -> bytes of planes staged"""
    src, m, hp = f["src"], b - a, hs.planes
    while True:
        e_out, nbytes, overflow = f["e_out"], 0, False
        for name in hap_pipeline.PILEUP_PLANES + hap_pipeline.HAPLOTYPE_PLANES:
            cnt = m * (src.Dp * 33 if name.startswith("pileup") else src.Dh * 11)
            v = hp.planes[name].numpy()[:cnt * e_out].view(np.int8 if e_out == 1 else np.int32)
            if src.stage_plane(name, a, b, v):
                overflow = True                            # a value outside int8 (e.g. a mapping quality of 255)
                break
            nbytes += v.nbytes
        if not overflow:
            break
        f["e_out"] = src.elem                              # this pass again, and the rest of the file, as the file's own dtype
    cand_f, hap_f = src.position_fields(a, b)
    cand_f = cand_f.reshape(m, -1)
    cp, cc = host.parse_ctg_pos(cand_f, reference.table)
    if (cc < 0).any():
        reference.add_names([bytes(r).rstrip(b"\0").split(b":")[0].decode() for r in cand_f[cc < 0]])
        cp, cc = host.parse_ctg_pos(cand_f, reference.table)
    hpos, hctg = host.parse_ctg_pos(hap_f.reshape(m, 11, -1), reference.table)
    hp.cand_pos.numpy()[:m] = cp; hp.cand_ctg.numpy()[:m] = cc
    hp.hap_pos.numpy()[:m] = hpos; hp.hap_ctg.numpy()[:m] = hctg
    hs.y.numpy()[:m] = f["y"][a:b]
    return nbytes


def _send_hap_pass(f, m, hs, ds):
    """the m filled rows of the pinned set hs to the device set ds, on the current stream"""
    src, e_out, hp, dp = f["src"], f["e_out"], hs.planes, ds.planes
    for name in hap_pipeline.PILEUP_PLANES + hap_pipeline.HAPLOTYPE_PLANES:
        cnt = m * (src.Dp * 33 if name.startswith("pileup") else src.Dh * 11) * e_out
        dp.planes[name][:cnt].copy_(hp.planes[name][:cnt], non_blocking=True)
    dp.cand_pos[:m].copy_(hp.cand_pos[:m], non_blocking=True); dp.cand_ctg[:m].copy_(hp.cand_ctg[:m], non_blocking=True)
    dp.hap_pos[:m].copy_(hp.hap_pos[:m], non_blocking=True); dp.hap_ctg[:m].copy_(hp.hap_ctg[:m], non_blocking=True)
    ds.y[:m].copy_(hs.y[:m], non_blocking=True)


def _hap_pass_features(ctx, f, m, ds, hs, reference, off33):
    """every row of the pass on the device set ds reduced to features -> (xp, xh); its label pass into ds.cls, ds.rows and hs.meta"""
    import torch
    src, e_out, dp = f["src"], f["e_out"], ds.planes
    ref_p = reference.rows(dp.cand_ctg[:m, None].expand(m, 33), dp.cand_pos[:m, None] - 1 + off33)      # as stream_segments fetches them
    ref_h = reference.rows(dp.hap_ctg[:m], dp.hap_pos[:m] - 1)
    tdt = torch.int8 if e_out == 1 else torch.int32
    pl = lambda name, D, L: dp.planes[name][:m * D * L * e_out].view(tdt).view(m, D, L)
    xp = ctx.hap_features(*[pl(nm, src.Dp, 33) for nm in hap_pipeline.PILEUP_PLANES], ref_p)
    xh = ctx.hap_features(*[pl(nm, src.Dh, 11) for nm in hap_pipeline.HAPLOTYPE_PLANES], ref_h)
    ctx.hap_label_classes(ds.y[:m], cls=ds.cls, rows=ds.rows, meta=hs.meta)
    return xp, xh


def evaluate_haplotype_bins(model, bin_paths, reference, batch_size=512, pass_sites=16384, narrow=True, keep_sites=False, stats=None):
    """``eval(config, model, validating_data, references, batch_size)`` of HaplotypeModel/evaluate_dev.py:16-86 over labelled haplotype site
    files (sitefile.write_haplotype_train_bin) -> dict

        sites, refcalls, variants   the rows LabelField keeps (dataset_dev.py:174-187) and the loaded heads can score, and their two kinds
        unscorable_labels     rows the filter keeps whose gt21 / zygosity the loaded heads have no class for (the reference's loss would fail)
        gt_confusion [n_gt,n_gt], zy_confusion [n_zy,n_zy]     int64 [target][predicted], torchnet's ConfusionMeter orientation (:52)
        gt_accuracy           100 * trace / sum - a PERCENTAGE (:63, quirk kept); zy_accuracy likewise
        gt_recall, gt_precision, gt_f1         macro means with the 1e-6 terms of :74-79; zy_recall, zy_precision, zy_f1 likewise (eval()
                              computes the zygosity logits and then ignores them)
        batch_accuracy        :50,81 - the mean over batches of each batch's genotype accuracy, a FRACTION
        loss                  :65-66, quirk kept - the sum over ALL files of each batch's mean of gt + zy, divided by the number of batches of
                              the LAST file that had a batch (NaN when no file had one)
        mean_loss, gt_loss, zy_loss            per-site means
        files                 with keep_sites: per file {path, rows int64 [k] (file rows, ascending), cls uint8 [k,2], pred uint8 [k,2],
                              site_loss fp32 [k,2]}

    model: a loaded haplotype_model.LSTMNetwork (its context's hap_precision selects the arithmetic); bin_paths: a list of paths or a
    directory (its files in os.listdir order, :24); reference: a hap_pipeline.DeviceReference.  Batches restart with every file.  The kept
    rows are scored in file order: the reference's order - refcalls, variants, then an unseeded shuffle - is random, and only `loss` and
    `batch_accuracy` depend on it (through which sites share a batch).
    Host loop: a file is read in passes of `pass_sites` rows through three pinned sets (HapBinSource.stage_plane, on the calling thread),
    sent on the package's copy stream with the label rows beside them; reference rows, the two feature reductions over ALL rows of the pass
    and the label pass (nsnp_hap_label_classes) of pass k + 1 are issued before the host reads the kept count of pass k from pinned
    memory, so the one host wait per pass is for work issued a pass earlier; then the kept rows' features are gathered (torch.index_select)
    and scored (nsnp_hap_eval).  Losses, predictions, classes and rows stay on the device until the run ends."""
    import torch
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("evaluate_haplotype_bins under a process group of more than one rank (validation is not sharded)")
    if not getattr(model, "_loaded", False):
        raise _lib.NanoSNPError("weights not loaded")
    if not isinstance(reference, hap_pipeline.DeviceReference):
        raise TypeError("reference: a hap_pipeline.DeviceReference")
    B = int(batch_size)
    if B < 1:
        raise ValueError("batch_size >= 1")
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    n_gt, n_zy = model.dims["gt_num_class"], model.dims["zy_num_class"]
    st = stats if stats is not None else {}
    for k in ("passes", "rows", "bytes_h2d", "passes_int8"):
        st.setdefault(k, 0)
    files = _open_hap_files(_paths(bin_paths, ""), narrow)                 # (a directory: every file of it)
    try:
        return _evaluate_haplotype(model, ctx, dev, files, reference, B, int(max(1, pass_sites)), keep_sites, st, n_gt, n_zy)
    finally:
        for f in files:
            f["src"].close()


def _evaluate_haplotype(model, ctx, dev, files, reference, B, P, keep_sites, st, n_gt, n_zy):
    import torch
    passes = [(fi, a, min(f["n"], a + P)) for fi, f in enumerate(files) for a in range(0, f["n"], P)]
    last_pass_of = {fi: k for k, (fi, _, _) in enumerate(passes)}
    counters = ctx.hap_eval_counters(dev)
    per_file = [None] * len(files)
    totals = np.zeros(4, np.int64)                         # kept, unscorable, refcalls, variants
    if passes:
        Pmax = max(b - a for _, a, b in passes)
        Dp, Dh = max(f["src"].Dp for f in files if f["n"]), max(f["src"].Dh for f in files if f["n"])
        elem = max(f["src"].elem for f in files if f["n"])                 # (an int32 file may turn out not to fit int8: room for its own dtype)
        sets = getattr(model, "_eval_sets", None)
        if not sets or not all(s_.planes.fits(Pmax, Dp, Dh, elem) for s_ in sets[0] + sets[1]):
            sets = model._eval_sets = ([_HapPassSet(Pmax, Dp, Dh, elem) for _ in range(3)], [_HapPassSet(Pmax, Dp, Dh, elem, dev) for _ in range(3)])
        hsets, dsets = sets
        copy_stream = host.copy_stream(dev)
        main = torch.cuda.current_stream(dev)
        for s_ in hsets:
            s_.h2d_done = None
        for s_ in dsets:
            s_.free = None
            s_.xp = s_.xh = None
        copy_stream.wait_stream(main)
        labelled = [None] * len(passes)                    # the event behind the label pass of pass k (blocking: the host sleeps on it)
        fill = {}                                          # file -> kept sites so far
        off33 = torch.arange(-16, 17, dtype=torch.int64, device=dev)[None, :]

        def issue(k):
            """stage pass k, send it, reduce every row to features, run its label pass"""
            fi, a, b = passes[k]
            f, m = files[fi], b - a
            hs, ds = hsets[k % 3], dsets[k % 3]
            if hs.h2d_done is not None:
                hs.h2d_done.synchronize()                  # (pass k - 3 has left this pinned set)
            nbytes = _fill_hap_pass(f, a, b, hs, reference)
            if ds.free is not None:
                copy_stream.wait_event(ds.free)            # (pass k - 3 has been scored out of this device set)
            with torch.cuda.stream(copy_stream):
                _send_hap_pass(f, m, hs, ds)
                hs.h2d_done = torch.cuda.Event(blocking=True); hs.h2d_done.record(copy_stream)
            main.wait_event(hs.h2d_done)
            ds.xp, ds.xh = _hap_pass_features(ctx, f, m, ds, hs, reference, off33)
            labelled[k] = torch.cuda.Event(blocking=True); labelled[k].record(main)
            st["passes"] += 1; st["rows"] += m; st["bytes_h2d"] += nbytes + m * (12 * 12 + 12); st["passes_int8"] += int(f["e_out"] == 1)

        def score(k):
            """the kept sites of pass k (its count is on the host by now) through forward, loss and counts"""
            fi, a, b = passes[k]
            f, m = files[fi], b - a
            hs, ds = hsets[k % 3], dsets[k % 3]
            labelled[k].synchronize()
            meta = hs.meta.numpy().copy()
            kept = int(meta[0])
            totals[:] += meta
            if per_file[fi] is None:
                mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
                per_file[fi] = dict(loss=mk((f["n"], 2), torch.float32), pred=mk((f["n"], 2), torch.uint8), cls=mk((f["n"], 2), torch.uint8),
                                    rows=mk(f["n"], torch.int64))
                fill[fi] = 0
            o, r = fill[fi], per_file[fi]
            if kept:
                xp, xh = ds.xp, ds.xh
                if kept < m:                               # (plumbing: the kept rows' features, in order)
                    xp, xh = torch.index_select(xp, 0, ds.rows[:kept]), torch.index_select(xh, 0, ds.rows[:kept])
                ctx.hap_eval(xp, xh, ds.cls, counters, n=kept, site_loss=r["loss"][o:o + kept], pred=r["pred"][o:o + kept])
                r["cls"][o:o + kept].copy_(ds.cls[:kept])
                r["rows"][o:o + kept].copy_(ds.rows[:kept] + a)
            fill[fi] = o + kept
            ds.xp = ds.xh = None
            ds.free = torch.cuda.Event(); ds.free.record(main)
            if last_pass_of[fi] == k:
                n_k = r["kept"] = fill[fi]
                r["batch_sum"] = ctx.hap_batch_loss(r["loss"], B, n=n_k)
                nb = -(-n_k // B)
                hit = torch.zeros(nb * B, dtype=torch.int64, device=dev)
                hit[:n_k] = (r["pred"][:n_k, 0] == r["cls"][:n_k, 0]).to(torch.int64)
                r["batch_hits"] = hit.view(nb, B).sum(1)                     # correct genotype calls per batch: integers

        for k in range(len(passes) + 1):
            if k < len(passes):
                issue(k)
            if k >= 1:
                score(k - 1)
    # everything of the run comes to the host here, once
    conf = counters.cpu().numpy()
    sites, total, head_sum, acc_sum, n_batches, last_batches = 0, 0.0, np.zeros(2), 0.0, 0, 0
    out_files = []
    for fi, f in enumerate(files):
        r = per_file[fi]
        kept = r["kept"] if r else 0
        if kept:
            bs = r["batch_sum"].cpu().numpy()                                  # float64 [batches, 2]: sums
            sizes = np.minimum(B, kept - B * np.arange(bs.shape[0])).astype(np.float64)
            total += float(((bs[:, 0] + bs[:, 1]) / sizes).sum())              # model_dev.py:128-130: the two means of a batch
            acc_sum += float((r["batch_hits"].cpu().numpy() / sizes).sum())    # evaluate_dev.py:50
            n_batches += bs.shape[0]
            last_batches = bs.shape[0]                                         # :66: step + 1 of the last file that had a batch
            head_sum += bs.sum(0)
            sites += kept
        if keep_sites:
            get = lambda key, dt, shape: r[key][:kept].cpu().numpy() if kept else np.zeros(shape, dt)
            out_files.append(dict(path=f["path"], rows=get("rows", np.int64, (0,)), cls=get("cls", np.uint8, (0, 2)),
                                  pred=get("pred", np.uint8, (0, 2)), site_loss=get("loss", np.float32, (0, 2))))
    div = max(sites, 1)
    nan = float("nan")
    res = {"sites": sites, "refcalls": int(totals[2]), "variants": int(totals[3]), "unscorable_labels": int(totals[1]),
           "loss": total / last_batches if last_batches else nan, "batch_accuracy": acc_sum / n_batches if n_batches else nan,
           "mean_loss": float(head_sum[0] + head_sum[1]) / div, "gt_loss": float(head_sum[0]) / div, "zy_loss": float(head_sum[1]) / div}
    for name, c, o in (("gt", n_gt, 0), ("zy", n_zy, n_gt * n_gt)):
        cm = conf[o:o + c * c].reshape(c, c).copy()
        res[f"{name}_confusion"] = cm
        res[f"{name}_accuracy"] = 100.0 * float(np.trace(cm)) / (float(cm.sum()) if cm.sum() > 0 else 1.0)       # :58-63
        res[f"{name}_recall"], res[f"{name}_precision"], res[f"{name}_f1"] = _macro_prf(cm)
    if keep_sites:
        res["files"] = out_files
    return res


def format_haplotype_report(result):
    """the line of evaluate_dev.py:81"""
    return ("AverageLoss: %.5f, GT:|Recall: %.4f, Precision: %.4f, F1: %.4f |, ACC: %.4f" %
            (result["loss"], result["gt_recall"], result["gt_precision"], result["gt_f1"], result["batch_accuracy"]))


def format_report(result, epoch):
    """the line of train.py:147.  The reference prints torchmetrics' F1Score beside the accuracy: with its defaults that is the MICRO
    average, and micro-F1 of a single-label multi-class problem equals the accuracy (every false positive of one class is a false negative
    of another, so micro precision = micro recall = accuracy) - the accuracy is printed in both places."""
    return ('-Validating-Epoch:%d, | Zygosity Accuracy:%.5f F1-Score:%.5f | Genotype Accuracy:%.5f F1-Score:%.5f' %
            (epoch, result["zy_accuracy"], result["zy_accuracy"], result["gt_accuracy"], result["gt_accuracy"]))
