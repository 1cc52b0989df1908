"""The rules of scoring a HaplotypeModel checkpoint on labelled haplotype site files, restated in float64 numpy: what the reference's
HaplotypeModel/evaluate_dev.py:16-86 computes with dataset_dev.LabelField / EvaluateDataset (:174-187,285-321), model_dev.LSTMNetwork.forward
(:120-131) and optim.LabelSmoothingLoss(C, 0.1).  Test infrastructure only: the product never imports it.

    label_filter        LabelField + the target rule of EvaluateDataset.__getitem__, in file order
    forward_logits_f64  the two 3-layer BiLSTM encoders, output_proj at the centre step, tanh(dense), the two heads: 58 tensors -> logits
    smoothed_loss, predictions, confusion
    result_from         every metric of eval() with its quirks, from per-file (site_loss, cls, pred)
"""
from __future__ import annotations

import numpy as np

MARGIN = 2e-4              # a float64 top-two margin under this may flip an fp32 argmax: such sites are excluded from argmax equality
MARGIN_SHARE = 0.01        # ... and at most this share of the sites may be


def label_filter(labels, n_gt=10, n_zy=3):
    """candidate_labels int [N,3] = {confident, gt21, zygosity} -> (rows int64 [k] ascending, cls uint8 [k,2], meta int64 [4]).
    dataset_dev.py:180: valid = cf == 1 and -1 <= zy < 10; :185 refcalls: zy == -1 and gt < 10; :187 variants: zy > 0 and gt < 10 (zy == 0 is
    valid and in neither list: dropped); :320 the zygosity target is max(zy, 0).  Kept rows whose classes the heads do not have (the
    reference's scatter_ fails on them) are counted in meta[1] and dropped.  meta = {kept, unscorable, refcalls kept, variants kept}."""
    y = np.asarray(labels).astype(np.int64).reshape(-1, 3)
    cf, gt, zy = y[:, 0], y[:, 1], y[:, 2]
    valid = (cf == 1) & (zy >= -1) & (zy < 10)
    refcall = valid & (zy == -1) & (gt < 10)
    variant = valid & (zy > 0) & (gt < 10)
    scorable = (gt >= 0) & (gt < n_gt) & (zy < n_zy)
    keep = (refcall | variant) & scorable
    rows = np.flatnonzero(keep)
    cls = np.stack([gt[rows], np.maximum(zy[rows], 0)], axis=1).astype(np.uint8)
    meta = np.array([rows.size, int(((refcall | variant) & ~scorable).sum()), int((refcall & scorable).sum()), int((variant & scorable).sum())],
                    np.int64)
    return rows, cls, meta


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse, steps):
    """x float64 [N,L,I] -> h of the first `steps` steps of this direction, at their positions: float64 [N,L,H] (zeros elsewhere);
    torch.nn.LSTM's gate order i, f, g, o"""
    N, L, _ = x.shape
    H = w_hh.shape[1]
    h, c = np.zeros((N, H)), np.zeros((N, H))
    out = np.zeros((N, L, H))
    b = b_ih + b_hh
    for s in range(steps):
        t = L - 1 - s if reverse else s
        g = x[:, t] @ w_ih.T + h @ w_hh.T + b
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[:, t] = h
    return out


def _encoder_centre(ws, x, n_layers=3):
    """ws: the 26 tensors of one BaseEncoder; x float64 [N,L,F] -> output_proj of the last layer at step L // 2: [N,H]"""
    L = x.shape[1]
    for l in range(n_layers):
        q = ws[l * 8:(l + 1) * 8]
        last = l == n_layers - 1
        fwd = _lstm_direction(x, *q[0:4], reverse=False, steps=L // 2 + 1 if last else L)
        bwd = _lstm_direction(x, *q[4:8], reverse=True, steps=L - L // 2 if last else L)
        x = np.concatenate([fwd, bwd], axis=2)
    return x[:, L // 2] @ ws[-2].T + ws[-1]


def forward_logits_f64(weights, xp, xh, n_layers=3):
    """weights: the 58 tensors in state-dict order (haplotype_model.state_dict_keys); xp [N,F,33], xh [N,F,11] -> float64 [N, n_gt + n_zy],
    genotype rows first (model_dev.py:123-127, ForwardLayer :96-105)"""
    w = [np.asarray(t, np.float64) for t in weights]
    per = n_layers * 8 + 2
    ep = _encoder_centre(w[:per], np.asarray(xp, np.float64).transpose(0, 2, 1), n_layers)
    eh = _encoder_centre(w[per:2 * per], np.asarray(xh, np.float64).transpose(0, 2, 1), n_layers)
    f = w[2 * per:]
    inner = np.tanh(np.concatenate([ep, eh], axis=1) @ f[0].T + f[1])
    return np.concatenate([inner @ f[2].T + f[3], inner @ f[4].T + f[5]], axis=1)


def heads_of(n_gt, n_zy):
    return ((0, n_gt), (n_gt, n_zy))              # (first logit row, classes)


def smoothed_loss(z, cls, n_gt, smoothing=0.1):
    """LabelSmoothingLoss(C, 0.1) on single rows: -sum(true_dist * log_softmax(z)), true_dist = 0.1 / (C - 1) everywhere, 0.9 at the target
    -> float64 [N,2].  A head of one class has loss 0 (the guard of the device entry; the reference divides by zero there)."""
    z = np.asarray(z, np.float64)
    cls = np.asarray(cls).astype(np.int64)
    out = np.zeros((z.shape[0], 2))
    for h, (r0, C) in enumerate(heads_of(n_gt, z.shape[1] - n_gt)):
        if C == 1:
            continue
        zz = z[:, r0:r0 + C]
        m = zz.max(1, keepdims=True)
        lp = zz - (m + np.log(np.exp(zz - m).sum(1, keepdims=True)))
        t = np.minimum(cls[:, h], C - 1)
        lpt = lp[np.arange(z.shape[0]), t]
        out[:, h] = -((1.0 - smoothing) * lpt + smoothing / (C - 1) * (lp.sum(1) - lpt))
    return out


def predictions(z, n_gt):
    """first maximum per head -> uint8 [N,2]"""
    z = np.asarray(z)
    return np.stack([z[:, r0:r0 + C].argmax(1) for r0, C in heads_of(n_gt, z.shape[1] - n_gt)], axis=1).astype(np.uint8)


def margins(z, n_gt):
    """top-two margin per head (inf for a head of one class) -> float64 [N,2]"""
    z = np.asarray(z, np.float64)
    out = np.full((z.shape[0], 2), np.inf)
    for h, (r0, C) in enumerate(heads_of(n_gt, z.shape[1] - n_gt)):
        if C > 1:
            s = np.sort(z[:, r0:r0 + C], axis=1)
            out[:, h] = s[:, -1] - s[:, -2]
    return out


def confusion(cls, pred, n_gt, n_zy):
    """-> (gt int64 [n_gt,n_gt], zy int64 [n_zy,n_zy]), [target][predicted]; a target outside its head counts as the last class"""
    out = []
    for h, C in enumerate((n_gt, n_zy)):
        m = np.zeros((C, C), np.int64)
        np.add.at(m, (np.minimum(np.asarray(cls)[:, h].astype(np.int64), C - 1), np.asarray(pred)[:, h].astype(np.int64)), 1)
        out.append(m)
    return out


def macro_prf(cm):
    """evaluate_dev.py:67-79"""
    cm = np.asarray(cm, np.float64)
    C = cm.shape[0]
    tp, fp, fn = np.zeros(C), np.zeros(C), np.zeros(C)
    for x in range(C):
        tp[x] += cm[x][x]
        fp[x] += cm[:, x].sum() - cm[x][x]
        fn[x] += cm[x, :].sum() - cm[x][x]
    recall = tp / (tp + fn + 1e-6)
    precision = tp / (tp + fp + 1e-6)
    f1 = 2 * (precision * recall) / (precision + recall + 1e-6)
    return float(recall.mean()), float(precision.mean()), float(f1.mean())


def result_from(parts, batch_size, n_gt, n_zy):
    """parts: per file (site_loss float [k,2], cls [k,2], pred [k,2]) of its kept rows in scoring order -> the metrics of eval().
    loss (:65-66): total_loss sums every batch's mean(gt) + mean(zy) over ALL files, avg_loss = total_loss / (step + 1) with `step` the
    index of the last batch of the LAST file that had one.  batch_accuracy (:50,81): the mean over batches of the batch's genotype accuracy.
    gt_accuracy (:58-63): a percentage of the confusion matrix."""
    B = int(batch_size)
    total_loss, total_acc, total_cnt, step, sites, head_sum = 0.0, 0.0, 0, None, 0, np.zeros(2)
    for loss, cls, pred in parts:
        loss = np.asarray(loss, np.float64)
        for s, a in enumerate(range(0, loss.shape[0], B)):
            l, c, p = loss[a:a + B], np.asarray(cls)[a:a + B], np.asarray(pred)[a:a + B]
            total_loss += float(l[:, 0].mean() + l[:, 1].mean())
            total_acc += float((p[:, 0] == c[:, 0]).astype(int).sum()) / len(p)
            total_cnt += 1
            step = s
        sites += loss.shape[0]
        head_sum += loss.sum(0)
    cls_all = np.concatenate([np.asarray(p[1]).reshape(-1, 2) for p in parts]) if parts else np.zeros((0, 2), np.uint8)
    pred_all = np.concatenate([np.asarray(p[2]).reshape(-1, 2) for p in parts]) if parts else np.zeros((0, 2), np.uint8)
    gcm, zcm = confusion(cls_all, pred_all, n_gt, n_zy)
    div = max(sites, 1)
    res = {"sites": sites, "loss": total_loss / (step + 1) if step is not None else float("nan"),
           "batch_accuracy": total_acc / total_cnt if total_cnt else float("nan"),
           "mean_loss": float(head_sum.sum()) / div, "gt_loss": float(head_sum[0]) / div, "zy_loss": float(head_sum[1]) / div}
    for name, cm in (("gt", gcm), ("zy", zcm)):
        denom = cm.sum() if cm.sum() > 0 else 1.0
        res[f"{name}_confusion"] = cm
        res[f"{name}_accuracy"] = 100.0 * float(np.trace(cm)) / float(denom)
        res[f"{name}_recall"], res[f"{name}_precision"], res[f"{name}_f1"] = macro_prf(cm)
    return res


def evaluate(weights, files, batch_size, n_gt=10, n_zy=3):
    """files: per file (xp [N,F,33], xh [N,F,11], candidate_labels [N,3]) -> result_from over the float64 forward, plus the label counts and
    per file (rows, cls, logits) for margin rules"""
    parts, detail, meta_sum = [], [], np.zeros(4, np.int64)
    for xp, xh, y in files:
        rows, cls, meta = label_filter(y, n_gt, n_zy)
        meta_sum += meta
        z = forward_logits_f64(weights, np.asarray(xp)[rows], np.asarray(xh)[rows]) if rows.size else np.zeros((0, n_gt + n_zy))
        parts.append((smoothed_loss(z, cls, n_gt), cls, predictions(z, n_gt)))
        detail.append((rows, cls, z))
    res = result_from(parts, batch_size, n_gt, n_zy)
    res.update({"refcalls": int(meta_sum[2]), "variants": int(meta_sum[3]), "unscorable_labels": int(meta_sum[1]), "detail": detail, "parts": parts})
    return res
