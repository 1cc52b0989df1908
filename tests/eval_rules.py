"""The scoring rules of the reference's eval() (PileupModel/train.py:93-150), restated in numpy for the tests of nanosnp_amd.evaluate and of
the C-ABI entries under it.  Test infrastructure: float64 everywhere, written from the published equations -

    LSTMNetwork.forward        PileupModel/model.py:97-112 (BaseEncoder.forward 31-39, ForwardLayer.forward 66-73)
    LabelSmoothingLoss         PileupModel/optim.py:137-144
    TrainDataset               PileupModel/dataset.py:78-82 (the label decode), 98-104 (for_evaluate: variant sites only)
    eval()                     train.py:103-136: a DataLoader per file, so batches restart with every file; total_loss adds the MEAN of each
                               batch, and is then divided by the number of sites (the quirk avg_loss keeps)

The forward restates the equations of oracle.pileup_forward_f64 up to the heads and returns all 90 logits instead of two softmaxes."""
from __future__ import annotations

import numpy as np

# (first head row, classes, first counter) of genotype, zygosity, indel1, indel2: the label row of a .td.bin and the rows of the logits
HEADS = ((0, 21, 0), (21, 3, 441), (24, 33, 450), (57, 33, 1539))
NAMES = ("gt", "zy", "id1", "id2")
N_COUNTERS = 2628
SMOOTHING = 0.1


def forward_logits_f64(weights, indel, x):
    """weights: the 24 tensors of nsnp_pileup_load_weights; indel: indel1 weight / bias, indel2 weight / bias; x [N,33,18] -> float64 [N,90]"""
    w = [np.asarray(t, np.float64) for t in weights]
    x = np.asarray(x, np.float64)
    N, T, H = x.shape[0], 33, 64
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))

    def layer(inp, base):
        out = np.zeros((N, T, 2 * H))
        for d in range(2):
            wih, whh, b = w[base + 4 * d], w[base + 4 * d + 1], w[base + 4 * d + 2] + w[base + 4 * d + 3]
            h = np.zeros((N, H)); c = np.zeros((N, H))
            for s in range(T):
                t = T - 1 - s if d else s
                g = inp[:, t] @ wih.T + h @ whh.T + b
                i, f, gg, o = sig(g[:, :H]), sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sig(g[:, 3 * H:])
                c = f * c + i * gg
                h = o * np.tanh(c)
                out[:, t, d * H:(d + 1) * H] = h
        return out

    h1 = layer(layer(x, 0), 8)
    enc = h1[:, 16] @ w[16].T + w[17]
    mid = np.tanh(enc @ w[18].T + w[19])
    i1w, i1b, i2w, i2b = (np.asarray(t, np.float64) for t in indel)
    return np.concatenate([mid @ w[20].T + w[21], mid @ w[22].T + w[23], mid @ i1w.T + i1b, mid @ i2w.T + i2b], axis=1)


def decode_labels(label):
    """label int [N,90] -> (cls uint8 [N,4], malformed bool [N]): per family np.argmax of its slice (first maximum; an all-zero slice gives
    0); a row is malformed when some family is not exactly one 1 among zeros"""
    y = np.asarray(label)
    cls = np.zeros((y.shape[0], 4), np.uint8)
    bad = np.zeros(y.shape[0], bool)
    for h, (r0, c, _) in enumerate(HEADS):
        s = y[:, r0:r0 + c]
        cls[:, h] = s.argmax(1)
        bad |= ((s == 1).sum(1) != 1) | ((s != 0).sum(1) != 1)
    return cls, bad


def keep_rows(cls, variants_only=True):
    """the rows TrainDataset(for_evaluate=True) keeps: zygosity class > 0 (dataset.py:99)"""
    return np.flatnonzero(cls[:, 1] > 0) if variants_only else np.arange(cls.shape[0])


def label_classes(label, variants_only=True):
    """what nsnp_pileup_label_classes writes: (cls of the kept rows, their centres 33 n + 16, meta)"""
    cls, bad = decode_labels(label)
    k = keep_rows(cls, variants_only)
    return cls[k], 33 * k.astype(np.int64) + 16, np.array([k.size, int(bad.sum()), 0, 0], np.int64)


def smoothed_loss(logits, cls):
    """float64 [N,4]: per head -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t])), lp = log_softmax of the head's logits"""
    z = np.asarray(logits, np.float64)
    out = np.zeros((z.shape[0], 4))
    rows = np.arange(z.shape[0])
    for h, (r0, c, _) in enumerate(HEADS):
        s = z[:, r0:r0 + c]
        m = s.max(1, keepdims=True)
        lp = s - (m + np.log(np.exp(s - m).sum(1, keepdims=True)))
        lpt = lp[rows, cls[:, h]]
        out[:, h] = -((1.0 - SMOOTHING) * lpt + SMOOTHING / (c - 1) * (lp.sum(1) - lpt))
    return out


def predictions(logits):
    z = np.asarray(logits)
    return np.stack([z[:, r0:r0 + c].argmax(1) for r0, c, _ in HEADS], axis=1).astype(np.uint8)


def confusion(cls, pred):
    """int64 [2628]: the four matrices [target][predicted], back to back"""
    out = np.zeros(N_COUNTERS, np.int64)
    for h, (_, c, o) in enumerate(HEADS):
        np.add.at(out, o + cls[:, h].astype(np.int64) * c + pred[:, h], 1)
    return out


def batch_means(site_loss, batch_size):
    """float64 [ceil(N / B), 4]: the mean of every batch of one file (the last batch may be short)"""
    n = site_loss.shape[0]
    return np.array([site_loss[a:a + batch_size].mean(0) for a in range(0, n, batch_size)]).reshape(-1, 4)


def result_from(files, batch_size, malformed=0):
    """files: per file (site_loss [n,4], cls [n,4], pred [n,4]) of its kept rows -> the dict of evaluate_train_bins (without keep_sites)"""
    sites = sum(f[0].shape[0] for f in files)
    total, per_batch = 0.0, []
    for loss, _, _ in files:
        bm = batch_means(np.asarray(loss, np.float64), batch_size)
        per_batch.append(bm)
        total += float((bm[:, 0] + bm[:, 1]).sum())                    # train.py:122: loss.item() of gt + zy, the batch's MEAN
    loss = np.concatenate([np.asarray(f[0], np.float64) for f in files]) if files else np.zeros((0, 4))
    cls = np.concatenate([f[1] for f in files]) if files else np.zeros((0, 4), np.uint8)
    pred = np.concatenate([f[2] for f in files]) if files else np.zeros((0, 4), np.uint8)
    conf = confusion(cls, pred)
    div = max(sites, 1)
    res = {"sites": sites, "avg_loss": total / div, "mean_loss": float((loss[:, 0] + loss[:, 1]).sum()) / div, "malformed_labels": int(malformed),
           "batch_means": per_batch}
    for h, (name, (_, c, o)) in enumerate(zip(NAMES, HEADS)):
        res[f"{name}_loss"] = float(loss[:, h].sum()) / div
        res[f"{name}_confusion"] = conf[o:o + c * c].reshape(c, c)
    res["gt_accuracy"] = float((cls[:, 0] == pred[:, 0]).sum()) / div
    res["zy_accuracy"] = float((cls[:, 1] == pred[:, 1]).sum()) / div
    return res


SYNTH_SEED, SYNTH_MAX = 20261020, 16384


def fixture_rows(case, workdir):
    """tests/golden/<case>.td.gz through sitefile.td_to_bin -> (path of the .td.bin, windows int32 [N,33,18], label int32 [N,90])"""
    import gzip
    import os
    from nanosnp_amd import sitefile
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    path = os.path.join(workdir, f"{case}.td.bin")
    sitefile.td_to_bin(gzip.open(os.path.join(here, f"{case}.td.gz")).read(), path)
    a = sitefile.read_train_bin(path, mmap=False)
    return path, np.ascontiguousarray(a[3], np.int32), np.ascontiguousarray(a[4], np.int32)


def synthetic_windows(base, n):
    """n <= SYNTH_MAX seeded windows with random classes: rows of `base` (the windows of train_cut) drawn with replacement, one entry in ten
    moved by -2..2.  The first n rows of the SYNTH_MAX the fixture maker measured (pileup_eval.npz: synth_dist_f64) -> (x int32, cls uint8)"""
    assert n <= SYNTH_MAX
    rng = np.random.default_rng(SYNTH_SEED)
    x = base[rng.integers(0, base.shape[0], SYNTH_MAX)].astype(np.int32)
    x += (rng.integers(-2, 3, x.shape) * (rng.random(x.shape) < 0.1)).astype(np.int32)
    cls = np.stack([rng.integers(0, c, SYNTH_MAX) for _, c, _ in HEADS], axis=1).astype(np.uint8)
    return np.ascontiguousarray(x[:n]), np.ascontiguousarray(cls[:n])


def evaluate(weights, indel, files, batch_size=1000, variants_only=True):
    """files: [(x [N,33,18], label [N,90])] -> result_from of the float64 forward"""
    parts, malformed = [], 0
    for x, label in files:
        cls, bad = decode_labels(label)
        malformed += int(bad.sum())
        k = keep_rows(cls, variants_only)
        z = forward_logits_f64(weights, indel, np.asarray(x)[k]) if k.size else np.zeros((0, 90))
        parts.append((smoothed_loss(z, cls[k]), cls[k], predictions(z)))
    return result_from(parts, batch_size, malformed)
