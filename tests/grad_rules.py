"""The loss gradients of the reference's training step (PileupModel/train.py:56-59: loss, ... = model(...); loss.backward()), restated in
float64 torch for the tests of nsnp_pileup_loss_grad and of nanosnp_amd.train.  Test infrastructure, written from the published equations -

    LSTMNetwork.forward        PileupModel/model.py:97-112 (BaseEncoder.forward 31-39, ForwardLayer.forward 66-73); loss = gt_loss + zy_loss
    nn.LSTM(dropout=p)         between the two layers, in train() mode: h0 * mask / (1 - p) - here an EXPLICIT keep mask and scale
    LabelSmoothingLoss         PileupModel/optim.py:137-144: mean over the batch of -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t]))

The forward is that of eval_rules.forward_logits_f64 (same gate order, same direction walk, every one of the 33 positions in both layers),
built from float64 torch tensors with requires_grad; autograd gives the 24 gradients.  The indel heads are not in the loss and get none."""
from __future__ import annotations

import numpy as np
import torch

HEADS = ((0, 21), (21, 3))             # (first logit, classes) of genotype and zygosity
SMOOTHING = 0.1
SHAPES = ([(256, 18), (256, 64), (256,), (256,)] * 2 + [(256, 128), (256, 64), (256,), (256,)] * 2 +
          [(128, 128), (128,), (256, 128), (256,), (21, 256), (21,), (3, 256), (3,)])
BIAS_PAIRS = ((2, 3), (6, 7), (10, 11), (14, 15))
assert sum(int(np.prod(s)) for s in SHAPES) == 198040


def _layer(inp, w, base):
    n, T, H = inp.shape[0], 33, 64
    outs = []
    for d in range(2):
        wih, whh, b = w[base + 4 * d], w[base + 4 * d + 1], w[base + 4 * d + 2] + w[base + 4 * d + 3]
        h = torch.zeros((n, H), dtype=inp.dtype)
        c = torch.zeros((n, H), dtype=inp.dtype)
        hs = [None] * T
        for s in range(T):
            t = T - 1 - s if d else s
            g = inp[:, t] @ wih.T + h @ whh.T + b
            i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            hs[t] = h
        outs.append(torch.stack(hs, dim=1))
    return torch.cat(outs, dim=2)


def forward(w, x, cls, keep_mask=None, keep_scale=1.0, dtype=torch.float64):
    """w: 24 tensors of `dtype`; x [N,33,18]; cls integer [N, >= 2] -> (loss scalar tensor, site_loss [N,2] tensor, logits [N,24] tensor).
    A class outside its head counts as the head's last class.  dtype torch.float32: the same restatement in fp32 torch on the CPU, the
    yardstick of what fp32 arithmetic costs on an input the fixture did not measure."""
    x = torch.as_tensor(np.asarray(x, np.float64)).to(dtype)
    h0 = _layer(x, w, 0)
    if keep_mask is not None:
        h0 = h0 * torch.as_tensor(np.asarray(keep_mask, np.float64)).to(dtype) * float(keep_scale)
    h1 = _layer(h0, w, 8)
    enc = h1[:, 16] @ w[16].T + w[17]
    mid = torch.tanh(enc @ w[18].T + w[19])
    z = torch.cat([mid @ w[20].T + w[21], mid @ w[22].T + w[23]], dim=1)
    cls = np.asarray(cls)
    rows = torch.arange(z.shape[0])
    site = []
    for h, (r0, c) in enumerate(HEADS):
        lp = torch.log_softmax(z[:, r0:r0 + c], dim=1)
        t = torch.as_tensor(np.minimum(cls[:, h].astype(np.int64), c - 1))
        lpt = lp[rows, t]
        site.append(-((1.0 - SMOOTHING) * lpt + SMOOTHING / (c - 1) * (lp.sum(1) - lpt)))
    site = torch.stack(site, dim=1)
    return site[:, 0].mean() + site[:, 1].mean(), site, z


def tensors(weights, requires_grad=True, dtype=torch.float64):
    return [torch.tensor(np.asarray(t, np.float64), dtype=dtype, requires_grad=requires_grad) for t in weights]


def loss_and_grad(weights, x, cls, keep_mask=None, keep_scale=1.0, dtype=torch.float64):
    """-> dict: grads (24 arrays of `dtype` in state-dict order), loss (float), site_loss [N,2], pred uint8 [N,2] (first maximum),
    logits [N,24]; float64 unless dtype says otherwise"""
    w = tensors(weights, dtype=dtype)
    loss, site, z = forward(w, x, cls, keep_mask, keep_scale, dtype)
    loss.backward()
    zn = z.detach().numpy()
    pred = np.stack([zn[:, r0:r0 + c].argmax(1) for r0, c in HEADS], axis=1).astype(np.uint8)
    return {"grads": [t.grad.numpy().copy() for t in w], "loss": float(loss.detach()), "site_loss": site.detach().numpy(), "pred": pred, "logits": zn}


def loss_only(weights, x, cls, keep_mask=None, keep_scale=1.0):
    with torch.no_grad():
        return float(forward(tensors(weights, False), x, cls, keep_mask, keep_scale)[0])


def top_two_gap(logits):
    """float64 [N,2]: the distance between the two largest logits of each head (a prediction is only comparable where it is not a near tie)"""
    out = []
    for r0, c in HEADS:
        s = np.sort(np.asarray(logits)[:, r0:r0 + c], axis=1)
        out.append(s[:, -1] - s[:, -2])
    return np.stack(out, axis=1)


def sgd_steps(weights, x, cls, lr, k):
    """k plain-SGD steps (no momentum, no clipping, no dropout) on one fixed batch -> (losses [k + 1]: the loss at the weights before step
    1, after step 1, ..., after step k; the weights after step k)"""
    w = [np.asarray(t, np.float64).copy() for t in weights]
    losses = []
    for _ in range(k):
        r = loss_and_grad(w, x, cls)
        losses.append(r["loss"])
        w = [a - lr * g for a, g in zip(w, r["grads"])]
    losses.append(loss_only(w, x, cls))
    return np.array(losses), w


def rel_dist(got, want):
    """max |got - want| / max |want| of one tensor: the distance the parity bound is stated in"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def sample_index(i, shape, n=64, seed=20261019):
    """n seeded flat indices into tensor i (with replacement): the entries the fixture keeps of the large batches"""
    return np.random.default_rng(seed + i).integers(0, int(np.prod(shape)), n)
