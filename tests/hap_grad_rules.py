"""The loss gradients of the reference's HaplotypeModel training step (HaplotypeModel/train_dev.py:58-59: loss, ... = model(...);
loss.backward()), restated in float64 torch for the tests of nsnp_hap_loss_grad and of nanosnp_amd.train.HaplotypeTrainer.  Test
infrastructure, written from the published equations -

    LSTMNetwork.forward        HaplotypeModel/model_dev.py:120-131 (BaseEncoder.forward 76-84, ForwardLayer.forward 96-105)
    nn.LSTM(dropout=p)         between the three layers, in train() mode: h * mask / (1 - p) - here EXPLICIT keep masks and one scale
    LabelSmoothingLoss(C, 0.1) the mean over the batch of -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t])); loss = gt_loss + zy_loss

The forward is that of hap_eval_rules.forward_logits_f64 (same gate order, same direction walk, the last layer cut to the steps the centre
reads - which changes neither the value nor the gradient), built from float64 torch tensors with requires_grad; autograd gives the 58
gradients."""
from __future__ import annotations

import numpy as np
import torch

SMOOTHING = 0.1
H = 256
# (bias_ih, bias_hh) of every layer and direction of both encoders: their gradients are the same sums
BIAS_PAIRS = tuple((26 * e + 8 * l + 4 * d + 2, 26 * e + 8 * l + 4 * d + 3) for e in range(2) for l in range(3) for d in range(2))
assert len(BIAS_PAIRS) == 12


def shapes(F=105, n_gt=10, n_zy=3):
    enc = []
    for l in range(3):
        enc += [(4 * H, F if l == 0 else 2 * H), (4 * H, H), (4 * H,), (4 * H,)] * 2
    enc += [(H, 2 * H), (H,)]
    return enc + enc + [(H, 2 * H), (H,), (n_gt, H), (n_gt,), (n_zy, H), (n_zy,)]


assert sum(int(np.prod(s)) for s in shapes()) == 8192013


def _direction(x, wih, whh, b, reverse, steps):
    """x [N,L,I] -> h of the first `steps` steps of this direction at their positions [N,L,H], zeros elsewhere"""
    n, L, _ = x.shape
    h = torch.zeros((n, H), dtype=x.dtype)
    c = torch.zeros((n, H), dtype=x.dtype)
    hs = [None] * L
    gin = x @ wih.T + b                                     # every position's input projection at once
    for s in range(steps):
        t = L - 1 - s if reverse else s
        g = gin[:, t] + h @ whh.T
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs[t] = h
    zero = torch.zeros((n, H), dtype=x.dtype)
    return torch.stack([v if v is not None else zero for v in hs], dim=1)


def _encoder(w, x, masks, scale):
    """w: the 26 tensors of one BaseEncoder; x [N,L,F]; masks: None or the two keep masks [N,L,512] behind layers 0 and 1 -> [N,H]"""
    L = x.shape[1]
    for l in range(3):
        q = w[8 * l:8 * l + 8]
        last = l == 2
        fwd = _direction(x, q[0], q[1], q[2] + q[3], False, L // 2 + 1 if last else L)
        bwd = _direction(x, q[4], q[5], q[6] + q[7], True, L - L // 2 if last else L)
        x = torch.cat([fwd, bwd], dim=2)
        if not last and masks is not None:
            x = x * torch.as_tensor(np.asarray(masks[l], np.float64)).to(x.dtype) * float(scale)
    return x[:, L // 2] @ w[24].T + w[25]


def forward(w, xp, xh, cls, keep_masks=None, keep_scale=1.0, n_gt=10, dtype=torch.float64):
    """w: 58 tensors of `dtype`; xp [N,F,33], xh [N,F,11]; cls integer [N,2] -> (loss scalar, site_loss [N,2], logits [N, n_gt + n_zy]).
    A class outside its head counts as the head's last class; a head of one class has loss 0."""
    tp = torch.as_tensor(np.asarray(xp, np.float64)).to(dtype).permute(0, 2, 1)
    th = torch.as_tensor(np.asarray(xh, np.float64)).to(dtype).permute(0, 2, 1)
    ep = _encoder(w[0:26], tp, keep_masks[0:2] if keep_masks is not None else None, keep_scale)
    eh = _encoder(w[26:52], th, keep_masks[2:4] if keep_masks is not None else None, keep_scale)
    mid = torch.tanh(torch.cat([ep, eh], dim=1) @ w[52].T + w[53])
    z = torch.cat([mid @ w[54].T + w[55], mid @ w[56].T + w[57]], dim=1)
    cls = np.asarray(cls)
    rows = torch.arange(z.shape[0])
    site = []
    for h, (r0, c) in enumerate(((0, n_gt), (n_gt, z.shape[1] - n_gt))):
        if c == 1:
            site.append(z[:, r0] * 0.0)
            continue
        lp = torch.log_softmax(z[:, r0:r0 + c], dim=1)
        t = torch.as_tensor(np.minimum(cls[:, h].astype(np.int64), c - 1))
        lpt = lp[rows, t]
        site.append(-((1.0 - SMOOTHING) * lpt + SMOOTHING / (c - 1) * (lp.sum(1) - lpt)))
    site = torch.stack(site, dim=1)
    return site[:, 0].mean() + site[:, 1].mean(), site, z


def tensors(weights, requires_grad=True, dtype=torch.float64):
    return [torch.tensor(np.asarray(t, np.float64), dtype=dtype, requires_grad=requires_grad) for t in weights]


def loss_and_grad(weights, xp, xh, cls, keep_masks=None, keep_scale=1.0, n_gt=10, dtype=torch.float64):
    """-> dict: grads (58 arrays in state-dict order), loss (float), site_loss [N,2], pred uint8 [N,2] (first maximum), logits"""
    w = tensors(weights, dtype=dtype)
    loss, site, z = forward(w, xp, xh, cls, keep_masks, keep_scale, n_gt, dtype)
    loss.backward()
    zn = z.detach().numpy()
    pred = np.stack([zn[:, :n_gt].argmax(1), zn[:, n_gt:].argmax(1)], axis=1).astype(np.uint8)
    grads = [t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape), zn.dtype) for t in w]
    return {"grads": grads, "loss": float(loss.detach()), "site_loss": site.detach().numpy(), "pred": pred, "logits": zn}


def loss_only(weights, xp, xh, cls, n_gt=10):
    with torch.no_grad():
        return float(forward(tensors(weights, False), xp, xh, cls, None, 1.0, n_gt)[0])


def sgd_steps(weights, xp, xh, cls, lr, k, n_gt=10):
    """k plain-SGD steps on one fixed batch -> (losses [k + 1]: before step 1, after step 1, ..., after step k; the weights after step k)"""
    w = [np.asarray(t, np.float64).copy() for t in weights]
    losses = []
    for _ in range(k):
        r = loss_and_grad(w, xp, xh, cls, n_gt=n_gt)
        losses.append(r["loss"])
        w = [a - lr * g for a, g in zip(w, r["grads"])]
    losses.append(loss_only(w, xp, xh, cls, n_gt))
    return np.array(losses), w


def rel_dist(got, want):
    """max |got - want| / max |want| of one tensor: the distance the parity bound is stated in"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def sample_index(i, shape, n=64, seed=20261020):
    """n seeded flat indices into tensor i (with replacement): the entries the fixture keeps of every gradient"""
    return np.random.default_rng(seed + i).integers(0, int(np.prod(shape)), n)
