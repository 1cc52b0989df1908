"""Train the PileupModel on training window files (<chr>.td.bin): the reference's ``train()`` (PileupModel/train.py:27-90) on the device.

``PileupTrainer`` owns the 24 parameters as fp32 device tensors; ``loss_and_grad`` is one C-ABI call (nsnp_pileup_loss_grad: forward that
keeps the gate activations, label-smoothed loss, backpropagation through time, weight gradients - hand-written HIP, fp32 MFMA) that
overwrites the gradient buffers each parameter's ``.grad`` is bound to.  PyTorch does the plumbing only: device tensors, the random keep
mask, gradient clipping and the optimiser.  fp32 only, one rank only.

Departures from the reference's loop:
  * the order is a seeded ``torch.randperm`` of each PASS of a file (fed to the kernel as centre indices, no window is copied), where the
    DataLoader shuffles a whole file;
  * the dropout mask between the two LSTM layers comes from a seeded torch generator on the device, not from the stream nn.LSTM draws from;
  * the default optimiser is plain Adam (lr 1e-4); the reference wraps it in Lookahead, which torch does not have - pass your own;
  * the two indel heads get no gradient, as in the reference (model.py:109-110 leaves their losses out), and are carried along unchanged.
Not here: ``balance_dataset``, the ``first_stage`` freeze, learning-rate decay, HaplotypeModel training, split precisions, sharding.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, sitefile
from .pileup_model import ENCODER_KEYS, FORWARD_KEYS, INDEL_KEYS, LSTMNetwork

PARAM_NAMES = ["encoder." + k for k in ENCODER_KEYS] + ["forward_layer." + k for k in FORWARD_KEYS]


class PileupTrainer:
    """The 24 parameters of the PileupModel on the device, with gradients from nsnp_pileup_loss_grad.

    ``params``: ``{name: torch.nn.Parameter}`` in state-dict order, named ``encoder.<key>`` / ``forward_layer.<key>``; every ``.grad`` is
    the buffer the kernel overwrites, so ``torch.optim.X(trainer.parameters())`` steps them.  ``chunk_sites``: the workspace reservation
    (about 194 KB per site); a larger batch runs in chunks of it."""

    def __init__(self, encoder, forward_layer, device=0, chunk_sites=2048, ctx=None):
        import torch
        self.ctx = ctx if ctx is not None else _lib.Context(device)
        self.device = torch.device("cuda", self.ctx.device)
        sd = {"encoder." + k: encoder[k] for k in ENCODER_KEYS}
        sd.update({"forward_layer." + k: forward_layer[k] for k in FORWARD_KEYS})
        as_np = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
        self.params = {}
        for name, shape in zip(PARAM_NAMES, self.ctx.TRAIN_SHAPES):
            a = as_np(sd[name])
            if a.shape != shape:
                raise _lib.NanoSNPError(f"{name}: shape {a.shape}, the kernels are built for {shape}")
            p = torch.nn.Parameter(torch.from_numpy(a).to(self.device), requires_grad=True)
            p.grad = torch.zeros_like(p)
            self.params[name] = p
        self._grads = [p.grad for p in self.params.values()]
        self.indel = {k: as_np(forward_layer[k]) for k in INDEL_KEYS} if all(k in forward_layer for k in INDEL_KEYS) else None
        self.chunk_sites = int(chunk_sites)
        self.ctx.pileup_train_reserve(self.chunk_sites)

    @classmethod
    def from_checkpoint(cls, path, device=0, **kw):
        """``torch.save`` dict {encoder, forward_layer, ...} as PileupModel/utils.py:67-77 writes it"""
        import torch
        ck = torch.load(path, map_location="cpu", weights_only=False)
        return cls(ck["encoder"], ck["forward_layer"], device, **kw)

    @classmethod
    def from_npz(cls, path, device=0, **kw):
        z = np.load(path)
        return cls({k: z["encoder." + k] for k in ENCODER_KEYS},
                   {k: z["forward_layer." + k] for k in FORWARD_KEYS + INDEL_KEYS if "forward_layer." + k in z.files}, device, **kw)

    def parameters(self):
        return list(self.params.values())

    def _check_grads(self):
        # an optimiser's zero_grad(set_to_none=True) unbinds a gradient: bind the kernel's buffer again
        for p, g in zip(self.params.values(), self._grads):
            if p.grad is not g:
                p.grad = g

    def loss_and_grad(self, inputs, gt_target, zy_target, keep_mask=None, p=0.0, center_idx=None, stream=None):
        """inputs: device int32 [N,33,18], or with center_idx (device int64 [N]) a pass flattened to [rows * 33, 18]; gt_target, zy_target:
        integer device tensors [N]; keep_mask: None or device uint8 [N,33,128], used with scale 1 / (1 - p) -> (loss, pred): the fp32
        scalar mean(gt) + mean(zy) of the label-smoothed losses, summed over the sites in float64, and pred uint8 [N,2].  Every
        parameter's .grad holds d loss / d parameter afterwards."""
        import torch
        x = (inputs if inputs.dtype == torch.int32 else inputs.to(torch.int32)).contiguous()
        n = int(center_idx.shape[0]) if center_idx is not None else int(x.shape[0])
        cls = torch.zeros((n, 4), dtype=torch.uint8, device=x.device)
        cls[:, 0] = gt_target.reshape(-1).to(device=x.device, dtype=torch.uint8)
        cls[:, 1] = zy_target.reshape(-1).to(device=x.device, dtype=torch.uint8)
        return self._loss_and_grad_cls(x, center_idx, cls, n, keep_mask, p, stream)

    def _loss_and_grad_cls(self, x, center_idx, cls, n, keep_mask, p, stream=None):
        import torch
        if keep_mask is not None and not 0.0 <= float(p) < 1.0:
            raise ValueError("dropout probability in [0, 1)")
        self._check_grads()
        scale = 1.0 / (1.0 - float(p)) if keep_mask is not None else 1.0
        site_loss, pred = self.ctx.pileup_loss_grad(self.parameters(), x, center_idx, cls, self._grads, keep_mask, scale, n=n, stream=stream)
        if n == 0:
            return torch.full((), float("nan"), dtype=torch.float32, device=x.device), pred
        s = self.ctx.hap_batch_loss(site_loss, n, stream=stream)[0]         # (the two-column batch sum: float64, a fixed tree)
        return ((s[0] + s[1]) / n).to(torch.float32), pred

    def state_dicts(self):
        """(encoder, forward_layer) dicts of CPU tensors; the indel tensors ride along unchanged when the source had them"""
        import torch
        enc = {k: self.params["encoder." + k].detach().cpu().clone() for k in ENCODER_KEYS}
        fwd = {k: self.params["forward_layer." + k].detach().cpu().clone() for k in FORWARD_KEYS}
        if self.indel is not None:
            fwd.update({k: torch.from_numpy(v.copy()) for k, v in self.indel.items()})
        return enc, fwd

    def save_checkpoint(self, path, epoch=0):
        """the ``torch.save`` dict {encoder, forward_layer, epoch} LSTMNetwork.from_checkpoint reads back"""
        import torch
        enc, fwd = self.state_dicts()
        torch.save({"encoder": enc, "forward_layer": fwd, "epoch": int(epoch)}, path)

    def to_model(self, model=None, **kw):
        """a pileup_model.LSTMNetwork with these weights, through the existing upload path (packs the inference images: once per epoch, not
        per step).  model: an LSTMNetwork to refresh instead of a new one."""
        enc, fwd = self.state_dicts()
        m = model if model is not None else LSTMNetwork(None, self.ctx.device, **kw)
        m.encoder.load_state_dict(enc)
        m.forward_layer.load_state_dict(fwd)
        return m


def _paths(training_paths):
    if isinstance(training_paths, (str, os.PathLike)):
        d = str(training_paths)
        return [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".bin")] if os.path.isdir(d) else [d]
    return [str(p) for p in training_paths]


def pass_order(generator, m):
    """the order of the m rows of one pass: a seeded torch.randperm on the CPU generator of the epoch"""
    import torch
    return torch.randperm(m, generator=generator)


def train_train_bins(trainer, training_paths, optimizer=None, batch_size=2000, dropout=0.3, max_grad_norm=20.0, seed=2022, pass_sites=65536,
                     stats=None):
    """One epoch of ``train(epoch, config, model, training_paths, batch_size, optimizer, ...)`` of PileupModel/train.py:27-90 over
    ``.td.bin`` files -> {sites, batches, mean_loss, gt_accuracy, zy_accuracy}.

    Every row trains (training has no for_evaluate filter).  A file is read in passes of `pass_sites` rows: staged in pinned memory, sent,
    widened to int32 on the device, its label rows decoded by nsnp_pileup_label_classes(variants_only=0).  The rows of a pass are visited
    in the order of a seeded ``torch.randperm`` (CPU generator seeded with `seed`, one draw per pass in file order), batches of
    `batch_size` restart with every pass; the order reaches the kernel as centre indices.  Per batch: a Bernoulli keep mask [n,33,128] with
    keep probability 1 - dropout from a device generator seeded with `seed` (none at dropout 0), loss_and_grad,
    clip_grad_norm_(parameters, max_grad_norm) (skipped when max_grad_norm is None), optimizer.step().  optimizer None: torch.optim.Adam(lr=1e-4,
    betas=(0.9, 0.999), eps=1e-8).  mean_loss is the mean over batches of the batch loss (the quantity train.py:60 accumulates, per batch
    rather than per site); the accuracies are over sites, from the argmax the loss kernel writes."""
    import torch
    import torch.distributed as tdist
    from .evaluate import _PassSet
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("train_train_bins under a process group of more than one rank (training is not sharded)")
    B = int(batch_size)
    if B < 1:
        raise ValueError("batch_size >= 1")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("dropout in [0, 1)")
    ctx, dev = trainer.ctx, trainer.device
    if optimizer is None:
        optimizer = torch.optim.Adam(trainer.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    st = stats if stats is not None else {}
    for k in ("passes", "rows", "bytes_h2d"):
        st.setdefault(k, 0)
    files = []
    for p in _paths(training_paths):                           # every header is checked before anything runs
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
    order_gen = torch.Generator().manual_seed(int(seed))
    mask_gen = torch.Generator(device=dev).manual_seed(int(seed))
    hs, ds = _PassSet(P), _PassSet(P, dev)
    batch_losses, correct = [], torch.zeros(2, dtype=torch.int64, device=dev)
    sites = 0
    for f in files:
        for a in range(0, f["n"], P):
            b = min(f["n"], a + P)
            m = b - a
            nb = m * 594 * f["elem"]
            torch.cuda.current_stream(dev).synchronize()       # (the previous pass has left both sets)
            hs.x.numpy()[:nb].view(np.int16 if f["elem"] == 2 else np.int32)[:] = np.asarray(f["x"][a:b]).reshape(-1)
            hs.y.numpy()[:m] = f["y"][a:b]
            ds.x[:nb].copy_(hs.x[:nb], non_blocking=True)
            ds.y[:m].copy_(hs.y[:m], non_blocking=True)
            ds.x32[:m * 33].view(-1).copy_(ds.x[:nb].view(torch.int16 if f["elem"] == 2 else torch.int32))
            ctx.pileup_label_classes(ds.y[:m], False, cls=ds.cls, center_idx=ds.centers, meta=hs.meta)
            st["passes"] += 1; st["rows"] += m; st["bytes_h2d"] += nb + m * 360
            order = pass_order(order_gen, m).to(dev)
            centers = ds.centers[:m].index_select(0, order)
            cls = ds.cls[:m].index_select(0, order).contiguous()
            for o in range(0, m, B):
                n = min(B, m - o)
                mask = None
                if dropout > 0.0:
                    mask = (torch.rand((n, 33, 128), generator=mask_gen, device=dev) >= float(dropout)).to(torch.uint8)
                loss, pred = trainer._loss_and_grad_cls(ds.x32[:m * 33], centers[o:o + n].contiguous(), cls[o:o + n], n, mask, dropout)
                if max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(trainer.parameters(), max_grad_norm)
                optimizer.step()
                batch_losses.append(loss)
                correct += (pred == cls[o:o + n, :2]).sum(0)
                sites += n
    div = max(sites, 1)
    correct = correct.cpu().numpy()
    mean_loss = float(torch.stack(batch_losses).double().mean()) if batch_losses else float("nan")
    return {"sites": sites, "batches": len(batch_losses), "mean_loss": mean_loss, "gt_accuracy": float(correct[0]) / div,
            "zy_accuracy": float(correct[1]) / div}
