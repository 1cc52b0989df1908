"""Train the PileupModel on training window files (<chr>.td.bin): the reference's ``train()`` (PileupModel/train.py:27-90) and the epoch loop
around it (train.py:222-247) on the device.

``PileupTrainer`` owns the 24 parameters as fp32 device tensors; ``loss_and_grad`` is one C-ABI call (nsnp_pileup_loss_grad: forward that
keeps the gate activations, label-smoothed loss, backpropagation through time, weight gradients - hand-written HIP, fp32 MFMA) that
overwrites the gradient buffers each parameter's ``.grad`` is bound to.  ``DeviceOptimizer`` is the rest of a step as one more C-ABI call
(nsnp_optim_step: gradient norm, clip, Adam / RAdam, Lookahead sync - two launches; nsnp_optim_step_kind, the same for Novograd, SGD and
Adadelta, every type of the reference's build_optimizer but Ranger), with the reference's ``Optimizer`` bookkeeping
(optim.py:10-39) around it; ``fit`` is the epoch loop with the learning-rate decay.  PyTorch does the plumbing only: device tensors and the
random keep mask - and, when the caller passes a torch optimiser of their own, the clipping and that optimiser.  fp32 only, one rank only.

Departures from the reference's loop:
  * the order is a seeded ``torch.randperm`` of each PASS of a file (fed to the kernel as centre indices, no window is copied), where the
    DataLoader shuffles a whole file;
  * the dropout mask between the two LSTM layers comes from a seeded torch generator on the device, not from the stream nn.LSTM draws from;
  * ``train_train_bins`` without an optimiser still steps plain Adam (lr 1e-4); ``fit`` defaults to the shipped configuration,
    ``DeviceOptimizer(kind="LookaheadAdam", lr=1e-4)``;
  * Adam's moments are updated as ``m = beta1 m + (1 - beta1) g`` and the denominator as ``sqrt(v) * (1 / sqrt(1 - beta2^t)) + eps``, where
    torch writes a lerp and a division: the same numbers up to fp32 rounding (tests/golden/pileup_optim.npz is the reference's own run);
  * a reference checkpoint's Lookahead slow buffers are keyed by ``id()`` and cannot be mapped to parameters: ``load_state_dict`` ignores them
    and the slow buffers restart at the next sync, which is what the reference itself does after such a load;
  * the two indel heads get no gradient, as in the reference (model.py:109-110 leaves their losses out), and are carried along unchanged;
  * ``use_balance`` (``balance_dataset``, dataset.py:32-66: every (genotype, zygosity) category upsampled to the largest, then K max / U
    samples drawn from that list) balances the rows of a PASS, not of a file (pass_sites >= a file's rows gives the reference's scope),
    with a seeded counter-based generator (Philox4x32-10, nsnp_pileup_balance_samples on the device) where the reference's np.random is
    unseeded: the same distribution, another stream; and a pass with no category below the largest (U == 0: one row, one category, equal
    sizes), where the reference divides by zero, trains on its rows as they are.
Kept quirks: Lookahead's slow buffer is created at the FIRST sync (step k) as a copy of the fast weights, so that sync changes nothing and
the first interpolation is at step 2k (lookahead.py:39-43); RAdam's weight decay is the decoupled ``p -= wd lr p`` (radam.py:69-70);
Novograd's second moment is one scalar per tensor that is COPIED from the gradient's squared norm whenever it is 0, not only at the first
step, has no bias correction, and its weight decay is added behind the division (novograd.py:201-221).  Novograd's departures: the
gradients are not divided in place (they are only read), and a tensor's squared norm is the float64 sum of the per-range fp32 sums the clip
already made, times the squared clip coefficient, where the reference squares and adds the clipped gradients in fp32.
Not here: the ``first_stage`` freeze, Ranger (its source is not in the reference tree), split precisions, sharding.

The HaplotypeModel (HaplotypeModel/train_dev.py:25-80, 258-291) has the same pieces: ``HaplotypeTrainer`` owns the 58 parameters,
``loss_and_grad`` is one call of nsnp_hap_loss_grad (two 3-layer BiLSTM encoders of hidden size 256, four keep masks), ``DeviceOptimizer``
steps them unchanged, ``train_haplotype_bins`` is one epoch over labelled haplotype site files - with ``pn_value`` the variants are
upsampled per block of 1,000 refcalls as TrainingDataset does it, by nsnp_hap_train_samples on the device - and ``fit_haplotype`` is the
epoch loop with validation, the best checkpoint by genotype macro-F1, the decay and its stop.  Its departures:
  * the variants of a block are drawn from the variants of the PASS, not of the file, by a seeded counter-based generator (Philox4x32-10)
    where the reference draws from an unseeded np.random: the same distribution, another stream;
  * the order is a seeded ``torch.randperm`` of the samples of each PASS, not of a file;
  * the four keep masks come from a seeded torch generator on the device, not from the stream nn.LSTM draws from;
  * ``fit_haplotype`` also writes the fused optimiser's state beside every epoch's checkpoint, so a run can resume (the reference saves no
    optimiser state and cannot);
  * Ranger, the other shipped optimiser type, is still out.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
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

    def save_checkpoint(self, path, epoch=0, optimizer=None):
        """the ``torch.save`` dict {encoder, forward_layer, epoch} LSTMNetwork.from_checkpoint reads back; with a DeviceOptimizer also
        {optimizer: its state_dict(), epoch: its current_epoch, step: its global_step}, the entries of PileupModel/utils.py:67-77"""
        import torch
        enc, fwd = self.state_dicts()
        ck = {"encoder": enc, "forward_layer": fwd, "epoch": int(epoch)}
        if optimizer is not None:
            ck.update(optimizer=optimizer.state_dict(), epoch=int(optimizer.current_epoch), step=int(optimizer.global_step))
        torch.save(ck, path)

    def to_model(self, model=None, **kw):
        """a pileup_model.LSTMNetwork with these weights, through the existing upload path (packs the inference images: once per epoch, not
        per step).  model: an LSTMNetwork to refresh instead of a new one."""
        enc, fwd = self.state_dicts()
        m = model if model is not None else LSTMNetwork(None, self.ctx.device, **kw)
        m.encoder.load_state_dict(enc)
        m.forward_layer.load_state_dict(fwd)
        return m


OPTIMIZER_KINDS = {"Adam": (False, False), "LookaheadAdam": (True, False), "Radam": (False, True), "LookaheadRadam": (True, True)}


def step_scalars(radam, t, lr, beta1, beta2, weight_decay):
    """the float64 scalars of step t (1-based) -> dict(a, b, form, wd_mode, decay) of include/nanosnp.h's nsnp_optim_args.
    Adam: torch.optim.Adam's bias corrections; RAdam: N_sma and step_size in the expression order of PileupModel/radam.py:55-67."""
    if not radam:
        return dict(a=lr / (1 - beta1 ** t), b=1.0 / math.sqrt(1 - beta2 ** t), form=0, wd_mode=1 if weight_decay != 0 else 0, decay=0.0)
    beta2_t = beta2 ** t
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * t * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (1 - beta1 ** t)
    else:
        step_size = 1.0 / (1 - beta1 ** t)
    return dict(a=step_size * lr, b=1.0, form=0 if N_sma >= 5 else 1, wd_mode=2 if weight_decay != 0 else 0, decay=-weight_decay * lr)


# the kinds of nsnp_optim_step_kind, under the names of PileupModel/optim.py:42-104: (lookahead, rule, the per-element states in torch's names)
RULE_KINDS = {"Novograd": (False, _lib.OPTIM_NOVOGRAD, ("exp_avg",)), "LookaheadNovograd": (True, _lib.OPTIM_NOVOGRAD, ("exp_avg",)),
              "sgd": (False, _lib.OPTIM_SGD, ("momentum_buffer",)), "adadelta": (False, _lib.OPTIM_ADADELTA, ("square_avg", "acc_delta"))}


class DeviceOptimizer:
    """The reference's ``Optimizer`` (PileupModel/optim.py:10-39) over one fused device step: clip_grad_norm_, the optimiser's rule and the
    Lookahead wrapper (lookahead.py) are ONE call of nsnp_optim_step (Adam, RAdam) or nsnp_optim_step_kind (Novograd, SGD, Adadelta) per batch.

    trainer_or_params: a PileupTrainer, or a list of contiguous fp32 device tensors whose ``.grad`` is set before every step (at most 64).
    kind: "LookaheadAdam" (the shipped configurations), "Adam", "LookaheadRadam", "Radam", "Novograd", "LookaheadNovograd", "sgd", "adadelta"
    - optim.py's names; betas (0.9, 0.999) and eps 1e-8 are what it gives every type but Adadelta, whose rho and eps default to torch's 0.9 and
    1e-6 (eps None: the kind's default); momentum / nesterov are SGD's.  Owns the state of its kind as device tensors and nothing else -
    exp_avg and exp_avg_sq (Adam, RAdam); exp_avg and ``layer_v``, one second moment per TENSOR (Novograd); momentum_buffer (SGD with a
    momentum); square_avg and acc_delta (Adadelta) - the slow buffers of a Lookahead kind and the step counters; ``lr``, ``global_step``
    (starts at 1), ``current_epoch`` and ``epoch()`` are optim.py's."""

    def __init__(self, trainer_or_params, kind="LookaheadAdam", lr=1e-4, betas=(0.9, 0.999), eps=None, weight_decay=0.0, alpha=0.5, k=6,
                 ctx=None, momentum=0.0, nesterov=False, rho=0.9):
        import torch
        if kind not in OPTIMIZER_KINDS and kind not in RULE_KINDS:
            raise ValueError(f"kind: one of {sorted(OPTIMIZER_KINDS) + sorted(RULE_KINDS)}, got {kind!r}")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"momentum in [0, 1), got {momentum}")
        if not 0.0 <= float(rho) < 1.0:
            raise ValueError(f"rho in [0, 1), got {rho}")
        if nesterov and float(momentum) == 0.0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if eps is None:
            eps = 1e-6 if kind == "adadelta" else 1e-8
        self.trainer = trainer_or_params if hasattr(trainer_or_params, "parameters") and hasattr(trainer_or_params, "ctx") else None
        self.params = list(self.trainer.parameters() if self.trainer is not None else trainer_or_params)
        if not self.params:
            raise ValueError("no parameters")
        self.ctx = ctx if ctx is not None else (self.trainer.ctx if self.trainer is not None else _lib.Context(self.params[0].device.index or 0))
        self.kind = kind
        if kind in OPTIMIZER_KINDS:
            (self.lookahead, self.radam), self.rule, self.state_names = OPTIMIZER_KINDS[kind], None, ("exp_avg", "exp_avg_sq")
        else:
            self.radam = False
            self.lookahead, self.rule, self.state_names = RULE_KINDS[kind]
            if self.rule == _lib.OPTIM_SGD and float(momentum) == 0.0:
                self.state_names = ()
        self.momentum, self.nesterov, self.rho = float(momentum), bool(nesterov), float(rho)
        beta1, beta2 = float(betas[0]), float(betas[1])
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"betas in [0, 1), got {betas}")
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if int(k) < 1:
            raise ValueError(f"Invalid lookahead steps: {k}")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (beta1, beta2), float(eps), float(weight_decay)
        self.alpha, self.k = float(alpha), int(k)
        self.global_step, self.current_epoch = 1, 0
        self.step_count = 0                                  # state['step'] of every parameter
        self.lookahead_step = 0
        self.slow_ready = False                              # the slow buffers hold weights (after the first sync)
        data = [p.detach() for p in self.params]
        # every per-element state of the kind under torch's name, and nothing the kind does not use
        for name in ("exp_avg", "exp_avg_sq", "momentum_buffer", "square_avg", "acc_delta"):
            setattr(self, name, [torch.zeros_like(p) for p in data] if name in self.state_names else None)
        self.slow = [torch.zeros_like(p) for p in data] if self.lookahead else None
        # Novograd's second moments, one per tensor: the kernel reads _layer[0] and writes _layer[1], step() swaps them
        self._layer = [torch.zeros(len(data), dtype=torch.float32, device=data[0].device) for _ in range(2)] \
            if self.rule == _lib.OPTIM_NOVOGRAD else None
        self._tensors = None
        self._scratch = None
        self._args = _lib.OptimArgs() if self.rule is None else _lib.OptimKindArgs()

    @property
    def layer_v(self):
        """Novograd: the second moment of every tensor after the last step, device fp32 [number of tensors]; None for the other kinds"""
        return self._layer[0] if self._layer is not None else None

    def _states(self):
        """the (up to two) state tables in the order of the C entry's exp_avg / exp_avg_sq (state_a / state_b) arguments"""
        tables = [getattr(self, name) for name in self.state_names]
        return tables + [None] * (2 - len(tables))

    def _bind(self):
        """the checked pointer tables; made again when a gradient buffer moved"""
        if self.trainer is not None:
            self.trainer._check_grads()
        grads = [p.grad for p in self.params]
        if any(g is None for g in grads):
            raise _lib.NanoSNPError("DeviceOptimizer.step: a parameter has no .grad")
        ot = self._tensors
        if ot is None or ot.grad_ptrs != tuple(g.data_ptr() for g in grads):
            import torch
            ot = self.ctx.optim_tensors([p.detach() for p in self.params], grads, *self._states(), self.slow)
            self._tensors = ot
            if self._scratch is None:
                self._scratch = torch.empty(ot.scratch_floats, dtype=torch.float32, device=ot.device)
        return ot

    def step(self, max_grad_norm=None, stream=None):
        """clip at max_grad_norm (None or <= 0: no clipping), one step of the kind's rule, the Lookahead sync when it is due -> the
        gradients' norm before clipping, a device scalar (nothing waits for it).  The gradient buffers are not written."""
        import torch
        ot = self._bind()
        self.global_step += 1
        self.step_count += 1
        a = self._args
        if self.rule is None:
            for key, val in step_scalars(self.radam, self.step_count, self.lr, self.betas[0], self.betas[1], self.weight_decay).items():
                setattr(a, key, val)
        else:
            a.kind, a.lr, a.momentum, a.nesterov, a.rho = self.rule, self.lr, self.momentum, int(self.nesterov), self.rho
        a.max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        a.weight_decay, a.beta1, a.beta2, a.eps, a.alpha = self.weight_decay, self.betas[0], self.betas[1], self.eps, self.alpha
        a.sync = 0
        if self.lookahead:
            self.lookahead_step += 1
            if self.lookahead_step % self.k == 0:
                a.sync = 1 if self.slow_ready else 2
                self.slow_ready = True
        norm = torch.empty((), dtype=torch.float32, device=ot.device)
        if self.rule is None:
            self.ctx.optim_step(ot, a, self._scratch, norm, stream=stream)
        elif self._layer is None:
            self.ctx.optim_kind_step(ot, a, None, None, self._scratch, norm, stream=stream)
        else:
            self.ctx.optim_kind_step(ot, a, self._layer[0], self._layer[1], self._scratch, norm, stream=stream)
            self._layer.reverse()                            # what this step wrote is what the next one reads
        return norm

    def zero_grad(self, set_to_none=False):
        """nothing: nsnp_pileup_loss_grad overwrites the gradients (kept for the call shape of optim.py:27-28)"""

    def epoch(self):
        self.current_epoch += 1

    def decay_lr(self, ratio):
        self.lr *= float(ratio)

    def state_dict(self):
        """{state: {i: {step, exp_avg, exp_avg_sq}}, slow_state: {i: {slow_buffer}}, param_groups: [...]} keyed by parameter index, CPU
        tensors: the layout of Lookahead.state_dict() (lookahead.py:60-72) with indices where it has id()s.  The state entries and the group
        are those of the kind's torch optimiser: Novograd {step, exp_avg, exp_avg_sq: a 0-d tensor} (novograd.py:182-187), SGD
        {momentum_buffer} (no entry without a momentum), Adadelta {step, square_avg, acc_delta}."""
        n = len(self.params)
        with_step = self.rule != _lib.OPTIM_SGD
        state = {}
        if self.step_count > 0 and self.state_names:
            v = self._layer[0].cpu() if self._layer is not None else None
            for i in range(n):
                state[i] = {"step": self.step_count} if with_step else {}
                state[i].update({name: getattr(self, name)[i].cpu().clone() for name in self.state_names})
                if v is not None:
                    state[i]["exp_avg_sq"] = v[i].clone()
        slow = {i: {"slow_buffer": self.slow[i].cpu().clone()} for i in range(n)} if self.lookahead and self.slow_ready else {}
        if self.rule is None:
            group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "params": list(range(n))}
        elif self.rule == _lib.OPTIM_NOVOGRAD:
            group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "grad_averaging": False,
                     "amsgrad": False, "params": list(range(n))}
        elif self.rule == _lib.OPTIM_SGD:
            group = {"lr": self.lr, "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay, "nesterov": self.nesterov,
                     "params": list(range(n))}
        else:
            group = {"lr": self.lr, "rho": self.rho, "eps": self.eps, "weight_decay": self.weight_decay, "params": list(range(n))}
        if self.lookahead:
            group.update(lookahead_alpha=self.alpha, lookahead_k=self.k, lookahead_step=self.lookahead_step)
        return {"state": state, "slow_state": slow, "param_groups": [group]}

    def load_state_dict(self, state_dict, global_step=None, current_epoch=None):
        """a state_dict() of this class, or the ``optimizer`` entry of a checkpoint the reference's utils.save_model wrote (torch's layout:
        state keyed by parameter index).  The reference's slow_state is keyed by id() and cannot be mapped: it is ignored and the slow
        buffers restart at the next sync, as after the reference's own load.  lr, weight_decay, the kind's own settings (betas, eps, momentum,
        nesterov, rho) and the Lookahead settings come from param_groups[0].  The state entries are the kind's (state_dict()): Novograd's
        exp_avg_sq is a 0-d tensor per parameter, SGD's momentum_buffer comes without a step.  global_step / current_epoch: the checkpoint's
        ``step`` / ``epoch`` entries, when given."""
        import torch
        n = len(self.params)
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != n:
            raise _lib.NanoSNPError(f"load_state_dict: one parameter group of {n} parameters expected")
        state = state_dict.get("state", {})
        if state and sorted(state) != list(range(n)):
            raise _lib.NanoSNPError(f"load_state_dict: state keyed by the parameter indices 0..{n - 1} expected")
        steps = {int(float(state[i]["step"])) for i in state if "step" in state[i]}
        if len(steps) > 1:
            raise _lib.NanoSNPError("load_state_dict: the parameters have different step counts")
        if self.rule == _lib.OPTIM_SGD and (float(groups[0].get("momentum", self.momentum)) != 0.0) != bool(self.state_names):
            raise _lib.NanoSNPError("load_state_dict: an SGD state with a momentum needs an optimizer built with one, one without an optimizer without")
        for i in range(n):
            for name in self.state_names:
                mine = getattr(self, name)
                if state:
                    src = state[i][name]
                    if tuple(src.shape) != tuple(mine[i].shape):
                        raise _lib.NanoSNPError(f"load_state_dict: {name} of parameter {i} has shape {tuple(src.shape)}")
                    mine[i].copy_(src.to(torch.float32))
                else:
                    mine[i].zero_()
        if self._layer is not None:                          # Novograd's exp_avg_sq: a 0-d tensor per parameter
            v = [float(state[i]["exp_avg_sq"]) for i in range(n)] if state else [0.0] * n
            self._layer[0].copy_(torch.tensor(v, dtype=torch.float64).to(torch.float32))
        # (torch's SGD keeps no step: any count above 0 says that the buffers hold a state)
        self.step_count = steps.pop() if steps else (1 if state else 0)
        g = groups[0]
        self.lr, self.weight_decay = float(g["lr"]), float(g["weight_decay"])
        if "betas" in g:
            self.betas = (float(g["betas"][0]), float(g["betas"][1]))
        if "eps" in g:
            self.eps = float(g["eps"])
        if self.rule == _lib.OPTIM_SGD:
            self.momentum, self.nesterov = float(g.get("momentum", self.momentum)), bool(g.get("nesterov", self.nesterov))
        if self.rule == _lib.OPTIM_ADADELTA:
            self.rho = float(g.get("rho", self.rho))
        if self.lookahead:
            self.alpha, self.k = float(g.get("lookahead_alpha", self.alpha)), int(g.get("lookahead_k", self.k))
            self.lookahead_step = int(g.get("lookahead_step", 0))
            slow = state_dict.get("slow_state", {})
            self.slow_ready = bool(slow) and set(slow) == set(range(n)) and all("slow_buffer" in slow[i] for i in range(n))
            if self.slow_ready:
                for i in range(n):
                    self.slow[i].copy_(slow[i]["slow_buffer"].to(torch.float32))
        if global_step is not None:
            self.global_step = int(global_step)
        if current_epoch is not None:
            self.current_epoch = int(current_epoch)


def pass_order(generator, m):
    """the order of the m rows of one pass: a seeded torch.randperm on the CPU generator of the epoch"""
    import torch
    return torch.randperm(m, generator=generator)


def balance_sample_count(sizes):
    """(M, K, U, max) of nsnp_pileup_balance_samples from the rows per (genotype, zygosity) category (63 counts, 3 gt + zy): max = the
    largest, K = the nonempty categories, U = those below max (balance_dataset's non_zero_categories, dataset.py:50-57: the categories at
    max are not counted), M = K max // U samples (int(len(total_indexes) / non_zero_categories), dataset.py:65).  M is None when U == 0,
    where the reference divides by zero.  M <= 2 sum(sizes)."""
    sizes = [int(s) for s in sizes]
    if any(s < 0 for s in sizes):
        raise ValueError("sizes: counts >= 0")
    mx = max(sizes, default=0)
    K = sum(1 for s in sizes if s > 0)
    U = sum(1 for s in sizes if 0 < s < mx)
    return (K * mx // U if U else None), K, U, mx


def train_train_bins(trainer, training_paths, optimizer=None, batch_size=2000, dropout=0.3, max_grad_norm=20.0, seed=2022, pass_sites=65536,
                     stats=None, use_balance=False):
    """One epoch of ``train(epoch, config, model, training_paths, batch_size, optimizer, ...)`` of PileupModel/train.py:27-90 over
    ``.td.bin`` files -> {sites, batches, mean_loss, gt_accuracy, zy_accuracy}; with use_balance also {rows, samples_drawn,
    passes_unbalanced}.

    Every row trains (training has no for_evaluate filter).  A file is read in passes of `pass_sites` rows: staged in pinned memory, sent,
    widened to int32 on the device, its label rows decoded by nsnp_pileup_label_classes(variants_only=0).  The rows of a pass are visited
    in the order of a seeded ``torch.randperm`` (CPU generator seeded with `seed`, one draw per pass in file order), batches of
    `batch_size` restart with every pass; the order reaches the kernel as centre indices.  Per batch: a Bernoulli keep mask [n,33,128] with
    keep probability 1 - dropout from a device generator seeded with `seed` (none at dropout 0), loss_and_grad,
    clip_grad_norm_(parameters, max_grad_norm) (skipped when max_grad_norm is None), optimizer.step() - with a DeviceOptimizer both are its
    one fused step(max_grad_norm), and torch's clip does not run.  optimizer None: torch.optim.Adam(lr=1e-4, betas=(0.9, 0.999), eps=1e-8).  mean_loss is the mean over batches of the batch loss (the quantity train.py:60 accumulates, per batch
    rather than per site); the accuracies are over sites, from the argmax the loss kernel writes.

    use_balance (TrainDataset(datapath, use_balance=True), dataset.py:84-90): behind the label pass ctx.pileup_balance_samples(cls, m, seed,
    draw = the pass's number in the epoch) lists M = K max // U rows of the pass, drawn with replacement from the list in which every
    (genotype, zygosity) category is upsampled to the largest (balance_sample_count; a buffer of 2 pass_sites entries, allocated once, always
    suffices); pass_order(M) permutes the LIST - which also stands for the reference's shuffle - and centres and classes are gathered
    through samples[order].  A pass with no category below the largest (status 1: one row, one category, equal sizes - where the reference
    divides by zero) trains on its rows as without use_balance.  `sites` counts what trained (a row drawn three times counts three times),
    `rows` the file rows read, `samples_drawn` the sum of M over the balanced passes, `passes_unbalanced` the passes with status 1."""
    import torch
    import torch.distributed as tdist
    from .evaluate import _PassSet, _open_window_files, _paths
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
    fused = isinstance(optimizer, DeviceOptimizer)
    st = stats if stats is not None else {}
    for k in ("passes", "rows", "bytes_h2d"):
        st.setdefault(k, 0)
    files = _open_window_files(_paths(training_paths, ".bin"))
    P = int(max(1, pass_sites))
    order_gen = torch.Generator().manual_seed(int(seed))
    mask_gen = torch.Generator(device=dev).manual_seed(int(seed))
    hs, ds = _PassSet(P), _PassSet(P, dev)
    batch_losses, correct = [], torch.zeros(2, dtype=torch.int64, device=dev)
    sites = 0
    if use_balance:
        samples = torch.empty(2 * P, dtype=torch.int64, device=dev)
        bal_meta = torch.zeros(8, dtype=torch.int64).pin_memory()
        rows_read, drawn, unbalanced, pass_no = 0, 0, 0, 0
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
            count, balanced = m, False                         # what trains: the rows of the pass, or its balanced list
            if use_balance:
                # (the entry waits for the stream once, in front of the launch that writes bal_meta: wait for that launch too)
                ctx.pileup_balance_samples(ds.cls, m, int(seed) & (2 ** 64 - 1), draw=pass_no, samples=samples, sizes=False, meta=bal_meta)
                torch.cuda.current_stream(dev).synchronize()
                rows_read, pass_no = rows_read + m, pass_no + 1
                if int(bal_meta[5]) == 0:
                    count, balanced = int(bal_meta[0]), True
                    drawn += count
                else:
                    unbalanced += 1
            order = pass_order(order_gen, count).to(dev)
            if balanced:
                order = samples[:count].index_select(0, order)
            centers = ds.centers[:m].index_select(0, order)
            cls = ds.cls[:m].index_select(0, order).contiguous()
            for o in range(0, count, B):
                n = min(B, count - o)
                mask = None
                if dropout > 0.0:
                    mask = (torch.rand((n, 33, 128), generator=mask_gen, device=dev) >= float(dropout)).to(torch.uint8)
                loss, pred = trainer._loss_and_grad_cls(ds.x32[:m * 33], centers[o:o + n].contiguous(), cls[o:o + n], n, mask, dropout)
                if fused:
                    optimizer.step(max_grad_norm)
                else:
                    if max_grad_norm is not None:
                        torch.nn.utils.clip_grad_norm_(trainer.parameters(), max_grad_norm)
                    optimizer.step()
                batch_losses.append(loss)
                correct += (pred == cls[o:o + n, :2]).sum(0)
                sites += n
    div = max(sites, 1)
    correct = correct.cpu().numpy()
    mean_loss = float(torch.stack(batch_losses).double().mean()) if batch_losses else float("nan")
    res = {"sites": sites, "batches": len(batch_losses), "mean_loss": mean_loss, "gt_accuracy": float(correct[0]) / div,
           "zy_accuracy": float(correct[1]) / div}
    if use_balance:
        res.update(rows=rows_read, samples_drawn=drawn, passes_unbalanced=unbalanced)
    return res



class HaplotypeTrainer:
    """The 58 parameters of the HaplotypeModel on the device, with gradients from nsnp_hap_loss_grad: the counterpart of PileupTrainer.

    state_dict: the tensors of model_dev.LSTMNetwork.state_dict() (haplotype_model.state_dict_keys(); the loss modules hold none); config: the
    reference's config (None: ont_haplotype.yaml's dims), validated by the rules of haplotype_model.LSTMNetwork.  ``params``:
    ``{key: torch.nn.Parameter}`` in state-dict order; every ``.grad`` is the buffer the kernel overwrites, so DeviceOptimizer(trainer, ...) and
    ``torch.optim.X(trainer.parameters())`` both step them.  ``chunk_sites``: the workspace reservation (1,652,864 bytes per site); a larger
    batch runs in chunks of it."""

    def __init__(self, state_dict, config=None, device=0, chunk_sites=512, ctx=None):
        import torch
        from . import haplotype_model
        self.ctx = ctx if ctx is not None else _lib.Context(device)
        self.device = torch.device("cuda", self.ctx.device)
        self.config = config
        self.dims = haplotype_model.LSTMNetwork(config, self.ctx.device, ctx=self.ctx).dims          # (its __init__ refuses what the kernels are not built for)
        self.keys = haplotype_model.state_dict_keys(self.dims["lstm_layers"])
        d = self.dims
        missing = [k for k in self.keys if k not in state_dict]
        if missing:
            raise KeyError(f"missing keys {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        self.params = {}
        for name, shape in zip(self.keys, _lib.Context.hap_train_shapes(d["pileup_dim"], d["gt_num_class"], d["zy_num_class"])):
            t = state_dict[name]
            a = np.array(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
            if a.shape != shape:
                raise _lib.NanoSNPError(f"{name}: shape {a.shape}, the configuration gives {shape}")
            p = torch.nn.Parameter(torch.from_numpy(a).to(self.device), requires_grad=True)
            p.grad = torch.zeros_like(p)
            self.params[name] = p
        self._grads = [p.grad for p in self.params.values()]
        self.chunk_sites = int(chunk_sites)
        self.ctx.hap_train_reserve(self.chunk_sites, d["pileup_dim"], d["gt_num_class"], d["zy_num_class"])

    @classmethod
    def from_checkpoint(cls, path, config=None, device=0, **kw):
        """a ``torch.save``d state dict, as HaplotypeModel/train_dev.py:276 writes it"""
        import torch
        return cls(torch.load(path, map_location="cpu", weights_only=False), config, device, **kw)

    def parameters(self):
        return list(self.params.values())

    def _check_grads(self):
        # an optimiser's zero_grad(set_to_none=True) unbinds a gradient: bind the kernel's buffer again
        for p, g in zip(self.params.values(), self._grads):
            if p.grad is not g:
                p.grad = g

    def loss_and_grad(self, pileup_x, haplotype_x, gt_target, zy_target, keep_masks=None, p=0.0, stream=None):
        """pileup_x [N,F,33], haplotype_x [N,F,11]: device tensors as LSTMNetwork.forward takes them (cast to fp32); gt_target, zy_target:
        integer device tensors [N]; keep_masks: None or four device uint8 tensors [N,33,512], [N,33,512], [N,11,512], [N,11,512] (behind
        pileup layers 0 and 1, haplotype layers 0 and 1), used with scale 1 / (1 - p) -> (loss, pred): the fp32 scalar mean(gt) + mean(zy) of
        the label-smoothed losses, summed over the sites in float64, and pred uint8 [N,2].  Every parameter's .grad holds
        d loss / d parameter afterwards."""
        import torch
        xp, xh = pileup_x.to(torch.float32).contiguous(), haplotype_x.to(torch.float32).contiguous()
        n = int(xp.shape[0])
        cls = torch.stack([t.reshape(-1).to(device=xp.device, dtype=torch.uint8) for t in (gt_target, zy_target)], dim=1).contiguous()
        if tuple(cls.shape) != (n, 2):
            raise ValueError(f"expected two targets of {n} classes")
        return self._loss_and_grad_cls(xp, xh, cls, n, keep_masks, p, stream)

    def _loss_and_grad_cls(self, xp, xh, cls, n, keep_masks, p, stream=None):
        import torch
        if keep_masks is not None and not 0.0 <= float(p) < 1.0:
            raise ValueError("dropout probability in [0, 1)")
        self._check_grads()
        scale = 1.0 / (1.0 - float(p)) if keep_masks is not None else 1.0
        site_loss, pred = self.ctx.hap_loss_grad(self.parameters(), xp, xh, cls, self._grads, keep_masks, scale, n=n, stream=stream)
        if n == 0:
            return torch.full((), float("nan"), dtype=torch.float32, device=xp.device), pred
        s = self.ctx.hap_batch_loss(site_loss, n, stream=stream)[0]         # (the two-column batch sum: float64, a fixed tree)
        return ((s[0] + s[1]) / n).to(torch.float32), pred

    def state_dict(self):
        """the 58 CPU tensors, keyed as model_dev.LSTMNetwork.state_dict() keys them"""
        return {k: p.detach().cpu().clone() for k, p in self.params.items()}

    def save_checkpoint(self, path):
        """``torch.save`` of exactly state_dict(): what train_dev.py:276 writes and haplotype_model.LSTMNetwork().load_state_dict reads"""
        import torch
        torch.save(self.state_dict(), path)

    def to_model(self, model=None):
        """a haplotype_model.LSTMNetwork with these weights, through the existing upload path (packs the inference images: once per epoch,
        not per step).  model: an LSTMNetwork to refresh instead of a new one on this trainer's context."""
        from . import haplotype_model
        m = model if model is not None else haplotype_model.LSTMNetwork(self.config, self.ctx.device, ctx=self.ctx)
        m.load_state_dict(self.state_dict())
        return m


def pn_sample_count(n_ref, n_var, pn_value):
    """M of nsnp_hap_train_samples from the counts the label pass reports: n_ref refcalls cut into blocks of 1,000, each followed by
    int(len * pn_value) variant draws (Python's float product, truncated: dataset_dev.py:214,224); no draws without a variant"""
    n_ref, n_var, pn_value = int(n_ref), int(n_var), float(pn_value)
    if n_ref <= 0:
        return 0
    if n_var <= 0:
        return n_ref
    blocks = -(-n_ref // 1000)
    return n_ref + (blocks - 1) * int(1000.0 * pn_value) + int(float(n_ref - (blocks - 1) * 1000) * pn_value)


def train_haplotype_bins(trainer, bin_paths, reference, optimizer=None, batch_size=512, dropout=0.1, max_grad_norm=2.0, seed=2022,
                         pass_sites=16384, stats=None, pn_value=None):
    """One epoch of ``train(...)`` of HaplotypeModel/train_dev.py:25-80 over labelled haplotype site files
    (sitefile.write_haplotype_train_bin) -> {sites, batches, mean_loss, gt_accuracy, zy_accuracy, refcalls, variants, unscorable_labels,
    samples_refcall, samples_variant}.

    The rows that train are those nsnp_hap_label_classes keeps: LabelField's filter (dataset_dev.py:174-187), the set
    evaluate_haplotype_bins scores.  A file is read in passes of `pass_sites` rows, synchronously on the calling thread: the eight planes
    staged in pinned memory (int8 while every value fits), sent, every row reduced to features (ctx.hap_features), the label pass, the kept
    rows gathered in the order of a seeded ``torch.randperm`` of the KEPT rows (pass_order on a CPU generator seeded with `seed`, one draw per
    pass that keeps a row, in file order); batches of `batch_size` restart with every pass.  Per batch: four Bernoulli keep masks ([n,33,512]
    twice, [n,11,512] twice, in that order) with keep probability 1 - dropout from a device generator seeded with `seed` (none at dropout 0),
    loss_and_grad, then optimizer.step(max_grad_norm) of a DeviceOptimizer - or clip_grad_norm_ (skipped when max_grad_norm is None) and
    step() of a torch optimiser.  optimizer None: DeviceOptimizer(trainer, kind="LookaheadAdam", lr=1e-5), the shipped configuration
    (ont_haplotype.yaml).  The label pass reads the class counts of the heads loaded on the context: the trainer's weights are uploaded once
    in front of the first pass when the context holds none of these dims.  mean_loss is the mean over batches of the batch loss; the
    accuracies are over sites.

    pn_value None: every kept row trains once, as above.  A float (the shipped configuration trains with 0.7): TrainingDataset's upsampling
    (dataset_dev.py:190-230) on the device.  After the label pass ctx.hap_train_samples(cls, kept, pn_value, seed, draw = the pass's number in
    the epoch) lists the pass's refcalls in blocks of 1,000, each followed by int(len * pn_value) variants drawn with replacement;
    pass_order of the list's length permutes it (this stands for the reference's shuffle inside a block and for its DataLoader's), and rows
    and classes are gathered through the result.  A pass whose list is empty - no kept refcall - is skipped without drawing an order.
    `sites` then counts samples (a variant drawn three times counts three times) and equals the sum of pn_sample_count over the passes;
    samples_refcall / samples_variant split it (without pn_value they equal refcalls / variants).

    Departures from the reference's loop: variants are drawn from the PASS's variants, not the file's
    (pass_sites >= the rows of a file gives the reference's scope), by a seeded counter-based generator where the reference's np.random is
    unseeded; the order is per pass, not per file; the masks come from a torch generator, not from the stream nn.LSTM draws from; the default
    optimiser here leaves out the shipped weight_decay of 1e-4 (fit_haplotype's default has it); Ranger is not implemented."""
    import torch
    import torch.distributed as tdist
    from . import evaluate, hap_pipeline
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("train_haplotype_bins under a process group of more than one rank (training is not sharded)")
    if not isinstance(reference, hap_pipeline.DeviceReference):
        raise TypeError("reference: a hap_pipeline.DeviceReference")
    B = int(batch_size)
    if B < 1:
        raise ValueError("batch_size >= 1")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("dropout in [0, 1)")
    pn = None if pn_value is None else float(pn_value)
    if pn is not None and not 0.0 <= pn <= _lib.Context.HAP_PN_VALUE_MAX:
        raise ValueError(f"pn_value: None or in [0, {_lib.Context.HAP_PN_VALUE_MAX:.0f}]")
    ctx, dev = trainer.ctx, trainer.device
    if optimizer is None:
        optimizer = DeviceOptimizer(trainer, kind="LookaheadAdam", lr=1e-5)
    fused = isinstance(optimizer, DeviceOptimizer)
    st = stats if stats is not None else {}
    for k in ("passes", "rows", "bytes_h2d"):
        st.setdefault(k, 0)
    if getattr(ctx, "_hap_dims", None) != (trainer.dims["gt_num_class"], trainer.dims["zy_num_class"]):
        trainer.to_model()
    P = int(max(1, pass_sites))
    files = evaluate._open_hap_files(evaluate._paths(bin_paths, ".bin"), True)
    try:
        order_gen = torch.Generator().manual_seed(int(seed))
        mask_gen = torch.Generator(device=dev).manual_seed(int(seed))
        batch_losses, correct = [], torch.zeros(2, dtype=torch.int64, device=dev)
        totals = np.zeros(4, np.int64)                         # kept, unscorable, refcalls, variants
        drawn = np.zeros(2, np.int64)                          # samples that are refcalls, samples that are variants
        samples, sample_meta, pass_no = None, torch.zeros(4, dtype=torch.int64, device=dev), 0
        live = [f for f in files if f["n"]]
        if live:
            Pmax = min(P, max(f["n"] for f in live))
            Dp, Dh, elem = max(f["src"].Dp for f in live), max(f["src"].Dh for f in live), max(f["src"].elem for f in live)
            hs, ds = evaluate._HapPassSet(Pmax, Dp, Dh, elem), evaluate._HapPassSet(Pmax, Dp, Dh, elem, dev)
            off33 = torch.arange(-16, 17, dtype=torch.int64, device=dev)[None, :]
        for f in live:
            for a in range(0, f["n"], P):
                b = min(f["n"], a + P)
                m = b - a
                torch.cuda.current_stream(dev).synchronize()   # (the previous pass has left both sets)
                nbytes = evaluate._fill_hap_pass(f, a, b, hs, reference)
                evaluate._send_hap_pass(f, m, hs, ds)
                xp, xh = evaluate._hap_pass_features(ctx, f, m, ds, hs, reference, off33)
                torch.cuda.current_stream(dev).synchronize()
                meta = hs.meta.numpy().copy()
                totals += meta
                kept = int(meta[0])
                st["passes"] += 1; st["rows"] += m; st["bytes_h2d"] += nbytes + m * (12 * 12 + 12)
                draw, pass_no = pass_no, pass_no + 1
                if pn is not None:
                    # the pass's sample list - refcall blocks, each with its variant draws - and the seeded order over the whole list
                    count = pn_sample_count(meta[2], meta[3], pn)
                    if not count:
                        continue
                    if samples is None or samples.numel() < count:
                        samples = torch.empty(count + count // 4, dtype=torch.int64, device=dev)
                    ctx.hap_train_samples(ds.cls, kept, pn, int(seed) & (2 ** 64 - 1), draw=draw, samples=samples, meta=sample_meta)
                    drawn += (int(meta[2]), count - int(meta[2]))
                    order = samples[:count].index_select(0, pass_order(order_gen, count).to(dev))
                else:
                    if not kept:
                        continue
                    count = kept
                    order = pass_order(order_gen, kept).to(dev)
                    drawn += (int(meta[2]), int(meta[3]))
                idx = ds.rows[:kept].index_select(0, order)
                xp, xh = torch.index_select(xp, 0, idx), torch.index_select(xh, 0, idx)
                cls = ds.cls[:kept].index_select(0, order).contiguous()
                for o in range(0, count, B):
                    n = min(B, count - o)
                    masks = None
                    if dropout > 0.0:
                        masks = [(torch.rand((n, L, 512), generator=mask_gen, device=dev) >= float(dropout)).to(torch.uint8) for L in (33, 33, 11, 11)]
                    loss, pred = trainer._loss_and_grad_cls(xp[o:o + n], xh[o:o + n], cls[o:o + n], n, masks, dropout)
                    if fused:
                        optimizer.step(max_grad_norm)
                    else:
                        if max_grad_norm is not None:
                            torch.nn.utils.clip_grad_norm_(trainer.parameters(), max_grad_norm)
                        optimizer.step()
                    batch_losses.append(loss)
                    correct += (pred == cls[o:o + n]).sum(0)
    finally:
        for f in files:
            f["src"].close()
    sites = int(totals[0]) if pn is None else int(drawn.sum())
    div = max(sites, 1)
    correct = correct.cpu().numpy()
    mean_loss = float(torch.stack(batch_losses).double().mean()) if batch_losses else float("nan")
    return {"sites": sites, "batches": len(batch_losses), "mean_loss": mean_loss, "gt_accuracy": float(correct[0]) / div,
            "zy_accuracy": float(correct[1]) / div, "refcalls": int(totals[2]), "variants": int(totals[3]), "unscorable_labels": int(totals[1]),
            "samples_refcall": int(drawn[0]), "samples_variant": int(drawn[1])}


def fit(trainer, training_paths, validating_paths=None, epochs=1, optimizer=None, batch_size=2000, dropout=0.3, max_grad_norm=20.0,
        decay_ratio=0.98, begin_to_adjust_lr=10, seed=2022, save_prefix=None, start_epoch=0, pass_sites=65536, eval_batch_size=None,
        use_balance=False, validate_precision=None):
    """The epoch loop of PileupModel/train.py:222-247 -> one dict per epoch: train_train_bins' result plus {epoch, lr (the rate the epoch
    ran with), global_step, eval (evaluate_train_bins' result or None), checkpoint (its path or None)}.

    Per epoch in range(start_epoch, epochs): optimizer.epoch(); train_train_bins with seed + epoch, so that every epoch has an order and masks
    of its own; evaluate.evaluate_train_bins on validating_paths when given (through trainer.to_model, one upload per epoch);
    validate_precision is its `precision` (None: fp32; 0 / 1 / 2 / "context": the arithmetic the checkpoint will be deployed in - training
    itself stays fp32 and does not depend on it);
    trainer.save_checkpoint(<save_prefix>.epoch<e>.chkpt, optimizer=optimizer) when save_prefix is given; optimizer.decay_lr(decay_ratio)
    once epoch >= begin_to_adjust_lr.  use_balance: train_train_bins' balance_dataset upsampling (config.training.use_balance); the lists
    differ from epoch to epoch through seed + epoch.  optimizer None: DeviceOptimizer(trainer, kind="LookaheadAdam", lr=1e-4), the shipped configuration.
    To resume: trainer from the checkpoint, optimizer.load_state_dict(ck["optimizer"], ck["step"], ck["epoch"]), start_epoch=ck["epoch"]."""
    from . import evaluate
    if optimizer is None:
        optimizer = DeviceOptimizer(trainer, kind="LookaheadAdam", lr=1e-4)
    fused = isinstance(optimizer, DeviceOptimizer)
    out, model = [], None
    for epoch in range(int(start_epoch), int(epochs)):
        if fused:
            optimizer.epoch()
        lr = optimizer.lr if fused else optimizer.param_groups[0]["lr"]
        res = train_train_bins(trainer, training_paths, optimizer=optimizer, batch_size=batch_size, dropout=dropout, max_grad_norm=max_grad_norm,
                               seed=int(seed) + epoch, pass_sites=pass_sites, use_balance=use_balance)
        res.update(epoch=epoch, lr=lr, global_step=optimizer.global_step if fused else None, eval=None, checkpoint=None)
        if validating_paths is not None:
            model = trainer.to_model(model)
            res["eval"] = evaluate.evaluate_train_bins(model, validating_paths, batch_size=int(eval_batch_size or batch_size), pass_sites=pass_sites,
                                                       precision=validate_precision)
        if save_prefix is not None:
            res["checkpoint"] = f"{save_prefix}.epoch{epoch}.chkpt"
            trainer.save_checkpoint(res["checkpoint"], epoch=epoch, optimizer=optimizer if fused else None)
        if epoch >= int(begin_to_adjust_lr):
            if fused:
                optimizer.decay_lr(decay_ratio)
            else:
                for g in optimizer.param_groups:
                    g["lr"] *= float(decay_ratio)
        out.append(res)
    return out


def fit_haplotype(trainer, bin_paths, reference, validating_paths=None, epochs=30, optimizer=None, batch_size=512, dropout=0.1,
                  max_grad_norm=2.0, pn_value=0.7, decay_ratio=0.98, begin_to_adjust_lr=3, min_lr=1e-7, finetune=False, seed=2021,
                  save_prefix=None, start_epoch=0, pass_sites=16384):
    """The epoch loop of HaplotypeModel/train_dev.py:258-291 -> one dict per epoch: train_haplotype_bins' result plus {epoch, lr (the rate the
    epoch ran with), global_step, eval (evaluate_haplotype_bins' result or None), checkpoint, best_checkpoint (paths or None), stopped}.

    Per epoch in range(start_epoch, epochs): optimizer.epoch(); train_haplotype_bins with seed + epoch and pn_value (None: no upsampling);
    with validating_paths, evaluate.evaluate_haplotype_bins through trainer.to_model (one upload per epoch, which also serves the next
    epoch's label pass).  With save_prefix: <save_prefix>.chkpt whenever eval["gt_f1"] >= the best so far (the best starts at 0; the
    reference's >=, so the last of tied epochs stays), and <save_prefix>.epoch<e>.chkpt every epoch - both plain state dicts, what
    train_dev.py:276,280 writes and haplotype_model.LSTMNetwork().load_state_dict reads.  From epoch >= begin_to_adjust_lr the rate decays by
    decay_ratio; when the new rate is below min_lr the loop ends behind this epoch and its dict has stopped True (train_dev.py:284-290).

    optimizer None: DeviceOptimizer(trainer, kind="LookaheadAdam", lr=1e-5, weight_decay=1e-4), the shipped ont_haplotype.yaml; finetune
    starts it at a tenth of that rate (optim.py:19-22).  finetune with an optimizer of the caller's is refused: that optimizer carries its
    own rate.  Defaults are the shipped file's (epochs 30, batch 512, dropout 0.1, max_grad_norm 2, pn_value 0.7, decay 0.98 from epoch 3,
    seed 2021).

    Beyond the reference, which saves no optimiser state and cannot resume: beside every epoch's checkpoint a fused optimiser leaves
    <save_prefix>.epoch<e>.optim = {optimizer: state_dict(), step, epoch, best_gt_f1}, written behind the epoch's decay, so it holds the
    rate the next epoch runs with.  To resume behind epoch e: trainer from <save_prefix>.epoch<e>.chkpt,
    optimizer.load_state_dict(ck["optimizer"], ck["step"], ck["epoch"]) with ck = torch.load of that .optim, start_epoch = e + 1; the best
    F1 so far is read from the same file when it is there."""
    import os
    import torch
    import torch.distributed as tdist
    from . import evaluate
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("fit_haplotype under a process group of more than one rank (training is not sharded)")
    if optimizer is None:
        optimizer = DeviceOptimizer(trainer, kind="LookaheadAdam", lr=1e-5 * (0.1 if finetune else 1.0), weight_decay=1e-4)
    elif finetune:
        raise ValueError("finetune scales the rate of the default optimizer; an optimizer of the caller's carries its own")
    fused = isinstance(optimizer, DeviceOptimizer)
    best = 0.0
    if save_prefix is not None and int(start_epoch) > 0 and os.path.exists(f"{save_prefix}.epoch{int(start_epoch) - 1}.optim"):
        best = float(torch.load(f"{save_prefix}.epoch{int(start_epoch) - 1}.optim").get("best_gt_f1", 0.0))
    out, model = [], None
    for epoch in range(int(start_epoch), int(epochs)):
        if fused:
            optimizer.epoch()
        lr = optimizer.lr if fused else optimizer.param_groups[0]["lr"]
        res = train_haplotype_bins(trainer, bin_paths, reference, optimizer=optimizer, batch_size=batch_size, dropout=dropout,
                                   max_grad_norm=max_grad_norm, seed=int(seed) + epoch, pass_sites=pass_sites, pn_value=pn_value)
        res.update(epoch=epoch, lr=lr, global_step=optimizer.global_step if fused else None, eval=None, checkpoint=None, best_checkpoint=None,
                   stopped=False)
        if validating_paths is not None:
            model = trainer.to_model(model)
            res["eval"] = evaluate.evaluate_haplotype_bins(model, validating_paths, reference, batch_size=batch_size, pass_sites=pass_sites)
            if res["eval"]["gt_f1"] >= best:
                best = float(res["eval"]["gt_f1"])
                if save_prefix is not None:
                    res["best_checkpoint"] = f"{save_prefix}.chkpt"
                    trainer.save_checkpoint(res["best_checkpoint"])
        if save_prefix is not None:
            res["checkpoint"] = f"{save_prefix}.epoch{epoch}.chkpt"
            trainer.save_checkpoint(res["checkpoint"])
        if epoch >= int(begin_to_adjust_lr):
            if fused:
                optimizer.decay_lr(decay_ratio)
            else:
                for g in optimizer.param_groups:
                    g["lr"] *= float(decay_ratio)
            res["stopped"] = (optimizer.lr if fused else optimizer.param_groups[0]["lr"]) < float(min_lr)
        if save_prefix is not None and fused:
            torch.save({"optimizer": optimizer.state_dict(), "step": optimizer.global_step, "epoch": optimizer.current_epoch, "best_gt_f1": best},
                       f"{save_prefix}.epoch{epoch}.optim")
        out.append(res)
        if res["stopped"]:
            break
    return out
