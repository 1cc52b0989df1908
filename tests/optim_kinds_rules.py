"""The remaining optimiser types of the reference's build_optimizer (PileupModel/optim.py:42-104), restated in float64 numpy for the tests of
nsnp_optim_step_kind and of the kinds "Novograd", "LookaheadNovograd", "sgd", "adadelta" of nanosnp_amd.train.DeviceOptimizer.  Test
infrastructure, written from the published rules; the clip, the Lookahead wrapper, the tensors, the step count, the recorded steps, the
bound and the fixture's byte planes are tests/optim_rules.py's -

    Novograd              PileupModel/novograd.py:197-221 (amsgrad and grad_averaging off): per TENSOR n = sum g^2 of the clipped gradient;
                          v = n if v == 0 else b2 v + (1 - b2) n - the test is made at every step;  g = g / (sqrt(v) + eps);  g += wd p;
                          m = b1 m + g;  p -= lr m.  No bias correction.
    torch.optim.SGD       dampening 0: g += wd p;  buf = g at the first step, mu buf + g later;  g = g + mu buf (nesterov) or buf;  p -= lr g
    torch.optim.Adadelta  g += wd p;  sq = rho sq + (1 - rho) g^2;  delta = sqrt(acc + eps) / sqrt(sq + eps) g;
                          acc = rho acc + (1 - rho) delta^2;  p -= lr delta

The fixture tests/golden/pileup_optim_kinds.npz (make_golden_optim_kinds.py) holds what the reference's own novograd.py / lookahead.py and
torch's SGD / Adadelta computed in fp32 on the cases listed here; load_fixture() reads it back.  In both Novograd cases the gradients of
tensor ZERO_TENSOR (21 floats) are all zero at steps 1 and 2: its v is still 0 after step 2 and it takes the copy branch at step 3, when
its neighbours are on the averaging branch."""
from __future__ import annotations

import math
import os
import zlib

import numpy as np

from tests import optim_rules
from tests.optim_rules import RECORD, SHAPES, SIZES, STEPS, TOTAL, case_grads, join, split, unpack

CASES = {
    "novograd_plain": dict(kind="Novograd", lr=1e-3, weight_decay=0.0, alpha=0.5, k=6, max_norm=20.0),
    "la_novograd_wd": dict(kind="LookaheadNovograd", lr=1e-2, weight_decay=1e-4, alpha=0.5, k=6, max_norm=2.0),
    "sgd_nesterov": dict(kind="sgd", lr=1e-2, weight_decay=1e-4, momentum=0.9, nesterov=True, max_norm=20.0),
    "sgd_plain": dict(kind="sgd", lr=1e-2, weight_decay=0.0, momentum=0.0, nesterov=False, max_norm=None),
    "adadelta_wd": dict(kind="adadelta", lr=1.0, weight_decay=1e-4, max_norm=2.0),
}
RULE = {"Novograd": "novograd", "LookaheadNovograd": "novograd", "sgd": "sgd", "adadelta": "adadelta"}
STATES = {"novograd": ("exp_avg",), "sgd": ("momentum_buffer",), "adadelta": ("square_avg", "acc_delta")}     # per element, torch's names
ZERO_TENSOR, ZERO_STEPS = SIZES.index(21), (1, 2)
BETAS, NOVOGRAD_EPS = (0.9, 0.999), 1e-8                     # optim.py:85-96
RHO, ADADELTA_EPS = 0.9, 1e-6                                # torch's defaults: the shipped yamls give the adadelta type neither


def optimizer_kwargs(cfg):
    """what a case passes to nanosnp_amd.train.DeviceOptimizer"""
    return {k: v for k, v in cfg.items() if k != "max_norm"}


def zero_the_tensor(grads):
    """a case's gradients [STEPS, TOTAL] with tensor ZERO_TENSOR zeroed at ZERO_STEPS (a copy)"""
    out = np.array(grads, np.float32)
    o = sum(SIZES[:ZERO_TENSOR])
    for s in ZERO_STEPS:
        out[s - 1, o:o + SIZES[ZERO_TENSOR]] = 0.0
    return out


class KindRules:
    """one optimiser over a list of float64 arrays; a, b: the per-element states in the order of STATES, v: Novograd's scalar per tensor"""

    def __init__(self, params, kind, lr, weight_decay=0.0, betas=BETAS, eps=None, momentum=0.0, nesterov=False, rho=RHO, alpha=0.5, k=6,
                 lookahead=None):
        self.rule = RULE[kind]
        self.lookahead = kind.startswith("Lookahead") if lookahead is None else bool(lookahead)
        self.p = [np.array(a, np.float64) for a in params]
        self.a = [np.zeros_like(a) for a in self.p]
        self.b = [np.zeros_like(a) for a in self.p]
        self.v = np.zeros(len(self.p))
        self.slow = None
        self.lr, self.wd, self.betas = float(lr), float(weight_decay), betas
        self.eps = float(eps) if eps is not None else (ADADELTA_EPS if self.rule == "adadelta" else NOVOGRAD_EPS)
        self.mu, self.nesterov, self.rho, self.alpha, self.k = float(momentum), bool(nesterov), float(rho), float(alpha), int(k)
        self.t = 0

    def step(self, grads, max_norm=None):
        """-> the norm of the gradients before clipping"""
        g = [np.array(a, np.float64) for a in grads]
        norm = math.sqrt(sum(float((a * a).sum()) for a in g))
        if max_norm is not None and max_norm > 0:
            c = min(1.0, max_norm / (norm + 1e-6))
            g = [a * c for a in g]
        self.t += 1
        for i in range(len(self.p)):
            x = g[i]
            if self.rule == "novograd":
                n = float((x * x).sum())
                self.v[i] = n if self.v[i] == 0 else self.betas[1] * self.v[i] + (1 - self.betas[1]) * n
                x = x / (math.sqrt(self.v[i]) + self.eps)
                if self.wd != 0:
                    x = x + self.wd * self.p[i]
                self.a[i] = self.betas[0] * self.a[i] + x
                self.p[i] = self.p[i] - self.lr * self.a[i]
                continue
            if self.wd != 0:
                x = x + self.wd * self.p[i]
            if self.rule == "sgd":
                if self.mu != 0:
                    self.a[i] = x.copy() if self.t == 1 else self.mu * self.a[i] + x
                    x = x + self.mu * self.a[i] if self.nesterov else self.a[i]
                self.p[i] = self.p[i] - self.lr * x
            else:
                self.a[i] = self.rho * self.a[i] + (1 - self.rho) * x * x
                delta = np.sqrt(self.b[i] + self.eps) / np.sqrt(self.a[i] + self.eps) * x
                self.b[i] = self.rho * self.b[i] + (1 - self.rho) * delta * delta
                self.p[i] = self.p[i] - self.lr * delta
        if self.lookahead and self.t % self.k == 0:
            if self.slow is None:
                self.slow = [a.copy() for a in self.p]
            for i in range(len(self.p)):
                self.slow[i] = self.slow[i] + self.alpha * (self.p[i] - self.slow[i])
                self.p[i] = self.slow[i].copy()
        return norm


def run(case, p0, grads, lookahead=None):
    """the float64 trajectory of a case -> dict(p={step: flat}, a, b (flat; what the kind does not use stays 0), v [8], v_at={step: [8]}
    (Novograd), slow (flat or None), norm [STEPS])"""
    cfg = CASES[case]
    r = KindRules(split(p0), lookahead=lookahead, **optimizer_kwargs(cfg))
    out = dict(p={}, v_at={}, norm=np.zeros(STEPS))
    for s in range(1, STEPS + 1):
        out["norm"][s - 1] = r.step(split(grads[s - 1]), cfg["max_norm"])
        out["v_at"][s] = r.v.copy()
        if s in RECORD:
            out["p"][s] = join(r.p)
    out["a"], out["b"], out["v"], out["slow"] = join(r.a), join(r.b), r.v.copy(), None if r.slow is None else join(r.slow)
    return out


def shared_crc(p0, base):
    return zlib.crc32(np.ascontiguousarray(base, np.float32).tobytes(), zlib.crc32(np.ascontiguousarray(p0, np.float32).tobytes()))


def load_fixture(path=None):
    """-> dict(p0 [TOTAL], base [STEPS, TOTAL], cases={name: dict(grads [STEPS, TOTAL], p {step: flat}, a, b (flat or None), v ([8] or None),
    v_at {2: [8], 3: [8]} (Novograd), slow or None, norm [STEPS], ref_abs_max dict(p, a, b, slow), ref_v_rel, ref_norm_rel)})"""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pileup_optim_kinds.npz")
    z = np.load(path)
    shared = optim_rules.load_fixture()                   # p0 and the base gradients are stored in pileup_optim.npz only
    assert tuple(z["record"].tolist()) == RECORD and tuple(z["sizes"].tolist()) == SIZES
    assert int(z["shared_crc"]) == shared_crc(shared["p0"], shared["base"]), "pileup_optim.npz is not the one this fixture was made with"
    out = dict(p0=shared["p0"], base=shared["base"], cases={})
    for name, cfg in CASES.items():
        ps = unpack(z[f"{name}_p"], (len(RECORD), TOTAL))
        ram = z[f"{name}_ref_abs_max"]
        novo = RULE[cfg["kind"]] == "novograd"
        grads = case_grads(out["base"], z[f"{name}_grad_scale"])
        get = lambda key: unpack(z[f"{name}_{key}"], (TOTAL,)) if f"{name}_{key}" in z.files else None
        out["cases"][name] = dict(
            grads=zero_the_tensor(grads) if novo else grads, p={s: ps[j] for j, s in enumerate(RECORD)}, a=get("a"), b=get("b"), slow=get("slow"),
            v=z[f"{name}_v"] if novo else None, v_at={2: z[f"{name}_v2"], 3: z[f"{name}_v3"]} if novo else None, norm=z[f"{name}_norm"],
            ref_abs_max=dict(p=float(ram[0]), a=float(ram[1]), b=float(ram[2]), slow=float(ram[3])),
            ref_v_rel=float(z[f"{name}_ref_v_rel"]) if novo else 0.0, ref_norm_rel=float(z[f"{name}_ref_norm_rel"]))
    return out
