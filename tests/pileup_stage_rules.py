"""The PileupModel forward (PileupModel/model.py:31-39, 66-73, 97-119; predict.py:49-51) restated as THREE plain torch operations, one per
launch of the GPU forward, from the 24 raw state-dict tensors and the four indel-head tensors.  Test infrastructure:
tests/test_pileup_stage_rules.py ties these rules to tests/eval_rules.py, the oracle and the reference-written goldens (the stages chained
in float64 reproduce all of them), tests/test_gpu_pileup_stages.py holds every launch of nsnp_pileup_forward - in the three arithmetics
and under every kernel option - to its one stage, applied to the GPU's own input of that stage (Context.pileup_forward_stage), so that
errors do not compound.

    layer0(w, x)            x [N,33,18] integer counts -> h of layer 0, all 33 steps of both directions      [N,33,128]  ("h0")
    layer1_centre(w, h0)    h0 [N,33,128] -> h of layer 1 at position 16: 17 steps per direction, forward steps 0..16 and
                            backward steps 32..16 (only position 16 is consumed, model.py:68)                  [N,128]     ("h1c")
    heads(w, h1c)           output_proj, tanh(dense), the four heads -> (90 logits, softmax gt [N,21], softmax zy [N,3]); rows 0-20 gt,
                            21-23 zy, 24-56 indel1, 57-89 indel2 as tests/eval_rules.forward_logits_f64

Every function computes in the dtype of the weights it is handed (weights_as(..., torch.float64 / torch.float32)), which is how the
float32 yardstick is the same code as the float64 reference.  The counts enter as predict.py:49 hands them to the model: int -> float32
(exact up to 2^24; 2^24 + 3 becomes 2^24 + 4 for the reference exactly as for every kernel), then the dtype of the weights.

The bound is the project's rule for recurrent stages, tests/cat_stage_rules.recurrent_bound: no bound is derivable through 33 recurrent
steps of approximated exponentials, so the yardstick is the reference side - the same stage in float32 torch on the CPU stands
d32 = max |stage32 - stage64| from float64 on the same inputs, the GPU may stand 8 d32 + 2^-23 from float64 in fp32 and bf16x3, six times
that in f16x3.  With the shipped ont_pileup weights on the 256 golden inputs d32 is 3.6e-6 on h0 (bound 2.9e-5, 1.7e-4 in f16x3) and
7.8e-7 on h1c from the float32 h0 (6.3e-6).

emulate_layer0 restates layer 0 with the operand formats of the two split arithmetics (gate rows scaled by log2 e, the g gate by
2 log2 e, in float32 as the weight packers scale them, then split into bf16 planes or an fp16 pair - the sign of the factor does not
matter to a split) and lets a named low-order part be LOST:
the cases tests/test_pileup_stage_rules.py holds against the bound, so that the bound is known to see the loss of one operand part."""
from __future__ import annotations

import numpy as np
import torch

from tests.cat_stage_rules import bf16_planes, recurrent_bound  # noqa: F401  (recurrent_bound: the bound of every stage here)
from tests.test_gpu_l0_prestage import SPLIT_COUNTS, _counts as _prestage_counts

T = 33
H = 64
CENTER = 16
STEPS1 = CENTER + 1
LOG2E = np.float32(1.4426950408889634)
SITE_COUNTS = (1, 17, 65, 129)          # and all of stage_inputs: site_count_properties() states why
STAGES = ("h0", "h1c", "heads")

# SPLIT_COUNTS, (site, column, channel, count), is that of tests/test_gpu_l0_prestage.py (imported above, so the two cannot drift):
# counts beyond +-256 at columns 0, 1, 16, 31 and 32 in the first and the third 16-site group of a 48-site block, the second group
# within +-256.  257 / -257 need two bf16 terms, 65,536 is one bf16 beyond +-256, 65,793 needs three terms, 2^24 + 3 casts to the
# float 2^24 + 4
SPLIT_BASE = 256                         # the 48-site block starts on a 16-site tile, so the counts keep their tile positions


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def weights_as(weights, indel, dtype):
    """the 24 tensors of nsnp_pileup_load_weights + indel1 weight / bias, indel2 weight / bias -> 28 torch tensors of dtype"""
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32))).to(dtype) for t in list(weights)[:24] + list(indel)]


# ---- the stages ---------------------------------------------------------------------------------------------------------------------
def _cell(z, c):
    i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
    c = f * c + i * g
    return o * torch.tanh(c), c


def _direction(x, wih, whh, b, order, h_feed=None):
    """one direction of an nn.LSTM layer over the columns `order` of x [N,T,I] (gate order i, f, g, o) -> {column: h [N,64]};
    h_feed: what the recurrent product reads of h (emulations only)"""
    N = x.shape[0]
    h = torch.zeros((N, H), dtype=wih.dtype); c = torch.zeros((N, H), dtype=wih.dtype)
    out = {}
    for t in order:
        z = x[:, t] @ wih.T + (h if h_feed is None else h_feed(h)) @ whh.T + b
        h, c = _cell(z, c)
        out[t] = h
    return out


def counts_as(x, dtype):
    """predict.py:49: the integer counts as a FloatTensor, then the dtype of the stage"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.float32))).to(dtype)


def layer0(w, x):
    dt = w[0].dtype
    xs = counts_as(x, dt)
    out = torch.zeros((xs.shape[0], T, 2 * H), dtype=dt)
    for d in range(2):
        hs = _direction(xs, w[4 * d], w[4 * d + 1], w[4 * d + 2] + w[4 * d + 3], range(T - 1, -1, -1) if d else range(T))
        for t, h in hs.items():
            out[:, t, d * H:(d + 1) * H] = h
    return out


def layer1_centre(w, h0):
    dt = w[0].dtype
    h0 = h0.to(dt)
    halves = []
    for d in range(2):
        order = range(T - 1, CENTER - 1, -1) if d else range(STEPS1)
        halves.append(_direction(h0, w[8 + 4 * d], w[9 + 4 * d], w[10 + 4 * d] + w[11 + 4 * d], order)[CENTER])
    return torch.cat(halves, 1)


def heads(w, h1c):
    enc = h1c.to(w[0].dtype) @ w[16].T + w[17]
    mid = torch.tanh(enc @ w[18].T + w[19])
    logits = torch.cat([mid @ w[20].T + w[21], mid @ w[22].T + w[23], mid @ w[24].T + w[25], mid @ w[26].T + w[27]], 1)
    return logits, torch.softmax(logits[:, :21], 1), torch.softmax(logits[:, 21:24], 1)


def chain(w, x):
    """every stage from the counts, each fed by the previous one's result in the dtype of w -> dict"""
    h0 = layer0(w, x)
    h1c = layer1_centre(w, h0)
    logits, gt, zy = heads(w, h1c)
    return {"h0": h0, "h1c": h1c, "logits": logits, "gt": gt, "zy": zy}


def dist(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- emulation of layer 0 in the split arithmetics ----------------------------------------------------------------------------------
def _scaled(w32):
    """[256,K] float32 rows as nsnp_pileup_pack_weights scales them: -log2 e for the gates i, f, o, -2 log2 e for g, in float32"""
    f = np.full((4 * H, 1), -LOG2E, np.float32)
    f[2 * H:3 * H] = np.float32(-2.0) * LOG2E
    return (f * np.asarray(w32, np.float32)).astype(np.float32), f.astype(np.float64)


def _f16_pair(v):
    with np.errstate(over="ignore", invalid="ignore"):           # (beyond 65504 the hi half is inf: such a value is no pair)
        hi = v.astype(np.float16).astype(np.float32)
        return hi, (v - hi).astype(np.float16).astype(np.float32)


def emulate_layer0(weights, x, prec, lost=None):
    """layer 0 in float64 on operands as arithmetic prec holds them.  prec 2 (bf16x3): W_ih, W_hh as the sum of their three bf16 planes,
    h as the sum of its three planes (exact).  prec 1 (f16x3): W_ih, W_hh and the h the recurrent product reads as fp16 pairs hi + lo.
    lost: None, or the low-order part that is dropped - "wih_p2" / "whh_p2" (the third bf16 plane of a weight), "h_lo" / "whh_lo" (the
    low half of the exchanged h / of W_hh).  Products and sums stay float64: what is measured is the operand loss alone."""
    assert prec in (1, 2) and lost in (None, "wih_p2", "whh_p2", "h_lo", "whh_lo")
    assert lost is None or (lost.endswith("p2") if prec == 2 else lost.endswith("lo"))

    def operand(w32, drop):
        ws, f = _scaled(w32)
        if prec == 2:
            p0, p1, p2 = bf16_planes(ws)
            v = p0.astype(np.float64) + p1 + (0 if drop else p2.astype(np.float64))
        else:
            hi, lo = _f16_pair(ws)
            v = hi.astype(np.float64) + (0 if drop else lo.astype(np.float64))
        return torch.from_numpy(v / f)

    def h_feed(h):
        if prec == 2:
            return h                                             # three planes of a float32 h are exact
        hi, lo = _f16_pair(h.numpy().astype(np.float32))
        return torch.from_numpy(hi.astype(np.float64) + (0 if lost == "h_lo" else lo.astype(np.float64)))

    w64 = [torch.from_numpy(np.asarray(t, np.float64)) for t in weights[:8]]
    xs = counts_as(x, torch.float64)
    out = torch.zeros((xs.shape[0], T, 2 * H), dtype=torch.float64)
    for d in range(2):
        wih = operand(weights[4 * d], lost == "wih_p2")
        whh = operand(weights[4 * d + 1], lost in ("whh_p2", "whh_lo"))
        hs = _direction(xs, wih, whh, w64[4 * d + 2] + w64[4 * d + 3], range(T - 1, -1, -1) if d else range(T), h_feed)
        for t, h in hs.items():
            out[:, t, d * H:(d + 1) * H] = h
    return out


# ---- inputs and site counts ---------------------------------------------------------------------------------------------------------
def crafted_sites():
    """the eight sites `xe` of test_f16x3_precision_mode: zeros, depth-144 saturation, large and deep counts (> 2048: the fp16 hi part
    alone is no longer exact) - every count the sum of an fp16 pair"""
    xe = np.zeros((8, T, 18), np.int32)
    xe[1] = 144; xe[2] = -144; xe[3, :, ::2] = 10000; xe[4, 16] = -60000; xe[5, ::3] = 4099; xe[6] = 2049; xe[7, :, 1] = 33001
    return xe


def split_sites():
    x = _prestage_counts(2460, (48, T, 18))                    # the block of test_split_counts_take_the_general_loop
    for site, t, ch, v in SPLIT_COUNTS:
        x[site, t, ch] = v
    return x


def fp16_pair_exact(x):
    v = np.asarray(x, np.float32)
    hi, lo = _f16_pair(v)
    with np.errstate(invalid="ignore"):
        return bool(np.all(hi.astype(np.float64) + lo == v))


def stage_inputs(prec):
    """int32 [N,33,18] of the stage tests in arithmetic prec: the 256 golden sites; in fp32 and bf16x3 the 48 split-count sites, on a
    tile boundary (f16x3 carries two fp16 halves of a count: 65,793 and 2^24 + 3 are beyond them); the eight crafted sites.
    N = 312 (264 in f16x3): the last 16-site tile is half full"""
    from tests.helpers import golden
    parts = [np.load(golden("pileup_fwd.npz"))["x"].astype(np.int32)]
    assert parts[0].shape[0] == SPLIT_BASE
    if prec != 1:
        parts.append(split_sites())
    parts.append(crafted_sites())
    return np.ascontiguousarray(np.concatenate(parts))


def site_counts(prec):
    """largest first: what the largest run leaves in the workspace lies behind every smaller one"""
    n_all = stage_inputs(prec).shape[0]
    return (n_all,) + tuple(sorted(SITE_COUNTS, reverse=True))


def site_count_properties(counts):
    """what the site counts of the GPU file must offer -> dict of booleans (tests/test_pileup_stage_rules.py asserts every one)"""
    return {
        "one_partly_filled_tile": 1 in counts,
        "second_tile_partial_and_partial_group_of_two": any(16 < n < 32 for n in counts),
        "crosses_64_site_workgroup_and_padding": any(64 < n < 80 for n in counts),
        "crosses_128_site_workgroup": any(128 < n < 144 for n in counts),
        "all_sites_with_a_partial_last_tile": max(counts) % 16 != 0 and max(counts) > 256,
    }
