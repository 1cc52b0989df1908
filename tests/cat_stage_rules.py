"""Every stage of the legacy CatModel forward (HaplotypeModel/model.py:332-358, crnn.py:84-190) restated as ONE plain torch
operation each, from the raw 132 state-dict tensors, BatchNorm unfolded (eval mode) as crnn.py and oracle/cat_forward_oracle.c
apply it.  Test infrastructure: tests/test_cat_stage_rules.py ties these rules to the oracle and the reference-written goldens (the
stages chained in float64 reproduce both), tests/test_gpu_cat_stages.py holds every GPU launch of nsnp_cat_forward to its one stage,
applied to the GPU's own input of that stage (Context.cat_forward_stage), so that errors do not compound.

A stage is (names of its input stages, function(weights, *inputs)).  Every function computes in the dtype of the weights it is
handed (weights64 / weights32), which is how the float32 yardstick of the recurrent stages is the same code as the float64 one.

Stage images (include/nanosnp.h, nsnp_cat_forward_stage):
    maps [N,C,H,W]; sequences [T,N,F]; an LSTM's h [T,N,512] = [h_fwd ; h_bwd]; a six-step layer [6,N,512]: row s = [h_fwd(column s) ;
    h_bwd(column 10 - s)] - the steps that ran, row 5 = column 5.

-----------------------------------------------------------------------------------------------------------------------------------
Bounds of a convolution stage (conv_bound).  u = 2^-24 (unit roundoff of fp32), K = 9 C_in (+ C_shortcut) products per output,
w' = s w and b' the BatchNorm-folded weight and bias (s = gamma / sqrt(var + eps)), A = conv(|x|, |w'|) + |b'|, S = conv(|x|, 1).

fp32     The kernel computes b' + sum_k w'_k x_k into an fp32 accumulator whose every partial sum is bounded by A, so every rounding
         of the accumulator is at most u A.  It is rounded once per matrix instruction, and an instruction adds at least two products
         (v_mfma_f32_32x32x2_f32; 8 per 16-channel chunk and tap, the channels padded from 10 to 16 in block 0 only): fewer than K
         roundings in any order, K u A.  The fold computes w' in fp32 from var + eps, a square root, a division and a product: four
         roundings, 4 u |w' x| per product, 4 u A in sum.  ReLU is 1-Lipschitz and exact.      |got - ref64| <= (K + 4) u A
bf16x3   Operands are split p0 + p1 + p2 with p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1): |p1| <= 2^-9 |v|,
         |p2| <= 2^-18 |v|, residue |v - p0 - p1 - p2| <= 2^-27 |v|.  Six of the nine plane products are taken, each exact in fp32.
         Dropped are p1 p2, p2 p1 (2^-27 |w x| each) and p2 p2 (2^-36); with the two residues (2^-27 |w x| each) that is
         4 x 2^-27 + 2^-36 < u |w x| per product, but each of the four is bounded separately by "about 2^-24 |w x|" in the coarser
         count used here: 4 u A.  The accumulator is rounded once per v_mfma_f32_32x32x16_bf16, six per 16 products: again fewer
         than K roundings, K u A.  With the fold's 4 u A:                                    |got - ref64| <= (K + 8) u A
f16x3    Operands are (hi, lo) = (fp16(v), fp16(v - hi)).  While lo is a normal fp16 number the pair carries v to 2^-22 |v|; fp16
         spacing ends at 2^-24, so below |v| ~ 2^-2 ... 2^-14 the low half is subnormal or zero and the pair is off by up to 2^-25
         absolutely: |w' - pair(w')| <= max(2^-22 |w'|, 2^-25).  Inputs are pairs already (the previous launch stored them so; the
         tapped image is their decoded value, and re-splitting a decoded pair returns it).
           weights   sum_k |x_k| max(2^-22 |w'_k|, 2^-25) <= 2^-22 A + 2^-25 S
           lo . lo   the dropped product: |w_lo| <= 2^-11 |w'|, |x_lo| <= 2^-11 |x|: 2^-22 A
                     (together 2^-21 A + 2^-25 S)
           sums      hi.hi, lo.hi, hi.lo are exact in fp32 and enter the fp32 accumulator as in the fp32 case: (K + 4) u A with the fold
           output    stored as a pair: max(2^-22 |ref|, 2^-25)
                                  |got - ref64| <= (K + 4) u A + 2^-21 A + 2^-25 S + max(2^-22 |ref|, 2^-25)

Recurrent stages, Linears and the head (recurrent_bound): no bound is derivable through eleven recurrent steps of approximated
exponentials.  The yardstick is the reference side: the same stage in float32 torch on the CPU stands d32 = max |stage32 - stage64|
from float64 on the same inputs; the GPU may stand 8 d32 + 2^-23 from float64 in fp32 and bf16x3 (8: another summation order over up
to 768 products), and six times that in f16x3 - the ratio tests/test_gpu_hap_tile_kernels.py records for this GEMM between the two
arithmetics (1.42e-5 / 2.83e-6 = 5.02), rounded up."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

CH = (10, 32, 64, 128, 128, 256, 256)
POOL = (2, 2, 0, 3, 0, 2)              # pool height after block i (crnn.py:134-160), width 3, padding (0, 1)
HS = (40, 20, 10, 10, 3, 3)            # map height at block i
L = 11
NH = 256
CENTER = 5
EPS = 1e-5
U = 2.0 ** -24

SEED = 21                              # seeded_cat_weights(SEED): the weights of the goldens
SITE_COUNTS = (1, 3, 5, 129)           # site_count_properties() states why
BIG_N = 129
BIG_SITES = (0, 1, 63, 64, 127, 128)   # the sites of BIG_N that are compared: both ends of both site tiles and the middle
INPUT_SEED = 3800                      # stage_inputs(N) = synth_cat_groups(INPUT_SEED + N, N), then the crafted rows
F16_OVER_FP32 = 6                      # ceil(1.42e-5 / 2.83e-6)


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def weights_as(ws, dtype):
    return [torch.from_numpy(np.ascontiguousarray(w)).to(dtype) for w in ws]


def _blk(w, i):
    return w[14 * i:14 * i + 14]


# ---- the stages ---------------------------------------------------------------------------------------------------------------------
def pack(w, g0, g1):
    """torch.cat((g0.permute(0,3,1,2), g1.permute(0,3,1,2)), 1): channel = group * 5 + plane (model.py:333-336,352)"""
    return torch.cat((g0.permute(0, 3, 1, 2), g1.permute(0, 3, 1, 2)), 1).to(w[0].dtype)


def percentage(w, g0, g1):
    """calculate_percentage (model.py:186-194) per (group, tag): shares of A, C, G, T, deletion among the tag's 20 rows that are not padding;
    torch evaluates int64 / (int64 + 1e-9) in FLOAT32 (oracle/cat_forward_oracle.c), so the rule is float32 whatever the dtype -> [11,N,20]"""
    feats = []
    for g in (g0, g1):
        base = g[..., 0]
        for tag in range(2):
            b = base[:, 20 * tag:20 * tag + 20]                                   # [N,20,11]
            den = (b != -2).sum(1).to(torch.float32) + torch.tensor(1e-9, dtype=torch.float32)
            for code in (1, 2, 3, 4, -1):
                feats.append((b == code).sum(1).to(torch.float32) / den)         # [N,11]
    return torch.stack(feats, -1).permute(1, 0, 2).contiguous()


def _bn(x, q, k):
    return (x - q[k + 2][None, :, None, None]) / torch.sqrt(q[k + 3] + EPS)[None, :, None, None] * q[k][None, :, None, None] + q[k + 1][None, :, None, None]


def conv_bn_relu(w, i, x):
    """ResBlock i, first half: relu(bn1(conv1(x))) (crnn.py:92-101)"""
    q = _blk(w, i)
    return torch.relu(_bn(F.conv2d(x.to(q[0].dtype), q[0], q[1], padding=1), q, 2))


def conv_bn_shortcut_relu(w, i, y, x):
    """ResBlock i, second half: relu(bn2(conv2(y)) + shortcut(x)), the shortcut a 1x1 convolution (crnn.py:102-115)"""
    q = _blk(w, i)
    dt = q[0].dtype
    return torch.relu(_bn(F.conv2d(y.to(dt), q[6], q[7], padding=1), q, 8) + F.conv2d(x.to(dt), q[12], q[13]))


def maxpool(x, kh):
    """nn.MaxPool2d((kh, 3), (kh, 1), (0, 1)): rows beyond the last whole window are dropped (10 -> 3, 3 -> 1)"""
    return F.max_pool2d(x, (kh, 3), (kh, 1), (0, 1))


def to_sequence(m):
    """[N,256,1,11] -> [11,N,256] (crnn.py:184-185)"""
    assert m.shape[2] == 1
    return m[:, :, 0, :].permute(2, 0, 1).contiguous()


def bilstm(q8, x, steps):
    """one bidirectional nn.LSTM layer on x [11,N,I]; q8 = (w_ih, w_hh, b_ih, b_hh) forward then reverse; gate order i, f, g, o.
    steps = 11 -> [11,N,512]; steps = 6 -> [6,N,512], row s = [h_fwd(column s) ; h_bwd(column 10 - s)]"""
    dt = q8[0].dtype
    x = x.to(dt)
    T, N = x.shape[0], x.shape[1]
    out = torch.zeros((steps, N, 2 * NH), dtype=dt)
    for d in range(2):
        wih, whh, b = q8[4 * d], q8[4 * d + 1], q8[4 * d + 2] + q8[4 * d + 3]
        h = torch.zeros((N, NH), dtype=dt); c = torch.zeros((N, NH), dtype=dt)
        for s in range(steps):
            t = T - 1 - s if d else s
            z = x[t] @ wih.T + h @ whh.T + b
            i, f, g, o = torch.sigmoid(z[:, :NH]), torch.sigmoid(z[:, NH:2 * NH]), torch.tanh(z[:, 2 * NH:3 * NH]), torch.sigmoid(z[:, 3 * NH:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[s if steps < T else t, :, d * NH:(d + 1) * NH] = h
    return out


def linear(wt, b, x):
    return x.to(wt.dtype) @ wt.T + b


def head(w, v):
    """out_layer Linear(512 -> 10) + softmax (model.py:354-357)"""
    return torch.softmax(linear(w[130], w[131], v), 1)


def _block_input(i):
    if i == 0:
        return "pixels"
    return {1: "pool0", 2: "pool1", 3: "block2_out", 4: "pool3", 5: "block4_out"}[i]


def _stages():
    st = {"pixels": (("g0", "g1"), pack), "pct_features": (("g0", "g1"), percentage)}
    for i in range(6):
        st[f"block{i}_y"] = ((_block_input(i),), lambda w, x, i=i: conv_bn_relu(w, i, x))
        st[f"block{i}_out"] = ((f"block{i}_y", _block_input(i)), lambda w, y, x, i=i: conv_bn_shortcut_relu(w, i, y, x))
    for i in (0, 1, 3):
        st[f"pool{i}"] = ((f"block{i}_out",), lambda w, x, i=i: maxpool(x, POOL[i]))
    st["seq0"] = (("block5_out",), lambda w, x: to_sequence(maxpool(x, POOL[5])))
    for l in range(3):
        st[f"pct_h{l}"] = (("pct_features" if l == 0 else f"pct_h{l - 1}",),
                           lambda w, x, l=l: bilstm(w[104 + 8 * l:112 + 8 * l], x, CENTER + 1 if l == 2 else L))
    st["pct_linear"] = (("pct_h2",), lambda w, h: linear(w[128], w[129], h[CENTER]))
    st["rnn0_h"] = (("seq0",), lambda w, x: bilstm(w[84:92], x, L))
    st["rnn0_emb"] = (("rnn0_h",), lambda w, h: linear(w[92], w[93], h))
    st["rnn1_h"] = (("rnn0_emb",), lambda w, x: bilstm(w[94:102], x, CENTER + 1))
    st["cat"] = (("pct_linear", "rnn1_h"), lambda w, p, h: torch.cat((p.to(w[0].dtype), linear(w[102], w[103], h[CENTER])), 1))
    st["prob"] = (("cat",), head)
    return st


STAGES = _stages()
ORDER = (["pct_features", "pct_h0", "pct_h1", "pct_h2", "pct_linear", "pixels"] +
         [s for i in range(6) for s in ([f"block{i}_y", f"block{i}_out"] + ([f"pool{i}"] if i in (0, 1, 3) else []))] +
         ["seq0", "rnn0_h", "rnn0_emb", "rnn1_h", "cat", "prob"])            # the order nsnp_cat_forward launches them in
CONV_STAGES = [s for i in range(6) for s in (f"block{i}_y", f"block{i}_out")]
POOL_STAGES = {"pool0": ("block0_out", 2), "pool1": ("block1_out", 2), "pool3": ("block3_out", 3), "seq0": ("block5_out", 2)}
RECURRENT_STAGES = ["pct_h0", "pct_h1", "pct_h2", "pct_linear", "rnn0_h", "rnn0_emb", "rnn1_h", "cat", "prob"]


def stage(name, w, inputs):
    """the stage's one operation on `inputs` (a dict of stage images, with g0 / g1 the raw groups)"""
    deps, fn = STAGES[name]
    return fn(w, *[inputs[d] for d in deps])


def chain(w, g0, g1):
    """every stage from the raw groups, each fed by the previous ones' results in the dtype of w -> dict"""
    out = {"g0": torch.as_tensor(g0), "g1": torch.as_tensor(g1)}
    for name in ORDER:
        out[name] = stage(name, w, out)
    return out


# ---- convolution magnitudes and bounds ----------------------------------------------------------------------------------------------
def conv_magnitude(w64, name, inputs):
    """(A, S, K) of a convolution stage on its inputs: A = conv(|x|, |w'|) + |b'| (+ the shortcut's products), S = conv(|x|, 1)
    (+ the shortcut's), K = 9 C_in (+ C_shortcut); w', b' the BatchNorm-folded weight and bias in float64"""
    i = int(name[5]); second = name.endswith("_out")
    q = _blk(w64, i)
    deps = STAGES[name][0]
    x = inputs[deps[0]].to(torch.float64).abs()
    k = 8 if second else 2
    s = q[k] / torch.sqrt(q[k + 3] + EPS)
    wf = (q[6 if second else 0] * s[:, None, None, None]).abs()
    bf = (q[7 if second else 1] - q[k + 2]) * s + q[k + 1]
    A = F.conv2d(x, wf, None, padding=1)
    S = F.conv2d(x, torch.ones_like(wf[:1]), None, padding=1).expand_as(A)
    K = 9 * x.shape[1]
    if second:
        xs = inputs[deps[1]].to(torch.float64).abs()
        A = A + F.conv2d(xs, q[12].abs())
        S = S + F.conv2d(xs, torch.ones_like(q[12][:1])).expand_as(A)
        bf = bf + q[13]
        K += xs.shape[1]
    return A + bf.abs()[None, :, None, None], S, K


def conv_bound(prec, A, S, K, ref):
    """elementwise bound on |got - ref64| of a convolution stage in arithmetic prec (0 fp32, 1 f16x3, 2 bf16x3): the module docstring"""
    if prec == 0:
        return (K + 4) * U * A
    if prec == 2:
        return (K + 8) * U * A
    return (K + 4) * U * A + 2.0 ** -21 * A + 2.0 ** -25 * S + torch.clamp(2.0 ** -22 * ref.abs(), min=2.0 ** -25)


def recurrent_bound(prec, d32):
    b = 8.0 * d32 + 2.0 ** -23
    return F16_OVER_FP32 * b if prec == 1 else b


# ---- storage formats ----------------------------------------------------------------------------------------------------------------
def f16_pair(v):
    """the value an f16x3 image holds for the float32 v: fp16(v) + fp16(v - fp16(v)) (hap_gemm.hpp split_h), as float32"""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    return hi + (v - hi).astype(np.float16).astype(np.float32)


def bf16(v):
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) & np.uint32(0xffff0000)).view(np.float32)


def bf16_planes(v):
    v = np.asarray(v, np.float32)
    p0 = bf16(v); r1 = v - p0; p1 = bf16(r1)
    return p0, p1, bf16(r1 - p1)


def stored(prec, v):
    """a float32 array as the activation image of arithmetic prec returns it"""
    return f16_pair(v) if prec == 1 else np.asarray(v, np.float32)


# ---- numpy emulation of the three convolution arithmetics ---------------------------------------------------------------------------
def emulate_conv(ws32, name, inputs, prec, rng):
    """The convolution stage as the kernels compute it, in numpy: BatchNorm folded in float32 as nsnp_cat_load_weights folds it, operands
    split as the packers split them (fp32: not at all), every partial product taken in float32, all of them added into a float32
    accumulator that starts at the bias, in a SHUFFLED order (the kernels' order is one of them), ReLU, the output stored as the
    arithmetic stores it.  inputs: float32 arrays as the previous stage stored them."""
    i = int(name[5]); second = name.endswith("_out")
    q = [np.asarray(t, np.float32) for t in ws32[14 * i:14 * i + 14]]
    k = 8 if second else 2
    s = q[k] / np.sqrt(q[k + 3] + np.float32(EPS))
    wf = (q[6 if second else 0] * s[:, None, None, None]).astype(np.float32)
    bf = ((q[7 if second else 1] - q[k + 2]) * s + q[k + 1]).astype(np.float32)
    deps = STAGES[name][0]
    x = torch.from_numpy(np.asarray(inputs[deps[0]], np.float32))
    N, C, H, W = x.shape
    cols = F.unfold(x, 3, padding=1).permute(0, 2, 1).reshape(N * H * W, C * 9).numpy()          # [pixels, C * 9], (channel, tap) order
    wmat = wf.reshape(wf.shape[0], C * 9)
    if second:
        xs = np.asarray(inputs[deps[1]], np.float32)
        cols = np.concatenate((cols, xs.transpose(0, 2, 3, 1).reshape(N * H * W, -1)), 1)
        wmat = np.concatenate((wmat, q[12].reshape(q[12].shape[0], -1)), 1)
        bf = (bf + q[13]).astype(np.float32)
    if prec == 0:
        terms = [(wmat, cols)]
    elif prec == 1:
        wh = wmat.astype(np.float16).astype(np.float32); wl = (wmat - wh).astype(np.float16).astype(np.float32)
        xh = cols.astype(np.float16).astype(np.float32); xl = (cols - xh).astype(np.float16).astype(np.float32)
        terms = [(wh, xh), (wl, xh), (wh, xl)]
    else:
        wp, xp = bf16_planes(wmat), bf16_planes(cols)
        terms = [(wp[a], xp[b]) for a, b in ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))]
    acc = np.broadcast_to(bf[None, :], (cols.shape[0], wmat.shape[0])).astype(np.float32).copy()
    order = [(t, kk) for t in range(len(terms)) for kk in range(cols.shape[1])]
    for j in rng.permutation(len(order)):
        t, kk = order[j]
        acc += terms[t][1][:, kk, None] * terms[t][0][None, :, kk]
    out = np.maximum(acc, np.float32(0)).reshape(N, H, W, -1).transpose(0, 3, 1, 2)
    return stored(prec, out)


# ---- inputs and site counts ---------------------------------------------------------------------------------------------------------
def stage_inputs(N):
    """g0, g1 [N,40,11,5] float32 of the stage tests: the synthetic generator, then crafted rows - site 0 of g0 loses every read of its first
    tag (a tag with no reads: 0 / 1e-9), the last site of g1 gets a second tag that holds every base code (0 not covered, -1 deletion, -2
    padding, 1..4) in known numbers"""
    from nanosnp_amd.fixtures import synth_cat_groups
    g0, g1 = synth_cat_groups(INPUT_SEED + N, N)
    g0[0, :20] = 0; g0[0, :20, :, 0] = -2
    codes = np.array([0, -1, -2, 1, 2, 3, 4, -1, 0, -2, 4, 4, 3, -2, -2, 1, -1, -1, 0, 2], np.float32)
    for x in range(L):
        g1[N - 1, 20:, x, 0] = np.roll(codes, x)
    g1[N - 1, 20:, :, 3] = g1[N - 1, 20:, :, 0] != -2
    return g0, g1


def pixel_tiles(N, H):
    return -(-N * H * L // 128)


def site_count_properties(counts=SITE_COUNTS):
    """what the site counts of the GPU file must offer -> dict of booleans (tests/test_cat_stage_rules.py asserts every one)
    - blocks 0 and 1 (<= 64 output channels) run two pixel tiles per workgroup (cat_conv_pix2): each must meet an even number of tiles
      (every workgroup full) and an odd one (the last workgroup holds one tile)
    - one count leaves the last tile partly filled at every resolution (heights 40, 20, 10, 3 and the site tiles of the sequences)
    - one count crosses the 128-site tile, and at it a pixel-tile boundary cuts an image row at every resolution"""
    p = {}
    for i in (0, 1):
        par = {pixel_tiles(n, HS[i]) % 2 for n in counts}
        p[f"block{i}_even_and_odd_tiles"] = par == {0, 1}
    p["partly_filled_everywhere"] = any(all(n * h * L % 128 for h in (40, 20, 10, 3)) and n % 128 for n in counts)
    p["crosses_site_tile"] = any(128 < n <= 256 for n in counts)
    p["tile_cuts_a_row"] = all(any((128 * t) % L for t in range(1, pixel_tiles(max(counts), h))) for h in (40, 20, 10, 3))
    p["big_sites_in_range"] = max(BIG_SITES) < BIG_N and BIG_N in counts
    return p


def dropped_rows_dominate(x, kh):
    """share of the pool's outputs whose 3-wide window, had it taken the rows that MaxPool2d((kh, 3), (kh, 1), (0, 1)) drops as well, would
    have held a larger value in its last output row: a pool that reads a dropped row shows there"""
    H = x.shape[2]
    Ho = H // kh
    if Ho * kh == H:
        return 0.0
    kept = maxpool(x, kh)[:, :, -1]
    tail = F.max_pool2d(x[:, :, Ho * kh:], (H - Ho * kh, 3), (1, 1), (0, 1))[:, :, 0]
    return float((tail > kept).double().mean())
