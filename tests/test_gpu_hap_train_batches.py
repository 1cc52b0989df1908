"""nsnp_hap_loss_grad and train.train_haplotype_bins on the paths tests/test_gpu_hap_train.py and tests/test_gpu_hap_train_bins.py leave
unvisited, against the float64 restatement tests/hap_grad_rules.py; the idiom is that of tests/test_gpu_train_batches.py, the helpers are
those of the two files.

  masks across chunks   keep masks with a reservation of 40 under N = 96: the four mask pointers move by base * (33 | 11) * 512 per chunk
  n below the tensors   n = 50 of 96 rows, masks of 96 rows, caller-owned site_loss and pred: nothing behind row 50 is touched, 1 / N is 1 / 50
  a side stream         the same bits as on the current stream
  one hot row           every feature zero but one (site, position) of each encoder, placed against the cuts of a weight-gradient slice
                        (HT_KCH = 128 rows of the (site, step) walk, forward and reverse): a lost or doubled row shows at 100 %
  deep features         features to 42,000, saturated gates, under the cells' libm activations
  edge dims             F = 128 and F = 1 (K of the layer-0 product), n_gt + n_zy = 16 (the last column of the logit row), a head of one class
  a dropout epoch       train_haplotype_bins with device-drawn masks, clip_grad_norm_, a torch optimiser and chunks inside the loop against a
                        float64 replay

Bounds.  Per tensor max |g_dev - g_f64| / max |g_f64| <= 4 x ref_rel_max of tests/golden/hap_grad.npz (1.35e-5), loss and site_loss within
1e-4, pred equal wherever the float64 margin is at least hap_eval_rules.MARGIN, at most MARGIN_SHARE of the sites nearer: check_parity of
tests/test_gpu_hap_train.py.  On inputs the fixture never measured (one hot row, deep features, edge dims) the bound per tensor is
max(that, 4 x the distance of the SAME restatement run in float32 torch on the CPU from float64), and that yardstick must itself stay at or
below 1e-4.  A tensor whose float64 gradient is exactly zero (the weight and bias of a head of one class) must be exactly zero on the
device.  The epoch: the bounds of test_one_epoch_follows_the_restatement.

Distances measured on an MI355X: docs/rounds/r33.md."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import hap_eval_rules as hr
from tests import hap_grad_rules as gr
from tests.helpers import seeded_hap_weights
from tests.test_gpu_hap_train import Harness, bound, check_parity
from tests.test_gpu_hap_train_bins import B, LR, PARITY, PASS, _params, _state, epoch_files  # noqa: F401
from tests.test_hap_eval_rules import file_features
from tests.test_hap_grad_rules import batch, seeded_masks, weights

pytestmark = pytest.mark.gpu
YARDSTICK_MAX = 1e-4
P_DROP = 0.1
SCALE = 1.0 / (1.0 - P_DROP)
MASK_SEED = 5                # 0 sites of the 96 within MARGIN under these masks (seeds 8, 9 and 11: 1 or 2)
# test_a_dropout_epoch_follows_the_float64_replay: between the gradient norms of its batches in the float64 replay.  The masks are the device
# generator's, so the replay's norms come from a run with a GPU.  Seed 7 without clipping: 548.1 656.2 1403.0 309.7 569.8 1105.6 393.2 1824.3
# 650.9 - nothing between 656 and 1106; clipped at 850: 548.1 656.2 1403.0 335.5 605.5 1199.7 451.5 1841.3 639.3, three batches clipped by
# factors 0.61, 0.71 and 0.46.  (The norms depend on the path: layer 0's W_ih moves by 0.3 of its largest entry in this epoch.  The first
# batch does not, and the third starts from two unclipped steps.)  The test asserts that one batch lies 5 % above and one 5 % below.
EPOCH_SEED = 7
CLIP = 850.0


@pytest.fixture(scope="module")
def small_harness():
    h = Harness(weights(), 32)
    yield h
    h.ctx.close()


def _dev(h, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(h.dev)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _exact_zeros(got, want):
    """rel_dist is undefined for a tensor whose float64 gradient is exactly zero: it must be exactly zero on the device, and both sides
    carry a unit in its place into check_parity -> (got, want, the indices of those tensors)"""
    g, w = list(got[0]), list(want["grads"])
    zero = [i for i, a in enumerate(w) if not a.any()]
    for i in zero:
        assert g[i].shape == w[i].shape and not g[i].any(), i
        g[i] = w[i] = np.ones(1)
    return (g, got[1], got[2]), dict(want, grads=w), zero


def _yardstick_bounds(w, xp, xh, cls, ref, what, n_gt=10):
    """per tensor max(bound(), 4 x distance of the float32 restatement from the float64 one) on this input"""
    import torch
    f32 = gr.loss_and_grad(w, xp, xh, cls, n_gt=n_gt, dtype=torch.float32)
    yard = np.zeros(len(ref["grads"]))
    for i, (a, b) in enumerate(zip(f32["grads"], ref["grads"])):
        if b.any():
            yard[i] = gr.rel_dist(a, b)
        else:
            assert not a.any(), i
    print(f"{what}: float32 restatement against float64, largest {yard.max():.2e} (tensor {int(yard.argmax())}) per tensor "
          + " ".join(f"{d:.1e}" for d in yard))
    assert yard.max() <= YARDSTICK_MAX, (what, yard.max())
    return np.maximum(bound(), 4.0 * yard)


def near_share(ref, n_gt=10):
    """the share of the sites with a head within MARGIN in the float64 logits"""
    return float((hr.margins(ref["logits"], n_gt) < hr.MARGIN).any(1).mean())


# ---- the inputs, shared with the CPU checks of docs/rounds/r33.md ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked96():
    """(inputs, masks, the restatement's result) of the 96-site fixture batch under seeded keep masks"""
    xp, xh, cls = batch(96)
    masks = seeded_masks(MASK_SEED, 96, P_DROP)
    return (xp, xh, cls), masks, gr.loss_and_grad(weights(), xp, xh, cls, masks, SCALE)


def _hot_vector(x, s, p):
    """the F features of (site s, position p) of x [N,F,L], or of the first (site, position) behind it (site-major, wrapping) that has at
    least four non-zero features; the PLACE of the hot row stays (s, p), which is what the slice cuts are about"""
    cols = x.transpose(0, 2, 1).reshape(-1, x.shape[1])
    k = s * x.shape[2] + p
    while np.count_nonzero(cols[k]) < 4:
        k = (k + 1) % cols.shape[0]
    return cols[k].copy()


HOT_PLACES = [((3, 28), (11, 6)), ((3, 29), (11, 7)), ((3, 4), (11, 4)), ((3, 3), (11, 3)), ((16, 32), (16, 10)), ((0, 0), (0, 0))]


def hot_inputs(place_p, place_h):
    """N = 17, every feature zero but position place_p[1] of site place_p[0] in xp and the like in xh -> (xp, xh, cls, hot_p, hot_h)"""
    bp, bh, cls = batch(17)
    xp, xh = np.zeros_like(bp), np.zeros_like(bh)
    hot_p, hot_h = _hot_vector(bp, *place_p), _hot_vector(bh, *place_h)
    xp[place_p[0], :, place_p[1]] = hot_p
    xh[place_h[0], :, place_h[1]] = hot_h
    return xp, xh, cls, hot_p, hot_h


def deep_inputs():
    xp, xh, cls = batch(17)
    return xp * np.float32(20.0), xh * np.float32(20.0), cls


EDGE_DIMS = [(128, 15, 1), (1, 1, 15), (7, 2, 2)]


def edge_inputs(F, n_gt, n_zy):
    """the 17-site fixture batch tiled or cut along F, the classes reduced into range, seeded weights of these dims"""
    xp, xh, cls = batch(17)
    reps = -(-F // xp.shape[1])
    xp, xh = np.tile(xp, (1, reps, 1))[:, :F], np.tile(xh, (1, reps, 1))[:, :F]
    cls = np.stack([cls[:, 0] % n_gt, cls[:, 1] % n_zy], axis=1).astype(np.uint8)
    return seeded_hap_weights(77, F=F, n_gt=n_gt, n_zy=n_zy), np.ascontiguousarray(xp), np.ascontiguousarray(xh), cls


# ---- 1: masks across chunks -------------------------------------------------------------------------------------------------------------
def test_masks_across_chunks():
    """N = 96 under a reservation of 40 (chunks of 40, 40, 16) with seeded masks: float64 on the same masks, the same call as ONE chunk
    (reservation 128), the same bits twice, and the same bits after reserving 64 and 40 again"""
    (xp, xh, cls), masks, want = masked96()
    assert all(0 < m.mean() < 1 for m in masks)
    small, whole = Harness(weights(), 40), Harness(weights(), 128)
    try:
        got = small.run(xp, xh, cls, masks, SCALE, fill=-2.0)
        one = whole.run(xp, xh, cls, masks, SCALE, fill=-2.0)
        twice = small.run(xp, xh, cls, masks, SCALE, fill=1.5)
        small.ctx.hap_train_reserve(64)
        small.ctx.hap_train_reserve(40)
        again = small.run(xp, xh, cls, masks, SCALE, fill=3.0)
    finally:
        small.ctx.close()
        whole.ctx.close()
    assert got[1].shape == (96, 2) and got[2].shape == (96, 2)
    check_parity(got, want, label="N = 96 in chunks of 40, masks")
    dist = np.array([gr.rel_dist(a, b) for a, b in zip(one[0], got[0])])
    print(f"one chunk of 128 against chunks of 40: per tensor {dist.min():.2e} .. {dist.max():.2e} (tensor {int(dist.argmax())})")
    assert dist.max() <= bound(), (int(dist.argmax()), float(dist.max()))
    assert np.abs(got[1] - one[1]).max() <= 1e-4
    far = hr.margins(want["logits"], 10) >= hr.MARGIN
    assert ((got[2] == one[2]) | ~far).all()
    assert _same_bits(got, twice)
    assert _same_bits(got, again)


# ---- 2: n below the tensors, caller-owned outputs -----------------------------------------------------------------------------------------
def test_n_below_the_tensors_and_caller_owned_outputs():
    """n = 50 of tensors and masks of 96 rows under a reservation of 40 (chunks of 40 and 10), site_loss and pred preallocated [96,2]"""
    import torch
    (xp, xh, cls), masks, _ = masked96()
    n = 50
    h = Harness(weights(), 40)
    try:
        site_loss = torch.full((96, 2), 7.5, dtype=torch.float32, device=h.dev)
        pred = torch.full((96, 2), 255, dtype=torch.uint8, device=h.dev)
        for g in h.grads:
            g.fill_(3.0)
        sl, pr = h.ctx.hap_loss_grad(h.params, _dev(h, xp), _dev(h, xh), _dev(h, cls), h.grads, [_dev(h, m) for m in masks], SCALE, n=n,
                                     site_loss=site_loss, pred=pred)
        torch.cuda.synchronize()
        assert sl is site_loss and pr is pred
        sl, pr = site_loss.cpu().numpy(), pred.cpu().numpy()
        got = ([g.cpu().numpy() for g in h.grads], sl[:n], pr[:n])
        own = h.run(xp[:n], xh[:n], cls[:n], [m[:n] for m in masks], SCALE, fill=-2.0)      # the first 50 rows in tensors of their own
    finally:
        h.ctx.close()
    assert (sl[n:] == 7.5).all() and (pr[n:] == 255).all()               # nothing behind row n is written
    assert own[1].shape == (n, 2) and _same_bits(got, own)               # the same chunks, the same arithmetic, no float atomics
    want = gr.loss_and_grad(weights(), xp[:n], xh[:n], cls[:n], [m[:n] for m in masks], SCALE)
    check_parity(got, want, label="n = 50 of 96 rows")                   # (1 / N is 1 / 50)


# ---- 3: a side stream -------------------------------------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_bits_of_the_current_one(small_harness):
    import torch
    h = small_harness
    xp, xh, cls = batch(17)
    masks = seeded_masks(MASK_SEED, 17, P_DROP)
    plain = h.run(xp, xh, cls, masks, SCALE, fill=-2.0)
    args = (_dev(h, xp), _dev(h, xh), _dev(h, cls))
    m = [_dev(h, a) for a in masks]
    for g in h.grads:
        g.fill_(3.0)
    side = torch.cuda.Stream(device=h.dev)
    side.wait_stream(torch.cuda.current_stream(h.dev))                   # the uploads and the fill
    site_loss, pred = h.ctx.hap_loss_grad(h.params, *args, h.grads, m, SCALE, stream=side)
    side.synchronize()
    got = ([g.cpu().numpy() for g in h.grads], site_loss.cpu().numpy(), pred.cpu().numpy())
    assert got[0][0].any() and _same_bits(plain, got)


# ---- 4: one hot row at the slice cuts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place_p,place_h", HOT_PLACES, ids=lambda v: f"{v[0]}_{v[1]}")
def test_one_hot_row(small_harness, place_p, place_h):
    """N = 17, every feature zero but one (site, position) of each encoder: the layer-0 W_ih gradients of both directions come from that
    one (site, step) row.  T = 33: row 33 s + p of the forward walk, (3, 28) is row 127, the last of slice 0, (3, 29) row 128, the first of
    slice 1; the reverse walk has them at positions 4 and 3.  T = 11: (11, 6) is row 127, (11, 7) row 128; reverse: positions 4 and 3.
    (16, 32) / (16, 10): the last site at the last position; (0, 0): the first at the first.  A feature column whose hot entry is 0 gets
    exact zeros (zero operands, zero padding), every other column something."""
    xp, xh, cls, hot_p, hot_h = hot_inputs(place_p, place_h)
    assert np.count_nonzero(hot_p) >= 4 and np.count_nonzero(hot_h) >= 4
    assert np.count_nonzero(xp) == np.count_nonzero(hot_p) and np.count_nonzero(xh) == np.count_nonzero(hot_h)
    got = small_harness.run(xp, xh, cls, fill=-2.0)
    for i, hot in ((0, hot_p), (4, hot_p), (26, hot_h), (30, hot_h)):
        live = np.abs(got[0][i]).max(0) > 0
        assert np.array_equal(live, hot != 0), (i, live, hot)
        assert (got[0][i][:, hot == 0] == 0.0).all()
    ref = gr.loss_and_grad(weights(), xp, xh, cls)
    what = f"hot rows {place_p} {place_h}"
    print(f"{what}: near-margin share {near_share(ref):.4f}")
    check_parity(got, ref, label=what, bounds=_yardstick_bounds(weights(), xp, xh, cls, ref, what))


# ---- 5: deep features -------------------------------------------------------------------------------------------------------------------
def test_deep_features(small_harness):
    """the 17-site fixture batch times 20: features to 42,000, saturated gates, under the cells' own sigmoid and tanh"""
    xp, xh, cls = deep_inputs()
    assert max(np.abs(xp).max(), np.abs(xh).max()) >= 40000
    got = small_harness.run(xp, xh, cls, fill=-2.0)
    assert all(np.isfinite(g).all() for g in got[0])
    ref = gr.loss_and_grad(weights(), xp, xh, cls)
    print(f"deep features: near-margin share {near_share(ref):.4f}")
    check_parity(got, ref, label="deep features, N = 17", bounds=_yardstick_bounds(weights(), xp, xh, cls, ref, "deep features"))


# ---- 6: edge dims -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n_gt,n_zy", EDGE_DIMS)
def test_edge_dims(F, n_gt, n_zy):
    """the edges of what nsnp_hap_train_reserve accepts, at a reservation of 8 (17 = 8 + 8 + 1, so the chunks' sums meet them too):
    (128, 15, 1) K = 128 in the layer-0 product, the last column of the 16-wide logit row, a zygosity head of one class; (1, 1, 15) K = 1,
    a genotype head of one class; (7, 2, 2) a K that is no multiple of 4, the smallest heads that have a loss"""
    w, xp, xh, cls = edge_inputs(F, n_gt, n_zy)
    assert xp.shape == (17, F, 33) and xh.shape == (17, F, 11) and xp.any() and xh.any()
    h = Harness(w, 8, F, n_gt, n_zy)
    try:
        got = h.run(xp, xh, cls, fill=-2.0)
    finally:
        h.ctx.close()
    ref = gr.loss_and_grad(w, xp, xh, cls, n_gt=n_gt)
    what = f"dims ({F}, {n_gt}, {n_zy})"
    print(f"{what}: near-margin share {near_share(ref, n_gt):.4f}")
    bounds = _yardstick_bounds(w, xp, xh, cls, ref, what, n_gt)
    got, ref, zero = _exact_zeros(got, ref)
    want_zero = ([54, 55] if n_gt == 1 else []) + ([56, 57] if n_zy == 1 else [])
    assert zero == want_zero                                              # a head of one class: no gradient; every other tensor has one
    for head, c in enumerate((n_gt, n_zy)):
        if c == 1:
            assert (got[1][:, head] == 0.0).all() and (got[2][:, head] == 0).all()
    check_parity(got, ref, n_gt=n_gt, label=what, bounds=bounds)


def test_refusals_at_the_sixteen_column_edge():
    from nanosnp_amd import _lib
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.NanoSNPError):
            ctx.hap_train_reserve(8, 105, 15, 2)                          # 17 logits
        ctx.hap_train_reserve(8, 105, 15, 1)                              # 16: the whole row
    finally:
        ctx.close()


# ---- 7: a dropout epoch against a float64 replay ------------------------------------------------------------------------------------------
def _float64_dropout_epoch(files, w0, seed, dev, clip, lr):
    """_float64_epoch of test_gpu_hap_train_bins.py with the masks train_haplotype_bins draws (a device generator seeded alike; per batch
    torch.rand((n, L, 512)) >= P_DROP for L in 33, 33, 11, 11, scale 1 / (1 - P_DROP)) and clip_grad_norm_'s rule (the total 2-norm of the
    58 tensors, the factor clip / (norm + 1e-6) capped at 1)"""
    import torch
    from nanosnp_amd import train
    order_gen = torch.Generator().manual_seed(seed)
    mask_gen = torch.Generator(device=dev).manual_seed(seed)
    w = [np.asarray(a, np.float64).copy() for a in w0]
    losses, norms, meta_sum = [], [], np.zeros(4, np.int64)
    correct, near, near_sites, sites = np.zeros(2, np.int64), np.zeros(2, np.int64), 0, 0
    for f in files:
        xp, xh = file_features(f)
        rows, cls, meta = hr.label_filter(f["labels"])
        meta_sum += meta
        for a in range(0, len(f["labels"]), PASS):
            sel = np.flatnonzero((rows >= a) & (rows < a + PASS))
            if not sel.size:
                continue
            sel = sel[train.pass_order(order_gen, sel.size).numpy()]
            for o in range(0, sel.size, B):
                s = sel[o:o + B]
                masks = [(torch.rand((s.size, L, 512), generator=mask_gen, device=dev) >= P_DROP).to(torch.uint8).cpu().numpy()
                         for L in (33, 33, 11, 11)]
                r = gr.loss_and_grad(w, xp[rows[s]], xh[rows[s]], cls[s], masks, SCALE)
                norms.append(float(np.sqrt(sum((g ** 2).sum() for g in r["grads"]))))
                factor = min(1.0, clip / (norms[-1] + 1e-6))
                w = [p - lr * factor * g for p, g in zip(w, r["grads"])]
                losses.append(r["loss"])
                far = hr.margins(r["logits"], 10) >= hr.MARGIN
                correct += ((r["pred"] == cls[s]) & far).sum(0)
                near += (~far).sum(0)
                near_sites += int((~far).any(1).sum())
                sites += s.size
    return dict(w=w, mean_loss=float(np.mean(losses)), batches=len(losses), meta=meta_sum, norms=norms, correct=correct, near=near,
                near_sites=near_sites, sites=sites)


def test_a_dropout_epoch_follows_the_float64_replay(epoch_files):
    """one epoch over the labelled files (batches of 32 as chunks of 20 and 12 on a trainer reserved at 20 sites), dropout 0.1 with the
    device-drawn masks, clip_grad_norm_ at CLIP, torch's SGD: a float64 replay with the same orders, masks and clipping rule"""
    import torch
    from nanosnp_amd import train
    ef = epoch_files
    tr = train.HaplotypeTrainer(_state(ef["weights"]), chunk_sites=20)
    try:
        res = train.train_haplotype_bins(tr, ef["paths"], ef["reference"], optimizer=torch.optim.SGD(tr.parameters(), lr=LR), batch_size=B,
                                         dropout=P_DROP, max_grad_norm=CLIP, seed=EPOCH_SEED, pass_sites=PASS)
        p = _params(tr)
        want = _float64_dropout_epoch(ef["files"], ef["weights"], EPOCH_SEED, tr.device, CLIP, LR)
    finally:
        tr.ctx.close()
    kept, unscorable, refcalls, variants = [int(v) for v in want["meta"]]
    sites, norms = want["sites"], want["norms"]
    dist = np.array([gr.rel_dist(a, b) for a, b in zip(p, want["w"])])
    moved = max(gr.rel_dist(a, b) for a, b in zip(want["w"], ef["weights"]))
    print(f"dropout epoch: device {res}")
    print(f"  float64 mean_loss {want['mean_loss']:.6f}, correct at far margins {want['correct'].tolist()}, near margins {want['near'].tolist()} of "
          f"{sites} sites; gradient norms " + " ".join(f"{v:.4f}" for v in norms) + f"; clip {CLIP}")
    print(f"  parameters (bound {PARITY:.2e}) {dist.min():.2e} .. {dist.max():.2e} (tensor {int(dist.argmax())}) " + " ".join(f"{d:.1e}" for d in dist))
    print(f"  the float64 epoch moved a tensor by up to {moved:.2e} of its largest entry")
    assert kept > 3 * B and kept % B != 0 and sites == kept
    assert (res["sites"], res["refcalls"], res["variants"], res["unscorable_labels"]) == (kept, refcalls, variants, unscorable)
    assert res["batches"] == want["batches"] > -(-kept // B)
    assert any(v > 1.05 * CLIP for v in norms) and any(v < 0.95 * CLIP for v in norms), norms       # one batch clipped, one not
    assert want["near_sites"] <= hr.MARGIN_SHARE * sites                 # the cap of check_parity on the sites with a near head
    assert abs(res["mean_loss"] - want["mean_loss"]) <= 1e-4
    for head, key in enumerate(("gt_accuracy", "zy_accuracy")):
        # a site within the margin may fall either way on the device: it is left out, so the device may count up to `near` more
        lo, hi = want["correct"][head] / sites, (want["correct"][head] + want["near"][head]) / sites
        assert lo - 1e-4 <= res[key] <= hi + 1e-4, (key, res[key], lo, hi)
    assert 100 * PARITY < moved <= 1.0                                    # the premise under which the gradient bound carries to parameters
    assert dist.max() <= PARITY, (int(dist.argmax()), float(dist.max()))
