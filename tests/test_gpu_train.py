"""The loss gradients of a batch on the device (nsnp_pileup_train_reserve / nsnp_pileup_loss_grad, nanosnp_amd.train) against the float64
restatement tests/grad_rules.py.

Parity bound: for every one of the 24 tensors max |g_dev - g_f64| / max |g_f64| <= 4 x ref_rel_max, ref_rel_max being the reference's OWN
fp32 distance from float64 recorded in tests/golden/pileup_grad.npz (5.6e-6): the factor the project grants its forward (1e-4 against inputs
admissible at 2.5e-5).  Loss and site_loss: 1e-4 absolute; pred: equal wherever the float64 top-two logits differ by more than 1e-4.
Inputs: eval_rules.synthetic_windows with the weights of nanosnp_amd/data/ont_pileup_weights.npz.  No kernel of pileup_train.hip is
persistent (no grid is capped by the CU count), so there is no case sized by the CU count.  The sizes that DO select other paths - more
than one slice of 1,024 reduction rows for the dense layers and heads (N >= 1025), every starting phase of a slice against the 33 and 17
steps of a site, a reservation that is no multiple of 16, chunks with a mask and centre indices - are in tests/test_gpu_train_batches.py.

Distances measured on an MI355X: docs/rounds/r23.md has the table per tensor."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import eval_rules as er
from tests import grad_rules as gr
from tests.helpers import ROOT, golden, load_pileup_weights

pytestmark = pytest.mark.gpu
ATOL = 1e-4
DATA_NPZ = os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def bound():
    return 4.0 * float(np.load(golden("pileup_grad.npz"))["ref_rel_max"])


@pytest.fixture(scope="module")
def weights():
    return load_pileup_weights()


@pytest.fixture(scope="module")
def params(weights):
    return [_dev(np.asarray(t, np.float32)) for t in weights]


@pytest.fixture(scope="module")
def ctx():
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    c.pileup_train_reserve(64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpu_train"))
    return {case: er.fixture_rows(case, d) for case in ("train_g1", "train_cut")}      # case -> (path, windows, labels)


@pytest.fixture(scope="module")
def synth(sets):
    return er.synthetic_windows(sets["train_cut"][1], 64)


@pytest.fixture(scope="module")
def f64(weights, synth):
    """float64 results per (n, masked), computed once and shared"""
    cache = {}

    def get(n, mask=None, scale=1.0, key=None):
        k = (n, key)
        if k not in cache:
            cache[k] = gr.loss_and_grad(weights, synth[0][:n], synth[1][:n], mask, scale)
        return cache[k]
    return get


def _mask(n, p=0.3, seed=11):
    return (np.random.default_rng([n, seed]).random((n, 33, 128)) >= p).astype(np.uint8)


def _run(ctx, params, x, cls, mask=None, scale=1.0, center_idx=None, fill=None):
    import torch
    grads = [torch.full_like(p, float("nan") if fill is None else fill) for p in params]
    site_loss, pred = ctx.pileup_loss_grad(params, _dev(x), None if center_idx is None else _dev(center_idx), _dev(cls), grads,
                                           None if mask is None else _dev(mask), scale)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], site_loss.cpu().numpy(), pred.cpu().numpy()


def _check(got, ref, n, bound, what):
    """bound: one number for every tensor, or 24 of them"""
    grads, site_loss, pred = got
    bounds = np.broadcast_to(np.asarray(bound, np.float64), (24,))
    dist = [gr.rel_dist(g, r) for g, r in zip(grads, ref["grads"])]
    loss = float(site_loss.astype(np.float64).sum() / n)
    dl, ds = abs(loss - ref["loss"]), float(np.abs(site_loss - ref["site_loss"]).max())
    print(f"{what}: max rel dist {max(dist):.3e} (bound {bounds.min():.3e}) per tensor " + " ".join(f"{d:.1e}" for d in dist) +
          f"; |loss - f64| {dl:.2e}, site_loss {ds:.2e}")
    for i, d in enumerate(dist):
        assert np.isfinite(grads[i]).all() and d <= bounds[i], (what, i, d, bounds[i])
    assert dl <= ATOL and ds <= ATOL, (what, dl, ds)
    clear = gr.top_two_gap(ref["logits"]) > ATOL
    assert np.array_equal(pred[clear], ref["pred"][clear]), what
    for a, b in gr.BIAS_PAIRS:
        assert np.array_equal(grads[a], grads[b]), (what, a)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_parity_without_mask(ctx, params, synth, f64, bound, n):
    """one site; a partial group of 16; exactly one group; one group plus one site; two groups plus one site"""
    _check(_run(ctx, params, synth[0][:n], synth[1][:n]), f64(n), n, bound, f"N = {n}")


def test_parity_with_a_seeded_mask(ctx, params, synth, f64, bound):
    n, p = 17, 0.3
    m = _mask(n, p)
    _check(_run(ctx, params, synth[0][:n], synth[1][:n], m, 1.0 / (1.0 - p)), f64(n, m, 1.0 / (1.0 - p), key="p0.3"), n, bound, "N = 17, p = 0.3")


def test_degenerate_masks(ctx, params, synth):
    n = 17
    x, cls = synth[0][:n], synth[1][:n]
    plain = _run(ctx, params, x, cls)
    ones = _run(ctx, params, x, cls, np.ones((n, 33, 128), np.uint8), 1.0)
    for a, b in zip(plain[0] + [plain[1], plain[2]], ones[0] + [ones[1], ones[2]]):
        assert np.array_equal(a, b)                                     # all ones with scale 1: the bits of NULL
    zeros = _run(ctx, params, x, cls, np.zeros((n, 33, 128), np.uint8), 1.0 / 0.7)
    for i in list(range(8)) + [8, 12]:                                  # layer 0 is cut off; layer 1 sees zeros as its input
        assert (zeros[0][i] == 0).all(), i
    assert np.abs(zeros[0][9]).max() > 0 and np.abs(zeros[0][10]).max() > 0


def test_center_idx_with_repeats(ctx, params, weights, synth, bound):
    """a shuffled order with repeated centres into a flattened pass against the contiguous call on the gathered windows; a repeated window
    counts twice"""
    rows, n = 20, 23
    rng = np.random.default_rng(5)
    order = rng.integers(0, rows, n)
    assert len(set(order.tolist())) < n
    x, cls = synth[0][:rows], synth[1][order]
    got = _run(ctx, params, x.reshape(rows * 33, 18), cls, center_idx=33 * order.astype(np.int64) + 16)
    same = _run(ctx, params, x[order], cls)
    for i, (a, b) in enumerate(zip(got[0], same[0])):
        assert gr.rel_dist(a, b) <= bound, i
    assert np.abs(got[1] - same[1]).max() <= ATOL and np.array_equal(got[2], same[2])
    _check(got, gr.loss_and_grad(weights, x[order], cls), n, bound, "center_idx, N = 23 of 20 rows")


def test_chunks_share_the_batch_mean(params, synth, f64, bound):
    """a reservation of 32 with N = 49: a full chunk plus a partial one, accumulated; the 1 / N in dz is the whole batch's"""
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    try:
        c.pileup_train_reserve(32)
        _check(_run(c, params, synth[0][:49], synth[1][:49]), f64(49), 49, bound, "N = 49 in chunks of 32")
    finally:
        c.close()


def test_same_call_same_bits(ctx, params, synth):
    n = 33
    m = _mask(n)
    a = _run(ctx, params, synth[0][:n], synth[1][:n], m, 1.0 / 0.7)
    b = _run(ctx, params, synth[0][:n], synth[1][:n], m, 1.0 / 0.7, fill=3.0)
    for u, v in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert np.array_equal(u, v)


def test_class_out_of_range_is_the_last_class(ctx, params, synth):
    n = 17
    x, cls = synth[0][:n], synth[1][:n].copy()
    cls[3, 0], cls[5, 1], cls[9, 0] = 21, 3, 255
    last = cls.copy()
    last[3, 0], last[5, 1], last[9, 0] = 20, 2, 20
    a, b = _run(ctx, params, x, cls), _run(ctx, params, x, last)
    for u, v in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert np.array_equal(u, v)


def test_refusals_and_empty_batch(ctx, params, synth):
    import torch
    from nanosnp_amd import _lib
    n = 4
    x, cls = _dev(synth[0][:n]), _dev(synth[1][:n])
    grads = [torch.full_like(p, 7.0) for p in params]
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.NanoSNPError, match="invalid argument"):          # no reservation
            fresh.pileup_loss_grad(params, x, None, cls, grads)
        fresh.pileup_train_reserve(16)
        fresh.set_option("pileup_precision", 2)
        with pytest.raises(_lib.NanoSNPError, match="invalid argument"):
            fresh.pileup_loss_grad(params, x, None, cls, grads)
        fresh.set_option("pileup_precision", 1)
        with pytest.raises(_lib.NanoSNPError, match="invalid argument"):
            fresh.pileup_loss_grad(params, x, None, cls, grads)
    finally:
        fresh.close()
    pp = (C.c_void_p * 24)(*[p.data_ptr() for p in params])
    gp = (C.c_void_p * 24)(*[g.data_ptr() for g in grads])
    hole = (C.c_void_p * 24)(*[None if i == 13 else g.data_ptr() for i, g in enumerate(grads)])
    lib, h, s = ctx.lib, ctx.handle, _lib._stream_ptr()
    call = lambda c_, p_, x_, cls_, g_: lib.nsnp_pileup_loss_grad(c_, p_, x_, None, cls_, n, None, 1.0, g_, None, None, s)
    xp, cp = C.c_void_p(x.data_ptr()), C.c_void_p(cls.data_ptr())
    assert call(None, pp, xp, cp, gp) == -1 and call(h, None, xp, cp, gp) == -1 and call(h, pp, None, cp, gp) == -1
    assert call(h, pp, xp, None, gp) == -1 and call(h, pp, xp, cp, None) == -1 and call(h, pp, xp, cp, hole) == -1
    assert lib.nsnp_pileup_loss_grad(h, pp, xp, None, cp, -1, None, 1.0, gp, None, None, s) == -1
    assert lib.nsnp_pileup_train_reserve(h, 0) == -1 and lib.nsnp_pileup_train_reserve(None, 16) == -1
    # N == 0: a no-op
    ctx.pileup_loss_grad(params, x, None, cls, grads, n=0)
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in grads)
    assert call(h, pp, xp, cp, gp) == 0                                            # (and the same arguments do run)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) and not bool((g == 7.0).all()) for g in grads)
    # the binding's own checks
    with pytest.raises(_lib.NanoSNPError):
        ctx.pileup_loss_grad(params[:23], x, None, cls, grads)
    with pytest.raises(_lib.NanoSNPError):
        ctx.pileup_loss_grad(params, x, None, cls, [g.double() for g in grads])
    with pytest.raises(_lib.NanoSNPError):
        ctx.pileup_loss_grad(params, x, None, cls, grads, keep_mask=torch.ones((n, 33, 64), dtype=torch.uint8, device="cuda"))


def test_trainer_equals_the_raw_entry_and_round_trips(ctx, params, synth, tmp_path):
    import torch
    from nanosnp_amd import train
    from nanosnp_amd.pileup_model import LSTMNetwork, ENCODER_KEYS, FORWARD_KEYS, INDEL_KEYS
    n = 33
    x, cls = synth[0][:n], synth[1][:n]
    m = _mask(n)
    raw = _run(ctx, params, x, cls, m, 1.0 / 0.7)
    tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
    assert list(tr.params) == train.PARAM_NAMES
    loss, pred = tr.loss_and_grad(_dev(x), _dev(cls[:, 0].astype(np.int64)), _dev(cls[:, 1].astype(np.int64)), keep_mask=_dev(m), p=0.3)
    torch.cuda.synchronize()
    for p, g in zip(tr.parameters(), raw[0]):
        assert np.array_equal(p.grad.cpu().numpy(), g)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(float(loss) - raw[1].astype(np.float64).sum() / n) <= 1e-6 and np.array_equal(pred.cpu().numpy(), raw[2])
    # state dicts and the checkpoint come back through LSTMNetwork.from_checkpoint
    z = np.load(DATA_NPZ)
    enc, fwd = tr.state_dicts()
    assert list(enc) == ENCODER_KEYS and list(fwd) == FORWARD_KEYS + INDEL_KEYS
    assert all(np.array_equal(enc[k].numpy(), z["encoder." + k]) for k in ENCODER_KEYS)
    assert all(np.array_equal(fwd[k].numpy(), z["forward_layer." + k]) for k in FORWARD_KEYS + INDEL_KEYS)
    path = str(tmp_path / "round.chkpt")
    tr.save_checkpoint(path, epoch=3)
    assert torch.load(path, map_location="cpu", weights_only=False)["epoch"] == 3
    back = LSTMNetwork.from_checkpoint(path)
    ref = LSTMNetwork.from_npz(DATA_NPZ)
    xs = _dev(x)
    for a, b in zip(back.predict(xs), ref.predict(xs)):
        assert torch.equal(a, b)
    assert back._indel_loaded


def test_three_sgd_steps_follow_float64(weights, synth):
    """torch.optim.SGD (no momentum, no clipping), lr 0.02, on a fixed batch of 33: the loss model.forward of trainer.to_model() reports
    before step 1 and after each step is within 1e-4 of grad_rules' float64 trajectory, and lower after step 3 than before step 1"""
    import torch
    from nanosnp_amd import train
    n, lr = 33, 0.02
    x, cls = synth[0][:n], synth[1][:n]
    want, _ = gr.sgd_steps(weights, x, cls, lr, 3)
    tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
    opt = torch.optim.SGD(tr.parameters(), lr=lr)
    xd, t = _dev(x), [_dev(cls[:, h].astype(np.int64)) for h in range(4)]
    model, got, step_loss = None, [], []
    for k in range(4):
        model = tr.to_model(model)
        got.append(float(model.forward(xd, *t)[0]))
        if k < 3:
            step_loss.append(float(tr.loss_and_grad(xd, t[0], t[1])[0]))
            opt.step()
    print("float64", want, "device", got, "loss_and_grad", step_loss)
    assert np.abs(np.array(got) - want).max() <= ATOL and np.abs(np.array(step_loss) - want[:3]).max() <= ATOL
    assert got[3] < got[0]


def test_train_train_bins_replays_in_float64(weights, sets, tmp_path):
    """one epoch over the two fixture files, batches of 64, passes of 500 rows (train_cut: three passes), dropout 0, SGD: mean_loss and the
    accuracies equal a float64 replay of the same batches in the same order (the permutation from the same seeded torch.randperm); the saved
    checkpoint loads into LSTMNetwork and scores with evaluate_train_bins"""
    import torch
    from nanosnp_amd import evaluate, train
    from nanosnp_amd.pileup_model import LSTMNetwork
    B, P, lr, seed = 64, 500, 0.005, 7
    cases = ("train_g1", "train_cut")
    paths = [sets[c][0] for c in cases]
    tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
    stats = {}
    res = train.train_train_bins(tr, paths, optimizer=torch.optim.SGD(tr.parameters(), lr=lr), batch_size=B, dropout=0.0, max_grad_norm=None,
                                 seed=seed, pass_sites=P, stats=stats)
    # the replay
    gen = torch.Generator().manual_seed(seed)
    w = [np.asarray(t, np.float64) for t in weights]
    losses, correct, sites = [], np.zeros(2), 0
    for c in cases:
        _, x, label = sets[c]
        cls_all, _ = er.decode_labels(label)
        for a in range(0, x.shape[0], P):
            b = min(x.shape[0], a + P)
            order = train.pass_order(gen, b - a).numpy() + a
            for o in range(0, b - a, B):
                rows = order[o:o + B]
                r = gr.loss_and_grad(w, x[rows], cls_all[rows])
                w = [u - lr * g for u, g in zip(w, r["grads"])]
                losses.append(r["loss"])
                correct += (r["pred"] == cls_all[rows][:, :2]).sum(0)
                sites += rows.size
    print("device", res, "float64 mean_loss", np.mean(losses), "accuracies", correct / sites, "stats", stats)
    assert res["sites"] == sites == 138 + 1231 and res["batches"] == len(losses) and stats["passes"] == 4
    assert abs(res["mean_loss"] - np.mean(losses)) <= ATOL
    assert abs(res["gt_accuracy"] - correct[0] / sites) <= ATOL and abs(res["zy_accuracy"] - correct[1] / sites) <= ATOL
    for p, u in zip(tr.parameters(), w):
        assert np.abs(p.detach().cpu().numpy() - u).max() <= ATOL
    path = str(tmp_path / "epoch0.chkpt")
    tr.save_checkpoint(path, epoch=0)
    scored = evaluate.evaluate_train_bins(LSTMNetwork.from_checkpoint(path), paths, batch_size=B)
    assert scored["sites"] == 18 and np.isfinite(scored["avg_loss"]) and scored["malformed_labels"] == 0
