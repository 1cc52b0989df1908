"""nsnp_hap_loss_grad on the device against the float64 restatement tests/hap_grad_rules.py.

The parity rule is the project's own: for every one of the 58 tensors max |g_dev - g_f64| / max |g_f64| <= 4 x ref_rel_max of
tests/golden/hap_grad.npz (the reference's own fp32 distance from the restatement; 4 is the factor the forward and the pileup gradients are
granted); loss and site_loss within 1e-4; pred equal wherever the float64 margin exceeds hap_eval_rules.MARGIN, and at most MARGIN_SHARE of
the sites nearer than that.

The kernel's site tile is 64 (k_tr_gemm: 64 x 64 tiles of C) and a weight-gradient slice is 128 (site, step) rows: N = 1 has 33, 11 and
fewer rows and crosses none, N = 17 crosses a slice boundary for both encoders at layers 0 and 1 (561 and 187 rows) and for neither at
layer 2's recurrent weights of the 11-step encoder (85 rows), N = 96 crosses it everywhere."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import hap_eval_rules as hr
from tests import hap_grad_rules as gr
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def bound():
    return FACTOR * float(np.load(golden("hap_grad.npz"))["ref_rel_max"])


class Harness:
    """a context with a reservation, the parameters on the device and gradient buffers"""

    def __init__(self, weights, reserve, F=105, n_gt=10, n_zy=3, ctx=None):
        import torch
        from nanosnp_amd import _lib
        self.ctx = ctx if ctx is not None else _lib.Context(0)
        self.dev = torch.device("cuda", 0)
        self.params = [torch.from_numpy(np.array(w, np.float32)).to(self.dev) for w in weights]
        self.grads = [torch.zeros_like(p) for p in self.params]
        if reserve:
            self.ctx.hap_train_reserve(reserve, F, n_gt, n_zy)

    def run(self, xp, xh, cls, masks=None, scale=1.0, fill=None):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        if fill is not None:
            for g in self.grads:
                g.fill_(fill)
        m = [t(a) for a in masks] if masks is not None else None
        site_loss, pred = self.ctx.hap_loss_grad(self.params, t(xp), t(xh), t(cls), self.grads, m, scale)
        torch.cuda.synchronize()
        return [g.cpu().numpy() for g in self.grads], site_loss.cpu().numpy(), pred.cpu().numpy()


@pytest.fixture(scope="module")
def main_harness():
    from tests.test_hap_grad_rules import weights
    return Harness(weights(), 512)


def check_parity(got, want, n_gt=10, label="", bounds=None):
    """bounds: None (bound() for every tensor) or one bound per tensor"""
    grads, site_loss, pred = got
    dist = np.array([gr.rel_dist(a, b) for a, b in zip(grads, want["grads"])])
    lim = np.full(dist.shape, bound()) if bounds is None else np.asarray(bounds, np.float64)
    assert lim.shape == dist.shape
    print(f"{label}: per-tensor distance {dist.min():.2e} .. {dist.max():.2e} (tensor {int(dist.argmax())}), bound {lim.min():.2e} .. {lim.max():.2e}")
    print("  " + " ".join(f"{d:.1e}" for d in dist))
    n = site_loss.shape[0]
    sl_err = float(np.abs(site_loss - want["site_loss"]).max())
    loss = float(site_loss.astype(np.float64).sum(0).sum() / n)
    print(f"  site_loss within {sl_err:.2e}, loss {loss:.6f} against {want['loss']:.6f}")
    assert np.isfinite(dist).all() and (dist <= lim).all(), (label, int((dist / lim).argmax()), float((dist / lim).max()))
    assert sl_err <= 1e-4 and abs(loss - want["loss"]) <= 1e-4
    far = hr.margins(want["logits"], n_gt) >= hr.MARGIN
    assert (~far).any(1).mean() <= hr.MARGIN_SHARE                        # a pred that may fall either way is the exception
    assert ((pred == want["pred"]) | ~far).all()
    for a, b in gr.BIAS_PAIRS:
        assert np.array_equal(grads[a], grads[b])


@pytest.mark.parametrize("n", [1, 17, 96, 257])
def test_fixture_batches(main_harness, n):
    from tests.test_hap_grad_rules import batch, f64_case
    check_parity(main_harness.run(*batch(n)), f64_case(n), label=f"N = {n}")


@pytest.mark.parametrize("n", [63, 64, 65])
def test_below_at_and_above_the_site_tile(main_harness, n):
    from tests.test_hap_grad_rules import batch, weights
    xp, xh, cls = [a[-n:] for a in batch(257)]                          # drawn from the 257-site batch
    check_parity(main_harness.run(xp, xh, cls), gr.loss_and_grad(weights(), xp, xh, cls), label=f"N = {n}")


def test_seeded_masks(main_harness):
    from tests.test_hap_grad_rules import batch, seeded_masks, weights
    xp, xh, cls = batch(17)
    masks = seeded_masks(5, 17, 0.1)
    assert all(0 < m.mean() < 1 for m in masks)
    check_parity(main_harness.run(xp, xh, cls, masks, 1.0 / 0.9), gr.loss_and_grad(weights(), xp, xh, cls, masks, 1.0 / 0.9), label="masks")


def test_degenerate_masks(main_harness):
    from tests.test_hap_grad_rules import batch
    xp, xh, cls = batch(17)
    plain = main_harness.run(xp, xh, cls)
    ones = [np.ones((17, L, 512), np.uint8) for L in (33, 33, 11, 11)]
    same = main_harness.run(xp, xh, cls, ones, 1.0, fill=3.0)
    assert all(np.array_equal(a, b) for a, b in zip(plain[0], same[0])) and np.array_equal(plain[1], same[1])      # the bits of NULL
    for enc in (0, 1):
        masks = [m.copy() for m in ones]
        masks[2 * enc][:] = 0
        g = main_harness.run(xp, xh, cls, masks, 1.0 / 0.9, fill=3.0)[0]
        base = 26 * enc
        for i in list(range(base, base + 8)) + [base + 8, base + 12]:
            assert not g[i].any(), i
        assert all(g[i].any() for i in (base + 9, base + 10, base + 13, base + 24))
        assert all(g[i].any() for i in range(26 * (1 - enc), 26 * (1 - enc) + 26))


def test_chunks_of_a_reservation_that_is_no_multiple_of_the_tile():
    from tests.test_hap_grad_rules import batch, f64_case, weights
    h = Harness(weights(), 40)                                           # 96 = 40 + 40 + 16; 1 / N is the batch's
    check_parity(h.run(*batch(96), fill=-2.0), f64_case(96), label="N = 96 in chunks of 40")


def test_same_call_same_bits(main_harness):
    from tests.test_hap_grad_rules import batch, seeded_masks
    xp, xh, cls = batch(96)
    masks = seeded_masks(6, 96, 0.1)
    a = main_harness.run(xp, xh, cls, masks, 1.0 / 0.9, fill=1.5)
    b = main_harness.run(xp, xh, cls, masks, 1.0 / 0.9, fill=-7.0)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_other_dims():
    from tests.test_hap_eval_rules import eval_case
    c = eval_case("dims")
    assert (c["F"], c["n_gt"], c["n_zy"]) == (96, 13, 3)
    h = Harness(c["weights"], 64, c["F"], c["n_gt"], c["n_zy"])
    want = gr.loss_and_grad(c["weights"], c["xp"], c["xh"], c["cls"], n_gt=c["n_gt"])
    check_parity(h.run(c["xp"], c["xh"], c["cls"]), want, n_gt=c["n_gt"], label="dims (96, 13, 3)")


def test_a_class_out_of_range_is_the_last_class(main_harness):
    from tests.test_hap_grad_rules import batch
    xp, xh, cls = batch(17)
    last = cls.copy(); last[::2, 0] = 9; last[1::3, 1] = 2
    out = last.copy(); out[::2, 0] = 200; out[1::3, 1] = 3
    a, b = main_harness.run(xp, xh, last), main_harness.run(xp, xh, out)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_site_loss_and_pred_are_those_of_hap_eval(main_harness):
    import torch
    from tests.test_hap_grad_rules import batch, f64_case, weights
    xp, xh, cls = batch(96)
    _, site_loss, pred = main_harness.run(xp, xh, cls)
    ctx = main_harness.ctx
    ctx.hap_load_weights(list(weights()))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(main_harness.dev)
    sl, pr, _ = ctx.hap_eval(t(xp), t(xh), t(cls), ctx.hap_eval_counters())
    torch.cuda.synchronize()
    assert np.abs(sl.cpu().numpy() - site_loss).max() <= 1e-4
    far = (hr.margins(f64_case(96)["logits"], 10) >= hr.MARGIN)
    assert ((pr.cpu().numpy() == pred) | ~far).all()


def test_refusals():
    from nanosnp_amd import _lib
    from tests.test_hap_grad_rules import batch, weights
    xp, xh, cls = batch(1)
    h = Harness(weights(), 0)
    with pytest.raises(_lib.NanoSNPError):                                # no reservation
        h.run(xp, xh, cls)
    h.ctx.hap_train_reserve(8)
    h.run(xp, xh, cls)
    for mode in (1, 2):                                                   # fp32 only
        h.ctx.set_option("hap_precision", mode)
        with pytest.raises(_lib.NanoSNPError):
            h.run(xp, xh, cls)
    h.ctx.set_option("hap_precision", 0)
    h.ctx.hap_train_reserve(8, 96, 13, 3)                                 # dims that differ from the tensors'
    with pytest.raises(_lib.NanoSNPError):
        h.run(xp, xh, cls)
    with pytest.raises(_lib.NanoSNPError):
        h.run(xp[:, :96], xh[:, :96], cls)                                # the features agree, the 58 shapes do not
    for bad in ((0, 105, 10, 3), (8, 0, 10, 3), (8, 129, 10, 3), (8, 105, 0, 3), (8, 105, 14, 3)):
        with pytest.raises(_lib.NanoSNPError):
            h.ctx.hap_train_reserve(*bad)


def test_no_site_leaves_the_gradients_untouched(main_harness):
    from tests.test_hap_grad_rules import batch
    xp, xh, cls = batch(1)
    g, site_loss, pred = main_harness.run(xp[:0], xh[:0], cls[:0], fill=4.25)
    assert all((a == 4.25).all() for a in g) and site_loss.shape == (0, 2) and pred.shape == (0, 2)
