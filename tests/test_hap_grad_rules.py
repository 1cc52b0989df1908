"""CPU side of HaplotypeModel training: the float64 restatement of the loss gradients (tests/hap_grad_rules.py) against what the reference's
own model_dev.LSTMNetwork left in param.grad (tests/golden/hap_grad.npz, made by tests/golden/make_golden_hap_grad.py), and the properties of
the keep masks and the bias pairs.  The batches and their float64 results are built once and shared with the GPU tests."""
from __future__ import annotations

import functools
import zlib

import numpy as np
import pytest

from tests import hap_eval_rules as hr
from tests import hap_grad_rules as gr
from tests.helpers import golden, seeded_hap_weights
from tests.test_hap_eval_rules import SEED_MAIN, eval_case, seeded_targets

MAIN_SIZES = (1, 17, 96)                 # the first N sites of the `main` case of hap_eval.npz
N_BIG, SEED_BIG = 257, 31                # one batch of 257 sites by the same recipe, planes seeded 540 / 640 + SEED_BIG


@functools.lru_cache(maxsize=None)
def weights():
    w = seeded_hap_weights(SEED_MAIN, H=256)
    for a in w:
        a.setflags(write=False)
    return tuple(w)


@functools.lru_cache(maxsize=None)
def big_inputs():
    """(xp [257,105,33], xh [257,105,11], cls [257,2]) rebuilt from their seeds; bytes other than those the fixture's maker saw are an error"""
    from nanosnp_amd import host
    from oracle import oracle
    xs = [oracle.hap_features_batch(*host.synth_hap_planes(sd + SEED_BIG, N_BIG, 30, 90, L), nthreads=4) for sd, L in ((540, 33), (640, 11))]
    cls = seeded_targets(SEED_BIG, N_BIG, 10, 3)
    z = np.load(golden("hap_grad.npz"))
    assert [zlib.crc32(xs[0].tobytes()), zlib.crc32(xs[1].tobytes())] == z["big_input_crc32"].tolist(), \
        "hap_grad.npz: the rebuilt 257-site batch is not the recorded one"
    assert np.array_equal(cls, z["big_cls"])
    return xs[0], xs[1], cls


def batch(n):
    """(xp, xh, cls) of a fixture batch: n in MAIN_SIZES or N_BIG"""
    if n == N_BIG:
        return big_inputs()
    c = eval_case("main")
    return c["xp"][:n], c["xh"][:n], c["cls"][:n]


@functools.lru_cache(maxsize=None)
def f64_case(n):
    """the restatement's result on a fixture batch, computed once and shared"""
    xp, xh, cls = batch(n)
    r = gr.loss_and_grad(weights(), xp, xh, cls)
    for g in r["grads"]:
        g.setflags(write=False)
    return r


def seeded_masks(seed, n, p):
    """four keep masks uint8 (pileup layers 0 and 1 [n,33,512], haplotype layers 0 and 1 [n,11,512]) with keep probability 1 - p"""
    rng = np.random.default_rng(8000 + seed)
    return [(rng.random((n, L, 512)) >= p).astype(np.uint8) for L in (33, 33, 11, 11)]


@pytest.mark.parametrize("n", MAIN_SIZES + (N_BIG,))
def test_rules_reproduce_the_reference_gradients(n):
    z = np.load(golden("hap_grad.npz"))
    bound = float(z["ref_rel_max"])
    assert 0 < bound <= 2.5e-5                                          # the project's admissibility rule for an fp32 reference
    assert float(z[f"dist_{n}"].max()) <= bound
    r = f64_case(n)
    assert abs(r["loss"] - float(z[f"loss_{n}"])) <= 1e-4
    assert len(r["grads"]) == 58 and [g.shape for g in r["grads"]] == gr.shapes()
    for i, g in enumerate(r["grads"]):
        top = np.abs(g).max()
        assert top > 0, i                                               # every tensor has a gradient
        assert np.abs(z[f"val_{n}"][i] - g.reshape(-1)[gr.sample_index(i, g.shape)]).max() <= bound * top, (n, i)
        assert abs(z[f"sum_{n}"][i] - g.sum()) <= bound * top * g.size, (n, i)
        assert abs(z[f"l2_{n}"][i] - np.sqrt((g ** 2).sum())) <= bound * top * np.sqrt(g.size), (n, i)
    near = hr.margins(r["logits"], 10) < hr.MARGIN
    assert near.any(1).sum() == int(z[f"near_{n}"]) and near.any(1).mean() <= hr.MARGIN_SHARE


def test_bias_pairs_are_equal():
    g = f64_case(17)["grads"]
    for a, b in gr.BIAS_PAIRS:
        assert np.array_equal(g[a], g[b])


def test_masks_of_ones_equal_no_mask():
    xp, xh, cls = batch(17)
    xp, xh, cls = xp[:3], xh[:3], cls[:3]
    a = gr.loss_and_grad(weights(), xp, xh, cls)
    b = gr.loss_and_grad(weights(), xp, xh, cls, [np.ones((3, L, 512), np.uint8) for L in (33, 33, 11, 11)], 1.0)
    assert a["loss"] == b["loss"] and all(np.array_equal(x, y) for x, y in zip(a["grads"], b["grads"]))


@pytest.mark.parametrize("enc", [0, 1])
def test_a_mask_of_zeros_behind_layer_0_cuts_the_gradient_below_it(enc):
    xp, xh, cls = batch(17)
    xp, xh, cls = xp[:3], xh[:3], cls[:3]
    masks = [np.ones((3, L, 512), np.uint8) for L in (33, 33, 11, 11)]
    masks[2 * enc][:] = 0
    g = gr.loss_and_grad(weights(), xp, xh, cls, masks, 1.0 / 0.9)["grads"]
    base = 26 * enc
    for i in range(base, base + 8):                                     # layer 0 of that encoder
        assert not g[i].any(), i
    for i in (base + 8, base + 12):                                     # W_ih of its layer 1, both directions: the input is zero
        assert not g[i].any(), i
    for i in (base + 9, base + 10, base + 13, base + 24):               # the rest of the encoder still learns
        assert g[i].any(), i
    other = 26 * (1 - enc)
    assert all(g[i].any() for i in range(other, other + 26)) and all(g[i].any() for i in range(52, 58))
