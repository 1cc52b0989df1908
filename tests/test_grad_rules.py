"""tests/grad_rules.py (the float64 restatement of the reference's training step, PileupModel/train.py:56-59) reproduces what the reference's
own model code wrote into tests/golden/pileup_grad.npz, its mask semantics agree with central finite differences, and the library declares,
exports and binds the training entries.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import eval_rules as er
from tests import grad_rules as gr
from tests.helpers import ROOT, golden, load_pileup_weights

NEW_SYMBOLS = ("nsnp_pileup_train_reserve", "nsnp_pileup_loss_grad")
FULL, SAMPLED = 17, (1, 33, 257, 2000)


@pytest.fixture(scope="module")
def gold():
    return np.load(golden("pileup_grad.npz"))


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return er.fixture_rows("train_cut", str(tmp_path_factory.mktemp("grad_rules")))[1]


@pytest.fixture(scope="module")
def weights():
    return load_pileup_weights()


def test_fixture_records_the_references_own_distance(gold):
    """ref_rel_max is the largest per-tensor distance of the reference's fp32 gradients from float64 over every batch of the fixture; the GPU
    tests grant the kernels four times it"""
    dist = np.stack([gold[f"dist_{n}"] for n in (FULL,) + SAMPLED])
    assert dist.shape == (5, 24) and float(gold["ref_rel_max"]) == dist.max()
    assert 1e-7 < float(gold["ref_rel_max"]) < 1e-5             # (fp32 arithmetic: a few hundred ulps of accumulated rounding, not more)


def test_full_batch_matches_the_reference(gold, base, weights):
    x, cls = er.synthetic_windows(base, FULL)
    mine = gr.loss_and_grad(weights, x, cls)
    assert abs(mine["loss"] - float(gold[f"loss_{FULL}"])) <= 1e-4
    for i, (g, shape) in enumerate(zip(mine["grads"], gr.SHAPES)):
        ref = gold[f"g{FULL}_{i:02d}"]
        assert ref.shape == shape == g.shape and ref.dtype == np.float32
        d = gr.rel_dist(ref, g)
        assert d <= float(gold["ref_rel_max"]) and abs(d - float(gold[f"dist_{FULL}"][i])) <= 1e-12, (i, d)


@pytest.mark.parametrize("n", SAMPLED)
def test_sampled_batches_match_the_reference(gold, base, weights, n):
    x, cls = er.synthetic_windows(base, n)
    mine = gr.loss_and_grad(weights, x, cls)
    bound = float(gold["ref_rel_max"])
    assert abs(mine["loss"] - float(gold[f"loss_{n}"])) <= 1e-4
    for i, g in enumerate(mine["grads"]):
        top = np.abs(g).max()
        assert np.abs(gold[f"val_{n}"][i] - g.reshape(-1)[gr.sample_index(i, g.shape)]).max() <= bound * top, i
        assert abs(gold[f"sum_{n}"][i] - g.sum()) <= bound * top * g.size, i
        assert abs(gold[f"l2_{n}"][i] - np.sqrt((g ** 2).sum())) <= bound * top * np.sqrt(g.size), i


def test_float32_restatement_is_as_close_as_the_reference(gold, base, weights):
    """grad_rules with dtype=torch.float32 (the yardstick tests/test_gpu_train_batches.py uses on inputs the fixture did not measure) is
    fp32 arithmetic of the reference's kind: within ref_rel_max of the reference's own fp32 gradients at N = 17; float64 is the default"""
    import torch
    x, cls = er.synthetic_windows(base, FULL)
    f32 = gr.loss_and_grad(weights, x, cls, dtype=torch.float32)
    assert all(g.dtype == np.float32 for g in f32["grads"]) and f32["site_loss"].dtype == np.float32
    assert all(g.dtype == np.float64 for g in gr.loss_and_grad(weights, x[:1], cls[:1])["grads"])
    dist = [gr.rel_dist(g, gold[f"g{FULL}_{i:02d}"]) for i, g in enumerate(f32["grads"])]
    print("float32 restatement against the reference's fp32 gradients, N = 17: " + " ".join(f"{d:.1e}" for d in dist))
    assert max(dist) <= float(gold["ref_rel_max"]), dist
    assert abs(f32["loss"] - float(gold[f"loss_{FULL}"])) <= 1e-4


def test_a_lost_site_is_visible_at_a_large_batch(gold, base, weights):
    """What the parity bound of the GPU tests (max |diff| / max |tensor| <= 4 x ref_rel_max per tensor) can see at N = 1040.  With g the
    gradient of the batch and g_j that of site j alone (N = 1), a kernel that loses site j changes a tensor by g_j / N.  For the sites
    next to the cuts of the 1,024-row slices (31: layer-0 rows 1023 | 1024; 60: layer-1 rows 1020..1036; 62: layer-0 row 2048; 1023 and
    1024: the dense layers' and heads' cut; 0, 1039: the ends) and nine seeded others, max |g_j| / (N max |g|) is at least four times
    the bound for tensors 0 to 21: a lost site fails the GPU test with room to spare.

    NOT so for the zygosity head (tensors 22 and 23): three classes, so a site whose prediction is confident contributes little, and the
    ratio falls to the bound's own size for some sites (1.1e-5 measured over 80 sites).  A single lost site can hide there; only the
    median over the chosen sites is asserted.  What guards those two tensors against a lost slice is that a slice holds 16 to 1,024
    sites, not one."""
    n = 1040
    bound = 4.0 * float(gold["ref_rel_max"])
    x, cls = er.synthetic_windows(base, n)
    sites = [0, 30, 31, 32, 60, 62, 1023, 1024, 1039] + sorted(np.random.default_rng(1040).choice(n, 7, replace=False).tolist())
    assert len(sites) == 16
    top = np.array([np.abs(g).max() for g in gr.loss_and_grad(weights, x, cls)["grads"]])
    ratio = np.array([[np.abs(g).max() for g in gr.loss_and_grad(weights, x[j:j + 1], cls[j:j + 1])["grads"]] for j in sites]) / (n * top)
    print("lost-site ratio max |g_j| / (N max |g|), smallest over the sites per tensor: " + " ".join(f"{v:.1e}" for v in ratio.min(0)) +
          "; median of tensors 22, 23: " + " ".join(f"{v:.1e}" for v in np.median(ratio[:, 22:], axis=0)) + f"; bound {bound:.3e}")
    assert ratio[:, :22].min() >= 4.0 * bound, ratio[:, :22].min(0)
    assert (np.median(ratio[:, 22:], axis=0) >= 4.0 * bound).all()


def test_bias_gradients_are_equal_pairs(base, weights):
    x, cls = er.synthetic_windows(base, 5)
    g = gr.loss_and_grad(weights, x, cls)["grads"]
    for a, b in gr.BIAS_PAIRS:
        assert np.array_equal(g[a], g[b]) and np.abs(g[a]).max() > 0


def test_masked_gradient_agrees_with_finite_differences(base, weights):
    """A seeded keep mask at p = 0.3 (scale 1 / 0.7), which the reference cannot be made to reproduce: central differences in float64 on
    seeded entries of every tensor against autograd.

    Step and bound.  d(h) = (L(w + h) - L(w - h)) / 2h = L' + h^2 L''' / 6 + O(h^4).  With h = 1e-5 and 2h the extrapolation
    (4 d(h) - d(2h)) / 3 cancels the h^2 term; what is left is the h^4 term, smaller than the h^2 term |d(2h) - d(h)| / 3 by another factor
    of the order (h / scale of the weight)^2 - a tenth of |d(2h) - d(h)| is a generous cover for it.  Rounding: L <= 8 is evaluated to
    about 1e-15 (a few thousand float64 operations deep), four evaluations divided by 2h = 2e-5 give 2e-10; the bound grants ten times that."""
    n, p, h = 3, 0.3, 1e-5
    x, cls = er.synthetic_windows(base, n)
    mask = (np.random.default_rng(77).random((n, 33, 128)) >= p).astype(np.uint8)
    assert 0.6 < mask.mean() < 0.8
    w = [np.asarray(t, np.float64) for t in weights]
    auto = gr.loss_and_grad(w, x, cls, mask, 1.0 / (1.0 - p))
    plain = gr.loss_and_grad(w, x, cls)
    assert gr.rel_dist(auto["grads"][0], plain["grads"][0]) > 1e-2           # (the mask is in the function)
    rng = np.random.default_rng(78)

    def at(i, j, delta):
        moved = [t if k != i else t.copy() for k, t in enumerate(w)]
        moved[i].reshape(-1)[j] += delta
        return gr.loss_only(moved, x, cls, mask, 1.0 / (1.0 - p))

    for i, t in enumerate(w):
        for j in rng.integers(0, t.size, 2):
            d1 = (at(i, j, h) - at(i, j, -h)) / (2 * h)
            d2 = (at(i, j, 2 * h) - at(i, j, -2 * h)) / (4 * h)
            fd = (4 * d1 - d2) / 3
            assert abs(fd - auto["grads"][i].reshape(-1)[j]) <= 2e-9 + 0.1 * abs(d2 - d1), (i, j, fd, auto["grads"][i].reshape(-1)[j])


def test_sgd_helper_descends(base, weights):
    x, cls = er.synthetic_windows(base, 4)
    losses, w = gr.sgd_steps(weights, x, cls, 0.05, 2)
    assert losses.shape == (3,) and losses[2] < losses[1] < losses[0] and len(w) == 24


def test_new_entries_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "nanosnp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nsnp_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(os.path.join(ROOT, "nanosnp_amd", "libnanosnp_hip.so"))
    from nanosnp_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTS, name
    assert [tuple(s) for s in _lib.Context.TRAIN_SHAPES] == gr.SHAPES
    assert hasattr(_lib.Context, "pileup_train_reserve") and hasattr(_lib.Context, "pileup_loss_grad")
    from nanosnp_amd import train
    assert len(train.PARAM_NAMES) == 24 and train.PARAM_NAMES[0] == "encoder.lstm.weight_ih_l0" and train.PARAM_NAMES[-1] == "forward_layer.zygosity_layer.bias"
