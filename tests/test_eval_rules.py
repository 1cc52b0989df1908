"""tests/eval_rules.py (the float64 restatement of the reference's eval(), PileupModel/train.py:93-150) reproduces everything the reference's
own model code wrote into tests/golden/pileup_eval.npz, and the library declares and exports the scoring entries.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import eval_rules as er
from tests.helpers import ROOT, golden, load_pileup_weights

SETS = (("g1", "train_g1"), ("cut", "train_cut"))
NEW_SYMBOLS = ("nsnp_pileup_load_indel_heads", "nsnp_pileup_label_classes", "nsnp_pileup_forward_logits", "nsnp_pileup_eval_windows",
               "nsnp_pileup_batch_loss")


@pytest.fixture(scope="module")
def gold():
    return np.load(golden("pileup_eval.npz"))


@pytest.fixture(scope="module")
def indel(gold):
    return [gold["indel1_weight"], gold["indel1_bias"], gold["indel2_weight"], gold["indel2_bias"]]


@pytest.fixture(scope="module")
def sets(tmp_path_factory, gold, indel):
    """per set: windows, labels and the float64 logits of all rows - computed once"""
    d = str(tmp_path_factory.mktemp("eval_rules"))
    w = load_pileup_weights()
    out = {}
    for tag, case in SETS:
        _, x, label = er.fixture_rows(case, d)
        out[tag] = (x, label, er.forward_logits_f64(w, indel, x))
    return out


def test_fixture_inputs_are_admissible(gold):
    """an input may carry a 1e-4 test only if the reference's own fp32 result lies within a quarter of the bound of float64"""
    for key in ("dist_f64_g1", "dist_f64_cut", "synth_dist_f64"):
        assert float(gold[key]) <= 2.5e-5, key


def test_indel_tensors_are_the_checkpoints(gold):
    z = np.load(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"))
    for k in ("indel1", "indel2"):
        assert np.array_equal(z[f"forward_layer.{k}_layer.weight"], gold[f"{k}_weight"]) and np.array_equal(z[f"forward_layer.{k}_layer.bias"], gold[f"{k}_bias"])


@pytest.mark.parametrize("tag", ["g1", "cut"])
def test_logits_match_the_reference(gold, sets, tag):
    x, label, z64 = sets[tag]
    ref = gold[f"logits_{tag}"]
    assert ref.shape == (x.shape[0], 90)
    d = np.abs(z64 - ref).max()
    assert d <= 1e-4 and abs(d - float(gold[f"dist_f64_{tag}"])) <= 1e-9, d


@pytest.mark.parametrize("tag", ["g1", "cut"])
def test_filter_losses_and_predictions_per_set(gold, sets, tag):
    x, label, z64 = sets[tag]
    cls, bad = er.decode_labels(label)
    assert not bad.any()
    k = er.keep_rows(cls)
    assert np.array_equal(k, gold[f"variants_{tag}"])
    loss = er.smoothed_loss(z64[k], cls[k])
    assert np.abs(loss - gold[f"site_loss_{tag}"]).max() <= 1e-4
    assert np.array_equal(er.predictions(z64[k]), gold[f"pred_{tag}"])
    bm = er.batch_means(loss, int(gold["batch_size"]))
    assert bm.shape[0] == len(gold[f"batch_loss_{tag}"]) and np.abs(bm[:, 0] + bm[:, 1] - gold[f"batch_loss_{tag}"]).max() <= 1e-4


def test_run_over_both_files(gold, sets, indel):
    w = load_pileup_weights()
    B = int(gold["batch_size"])
    res = er.evaluate(w, indel, [sets["g1"][:2], sets["cut"][:2]], B)
    assert res["sites"] == int(gold["sites"]) and res["malformed_labels"] == 0
    assert abs(res["avg_loss"] - float(gold["avg_loss"])) <= 1e-4
    assert abs(res["avg_loss"] * res["sites"] - float(gold["total_loss"])) <= 1e-4 * 6      # (six batches, each mean within the bound)
    assert res["gt_accuracy"] == float(gold["gt_accuracy"]) and res["zy_accuracy"] == float(gold["zy_accuracy"])
    conf = gold["confusion"]
    for name, (_, c, o) in zip(er.NAMES, er.HEADS):
        assert np.array_equal(res[f"{name}_confusion"], conf[o:o + c * c].reshape(c, c)), name
    assert res["gt_confusion"].sum() == res["sites"] and abs(res["mean_loss"] - res["gt_loss"] - res["zy_loss"]) <= 1e-12


def test_batches_restart_with_every_file(gold, sets):
    """9 + 9 variants in batches of 4: per file 4, 4, 1 - not 4, 4, 4, 4, 2 over the concatenation"""
    B = int(gold["batch_size"])
    parts = []
    for tag in ("g1", "cut"):
        x, label, z64 = sets[tag]
        cls, _ = er.decode_labels(label)
        k = er.keep_rows(cls)
        parts.append((er.smoothed_loss(z64[k], cls[k]), cls[k], er.predictions(z64[k])))
    res = er.result_from(parts, B)
    assert [bm.shape[0] for bm in res["batch_means"]] == [3, 3]
    joined = er.result_from([tuple(np.concatenate([p[i] for p in parts]) for i in range(3))], B)
    assert joined["batch_means"][0].shape[0] == 5 and abs(joined["avg_loss"] - res["avg_loss"]) > 1e-3
    assert abs(res["avg_loss"] - float(gold["avg_loss"])) <= 1e-4 < abs(joined["avg_loss"] - float(gold["avg_loss"]))


def test_label_decode_ties_and_empty_slices():
    y = np.zeros((5, 90), np.int32)
    y[0, [3, 22, 24 + 16, 57 + 16]] = 1                      # one-hot everywhere
    y[1, [2, 5]] = 1; y[1, 23] = 1; y[1, 30] = 1; y[1, 60] = 1        # two maxima in the genotype family: the first wins
    y[2, 20] = 1                                             # the other three families all zero: class 0, malformed
    y[3, [0, 21, 24, 57]] = 2                                # a single non-zero that is not 1: its argmax, malformed
    y[4, [7, 21, 56, 89]] = 1; y[4, 8] = -1                  # a negative beside the 1: malformed
    cls, bad = er.decode_labels(y)
    assert cls.tolist() == [[3, 1, 16, 16], [2, 2, 6, 3], [20, 0, 0, 0], [0, 0, 0, 0], [7, 0, 32, 32]]
    assert bad.tolist() == [False, True, True, True, True]
    c, centers, meta = er.label_classes(y, variants_only=True)
    assert c.tolist() == [[3, 1, 16, 16], [2, 2, 6, 3]] and centers.tolist() == [16, 49] and meta.tolist() == [2, 4, 0, 0]
    c, centers, meta = er.label_classes(y, variants_only=False)
    assert c.shape == (5, 4) and centers.tolist() == [16, 49, 82, 115, 148] and meta.tolist() == [5, 4, 0, 0]


def test_smoothed_loss_is_the_published_formula():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((7, 90)) * 4
    cls = np.stack([rng.integers(0, c, 7) for _, c, _ in er.HEADS], axis=1)
    loss = er.smoothed_loss(z, cls)
    for h, (r0, c, _) in enumerate(er.HEADS):
        for n in range(7):
            s = z[n, r0:r0 + c]
            lp = s - np.log(np.exp(s).sum())
            true_dist = np.full(c, 0.1 / (c - 1)); true_dist[cls[n, h]] = 0.9         # optim.py:141-143
            assert abs(loss[n, h] - float((-true_dist * lp).sum())) <= 1e-12


def test_new_entries_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "nanosnp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(nsnp_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(os.path.join(ROOT, "nanosnp_amd", "libnanosnp_hip.so"))
    from nanosnp_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTS, name
    assert re.search(r"#define\s+NSNP_EVAL_COUNTERS\s+2628\b", src) and _lib.Context.EVAL_COUNTERS == er.N_COUNTERS == 2628
    assert tuple(_lib.Context.EVAL_HEADS) == er.HEADS
