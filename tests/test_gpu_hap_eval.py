"""Scoring a HaplotypeModel checkpoint on the device: the label pass (nsnp_hap_label_classes), the forward with the scoring heads
(nsnp_hap_eval) under all three arithmetics, the batch sums (nsnp_hap_batch_loss), haplotype_model.LSTMNetwork.forward and
evaluate.evaluate_haplotype_bins - against what the reference's own code computed (tests/golden/hap_eval.npz) and against the float64 rules
(tests/hap_eval_rules.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from nanosnp_amd import _lib, evaluate, sitefile
from tests import hap_eval_rules as hr
from tests.helpers import PROB_ATOL, seeded_hap_weights
from tests.test_hap_eval_rules import FILES_WEIGHTS, eval_case, eval_case_f64, file_features, labelled_files

pytestmark = pytest.mark.gpu
PRECISIONS = (0, 1, 2)


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _model(case=None, weights=None, dims=(105, 10, 3)):
    from nanosnp_amd.haplotype_model import LSTMNetwork
    F, n_gt, n_zy = (case["F"], case["n_gt"], case["n_zy"]) if case else dims
    m = LSTMNetwork({"model": {"pileup_dim": F, "haplotype_dim": F, "pileup_length": 33, "haplotype_length": 11, "hidden_size": 256,
                               "lstm_layers": 3, "gt_num_class": n_gt, "zy_num_class": n_zy}})
    m.ctx.set_option("hap_pass_sites", 1024)                 # (the workspace of these tests: 0.2 GB instead of 3.2 GB)
    m.load_weight_list(case["weights"] if case else weights)
    return m


@pytest.fixture(scope="module")
def models():
    made = {tag: _model(eval_case(tag)) for tag in ("main", "dims")}
    yield made
    for m in made.values():
        m.ctx.close()


@pytest.fixture
def precision(request, models):
    """sets hap_precision on both models for one test, fp32 again afterwards"""
    for m in models.values():
        m.ctx.set_option("hap_precision", request.param)
    yield request.param
    for m in models.values():
        m.ctx.set_option("hap_precision", 0)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- label pass -------------------------------------------------------------------------------------------------------------------------
BRANCH_ROWS = np.array([[0, 1, -1], [1, 2, 0], [1, 2, -2], [1, 4, 3], [1, 4, 9], [1, 4, 10], [1, 9, -1], [1, 10, -1], [1, 65, 1], [1, -1, 2],
                        [1, 0, -1], [1, 1, 1], [1, 2, 2], [2, 1, 1], [1, 9, 2]], np.int32)


def _pattern(name, n, rng):
    kept = np.stack([np.ones(n), rng.integers(0, 10, n), rng.choice([-1, 1, 2], n)], axis=1).astype(np.int32)
    dropped = kept.copy(); dropped[:, 0] = 0
    if name == "none":
        return dropped
    if name == "all":
        return kept
    if name == "last":
        dropped[-1] = kept[-1]
        return dropped
    if name == "alternating":
        kept[::2] = dropped[::2]
        return kept
    return BRANCH_ROWS[rng.integers(0, len(BRANCH_ROWS), n)]          # seeded: every branch


def _label_pass(torch, ctx, y):
    n = y.shape[0]
    cls = torch.full((n + 8, 2), 0xAB, dtype=torch.uint8, device="cuda")
    rows = torch.full((n + 8,), -7, dtype=torch.int64, device="cuda")
    _, _, meta = ctx.hap_label_classes(_dev(torch, y), cls=cls, rows=rows)
    return cls.cpu().numpy(), rows.cpu().numpy(), meta.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 65537])
def test_label_pass_equals_the_rules_and_writes_nothing_behind_the_kept_rows(torch_, models, n):
    ctx = models["main"].ctx
    rng = np.random.default_rng(n)
    for name in ("none", "all", "last", "alternating", "seeded"):
        y = _pattern(name, n, rng)
        cls, rows, meta = _label_pass(torch_, ctx, y)
        want_rows, want_cls, want_meta = hr.label_filter(y)
        k = want_rows.size
        assert meta.tolist() == want_meta.tolist(), (name, n)
        assert np.array_equal(rows[:k], want_rows) and np.array_equal(cls[:k], want_cls), (name, n)
        assert (cls[k:] == 0xAB).all() and (rows[k:] == -7).all(), (name, n)
        if name == "all":
            assert k == n
        if name == "last":
            assert rows[:k].tolist() == [n - 1]


def test_label_pass_branches_under_two_models(torch_, models):
    y = np.concatenate([BRANCH_ROWS, BRANCH_ROWS[::-1]])
    cls, rows, meta = _label_pass(torch_, models["main"].ctx, y)
    want_rows, want_cls, want_meta = hr.label_filter(y, 10, 3)
    assert meta.tolist() == want_meta.tolist() == [10, 6, 4, 6] and np.array_equal(rows[:10], want_rows) and np.array_equal(cls[:10], want_cls)
    # a model with three genotype classes: gt 3.. becomes unscorable
    small = _model(weights=seeded_hap_weights(5, F=16, n_gt=3, n_zy=3), dims=(16, 3, 3))
    try:
        cls, rows, meta = _label_pass(torch_, small.ctx, y)
        want_rows, want_cls, want_meta = hr.label_filter(y, 3, 3)
        k = want_rows.size
        assert meta.tolist() == want_meta.tolist() and k == 6 and meta[1] == 10
        assert np.array_equal(rows[:k], want_rows) and np.array_equal(cls[:k], want_cls) and (rows[k:] == -7).all()
    finally:
        small.ctx.close()


# ---- logits, loss and pred against the reference's numbers ------------------------------------------------------------------------------
def _eval(torch, model, xp, xh, cls, counters=None, want_logits=True):
    ctx = model.ctx
    counters = counters if counters is not None else ctx.hap_eval_counters()
    loss, pred, z = ctx.hap_eval(xp, xh, cls, counters, want_logits=want_logits)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), pred.cpu().numpy(), (z.cpu().numpy() if z is not None else None), counters.cpu().numpy()


def _check_against_own_logits(z, loss, pred, counters, cls, n_gt, n_zy, what):
    """loss, pred and counters follow the rules applied to the entry's own logits; -> the largest loss distance"""
    assert np.array_equal(pred, hr.predictions(z, n_gt)), what                       # the first argmax of its OWN logits, exactly and everywhere
    d = float(np.abs(hr.smoothed_loss(z, cls, n_gt) - loss).max())
    gcm, zcm = hr.confusion(cls, pred, n_gt, n_zy)
    assert np.array_equal(counters, np.concatenate([gcm.reshape(-1), zcm.reshape(-1)])), what
    return d


@pytest.mark.parametrize("tag", ["main", "dims"])
@pytest.mark.parametrize("precision", PRECISIONS, indirect=True)
def test_eval_equals_the_reference_forward_and_loss(torch_, models, precision, tag):
    """Bound: 1e-4 absolute on logits and per-site losses (helpers.PROB_ATOL), under every hap_precision.  Measured on an MI355X, largest
    distance to the reference's fp32 logits / per-site losses (docs/rounds/r22.md; printed by this test):
        main   hap_precision 0: 8.3e-7 / 7.2e-7    1 (f16x3): 7.4e-6 / 4.8e-6    2 (bf16x3): 7.7e-7 / 9.5e-7
        dims   hap_precision 0: 1.4e-5 / 1.0e-5    1 (f16x3): 5.5e-5 / 5.8e-5    2 (bf16x3): 1.5e-5 / 1.3e-5
    (dims runs the scaled weights, head rows x 120.)  No site of either case lies within the argmax margin, so every pred equals the float64
    argmax."""
    c, m = eval_case(tag), models[tag]
    n_gt, n_zy = c["n_gt"], c["n_zy"]
    loss, pred, z, counters = _eval(torch_, m, _dev(torch_, c["xp"]), _dev(torch_, c["xh"]), _dev(torch_, c["cls"]))
    dz, dl = float(np.abs(z - c["logits"]).max()), float(np.abs(loss - c["site_loss"]).max())
    z64 = eval_case_f64(tag)
    print(f"hap_eval {tag} hap_precision {precision}: |logits - reference| = {dz:.3e}, |loss - reference| = {dl:.3e}, "
          f"|logits - float64| = {np.abs(z - z64).max():.3e}")
    assert dz <= PROB_ATOL and dl <= PROB_ATOL
    assert _check_against_own_logits(z, loss, pred, counters, c["cls"], n_gt, n_zy, tag) <= 1e-5
    near = hr.margins(z64, n_gt) < hr.MARGIN
    assert near.any(1).mean() <= hr.MARGIN_SHARE
    assert ((pred == hr.predictions(z64, n_gt)) | near).all()
    # what the model said is what nsnp_hap_forward says
    gt, zy = m.predict(_dev(torch_, c["xp"]), _dev(torch_, c["xh"]))
    sm = lambda a: np.exp(a - a.max(1, keepdims=True)) / np.exp(a - a.max(1, keepdims=True)).sum(1, keepdims=True)
    assert np.abs(sm(z[:, :n_gt].astype(np.float64)) - gt.cpu().numpy()).max() <= PROB_ATOL
    assert np.abs(sm(z[:, n_gt:].astype(np.float64)) - zy.cpu().numpy()).max() <= PROB_ATOL


# ---- shapes at which the kernels can still go wrong -------------------------------------------------------------------------------------
def _random_inputs(torch, n, F, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    xp = torch.randn((n, F, 33), generator=g, device="cuda") * 40
    xh = torch.randn((n, F, 11), generator=g, device="cuda") * 40
    return xp, xh


def _self_consistent(torch, model, n, seed, n_gt=10, n_zy=3):
    xp, xh = _random_inputs(torch, n, model.dims["pileup_dim"], seed)
    rng = np.random.default_rng(seed)
    cls = np.stack([rng.integers(0, n_gt, n), rng.integers(0, n_zy, n)], axis=1).astype(np.uint8)
    loss, pred, z, counters = _eval(torch, model, xp, xh, _dev(torch, cls))
    d = _check_against_own_logits(z, loss, pred, counters, cls, n_gt, n_zy, n)
    gt, zy = model.predict(xp, xh)
    sm = lambda a: np.exp(a - a.max(1, keepdims=True)) / np.exp(a - a.max(1, keepdims=True)).sum(1, keepdims=True)
    dp = max(float(np.abs(sm(z[:, :n_gt].astype(np.float64)) - gt.cpu().numpy()).max()),
             float(np.abs(sm(z[:, n_gt:].astype(np.float64)) - zy.cpu().numpy()).max()))
    print(f"hap_eval N = {n}: |loss - rules(own logits)| = {d:.3e}, |softmax(own logits) - hap_forward| = {dp:.3e}")
    assert d <= 1e-5 and dp <= PROB_ATOL
    assert counters.sum() == 2 * n
    return z


@pytest.mark.parametrize("n", [1, 3, 4, 5, 127, 128, 129])
def test_eval_at_the_edges_of_the_site_tile(torch_, models, n):
    """loss against the rules on the entry's own logits: bound 1e-5 (measured over these N, 8,197 and the two-pass case: at most 6.1e-7);
    float64 softmax of those logits against nsnp_hap_forward's probabilities: bound PROB_ATOL (measured: at most 4.2e-8)"""
    _self_consistent(torch_, models["main"], n, 100 + n)


def test_eval_heads_take_a_second_partial_trip(torch_, models):
    """the scoring heads are persistent: multi_processor_count * HAP_EVAL_WAVES_PER_CU waves take one site each per trip"""
    waves = torch_.cuda.get_device_properties(0).multi_processor_count * _lib.Context.HAP_EVAL_WAVES_PER_CU
    ctx = models["main"].ctx
    n = waves + 5
    ctx.set_option("hap_pass_sites", ((n + 127) // 128) * 128)           # one forward pass: one heads launch over all n sites
    try:
        _self_consistent(torch_, models["main"], n, 7)
    finally:
        ctx.set_option("hap_pass_sites", 1024)


@pytest.mark.parametrize("precision", PRECISIONS, indirect=True)
def test_eval_loops_over_two_forward_passes(torch_, models, precision):
    ctx = models["main"].ctx
    ctx.set_option("hap_pass_sites", 128)                                # the smallest value the option accepts
    try:
        _self_consistent(torch_, models["main"], 129, 11)
    finally:
        ctx.set_option("hap_pass_sites", 1024)


# ---- other properties of the entry ------------------------------------------------------------------------------------------------------
def test_eval_without_logits_adds_to_counters_and_repeats_its_bits(torch_, models):
    c, m = eval_case("main"), models["main"]
    xp, xh, cls = _dev(torch_, c["xp"]), _dev(torch_, c["xh"]), _dev(torch_, c["cls"])
    loss, pred, z, counters = _eval(torch_, m, xp, xh, cls)
    loss2, pred2, z2, counters2 = _eval(torch_, m, xp, xh, cls)
    assert loss.tobytes() == loss2.tobytes() and pred.tobytes() == pred2.tobytes() and z.tobytes() == z2.tobytes()
    assert np.array_equal(counters, counters2)
    loss3, pred3, z3, counters3 = _eval(torch_, m, xp, xh, cls, want_logits=False)
    assert z3 is None and loss.tobytes() == loss3.tobytes() and pred.tobytes() == pred3.tobytes() and np.array_equal(counters, counters3)
    start = np.arange(counters.size, dtype=np.int64) * 1000 + 1
    acc = _dev(torch_, start)
    _eval(torch_, m, xp, xh, cls, counters=acc)
    *_, twice = _eval(torch_, m, xp, xh, cls, counters=acc)
    assert np.array_equal(twice, start + 2 * counters)


def test_targets_outside_a_head_count_as_its_last_class(torch_, models):
    c, m = eval_case("main"), models["main"]
    xp, xh = _dev(torch_, c["xp"][:8]), _dev(torch_, c["xh"][:8])
    wild = np.array([[10, 3], [200, 255], [9, 2], [0, 0], [77, 1], [3, 9], [255, 255], [5, 2]], np.uint8)
    clamped = np.minimum(wild, np.array([9, 2], np.uint8))
    a, b = _eval(torch_, m, xp, xh, _dev(torch_, wild)), _eval(torch_, m, xp, xh, _dev(torch_, clamped))
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert _check_against_own_logits(a[2], a[0], a[1], a[3], wild, 10, 3, "wild") <= 1e-5


def test_status_codes(torch_, models):
    lib = _lib.load()
    c, m = eval_case("main"), models["main"]
    xp, xh, cls = _dev(torch_, c["xp"][:4]), _dev(torch_, c["xh"][:4]), _dev(torch_, c["cls"][:4])
    loss = torch_.empty((4, 2), dtype=torch_.float32, device="cuda"); pred = torch_.empty((4, 2), dtype=torch_.uint8, device="cuda")
    counters = m.ctx.hap_eval_counters()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda h, *a: lib.nsnp_hap_eval(h, p(a[0]), p(a[1]), p(a[2]), a[3], p(a[4]), p(a[5]), p(a[6]), None, None)
    EINVAL, ENOWEIGHTS = -1, -4                                                      # include/nanosnp.h
    bare = _lib.Context(0)
    try:
        assert call(bare.handle, xp, xh, cls, 4, loss, pred, counters) == ENOWEIGHTS
        meta = torch_.zeros(4, dtype=torch_.int64, device="cuda")
        assert lib.nsnp_hap_label_classes(bare.handle, None, 0, None, None, p(meta), None) == ENOWEIGHTS
    finally:
        bare.close()
    h = m.ctx.handle
    assert call(h, None, None, None, 0, None, None, None) == 0                       # N == 0
    for k in range(7):
        if k == 3:
            continue
        a = [xp, xh, cls, 4, loss, pred, counters]
        a[k] = None
        assert call(h, *a) == EINVAL, k
    assert call(h, xp, xh, cls, -1, loss, pred, counters) == EINVAL
    assert call(h, xp, xh, cls, 4, loss, pred, counters) == 0
    assert lib.nsnp_hap_batch_loss(h, p(loss), 4, 0, p(loss), None) == EINVAL
    assert lib.nsnp_hap_batch_loss(h, None, 0, 4, None, None) == 0
    assert lib.nsnp_hap_label_classes(h, None, 4, None, None, None, None) == EINVAL
    torch_.cuda.synchronize()


def test_batch_sums_are_float64_trees(torch_, models):
    ctx = models["main"].ctx
    n = 1337
    rng = np.random.default_rng(3)
    loss = (rng.random((n, 2)) * 5).astype(np.float32)
    d = _dev(torch_, loss)
    for B in (1, 4, 512, n + 1):
        got = ctx.hap_batch_loss(d, B).cpu().numpy()
        nb = -(-n // B)
        want = np.array([loss[b * B:(b + 1) * B].astype(np.float64).sum(0) for b in range(nb)])
        assert got.shape == (nb, 2) and got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
        assert got.tobytes() == ctx.hap_batch_loss(d, B).cpu().numpy().tobytes()
    assert n % 4 and n % 512                                                        # short last batches


# ---- LSTMNetwork.forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["main", "dims"])
def test_model_forward_equals_the_reference_batch_losses(torch_, models, tag):
    """batches of 4 against the reference's loss.item(): bound PROB_ATOL (measured: main 4.8e-7, dims 7.6e-6)"""
    c, m = eval_case(tag), models[tag]
    B, worst = c["batch_size"], 0.0
    for b, a in enumerate(range(0, c["xp"].shape[0], B)):
        t = [_dev(torch_, c["cls"][a:a + B, h].astype(np.int64)) for h in range(2)]
        loss, gz, zz = m.forward(_dev(torch_, c["xp"][a:a + B]), _dev(torch_, c["xh"][a:a + B]), t[0], t[1])
        assert loss.dtype == torch_.float32 and loss.dim() == 0 and gz.shape == (B, c["n_gt"]) and zz.shape == (B, c["n_zy"])
        worst = max(worst, abs(float(loss) - c["batch_loss"][b]))
        assert np.abs(np.concatenate([gz.cpu().numpy(), zz.cpu().numpy()], 1) - c["logits"][a:a + B]).max() <= PROB_ATOL
    print(f"LSTMNetwork.forward {tag}: |loss - reference| = {worst:.3e}")
    assert worst <= PROB_ATOL
    F = c["F"]
    e = torch_.empty
    loss, gz, zz = m.forward(e((0, F, 33), device="cuda"), e((0, F, 11), device="cuda"), e(0, dtype=torch_.int64, device="cuda"),
                             e(0, dtype=torch_.int64, device="cuda"))
    assert bool(torch_.isnan(loss)) and gz.shape == (0, c["n_gt"]) and zz.shape == (0, c["n_zy"])


# ---- evaluate_haplotype_bins ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored_files(tmp_path_factory):
    """the three labelled files, the model, and the float64 rules on oracle features - computed once"""
    from nanosnp_amd.hap_pipeline import DeviceReference
    d = tmp_path_factory.mktemp("hap_eval_bins")
    files = labelled_files(d)
    ws = seeded_hap_weights(**FILES_WEIGHTS)
    model = _model(weights=ws)
    refs = {}
    for f in files:
        refs.update(f["refs"])
    want = hr.evaluate(ws, [(*file_features(f), f["labels"]) for f in files], 16)
    yield dict(files=files, model=model, reference=DeviceReference(refs, 0), want=want, dir=d)
    model.ctx.close()


INT_KEYS = ("sites", "refcalls", "variants", "unscorable_labels")
FLOAT_KEYS = ("loss", "mean_loss", "gt_loss", "zy_loss", "batch_accuracy", "gt_accuracy", "gt_recall", "gt_precision", "gt_f1", "zy_accuracy",
              "zy_recall", "zy_precision", "zy_f1")


def test_evaluate_haplotype_bins_equals_the_rules(torch_, scored_files):
    s = scored_files
    paths = [f["path"] for f in s["files"]]
    st = {}
    res = evaluate.evaluate_haplotype_bins(s["model"], paths, s["reference"], batch_size=16, pass_sites=64, keep_sites=True, stats=st)
    want = s["want"]
    assert st["rows"] == sum(f["labels"].shape[0] for f in s["files"]) and st["passes"] == 3 + 2 + 1 and 0 < st["passes_int8"] < st["passes"]
    for k in INT_KEYS:
        assert res[k] == want[k], k
    assert res["sites"] == res["refcalls"] + res["variants"] > 100 and res["unscorable_labels"] > 0
    # the margin rule: no kept site of these files lies within it (the fixture maker checked), so every integer is equal
    assert all((hr.margins(z, 10) >= hr.MARGIN).all() for _, _, z in want["detail"])
    assert np.array_equal(res["gt_confusion"], want["gt_confusion"]) and np.array_equal(res["zy_confusion"], want["zy_confusion"])
    assert res["gt_confusion"].dtype == np.int64 and res["gt_confusion"].shape == (10, 10) and res["zy_confusion"].shape == (3, 3)
    assert np.count_nonzero(res["gt_confusion"].sum(0)) >= 2                          # predictions that differ from site to site
    for k in FLOAT_KEYS:
        print(f"evaluate_haplotype_bins {k}: {res[k]:.6f} (rules {want[k]:.6f})")
        assert abs(res[k] - want[k]) <= 1e-4, k
    assert res["gt_accuracy"] == 100.0 * np.trace(res["gt_confusion"]) / res["sites"]
    # keep_sites: file rows in order, the rules' classes, predictions and losses
    assert [f["path"] for f in res["files"]] == paths
    for got, (rows, cls, z), (loss, _, pred) in zip(res["files"], want["detail"], want["parts"]):
        assert np.array_equal(got["rows"], rows) and np.array_equal(got["cls"], cls) and np.array_equal(got["pred"], pred)
        assert got["site_loss"].shape == (rows.size, 2) and (rows.size == 0 or np.abs(got["site_loss"] - loss).max() <= 1e-4)
    assert res["files"][2]["rows"].size == 0
    line = evaluate.format_haplotype_report(res)
    assert line.startswith("AverageLoss: %.5f, GT:|Recall: " % res["loss"]) and line.endswith("ACC: %.4f" % res["batch_accuracy"])
    # the pass size does not change a result
    for P in (16384, 7):
        other = evaluate.evaluate_haplotype_bins(s["model"], paths, s["reference"], batch_size=16, pass_sites=P, keep_sites=True)
        for k in INT_KEYS + FLOAT_KEYS:
            assert other[k] == res[k], (P, k)
        assert np.array_equal(other["gt_confusion"], res["gt_confusion"]) and np.array_equal(other["zy_confusion"], res["zy_confusion"])
        for a, b in zip(other["files"], res["files"]):
            assert all(a[k].tobytes() == b[k].tobytes() for k in ("rows", "cls", "pred", "site_loss"))
    # a directory: its files in os.listdir order; the last file with a batch sets the divisor of `loss`
    import os
    by_dir = evaluate.evaluate_haplotype_bins(s["model"], str(s["dir"]), s["reference"], batch_size=16, pass_sites=64)
    order = [os.path.join(str(s["dir"]), f) for f in os.listdir(str(s["dir"]))]
    again = evaluate.evaluate_haplotype_bins(s["model"], order, s["reference"], batch_size=16, pass_sites=64)
    assert by_dir["loss"] == again["loss"] and by_dir["sites"] == res["sites"] and np.array_equal(by_dir["gt_confusion"], res["gt_confusion"])


def test_labelled_files_feed_the_predict_path(torch_, scored_files, tmp_path):
    """a labelled file stays a valid input of read_haplotype_bin, HapBinSource and predict_haplotype_bins, which ignore the extra array"""
    from nanosnp_amd.hap_pipeline import HapBinSource, predict_haplotype_bins
    s = scored_files
    f = s["files"][0]
    cand, hpos, planes = sitefile.read_haplotype_bin(f["path"])
    assert cand == f["cands"]
    src = HapBinSource(f["path"]); assert src.n == len(cand); src.close()
    plain = tmp_path / "plain.bin"
    sitefile.write_haplotype_bin(plain, cand, hpos, {k: np.asarray(v) for k, v in planes.items()})
    a, b = tmp_path / "a.csv", tmp_path / "b.csv"
    assert predict_haplotype_bins(s["model"].ctx, [f["path"]], s["reference"], str(a)) == len(cand)
    assert predict_haplotype_bins(s["model"].ctx, [str(plain)], s["reference"], str(b)) == len(cand)
    assert a.read_bytes() == b.read_bytes() and a.stat().st_size > 0


def test_evaluate_refusals(torch_, scored_files, tmp_path, monkeypatch):
    s = scored_files
    f = s["files"][0]
    cand, hpos, planes = sitefile.read_haplotype_bin(f["path"])
    plain = tmp_path / "plain.bin"
    sitefile.write_haplotype_bin(plain, cand, hpos, {k: np.asarray(v) for k, v in planes.items()})
    with pytest.raises(sitefile.SiteFileError, match="candidate_labels"):
        evaluate.evaluate_haplotype_bins(s["model"], [f["path"], str(plain)], s["reference"])
    with pytest.raises(ValueError):
        evaluate.evaluate_haplotype_bins(s["model"], [f["path"]], s["reference"], batch_size=0)
    from nanosnp_amd.haplotype_model import LSTMNetwork
    with pytest.raises(_lib.NanoSNPError):
        evaluate.evaluate_haplotype_bins(LSTMNetwork(None, ctx=s["model"].ctx), [f["path"]], s["reference"])
    import torch.distributed as tdist
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError):
        evaluate.evaluate_haplotype_bins(s["model"], [f["path"]], s["reference"])
