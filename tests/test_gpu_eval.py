"""Scoring a checkpoint on training windows on the device (nsnp_pileup_label_classes / forward_logits / eval_windows / batch_loss,
pileup_model.LSTMNetwork.forward, evaluate.evaluate_train_bins) against the reference's own numbers (tests/golden/pileup_eval.npz, written
by PileupModel's model code) and the float64 restatement tests/eval_rules.py.  Floats: 1e-4 absolute, the project's contract; every input
lies within 2.5e-5 of float64 in the reference's own fp32 arithmetic (the fixture records it), the rest of the bound is the kernel's.

Distances measured on an MI355X (docs/rounds/r20.md has the table): see the docstrings of the tests."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import eval_rules as er
from tests.helpers import ROOT, golden, load_pileup_weights

pytestmark = pytest.mark.gpu
ATOL = 1e-4
SETS = (("g1", "train_g1"), ("cut", "train_cut"))
DATA_NPZ = os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def gold():
    return np.load(golden("pileup_eval.npz"))


@pytest.fixture(scope="module")
def indel(gold):
    return [gold["indel1_weight"], gold["indel1_bias"], gold["indel2_weight"], gold["indel2_bias"]]


def _context(indel, chunk_sites=None, heads=True):
    from nanosnp_amd import _lib
    ctx = _lib.Context(0, chunk_sites)
    ctx.pileup_load_weights(load_pileup_weights())
    if heads:
        ctx.pileup_load_indel_heads(indel)
    return ctx


@pytest.fixture(scope="module")
def ctx(indel):
    c = _context(indel)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpu_eval"))
    return {tag: er.fixture_rows(case, d) for tag, case in SETS}              # tag -> (path of the .td.bin, windows, labels)


@pytest.fixture(scope="module")
def n_big():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 16 + 17      # second trip of the persistent loop, partial group


@pytest.fixture(scope="module")
def synth(sets, indel, n_big):
    """the seeded synthetic windows with random classes and their float64 logits / losses, once for every test"""
    n = max(n_big, 4097)
    x, cls = er.synthetic_windows(sets["cut"][1], n)
    z = er.forward_logits_f64(load_pileup_weights(), indel, x)
    return x, cls, z, er.smoothed_loss(z, cls)


def _eval(ctx, x, cls, logits=True, counters=None):
    import torch
    counters = counters if counters is not None else torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
    loss, pred, z = ctx.pileup_eval_windows(_dev(x), None, _dev(cls), counters, want_logits=logits)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), pred.cpu().numpy(), None if z is None else z.cpu().numpy(), counters.cpu().numpy()


# ---- 1. the label pass --------------------------------------------------------------------------------------------------------------
def _labels(n, pattern, seed=0):
    rng = np.random.default_rng([n, seed])
    cls = np.stack([rng.integers(0, c, n) for _, c, _ in er.HEADS], axis=1)
    keep = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "last": np.arange(n) == n - 1, "alternating": np.arange(n) % 2 == 1,
            "seeded": rng.random(n) < 0.15}[pattern]
    cls[:, 1] = np.where(keep, rng.integers(1, 3, n), 0)
    y = np.zeros((n, 90), np.int32)
    for h, (r0, _, _) in enumerate(er.HEADS):
        y[np.arange(n), r0 + cls[:, h]] = 1
    return y


def _label_pass(ctx, y, variants_only):
    """the entry on buffers 8 rows LONGER than N, guard-filled -> (meta, cls buffer, centre buffer)"""
    import torch
    n = y.shape[0]
    cls = torch.full((n + 8, 4), 0xEE, dtype=torch.uint8, device="cuda")
    cen = torch.full((n + 8,), -7, dtype=torch.int64, device="cuda")
    meta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    ctx.pileup_label_classes(_dev(y), variants_only, cls=cls[:n], center_idx=cen[:n], meta=meta)
    torch.cuda.synchronize()
    return meta.numpy().copy(), cls.cpu().numpy(), cen.cpu().numpy()


def _check_label_pass(ctx, y, variants_only):
    c, centers, meta = er.label_classes(y, variants_only)
    got_meta, got_cls, got_cen = _label_pass(ctx, y, variants_only)
    k = int(meta[0])
    assert got_meta.tolist() == meta.tolist()
    assert np.array_equal(got_cls[:k], c) and np.array_equal(got_cen[:k], centers)
    assert (got_cls[k:] == 0xEE).all() and (got_cen[k:] == -7).all()         # nothing behind the kept rows, nothing behind the buffers


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 65537])
def test_label_pass(ctx, n):
    for pattern in ("none", "all", "last", "alternating", "seeded"):
        _check_label_pass(ctx, _labels(n, pattern), True)
    _check_label_pass(ctx, _labels(n, "seeded", seed=1), False)


def test_label_pass_rows_that_are_not_one_hot(ctx):
    y = _labels(1025, "seeded", seed=2)
    rng = np.random.default_rng(9)
    rows = rng.choice(1025, 200, replace=False)
    y[rows[:50], rng.integers(0, 90, 50)] += 1               # a second 1, or a 2: ties resolve to the first maximum
    y[rows[50:100], 21:24] = 0                               # an all-zero family: class 0
    y[rows[100:150], :21] = 0
    y[rows[150:], rng.integers(24, 90, 50)] = -1
    assert er.decode_labels(y)[1].sum() >= 150
    _check_label_pass(ctx, y, True)
    _check_label_pass(ctx, y, False)


# ---- 2. logits against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["g1", "cut"])
def test_logits_against_the_reference(ctx, gold, sets, tag):
    """measured: max |logit - reference| 2.4e-6 (g1), 2.9e-6 (cut); softmax of rows 0..23 against nsnp_pileup_forward: 2.0e-7 at most"""
    import torch
    x = _dev(sets[tag][1])
    z = ctx.pileup_forward_logits(x)
    gt, zy = ctx.pileup_forward(x)
    torch.cuda.synchronize()
    z, gt, zy = z.cpu().numpy(), gt.cpu().numpy(), zy.cpu().numpy()
    d = np.abs(z - gold[f"logits_{tag}"]).max()
    print(f"{tag}: max |logit - reference| = {d:.3e}")
    assert d <= ATOL
    for a, b, p in ((0, 21, gt), (21, 24, zy)):
        s = z[:, a:b].astype(np.float64)
        e = np.exp(s - s.max(1, keepdims=True))
        sm = e / e.sum(1, keepdims=True)
        print(f"{tag}: max |softmax(logits[{a}:{b}]) - forward| = {np.abs(sm - p).max():.3e}")
        assert np.abs(sm - p).max() <= 1e-6
        top = np.sort(p, axis=1)
        clear = top[:, -1] != top[:, -2]
        assert np.array_equal(z[clear, a:b].argmax(1), p[clear].argmax(1))


# ---- 3. loss and counts ---------------------------------------------------------------------------------------------------------------
def test_loss_and_counts_against_the_reference(ctx, gold, sets):
    """measured: max |site loss - reference| 1.9e-6 (g1), 4.3e-6 (cut); batch means 1.4e-6 (g1), 8.9e-7 (cut)"""
    import torch
    B = int(gold["batch_size"])
    counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
    total, sites, all_cls, all_pred = 0.0, 0, [], []
    for tag in ("g1", "cut"):
        _, x, label = sets[tag]
        xd = _dev(x).view(-1, 18)
        cls, centers, meta = ctx.pileup_label_classes(_dev(label), True)
        torch.cuda.synchronize()
        k = int(meta[0])
        assert k == len(gold[f"variants_{tag}"]) and np.array_equal((centers[:k].cpu().numpy() - 16) // 33, gold[f"variants_{tag}"])
        loss, pred, _ = ctx.pileup_eval_windows(xd, centers[:k].contiguous(), cls, counters, n=k)
        sums = ctx.pileup_batch_loss(loss, B).cpu().numpy()
        loss = loss.cpu().numpy()
        print(f"{tag}: max |site loss - reference| = {np.abs(loss - gold[f'site_loss_{tag}']).max():.3e}")
        assert np.abs(loss - gold[f"site_loss_{tag}"]).max() <= ATOL
        sizes = np.minimum(B, k - B * np.arange(sums.shape[0]))
        means = (sums[:, 0] + sums[:, 1]) / sizes
        print(f"{tag}: max |batch mean - reference| = {np.abs(means - gold[f'batch_loss_{tag}']).max():.3e}")
        assert means.shape == gold[f"batch_loss_{tag}"].shape and np.abs(means - gold[f"batch_loss_{tag}"]).max() <= ATOL
        assert np.array_equal(pred.cpu().numpy(), gold[f"pred_{tag}"])
        total += float(means.sum()); sites += k
        all_cls.append(cls[:k].cpu().numpy()); all_pred.append(pred.cpu().numpy())
    assert sites == int(gold["sites"]) and abs(total / sites - float(gold["avg_loss"])) <= ATOL
    conf = counters.cpu().numpy()
    cls, pred = np.concatenate(all_cls), np.concatenate(all_pred)
    assert np.array_equal(conf[:450], gold["confusion"][:450])                                   # genotype and zygosity: the reference's
    assert np.trace(conf[:441].reshape(21, 21)) / sites == float(gold["gt_accuracy"])
    assert np.trace(conf[441:450].reshape(3, 3)) / sites == float(gold["zy_accuracy"])
    for h in (2, 3):                                                                             # the indel heads: np.add.at over pred and cls
        _, c, o = er.HEADS[h]
        want = np.zeros(c * c, np.int64)
        np.add.at(want, cls[:, h].astype(np.int64) * c + pred[:, h], 1)
        assert np.array_equal(conf[o:o + c * c], want)


# ---- 4. shapes where the heads kernel can go wrong ------------------------------------------------------------------------------------
def _check_shape(ctx, synth, n):
    x, cls, z64, loss64 = (a[:n] for a in synth)
    loss, pred, z, conf = _eval(ctx, x, cls)
    print(f"N = {n}: max |logit - f64| = {np.abs(z - z64).max():.3e}, max |loss - f64| = {np.abs(loss - loss64).max():.3e}")
    assert np.abs(z - z64).max() <= ATOL and np.abs(loss - loss64).max() <= ATOL
    assert np.array_equal(pred, er.predictions(z)) and np.array_equal(conf, er.confusion(cls, pred))
    # a second run: the same bits
    loss2, pred2, z2, conf2 = _eval(ctx, x, cls)
    assert loss2.tobytes() == loss.tobytes() and z2.tobytes() == z.tobytes() and np.array_equal(pred2, pred) and np.array_equal(conf2, conf)
    # without logits: the same losses and counts
    loss3, pred3, z3, conf3 = _eval(ctx, x, cls, logits=False)
    assert z3 is None and loss3.tobytes() == loss.tobytes() and np.array_equal(pred3, pred) and np.array_equal(conf3, conf)
    # two calls over the halves, into the same counters: bit for bit the one call
    import torch
    if n > 1:
        counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
        h = n // 2
        a = _eval(ctx, x[:h], cls[:h], counters=counters)
        b = _eval(ctx, x[h:], cls[h:], counters=counters)
        assert np.concatenate([a[0], b[0]]).tobytes() == loss.tobytes() and np.concatenate([a[2], b[2]]).tobytes() == z.tobytes()
        assert np.array_equal(np.concatenate([a[1], b[1]]), pred) and np.array_equal(b[3], conf)
    # forward_logits is the same forward
    zl = ctx.pileup_forward_logits(_dev(x)).cpu().numpy()
    assert zl.tobytes() == z.tobytes()


@pytest.mark.parametrize("n", [1, 15, 16, 17, "two trips"])
def test_heads_kernel_shapes(ctx, synth, n_big, n):
    """measured at N = 8209: max |logit - f64| 5.0e-6, max |loss - f64| 4.5e-6 (N = 4097 over a chunk boundary: 4.4e-6, 4.3e-6)"""
    _check_shape(ctx, synth, n_big if n == "two trips" else n)


def test_heads_kernel_across_a_chunk_boundary(indel, synth):
    c = _context(indel, chunk_sites=4096)
    try:
        _check_shape(c, synth, 4097)
    finally:
        c.close()


# ---- 5. the batch sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 4, 1000, 5000])
def test_batch_loss(ctx, batch):
    import torch
    n = 4099
    loss = (np.random.default_rng(3).random((n, 4)) * 20).astype(np.float32)
    d = _dev(loss)
    a = ctx.pileup_batch_loss(d, batch).cpu().numpy()
    b = ctx.pileup_batch_loss(d, batch).cpu().numpy()
    want = np.array([loss[o:o + batch].astype(np.float64).sum(0) for o in range(0, n, batch)])
    assert a.shape == want.shape == (-(-n // batch), 4)
    rel = np.abs(a - want).max() / np.abs(want).max()
    print(f"batch {batch}: relative distance to the float64 sum {rel:.1e}")
    assert rel <= 1e-12 and a.tobytes() == b.tobytes()
    assert ctx.pileup_batch_loss(d, batch, n=0).shape == (0, 4)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from nanosnp_amd import pileup_model
    return pileup_model.LSTMNetwork.from_npz(DATA_NPZ)


def _same(a, b, atol):
    assert set(a) - {"files", "batch_means"} == set(b) - {"files", "batch_means"}
    for k in a:
        if k in ("files", "batch_means"):
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        elif isinstance(a[k], float) and "accuracy" not in k:
            assert abs(a[k] - b[k]) <= atol, (k, a[k], b[k])
        else:
            assert a[k] == b[k], k


def test_evaluate_train_bins(model, gold, sets):
    from nanosnp_amd import evaluate
    B = int(gold["batch_size"])
    paths = [sets["g1"][0], sets["cut"][0]]
    parts = []
    for tag in ("g1", "cut"):
        cls = er.decode_labels(sets[tag][2])[0][gold[f"variants_{tag}"]]
        parts.append((gold[f"site_loss_{tag}"], cls, gold[f"pred_{tag}"]))
    want = er.result_from(parts, B)                          # the dict built from the reference's numbers
    assert abs(want["avg_loss"] - float(gold["avg_loss"])) <= 1e-6
    runs = {p: evaluate.evaluate_train_bins(model, paths, batch_size=B, pass_sites=p, keep_sites=True) for p in (4, 65536)}
    for p, got in runs.items():
        _same(got, want, ATOL)
        assert got["sites"] == 18 and abs(got["avg_loss"] - float(gold["avg_loss"])) <= ATOL
        for f, tag in zip(got["files"], ("g1", "cut")):
            assert np.array_equal(f["rows"], gold[f"variants_{tag}"]) and np.array_equal(f["pred"], gold[f"pred_{tag}"])
            assert np.array_equal(f["cls"], er.decode_labels(sets[tag][2])[0][f["rows"]]) and np.abs(f["site_loss"] - gold[f"site_loss_{tag}"]).max() <= ATOL
    _same(runs[4], runs[65536], 0.0)                         # the pass size changes nothing, to the bit
    for fa, fb in zip(runs[4]["files"], runs[65536]["files"]):
        assert all(fa[k].tobytes() == fb[k].tobytes() for k in ("rows", "cls", "pred", "site_loss"))
    # batches restart at the file boundary: one file of the same 18 sites gives 5 batches, not 3 + 3, and another avg_loss
    joined = er.result_from([tuple(np.concatenate([p[i] for p in parts]) for i in range(3))], B)
    assert abs(runs[4]["avg_loss"] - joined["avg_loss"]) > 1e-3
    line = evaluate.format_report(runs[4], 7)
    assert line == "-Validating-Epoch:7, | Zygosity Accuracy:%.5f F1-Score:%.5f | Genotype Accuracy:%.5f F1-Score:%.5f" % (
        (float(gold["zy_accuracy"]),) * 2 + (float(gold["gt_accuracy"]),) * 2)


def test_evaluate_every_row(model, gold, sets, indel):
    """variants_only=False counts every row; the losses against the float64 restatement of the same rows"""
    from nanosnp_amd import evaluate
    B = 1000
    got = evaluate.evaluate_train_bins(model, [sets["g1"][0], sets["cut"][0]], batch_size=B, variants_only=False, pass_sites=500)
    want = er.evaluate(load_pileup_weights(), indel, [sets["g1"][1:], sets["cut"][1:]], B, variants_only=False)
    assert got["sites"] == sets["g1"][1].shape[0] + sets["cut"][1].shape[0] == 1369
    _same(got, want, ATOL)


def test_evaluate_refusals(model, sets, tmp_path):
    import gzip
    from nanosnp_amd import _lib, evaluate, pileup_model, sitefile
    pd = str(tmp_path / "x.pd.bin")
    sitefile.pd_to_bin(gzip.open(golden("encode_g1.pd.gz")).read(), pd)
    with pytest.raises(sitefile.SiteFileError, match="label"):
        evaluate.evaluate_train_bins(model, [sets["g1"][0], pd])
    bare = pileup_model.LSTMNetwork().load_weight_list(load_pileup_weights())
    with pytest.raises(_lib.NanoSNPError, match="indel"):
        evaluate.evaluate_train_bins(bare, [sets["g1"][0]])
    assert evaluate.evaluate_train_bins(model, [])["sites"] == 0


def test_model_forward_is_the_references(model, gold, sets):
    """LSTMNetwork.forward argument for argument: the first batch of four variants of train_g1"""
    import torch
    _, x, label = sets["g1"]
    k = gold["variants_g1"][:4]
    cls = er.decode_labels(label)[0][k]
    t = [torch.from_numpy(cls[:, h].astype(np.int64)).cuda() for h in range(4)]
    loss, gt, zy, id1, id2 = model.forward(_dev(x[k]).to(torch.float32), *t)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and abs(float(loss) - float(gold["batch_loss_g1"][0])) <= ATOL
    z = torch.cat([gt, zy, id1, id2], dim=1).cpu().numpy()
    assert z.shape == (4, 90) and np.abs(z - gold["logits_g1"][k]).max() <= ATOL


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(indel, synth):
    import torch
    x, cls = _dev(synth[0][:16]), _dev(synth[1][:16])
    z = torch.empty((16, 90), dtype=torch.float32, device="cuda")
    loss = torch.empty((16, 4), dtype=torch.float32, device="cuda"); pred = torch.empty((16, 4), dtype=torch.uint8, device="cuda")
    counters = torch.zeros(2628, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    c = _context(indel, heads=False)
    try:
        logits = lambda n=16: c.lib.nsnp_pileup_forward_logits(c.handle, p(x), None, n, p(z), None)
        windows = lambda n=16: c.lib.nsnp_pileup_eval_windows(c.handle, p(x), None, p(cls), n, p(loss), p(pred), p(counters), None, None)
        assert logits() == -4 and windows() == -4                      # NSNP_ENOWEIGHTS: no indel heads yet
        c.pileup_load_indel_heads(indel)
        assert logits() == 0 and windows() == 0
        c.pileup_load_weights(load_pileup_weights())                   # a later load invalidates them
        assert logits() == -4
        c.pileup_load_indel_heads(indel)
        for mode in (1, 2):
            c.set_option("pileup_precision", mode)
            assert logits() == -1 and windows() == -1                  # NSNP_EINVAL: fp32 only
        c.set_option("pileup_precision", 0)
        torch.cuda.synchronize()
        before = counters.clone()
        assert logits(0) == 0 and windows(0) == 0                      # N = 0: a no-op
        assert c.lib.nsnp_pileup_batch_loss(c.handle, None, 0, 4, None, None) == 0
        meta = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        assert c.lib.nsnp_pileup_label_classes(c.handle, None, 0, 1, None, None, p(meta), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(counters, before) and meta.tolist() == [0, 0, 0, 0]
    finally:
        c.close()
    bare = _context(indel, heads=False)
    try:
        from nanosnp_amd import _lib
        with pytest.raises(_lib.NanoSNPError, match="weights not loaded"):
            bare.pileup_forward_logits(x)
    finally:
        bare.close()
