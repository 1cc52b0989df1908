"""Scoring a PileupModel checkpoint in a chosen arithmetic (nsnp_pileup_forward_logits2 / nsnp_pileup_eval_windows2 and the `precision`
keyword above them): fp32 (0), f16x3 (1) and bf16x3 (2) against the reference's own numbers (tests/golden/pileup_eval.npz), the float64
restatement tests/eval_rules.py and the probabilities nsnp_pileup_forward gives in the same arithmetic.

Bounds.  Floats: 1e-4 absolute, the project's contract (ATOL of tests/test_gpu_eval.py).  Predictions: equal to the reference on the 18
variant sites (their top-two margins are at least 6.4e-3) and equal to float64 on every synthetic row whose float64 margins all exceed
2e-4; tests/test_eval_precision_inputs.py pins both facts and that the rows left out are at most 1 %.  Probabilities: 1e-6 from the
softmax of the scoring logits, the bound of the fp32 test.

Measured on an MI355X (docs/rounds/r36.md has the table): see the docstrings of the tests."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import eval_rules as er
from tests.helpers import ROOT, load_pileup_weights, golden
from tests.test_eval_precision_inputs import LEFT_OUT_CAP, MARGIN_SYNTH, margins

pytestmark = pytest.mark.gpu
ATOL = 1e-4
PRECISIONS = (0, 1, 2)
SETS = (("g1", "train_g1"), ("cut", "train_cut"))
DATA_NPZ = os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz")
N_SYNTH = 4097


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
    d = str(tmp_path_factory.mktemp("gpu_eval_precisions"))
    return {tag: er.fixture_rows(case, d) for tag, case in SETS}              # tag -> (path of the .td.bin, windows, labels)


@pytest.fixture(scope="module")
def synth(sets, indel):
    """the seeded synthetic windows with random classes, their float64 logits / losses / predictions and the rows whose float64 margins
    are all clear, once for every test"""
    x, cls = er.synthetic_windows(sets["cut"][1], N_SYNTH)
    z = er.forward_logits_f64(load_pileup_weights(), indel, x)
    return x, cls, z, er.smoothed_loss(z, cls), er.predictions(z), margins(z).min(1) > MARGIN_SYNTH


def _eval(ctx, x, cls, p, logits=True, counters=None, stream=None):
    import torch
    counters = counters if counters is not None else torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
    xd, cd = _dev(x), _dev(cls)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())      # (the inputs and the zeroed counters were made on the current stream)
    loss, pred, z = ctx.pileup_eval_windows(xd, None, cd, counters, want_logits=logits, precision=p, stream=stream)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), pred.cpu().numpy(), None if z is None else z.cpu().numpy(), counters.cpu().numpy()


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["g1", "cut"])
@pytest.mark.parametrize("p", PRECISIONS)
def test_logits_against_the_reference(ctx, gold, sets, p, tag):
    """measured max |logit - reference|, g1 / cut: fp32 2.4e-6 / 2.9e-6, f16x3 4.8e-6 / 4.8e-6, bf16x3 4.3e-6 / 5.2e-6"""
    import torch
    z = ctx.pileup_forward_logits(_dev(sets[tag][1]), precision=p)
    torch.cuda.synchronize()
    d = np.abs(z.cpu().numpy() - gold[f"logits_{tag}"]).max()
    print(f"precision {p}, {tag}: max |logit - reference| = {d:.3e}")
    assert d <= ATOL


@pytest.mark.parametrize("p", PRECISIONS)
def test_loss_and_counts_against_the_reference(ctx, gold, sets, p):
    """measured max |site loss - reference|, g1 / cut: fp32 1.9e-6 / 4.3e-6, f16x3 9.5e-7 / 2.4e-6, bf16x3 2.4e-6 / 1.9e-6;
    max |batch mean - reference|: fp32 1.4e-6 / 8.9e-7, f16x3 7.2e-7 / 1.4e-6, bf16x3 1.1e-6 / 7.2e-7"""
    import torch
    B = int(gold["batch_size"])
    counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
    total, sites = 0.0, 0
    for tag in ("g1", "cut"):
        _, x, label = sets[tag]
        cls, centers, meta = ctx.pileup_label_classes(_dev(label), True)
        torch.cuda.synchronize()
        k = int(meta[0])
        assert k == len(gold[f"variants_{tag}"])
        loss, pred, _ = ctx.pileup_eval_windows(_dev(x).view(-1, 18), centers[:k].contiguous(), cls, counters, n=k, precision=p)
        sums = ctx.pileup_batch_loss(loss, B).cpu().numpy()
        loss = loss.cpu().numpy()
        print(f"precision {p}, {tag}: max |site loss - reference| = {np.abs(loss - gold[f'site_loss_{tag}']).max():.3e}")
        assert np.abs(loss - gold[f"site_loss_{tag}"]).max() <= ATOL
        means = (sums[:, 0] + sums[:, 1]) / np.minimum(B, k - B * np.arange(sums.shape[0]))
        print(f"precision {p}, {tag}: max |batch mean - reference| = {np.abs(means - gold[f'batch_loss_{tag}']).max():.3e}")
        assert means.shape == gold[f"batch_loss_{tag}"].shape and np.abs(means - gold[f"batch_loss_{tag}"]).max() <= ATOL
        assert np.array_equal(pred.cpu().numpy(), gold[f"pred_{tag}"])            # (margins of at least 6.4e-3: no room)
        total += float(means.sum()); sites += k
    assert sites == int(gold["sites"]) and abs(total / sites - float(gold["avg_loss"])) <= ATOL
    conf = counters.cpu().numpy()
    assert np.array_equal(conf[:450], gold["confusion"][:450])
    assert np.trace(conf[:441].reshape(21, 21)) / sites == float(gold["gt_accuracy"])
    assert np.trace(conf[441:450].reshape(3, 3)) / sites == float(gold["zy_accuracy"])


# ---- 2. against float64, at the row counts where the heads kernels can go wrong ------------------------------------------------------------
def _check_shape(ctx, synth, n, p):
    import torch
    x, cls, z64, loss64, pred64, clear = (a[:n] for a in synth)
    loss, pred, z, conf = _eval(ctx, x, cls, p)
    print(f"precision {p}, N = {n}: max |logit - f64| = {np.abs(z - z64).max():.3e}, max |loss - f64| = {np.abs(loss - loss64).max():.3e}, "
          f"rows left out of the prediction comparison: {int((~clear).sum())}")
    assert np.abs(z - z64).max() <= ATOL and np.abs(loss - loss64).max() <= ATOL
    assert np.array_equal(pred, er.predictions(z)) and np.array_equal(conf, er.confusion(cls, pred))
    assert (~clear).sum() <= LEFT_OUT_CAP * n and np.array_equal(pred[clear], pred64[clear])
    # a second run: the same bits
    loss2, pred2, z2, conf2 = _eval(ctx, x, cls, p)
    assert loss2.tobytes() == loss.tobytes() and z2.tobytes() == z.tobytes() and np.array_equal(pred2, pred) and np.array_equal(conf2, conf)
    # without logits: the same losses and counts
    loss3, pred3, z3, conf3 = _eval(ctx, x, cls, p, logits=False)
    assert z3 is None and loss3.tobytes() == loss.tobytes() and np.array_equal(pred3, pred) and np.array_equal(conf3, conf)
    # two calls over the halves, into the same counters: bit for bit the one call
    if n > 1:
        counters = torch.zeros(ctx.EVAL_COUNTERS, dtype=torch.int64, device="cuda")
        h = n // 2
        a = _eval(ctx, x[:h], cls[:h], p, counters=counters)
        b = _eval(ctx, x[h:], cls[h:], p, counters=counters)
        assert np.concatenate([a[0], b[0]]).tobytes() == loss.tobytes() and np.concatenate([a[2], b[2]]).tobytes() == z.tobytes()
        assert np.array_equal(np.concatenate([a[1], b[1]]), pred) and np.array_equal(b[3], conf)
    # forward_logits2 is the same forward
    assert ctx.pileup_forward_logits(_dev(x), precision=p).cpu().numpy().tobytes() == z.tobytes()
    # a side stream
    side = torch.cuda.Stream()
    loss4, pred4, z4, conf4 = _eval(ctx, x, cls, p, stream=side)
    assert loss4.tobytes() == loss.tobytes() and z4.tobytes() == z.tobytes() and np.array_equal(pred4, pred) and np.array_equal(conf4, conf)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 128, 129])
@pytest.mark.parametrize("p", PRECISIONS)
def test_heads_kernel_shapes(ctx, synth, p, n):
    """a workgroup of the split heads kernels holds 8 waves x 16 sites and does not loop: one site, a wave short of / at / past 16, a
    workgroup short of / at / past 128.  Measured at N = 129, max |logit - f64| / max |loss - f64|: fp32 2.4e-6 / 2.3e-6, f16x3
    2.2e-6 / 2.1e-6, bf16x3 2.3e-6 / 2.1e-6; no row is left out of the prediction comparison at these counts"""
    _check_shape(ctx, synth, n, p)


@pytest.mark.parametrize("p", PRECISIONS)
def test_heads_kernel_across_a_chunk_boundary(indel, synth, p):
    """4097 sites at chunk_sites 4096: a second chunk of one site, counters added to across chunks.  Measured max |logit - f64| /
    max |loss - f64|: fp32 4.4e-6 / 4.3e-6, f16x3 3.0e-6 / 3.4e-6, bf16x3 3.3e-6 / 2.9e-6; 7 rows left out of the prediction comparison"""
    c = _context(indel, chunk_sites=4096)
    try:
        _check_shape(c, synth, N_SYNTH, p)
    finally:
        c.close()


# ---- 3. the logits predict sees -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRECISIONS)
def test_same_logits_as_predict(indel, sets, p):
    """with the context option at p: the float64 softmax of the scoring logits against nsnp_pileup_forward's probabilities.
    Measured, the larger of genotype and zygosity over g1 and cut: fp32 2.0e-7, f16x3 2.4e-7, bf16x3 2.1e-7 (bound 1e-6)"""
    import torch
    c = _context(indel)
    try:
        c.set_option("pileup_precision", p)
        for tag in ("g1", "cut"):
            x = _dev(sets[tag][1])
            z = c.pileup_forward_logits(x, precision=p)
            gt, zy = c.pileup_forward(x)
            torch.cuda.synchronize()
            z, gt, zy = z.cpu().numpy(), gt.cpu().numpy(), zy.cpu().numpy()
            for a, b, prob in ((0, 21, gt), (21, 24, zy)):
                s = z[:, a:b].astype(np.float64)
                e = np.exp(s - s.max(1, keepdims=True))
                sm = e / e.sum(1, keepdims=True)
                print(f"precision {p}, {tag}: max |softmax(logits[{a}:{b}]) - forward| = {np.abs(sm - prob).max():.3e}")
                assert np.abs(sm - prob).max() <= 1e-6
                top = np.sort(prob, axis=1)
                clear = top[:, -1] != top[:, -2]
                assert np.array_equal(z[clear, a:b].argmax(1), prob[clear].argmax(1))
    finally:
        c.close()


# ---- 4. invariants ------------------------------------------------------------------------------------------------------------------------
def test_precision_0_is_the_old_entries(ctx, synth):
    import torch
    x, cls = synth[0][:129], synth[1][:129]
    new = _eval(ctx, x, cls, 0)
    old = _eval(ctx, x, cls, None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(new, old))
    assert ctx.pileup_forward_logits(_dev(x), precision=0).cpu().numpy().tobytes() == ctx.pileup_forward_logits(_dev(x)).cpu().numpy().tobytes()


def test_the_context_option_matters_only_when_asked(indel, synth):
    """an explicit precision gives the same bytes whatever pileup_precision is (on a context that starts in fp32, so that the bf16x3 pass
    has to widen the workspace itself); "context" (-1) is the explicit value of the option"""
    x, cls = synth[0][:129], synth[1][:129]
    c = _context(indel, chunk_sites=4096)
    try:
        want = {}
        for option in (0, 2, 1):
            c.set_option("pileup_precision", option)
            for p in (2, 1, 0):
                got = _eval(c, x, cls, p)
                want.setdefault(p, got)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want[p])), (option, p)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(_eval(c, x, cls, "context"), want[option])), option
        assert want[0][2].tobytes() != want[1][2].tobytes() and want[1][2].tobytes() != want[2][2].tobytes()        # (three arithmetics,
        assert want[0][2].tobytes() != want[2][2].tobytes()                                                         # not one)
    finally:
        c.close()


# ---- 5. refusals, on poisoned buffers ---------------------------------------------------------------------------------------------------------
def test_refusals(indel, synth):
    import torch
    x, cls = _dev(synth[0][:16]), _dev(synth[1][:16])
    z = torch.full((16, 90), -7.0, dtype=torch.float32, device="cuda")
    loss = torch.full((16, 4), -7.0, dtype=torch.float32, device="cuda"); pred = torch.full((16, 4), 0xEE, dtype=torch.uint8, device="cuda")
    counters = torch.full((2628,), 5, dtype=torch.int64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def untouched():
        torch.cuda.synchronize()
        return bool((z == -7.0).all() and (loss == -7.0).all() and (pred == 0xEE).all() and (counters == 5).all())
    c = _context(indel, heads=False)
    try:
        logits = lambda p, n=16: c.lib.nsnp_pileup_forward_logits2(c.handle, ptr(x), None, n, p, ptr(z), None)
        windows = lambda p, n=16: c.lib.nsnp_pileup_eval_windows2(c.handle, ptr(x), None, ptr(cls), n, p, ptr(loss), ptr(pred), ptr(counters),
                                                                  ptr(z), None)
        for p in (-1, 0, 1, 2):
            assert logits(p) == -4 and windows(p) == -4                  # NSNP_ENOWEIGHTS: no indel heads yet
        assert untouched()
        c.pileup_load_indel_heads(indel)
        for p in (3, -2, 100):
            assert logits(p) == -1 and windows(p) == -1                  # NSNP_EINVAL: no such arithmetic
        assert c.lib.nsnp_pileup_forward_logits2(c.handle, ptr(x), None, 16, 2, None, None) == -1
        assert c.lib.nsnp_pileup_eval_windows2(c.handle, ptr(x), None, None, 16, 2, ptr(loss), ptr(pred), ptr(counters), None, None) == -1
        assert c.lib.nsnp_pileup_eval_windows2(c.handle, None, None, ptr(cls), 16, 1, ptr(loss), ptr(pred), ptr(counters), None, None) == -1
        for p in (-1, 0, 1, 2):
            assert logits(p, 0) == 0 and windows(p, 0) == 0              # N = 0: a no-op
        assert untouched()
        c.pileup_load_weights(load_pileup_weights())                     # a later load invalidates all three images
        for p in (0, 1, 2):
            assert logits(p) == -4 and windows(p) == -4
        assert untouched()
        c.pileup_load_indel_heads(indel)
        for p in (0, 1, 2):
            assert logits(p) == 0
        old_logits = lambda: c.lib.nsnp_pileup_forward_logits(c.handle, ptr(x), None, 16, ptr(z), None)
        old_windows = lambda: c.lib.nsnp_pileup_eval_windows(c.handle, ptr(x), None, ptr(cls), 16, ptr(loss), ptr(pred), ptr(counters), None, None)
        z.fill_(-7.0)
        for mode in (1, 2):
            c.set_option("pileup_precision", mode)
            assert old_logits() == -1 and old_windows() == -1            # the old entries stay fp32 only
        assert untouched()
    finally:
        c.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from nanosnp_amd import pileup_model
    return pileup_model.LSTMNetwork.from_npz(DATA_NPZ)


def _same(a, b, atol, skip=("files", "batch_means", "precision")):
    assert set(a) - set(skip) == set(b) - set(skip)
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        elif isinstance(a[k], float) and "accuracy" not in k:
            assert abs(a[k] - b[k]) <= atol, (k, a[k], b[k])
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("p", PRECISIONS)
def test_evaluate_train_bins(model, gold, sets, p):
    from nanosnp_amd import evaluate
    B = int(gold["batch_size"])
    paths = [sets["g1"][0], sets["cut"][0]]
    parts = []
    for tag in ("g1", "cut"):
        cls = er.decode_labels(sets[tag][2])[0][gold[f"variants_{tag}"]]
        parts.append((gold[f"site_loss_{tag}"], cls, gold[f"pred_{tag}"]))
    want = er.result_from(parts, B)                          # the dict built from the reference's numbers
    runs = {ps: evaluate.evaluate_train_bins(model, paths, batch_size=B, pass_sites=ps, keep_sites=True, precision=p) for ps in (4, 65536)}
    for got in runs.values():
        assert got["precision"] == p
        _same(got, want, ATOL)
        assert got["sites"] == 18 and abs(got["avg_loss"] - float(gold["avg_loss"])) <= ATOL
        for f, tag in zip(got["files"], ("g1", "cut")):
            assert np.array_equal(f["rows"], gold[f"variants_{tag}"]) and np.array_equal(f["pred"], gold[f"pred_{tag}"])
            assert np.abs(f["site_loss"] - gold[f"site_loss_{tag}"]).max() <= ATOL
    _same(runs[4], runs[65536], 0.0, skip=("files",))        # the pass size changes nothing, to the bit
    for fa, fb in zip(runs[4]["files"], runs[65536]["files"]):
        assert all(fa[k].tobytes() == fb[k].tobytes() for k in ("rows", "cls", "pred", "site_loss"))
    assert "precision" not in evaluate.evaluate_train_bins(model, paths, batch_size=B)


def test_evaluate_train_bins_in_the_contexts_arithmetic(model, gold, sets):
    """precision="context" with the option at 2: byte for byte precision=2, and reported as "context"; the same through compare_precisions"""
    from nanosnp_amd import evaluate
    paths, kw = [sets["g1"][0], sets["cut"][0]], dict(batch_size=int(gold["batch_size"]), keep_sites=True)
    want = evaluate.evaluate_train_bins(model, paths, precision=2, **kw)
    base = evaluate.evaluate_train_bins(model, paths, precision=0, **kw)
    model.ctx.set_option("pileup_precision", 2)
    try:
        got = evaluate.evaluate_train_bins(model, paths, precision="context", **kw)
        cmp = evaluate.compare_precisions(model, paths, precisions=(0, "context"), batch_size=kw["batch_size"])
    finally:
        model.ctx.set_option("pileup_precision", 0)
    assert got["precision"] == "context" and want["precision"] == 2 and got["sites"] == 18
    _same(got, want, 0.0, skip=("files", "precision"))
    for fa, fb in zip(got["files"], want["files"]):
        assert all(fa[k].tobytes() == fb[k].tobytes() for k in ("rows", "cls", "pred", "site_loss"))
    assert any(fa["site_loss"].tobytes() != fb["site_loss"].tobytes() for fa, fb in zip(got["files"], base["files"]))     # (not fp32's)
    assert list(cmp) == [0, "context"] and cmp["context"]["result"]["precision"] == "context"
    assert cmp["context"] == dict(result=cmp["context"]["result"], **evaluate.precision_differences(base, want))


@pytest.mark.parametrize("p", PRECISIONS)
def test_model_forward(model, gold, sets, p):
    """LSTMNetwork.forward(..., precision=p): the first batch of four variants of train_g1"""
    import torch
    _, x, label = sets["g1"]
    k = gold["variants_g1"][:4]
    cls = er.decode_labels(label)[0][k]
    t = [torch.from_numpy(cls[:, h].astype(np.int64)).cuda() for h in range(4)]
    loss, gt, zy, id1, id2 = model.forward(_dev(x[k]).to(torch.float32), *t, precision=p)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and abs(float(loss) - float(gold["batch_loss_g1"][0])) <= ATOL
    z = torch.cat([gt, zy, id1, id2], dim=1).cpu().numpy()
    assert z.shape == (4, 90) and np.abs(z - gold["logits_g1"][k]).max() <= ATOL


def test_compare_precisions(model, gold, sets):
    """measured against fp32: bf16x3 largest site-loss difference 3.8e-6, avg_loss difference 1.9e-7; f16x3 2.4e-6, 1.5e-7; 0 differing sites"""
    from nanosnp_amd import evaluate
    got = evaluate.compare_precisions(model, [sets["g1"][0], sets["cut"][0]], batch_size=int(gold["batch_size"]))
    assert list(got) == [0, 2, 1]
    for p, r in got.items():
        print(f"precision {p} against fp32: {r['differing_sites']} differing sites, max |site loss| difference {r['max_site_loss_diff']:.3e}, "
              f"avg_loss difference {r['avg_loss_diff']:.3e}")
        assert r["result"]["sites"] == 18 and r["result"]["precision"] == p
        assert r["differing_sites"] == 0                     # (margins of at least 6.4e-3)
        assert r["max_site_loss_diff"] < 2e-4 and abs(r["avg_loss_diff"]) < 2e-4        # each within 1e-4 of the reference
    assert got[0]["max_site_loss_diff"] == 0.0 and got[0]["avg_loss_diff"] == 0.0


def test_fit_validates_in_bf16x3_and_trains_the_same_bits(sets):
    import torch
    from nanosnp_amd import train
    path = sets["g1"][0]
    outs, params = {}, {}
    for vp in (None, 2, "context"):
        tr = train.PileupTrainer.from_npz(DATA_NPZ, chunk_sites=64)
        outs[vp] = train.fit(tr, path, validating_paths=path, epochs=1, batch_size=10, dropout=0.0, validate_precision=vp)
        torch.cuda.synchronize()
        params[vp] = [q.detach().cpu().numpy().copy() for q in tr.parameters()]
    assert outs[2][0]["eval"]["precision"] == 2 and "precision" not in outs[None][0]["eval"]
    assert outs[2][0]["eval"]["sites"] == outs[None][0]["eval"]["sites"] > 0
    print(f"avg_loss of the trained epoch: fp32 {outs[None][0]['eval']['avg_loss']:.7f}, bf16x3 {outs[2][0]['eval']['avg_loss']:.7f}")
    assert len(params[2]) == len(params[None]) > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(params[2], params[None]))
    # "context" on a trainer's fp32 context: reported as such, the numbers of the fp32 entry to the bit
    assert outs["context"][0]["eval"]["precision"] == "context"
    assert all(outs["context"][0]["eval"][k] == outs[None][0]["eval"][k] for k in ("sites", "avg_loss", "mean_loss", "gt_loss", "zy_loss"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(params["context"], params[None]))
