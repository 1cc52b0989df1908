"""The facts the bounds of tests/test_gpu_eval_precisions.py rest on, and the host side of scoring in a chosen arithmetic (no GPU).

1. Margins.  A prediction can only be compared across arithmetics where the two largest logits of a head are further apart than the
   arithmetics may be: the 18 variant sites of pileup_eval.npz have top-two margins of at least 6.4e-3 in every head (64 times the 1e-4
   contract), so their predictions must be equal in every arithmetic; of the 4097 synthetic windows a handful of rows have a margin below
   2e-4 (two logits 1e-4 off each), and those are the only rows the float64 comparison of predictions may leave out - at most 1 %.
2. evaluate.precision_differences / compare_precisions assemble their differences from results, and the `precision` keyword reaches the
   right C entry with the right argument (a stub context records the calls)."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_rules as er
from tests.helpers import golden, load_pileup_weights

MARGIN_GOLD = 6.4e-3            # smallest top-two margin of a head on the 18 variant sites (measured: 6.48e-3, indel2 of g1)
MARGIN_SYNTH = 2e-4             # twice the 1e-4 contract: below it two arithmetics within the contract may order two logits differently
LEFT_OUT_CAP = 0.01


def margins(z):
    """float [N,4]: per head the distance between its two largest logits"""
    out = np.zeros((z.shape[0], 4))
    for h, (r0, c, _) in enumerate(er.HEADS):
        s = np.sort(np.asarray(z[:, r0:r0 + c], np.float64), axis=1)
        out[:, h] = s[:, -1] - s[:, -2]
    return out


def test_margins_of_the_variant_sites():
    gold = np.load(golden("pileup_eval.npz"))
    smallest = {}
    for tag in ("g1", "cut"):
        m = margins(gold[f"logits_{tag}"][gold[f"variants_{tag}"]])
        assert m.shape == (9, 4)
        smallest[tag] = (float(m.min()), int(m.min(0).argmin()))
    print("smallest top-two margins (value, head):", smallest)
    assert min(v for v, _ in smallest.values()) >= MARGIN_GOLD
    assert smallest["g1"][1] == 3 and abs(smallest["g1"][0] - 6.48e-3) < 1e-5          # indel2 of g1


def test_margins_of_the_synthetic_windows(tmp_path):
    gold = np.load(golden("pileup_eval.npz"))
    indel = [gold["indel1_weight"], gold["indel1_bias"], gold["indel2_weight"], gold["indel2_bias"]]
    x, _ = er.synthetic_windows(er.fixture_rows("train_cut", str(tmp_path))[1], 4097)
    m = margins(er.forward_logits_f64(load_pileup_weights(), indel, x))
    close = int((m.min(1) < MARGIN_SYNTH).sum())
    print(f"rows with a head margin below {MARGIN_SYNTH}: {close} of {m.shape[0]}")
    assert close == 7                                        # 0.17 %
    assert close <= LEFT_OUT_CAP * m.shape[0]


def _result(path, rows, pred, loss, avg):
    return {"avg_loss": avg, "files": [dict(path=path, rows=np.asarray(rows, np.int64), cls=np.zeros((len(rows), 4), np.uint8),
                                            pred=np.asarray(pred, np.uint8), site_loss=np.asarray(loss, np.float32))]}


def test_differences_between_results(monkeypatch):
    from nanosnp_amd import evaluate
    rows = [3, 5, 9]
    base = _result("a", rows, [[1, 2, 3, 4], [0, 1, 0, 0], [7, 2, 1, 1]], np.zeros((3, 4)), 1.0)
    same = _result("a", rows, base["files"][0]["pred"], np.zeros((3, 4)), 1.0)
    loss = np.zeros((3, 4)); loss[1, 2] = -0.25; loss[2, 0] = 0.125
    # site 0 differs in an indel head only, site 2 in two heads: two sites
    other = _result("a", rows, [[1, 2, 3, 5], [0, 1, 0, 0], [6, 1, 1, 1]], loss, 1.5)
    assert evaluate.precision_differences(base, same) == {"differing_sites": 0, "max_site_loss_diff": 0.0, "avg_loss_diff": 0.0}
    assert evaluate.precision_differences(base, other) == {"differing_sites": 2, "max_site_loss_diff": 0.25, "avg_loss_diff": 0.5}
    with pytest.raises(ValueError):
        evaluate.precision_differences(base, _result("a", [3, 5, 10], base["files"][0]["pred"], np.zeros((3, 4)), 1.0))
    with pytest.raises(ValueError):
        evaluate.precision_differences(base, dict(avg_loss=1.0, files=[]))

    calls = []

    def fake(model, paths, precision=None, **kw):
        calls.append((model, paths, precision, kw))
        return dict({0: base, 2: same, 1: other}[precision], precision=precision)
    monkeypatch.setattr(evaluate, "evaluate_train_bins", fake)
    got = evaluate.compare_precisions("m", ["p"], batch_size=4)
    assert list(got) == [0, 2, 1] and [c[2] for c in calls] == [0, 2, 1]
    assert all(c[0] == "m" and c[1] == ["p"] and c[3] == {"batch_size": 4, "keep_sites": True} for c in calls)
    assert got[0]["differing_sites"] == 0 and got[0]["result"]["precision"] == 0
    assert (got[2]["differing_sites"], got[2]["max_site_loss_diff"], got[2]["avg_loss_diff"]) == (0, 0.0, 0.0)
    assert (got[1]["differing_sites"], got[1]["max_site_loss_diff"], got[1]["avg_loss_diff"]) == (2, 0.25, 0.5)
    # the first entry is the base, whichever it is
    got = evaluate.compare_precisions("m", ["p"], precisions=(1, 0))
    assert list(got) == [1, 0] and got[0]["differing_sites"] == 2 and got[0]["avg_loss_diff"] == -0.5
    n_calls = len(calls)
    for bad in ((None, 1), (0, 2, 0), (1, np.int64(1))):     # None is not an arithmetic; a repeated one would overwrite its own entry
        with pytest.raises(ValueError):
            evaluate.compare_precisions("m", ["p"], precisions=bad)
    assert len(calls) == n_calls                             # refused before anything runs


class _Tensor:
    """what the argument checks of _lib.Context read of a device tensor"""
    is_cuda = True

    def __init__(self, dtype, shape, ptr):
        self.dtype, self.shape, self.ptr, self.device = dtype, tuple(shape), ptr, "stub"

    def is_contiguous(self): return True
    def dim(self): return len(self.shape)
    def numel(self): return int(np.prod(self.shape))
    def data_ptr(self): return self.ptr


class _Lib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [a.value if isinstance(a, C.c_void_p) else a for a in args]))
            return 0
        return entry


class _Stream:
    cuda_stream = 77


def test_the_precision_keyword_reaches_the_right_entry():
    import torch
    from nanosnp_amd import _lib
    arg = _lib.Context.eval_precision_arg
    assert [arg(p) for p in (None, 0, 1, 2, "context", np.int64(2))] == [None, 0, 1, 2, -1, 2]
    for bad in (3, -1, -2, 1.5, "fp32", True, [1], (None, 2), np.array([1, 2]), np.array([0.5]), object()):
        with pytest.raises(_lib.NanoSNPError):
            arg(bad)
    ctx = object.__new__(_lib.Context)
    ctx.lib, ctx.handle = _Lib(), 5
    x = _Tensor(torch.int32, (8, 33, 18), 100)
    z = _Tensor(torch.float32, (8, 90), 200)
    cls, loss, pred = _Tensor(torch.uint8, (8, 4), 300), _Tensor(torch.float32, (8, 4), 400), _Tensor(torch.uint8, (8, 4), 500)
    counters = _Tensor(torch.int64, (2628,), 600)
    for p, name, tail in ((None, "nsnp_pileup_forward_logits", [200, 77]), (0, "nsnp_pileup_forward_logits2", [0, 200, 77]),
                          (1, "nsnp_pileup_forward_logits2", [1, 200, 77]), (2, "nsnp_pileup_forward_logits2", [2, 200, 77]),
                          ("context", "nsnp_pileup_forward_logits2", [-1, 200, 77])):
        ctx.lib.calls.clear()
        assert ctx.pileup_forward_logits(x, logits=z, stream=_Stream(), precision=p) is z
        assert ctx.lib.calls == [(name, [5, 100, None, 8] + tail)]
    for p, name, mid in ((None, "nsnp_pileup_eval_windows", []), (0, "nsnp_pileup_eval_windows2", [0]), (1, "nsnp_pileup_eval_windows2", [1]),
                         (2, "nsnp_pileup_eval_windows2", [2]), ("context", "nsnp_pileup_eval_windows2", [-1])):
        ctx.lib.calls.clear()
        got = ctx.pileup_eval_windows(x, None, cls, counters, n=6, site_loss=loss, pred=pred, stream=_Stream(), precision=p)
        assert got == (loss, pred, None)
        assert ctx.lib.calls == [(name, [5, 100, None, 300, 6] + mid + [400, 500, 600, None, 77])]
    ctx.lib.calls.clear()
    with pytest.raises(_lib.NanoSNPError):
        ctx.pileup_eval_windows(x, None, cls, counters, site_loss=loss, pred=pred, stream=_Stream(), precision=3)
    assert ctx.lib.calls == []                               # refused before anything is called
