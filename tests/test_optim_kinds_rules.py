"""The float64 restatement tests/optim_kinds_rules.py against what the reference's own Novograd / LookaheadNovograd and torch's SGD /
Adadelta computed in fp32 (tests/golden/pileup_optim_kinds.npz), and the argument rules of DeviceOptimizer's new kinds that need no device.

The bound is the fixture's own: optim_rules.FACTOR x max(the reference's recorded distance from float64, one fp32 rounding of the largest
stored magnitude); per-tensor v and the norms relative, FACTOR x max(the recorded relative distance, 2^-23)."""
import numpy as np
import pytest

from tests import optim_kinds_rules as okr
from tests import optim_rules as orl


@pytest.fixture(scope="module")
def fx():
    return okr.load_fixture()


@pytest.fixture(scope="module")
def f64(fx):
    """the float64 trajectories, computed once and shared"""
    return {name: okr.run(name, fx["p0"], c["grads"]) for name, c in fx["cases"].items()}


def test_the_cases_are_the_issue_s():
    c = okr.CASES
    assert list(c) == ["novograd_plain", "la_novograd_wd", "sgd_nesterov", "sgd_plain", "adadelta_wd"]
    assert (c["novograd_plain"]["lr"], c["novograd_plain"]["weight_decay"], c["novograd_plain"]["max_norm"]) == (1e-3, 0.0, 20.0)
    la = c["la_novograd_wd"]
    assert (la["lr"], la["weight_decay"], la["alpha"], la["k"], la["max_norm"]) == (1e-2, 1e-4, 0.5, 6, 2.0)
    sn = c["sgd_nesterov"]
    assert (sn["momentum"], sn["nesterov"], sn["weight_decay"], sn["max_norm"]) == (0.9, True, 1e-4, 20.0)
    assert c["sgd_plain"]["momentum"] == 0.0 and c["sgd_plain"]["max_norm"] is None
    assert (c["adadelta_wd"]["lr"], c["adadelta_wd"]["weight_decay"], c["adadelta_wd"]["max_norm"]) == (1.0, 1e-4, 2.0)
    assert orl.SIZES[okr.ZERO_TENSOR] == 21 and okr.ZERO_STEPS == (1, 2)


@pytest.mark.parametrize("name", list(okr.CASES))
def test_restatement_against_the_fixture(fx, f64, name):
    c, got = fx["cases"][name], f64[name]
    for s in orl.RECORD:
        assert np.abs(c["p"][s] - got["p"][s]).max() <= orl.bound(c["ref_abs_max"]["p"], c["p"][s]), (name, s)
    for q in ("a", "b", "slow"):
        if c[q] is not None:
            assert np.abs(c[q] - got[q]).max() <= orl.bound(c["ref_abs_max"][q], c[q]), (name, q)
        elif q != "slow":
            assert not got[q].any(), (name, q)                       # a state the kind does not have stays untouched
    assert (c["slow"] is None) == (got["slow"] is None)
    if c["v"] is not None:
        vb = orl.FACTOR * max(c["ref_v_rel"], orl.ULP)
        for want, mine in ((c["v"], got["v"]), (c["v_at"][2], got["v_at"][2]), (c["v_at"][3], got["v_at"][3])):
            assert np.array_equal(want != 0, mine != 0)
            nz = want != 0
            assert np.abs(mine[nz] / want[nz].astype(np.float64) - 1.0).max() <= vb, name
    assert np.abs(got["norm"] / c["norm"].astype(np.float64) - 1.0).max() <= orl.FACTOR * max(c["ref_norm_rel"], orl.ULP)
    if okr.CASES[name]["max_norm"]:
        m = okr.CASES[name]["max_norm"]
        assert (c["norm"] > m).sum() >= 3 and (c["norm"] < m).sum() >= 3


def test_first_lookahead_sync_is_a_no_op(fx, f64):
    name = "la_novograd_wd"
    c, k = fx["cases"][name], okr.CASES[name]["k"]
    free = okr.run(name, fx["p0"], c["grads"], lookahead=False)
    assert k in orl.RECORD and 2 * k in orl.RECORD
    for s in orl.RECORD:
        if s < 2 * k:
            assert np.array_equal(free["p"][s], f64[name]["p"][s]), s            # the float64 rules: not a bit moves
            assert np.abs(c["p"][s] - free["p"][s]).max() <= orl.bound(c["ref_abs_max"]["p"], c["p"][s]), s
    assert np.abs(c["p"][2 * k] - free["p"][2 * k]).max() > 100 * orl.bound(c["ref_abs_max"]["p"], c["p"][2 * k])


@pytest.mark.parametrize("name", ["novograd_plain", "la_novograd_wd"])
def test_zero_gradient_tensor_copies_at_step_3(fx, f64, name):
    c, z = fx["cases"][name], okr.ZERO_TENSOR
    o = sum(orl.SIZES[:z])
    assert not c["grads"][0, o:o + 21].any() and not c["grads"][1, o:o + 21].any() and c["grads"][2, o:o + 21].all()
    assert c["v_at"][2][z] == 0.0 and f64[name]["v_at"][2][z] == 0.0
    assert (np.delete(c["v_at"][2], z) > 0).all()                              # its neighbours left 0 at step 1
    g3 = c["grads"][2].astype(np.float64)
    coef = min(1.0, okr.CASES[name]["max_norm"] / (np.sqrt((g3 * g3).sum()) + 1e-6))
    n3 = float((g3[o:o + 21] ** 2).sum()) * coef * coef
    vb = orl.FACTOR * max(c["ref_v_rel"], orl.ULP)
    assert abs(c["v_at"][3][z] / n3 - 1.0) <= vb and abs(f64[name]["v_at"][3][z] / n3 - 1.0) <= 1e-12
    for i in (z - 1, z + 1):                                                  # and they average at step 3
        lo, n = sum(orl.SIZES[:i]), orl.SIZES[i]
        ni = float((g3[lo:lo + n] ** 2).sum()) * coef * coef
        mix = okr.BETAS[1] * f64[name]["v_at"][2][i] + (1 - okr.BETAS[1]) * ni
        assert abs(c["v_at"][3][i] / mix - 1.0) <= vb, i
    # the parameters of the zeroed tensor do not move while its gradients are zero and there is no weight decay
    if okr.CASES[name]["weight_decay"] == 0:
        assert np.array_equal(c["p"][1][o:o + 21], fx["p0"][o:o + 21])


def test_device_optimizer_refusals_without_a_device():
    import torch
    from nanosnp_amd import train
    params = [torch.zeros(3)]
    for bad in (dict(kind="novograd"), dict(kind="Ranger"), dict(kind="SGD"), dict(kind="sgd", momentum=1.0), dict(kind="sgd", momentum=-0.1),
                dict(kind="sgd", nesterov=True), dict(kind="sgd", momentum=0.0, nesterov=True), dict(kind="adadelta", rho=1.0),
                dict(kind="adadelta", rho=-0.5)):
        with pytest.raises(ValueError):
            train.DeviceOptimizer(params, **bad)
    assert set(train.RULE_KINDS) == {"Novograd", "LookaheadNovograd", "sgd", "adadelta"}
    assert {k: v[0] for k, v in train.RULE_KINDS.items()} == {"Novograd": False, "LookaheadNovograd": True, "sgd": False, "adadelta": False}
    assert set(train.OPTIMIZER_KINDS) == {"Adam", "LookaheadAdam", "Radam", "LookaheadRadam"}


def test_args_struct_matches_the_header():
    """nsnp_optim_kind_args: the fields of the binding in the order of include/nanosnp.h, and the kind numbers"""
    import os
    import re
    from nanosnp_amd import _lib
    from tests.helpers import ROOT
    src = open(os.path.join(ROOT, "include", "nanosnp.h")).read()
    body = re.search(r"typedef struct nsnp_optim_kind_args \{(.*?)\}", src, re.S).group(1)
    doubles = re.search(r"double ([^;]*);", body).group(1).replace(" ", "").split(",")
    ints = re.search(r"int ([^;]*);", body).group(1).replace(" ", "").split(",")
    assert [f[0] for f in _lib.OptimKindArgs._fields_] == doubles + ints
    for name, value in (("NOVOGRAD", _lib.OPTIM_NOVOGRAD), ("SGD", _lib.OPTIM_SGD), ("ADADELTA", _lib.OPTIM_ADADELTA)):
        assert int(re.search(rf"#define NSNP_OPTIM_{name} (\d+)", src).group(1)) == value
    assert hasattr(_lib.load(), "nsnp_optim_step_kind")
