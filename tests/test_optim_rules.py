"""tests/optim_rules.py, the float64 restatement of clip_grad_norm_ + Adam / RAdam + Lookahead, against what the reference's own optimisers
computed in fp32 (tests/golden/pileup_optim.npz, written by tests/golden/make_golden_optim.py), and the host-side parts of the fused step
that need no device: the step scalars of nanosnp_amd.train, the scratch query and the symbols.

Bound: every recorded value within 4 x max(ref_abs_max, 2^-23 max |value|) of the restatement - ref_abs_max being the reference's own fp32
distance from float64 recorded per case and quantity, the floor one rounding of a stored fp32 value."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import optim_rules as orl
from tests.helpers import ROOT


@pytest.fixture(scope="module")
def fx():
    return orl.load_fixture()


@pytest.fixture(scope="module")
def f64(fx):
    return {name: orl.run(name, fx["p0"], c["grads"]) for name, c in fx["cases"].items()}


def test_fixture_is_what_the_issue_asks_for(fx):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pileup_optim.npz")) < 512 * 1024
    assert orl.SIZES == (1, 3, 7, 21, 1023, 1024, 1025, 165) and orl.STEPS == 14
    for name, cfg in orl.CASES.items():
        c = fx["cases"][name]
        assert c["grads"].shape == (orl.STEPS, orl.TOTAL) and c["grads"].dtype == np.float32 and sorted(c["p"]) == list(orl.RECORD)
        assert (c["slow"] is None) == (cfg["kind"] == "Adam")
        if cfg["max_norm"]:
            assert (c["norm"] > cfg["max_norm"]).sum() >= 3 and (c["norm"] < cfg["max_norm"]).sum() >= 3, name      # both kinds of step


@pytest.mark.parametrize("name", list(orl.CASES))
def test_restatement_reproduces_the_reference(fx, f64, name):
    c, r = fx["cases"][name], f64[name]
    for s in orl.RECORD:
        for i, (got, want) in enumerate(zip(orl.split(r["p"][s]), orl.split(c["p"][s]))):
            assert np.abs(got - want).max() <= orl.bound(c["ref_abs_max"]["p"], want), (name, s, i)
    for q in ("m", "v", "slow"):
        if c[q] is not None:
            for i, (got, want) in enumerate(zip(orl.split(r[q]), orl.split(c[q]))):
                assert np.abs(got - want).max() <= orl.bound(c["ref_abs_max"][q], want), (name, q, i)
    assert np.abs(r["norm"] / c["norm"].astype(np.float64) - 1.0).max() <= orl.FACTOR * max(c["ref_norm_rel"], orl.ULP)


@pytest.mark.parametrize("name", [n for n, cfg in orl.CASES.items() if cfg["kind"] != "Adam"])
def test_first_sync_changes_nothing(fx, name):
    """the slow buffer is created at step k as a copy of the fast weights: up to step 2k - 1 the reference's parameters are those of the
    base optimiser alone (steps 5, 6 and 7 around the first sync at k = 6); the second sync does move them"""
    c, k = fx["cases"][name], orl.CASES[name]["k"]
    free = orl.run(name, fx["p0"], c["grads"], lookahead=False)
    early = [s for s in orl.RECORD if s < 2 * k]
    assert early and (k != 6 or {5, 6, 7} <= set(early))
    for s in early:
        assert np.abs(free["p"][s] - c["p"][s]).max() <= orl.bound(c["ref_abs_max"]["p"], c["p"][s]), (name, s)
    assert np.abs(free["p"][14] - c["p"][14]).max() > 100 * orl.bound(c["ref_abs_max"]["p"], c["p"][14])


def test_step_scalars_of_the_binding():
    from nanosnp_amd import train
    lr, b1, b2 = 1e-3, 0.9, 0.999
    for t in range(1, 15):
        a = train.step_scalars(False, t, lr, b1, b2, 1e-4)
        assert a == dict(a=lr / (1 - b1 ** t), b=1 / math.sqrt(1 - b2 ** t), form=0, wd_mode=1, decay=0.0)
        r = train.step_scalars(True, t, lr, b1, b2, 1e-4)
        n_max = 2 / (1 - b2) - 1
        n_sma = n_max - 2 * t * b2 ** t / (1 - b2 ** t)
        assert r["form"] == (0 if n_sma >= 5 else 1) == (0 if t >= 6 else 1) and r["b"] == 1.0 and r["wd_mode"] == 2 and r["decay"] == -1e-4 * lr
        if t < 6:
            assert r["a"] == lr * (1.0 / (1 - b1 ** t))
        else:
            want = math.sqrt((1 - b2 ** t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t) * lr
            assert r["a"] == want
    n5, n6 = (2 / (1 - b2) - 1 - 2 * t * b2 ** t / (1 - b2 ** t) for t in (5, 6))
    assert abs(n5 - 4.996) < 1e-3 and abs(n6 - 5.994) < 1e-3                       # the switch lies between steps 5 and 6
    assert train.step_scalars(False, 3, lr, b1, b2, 0.0)["wd_mode"] == 0 and train.step_scalars(True, 3, lr, b1, b2, 0.0)["wd_mode"] == 0


PLAN_TABLE = [
    [1], [1024], [1025], list(orl.SIZES), [1] * 64,
    [2048 * 1024 - 1], [2048 * 1024], [2048 * 1024 + 1],                        # 2,048 workgroups are the limit: mult 1, 1, 2
    [2047 * 1024, 1], [2047 * 1024, 1, 1], [2047 * 1024 + 1, 1],                # the same limit reached by several tensors: 1, 2, 2
    [4096 * 1024], [4096 * 1024 + 1], [2048 * 2048, 1],                         # and the next one: 2, 4, 4
    [32 * 1024 + 1] * 64,                                                       # 33 tiles each, 2,112 at mult 1: 17 ranges each at mult 2
    [32 * 1024] * 64, [1 << 31, 3],
] + [list(s["counts"]) for s in orl.RANGE_SETS.values()]


def test_range_map_restated():
    """optim_rules.plan against the library's own opt_plan, through the only figure the library gives away (the grid), and the claims the
    docstring of tests/test_gpu_optim_ranges.py makes of its tensor sets"""
    from nanosnp_amd import _lib
    lib = _lib.load()
    for counts in PLAN_TABLE:
        mult, first = orl.plan(counts)
        assert len(first) == len(counts) + 1 and first[0] == 0 and all(b > a for a, b in zip(first, first[1:])), counts
        assert first[-1] <= 2048 and mult & (mult - 1) == 0, counts
        assert mult == 1 or sum(-(-n // (1024 * (mult // 2))) for n in counts) > 2048, counts             # the SMALLEST such power of two
        assert lib.nsnp_optim_scratch_floats(len(counts), (C.c_int64 * len(counts))(*counts)) == first[-1], counts
    want = {(2048 * 1024 - 1,): (1, 2048), (2048 * 1024,): (1, 2048), (2048 * 1024 + 1,): (2, 1025), (2047 * 1024, 1): (1, 2048),
            (2047 * 1024, 1, 1): (2, 1026), (2047 * 1024 + 1, 1): (2, 1025), (4096 * 1024,): (2, 2048), (4096 * 1024 + 1,): (4, 1025),
            (2048 * 2048, 1): (4, 1025), (32 * 1024 + 1,) * 64: (2, 64 * 17), (32 * 1024,) * 64: (1, 2048)}
    for counts, (mult, grid) in want.items():
        got = orl.plan(counts)
        assert (got[0], got[1][-1]) == (mult, grid), counts
    # the sets of the device test are what it says they are: an accidental change of sizes cannot turn it back into a mult = 1 test
    for name, s in orl.RANGE_SETS.items():
        mult, first = orl.plan(s["counts"])
        assert (mult, first[-1]) == (s["mult"], s["grid"]), name
        assert first[-1] > 257 and s["counts"][s["filler"]] == max(s["counts"]), name                    # a second trip over the partial sums
    two, four = orl.RANGE_SETS["mult2"], orl.RANGE_SETS["mult4"]
    assert sum(-(-n // 1024) for n in two["counts"]) == 2058 and sum(-(-n // 2048) for n in four["counts"]) == 2065
    assert sorted(set(two["counts"]) - {max(two["counts"])}) == [1, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
    assert sorted(set(four["counts"]) - {max(four["counts"])}) == [1, 1023, 1024, 1025, 3073, 4095, 4096, 4097, 6145]
    assert orl.RANGE_SETS["partials"]["counts"] == (300 * 1024 + 5,)
    # the last range of each filler ends inside a tile that is not its first: lanes leave the tile loop at different k
    assert (2041 * 1024 + 5) % 2048 == 1024 + 5 and (2047 * 2048 + 5) % 4096 == 2048 + 5
    assert orl.owner(two["counts"], 4, 2048 * 7 + 1024) == (4 + 7, 1) and orl.first_float_of(two["counts"], 4 + 7) == (4, 2048 * 7)
    assert orl.owner(four["counts"], 9, 6144) == (1034, 2) and orl.first_float_of(four["counts"], 1034) == (9, 4096)


def test_symbols_struct_and_scratch_query():
    from nanosnp_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nanosnp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsnp_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in ("nsnp_optim_step", "nsnp_optim_scratch_floats"):
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTS, name
    fields = re.search(r"typedef struct nsnp_optim_args \{(.*?)\} nsnp_optim_args;", src, flags=re.S).group(1)
    names = [n.strip() for part in fields.split(";") if part.strip() for n in part.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.OptimArgs._fields_] and C.sizeof(_lib.OptimArgs) == 9 * 8 + 3 * 4 + 4
    assert "#define NSNP_OPTIM_MAX_TENSORS 64" in src and _lib.OPTIM_MAX_TENSORS == 64

    def floats(counts):
        arr = (C.c_int64 * max(len(counts), 1))(*counts)
        return lib.nsnp_optim_scratch_floats(len(counts), arr)
    assert floats([1]) == 1 and floats([1024]) == 1 and floats([1025]) == 2 and floats(list(orl.SIZES)) == 9
    assert floats([1] * 64) == 64 and floats([1] * 65) == -1 and floats([]) == -1 and floats([5, 0]) == -1 and floats([-3]) == -1
    assert lib.nsnp_optim_scratch_floats(1, None) == -1
    real = [int(np.prod(s)) for s in _lib.Context.TRAIN_SHAPES]
    assert floats(real) == sum(-(-n // 1024) for n in real)                         # one workgroup per 1,024 floats of a tensor
    assert 1024 < floats([1 << 31, 3]) <= 2048 + 2                                  # a huge tensor: wider ranges, the grid stays bounded
    # without a context the entry refuses before it looks at anything else
    assert lib.nsnp_optim_step(None, 1, None, None, None, None, None, None, None, None, None, None) == -1
