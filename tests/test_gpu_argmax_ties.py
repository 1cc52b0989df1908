"""Exact ties through every argmax of the PileupModel: "first maximum wins, as np.argmax, bit for bit" (include/nanosnp.h,
nsnp_pileup_forward_windows_calls) with outputs in which the tie rules really decide.

Construction, exact in every arithmetic mode: the shipped weights with genotype_layer.weight and zygosity_layer.weight set to zero.  The
logits are then the biases themselves - every product is a zero, the fp32 accumulators start at the bias, and a zero splits into zeros
in the f16x3 and bf16x3 modes - so classes with equal biases have bitwise-equal probabilities at every site, whatever the window holds.

The fused fp32 heads kernel finds the genotype argmax in three stages, each with a tie rule of its own: inside a lane over classes
4q .. 4q + 3, against the lane's extra classes (16 .. 19 in lane q = 0, 20 in lane q = 1), across the four q lanes of a site.  Every pair
of the 21 classes is tied once, so every pair of lanes and every lane boundary is."""
import itertools

import numpy as np
import pytest

GT_W, GT_B, ZY_W, ZY_B = 20, 21, 22, 23            # positions in nanosnp_amd.fixtures.PILEUP_WEIGHT_KEYS
N_SITES = 130                                       # eight 16-site groups and a ragged one of two


def _bias(n, level):
    b = np.zeros(n, np.float32)
    for classes, v in level.items():
        b[list(classes)] = v
    return b


def _patterns(group):
    """[(name, genotype bias [21], zygosity bias [3])].  Tied classes share the bias 2 over a floor of 0; "beside" adds one class at 3:
    the tie is then for second place and must not win.  The zygosity patterns ride along, cycling."""
    zy = [_bias(3, {p: 2.0}) for p in itertools.combinations(range(3), 2)] + [_bias(3, {(0, 1, 2): 2.0})]
    zy += [_bias(3, {(0, 1): 2.0, (2,): 3.0}), _bias(3, {(1, 2): 2.0, (0,): 3.0}), _bias(3, {(0, 2): 2.0, (1,): 3.0})]
    if group == "pairs":
        gt = [("pair %d %d" % p, _bias(21, {p: 2.0})) for p in itertools.combinations(range(21), 2)]
        assert len(gt) == 210
    elif group == "triples-and-all":
        gt = [("triple %d %d %d" % t, _bias(21, {t: 2.0})) for t in ((3, 4, 16), (7, 12, 20), (0, 19, 20))]
        gt += [("all equal", _bias(21, {tuple(range(21)): 2.0})), ("all zero", np.zeros(21, np.float32))]
        gt += [("all but %d" % k, _bias(21, {tuple(c for c in range(21) if c != k): 2.0})) for k in (0, 3, 16, 20)]
    else:
        gt = [("pair %d %d beside %d" % (a, b, c), _bias(21, {(a, b): 2.0, (c,): 3.0}))
              for a, b, c in ((0, 1, 20), (0, 1, 2), (16, 20, 5), (3, 4, 19), (17, 18, 16), (4, 20, 7), (19, 20, 0), (2, 3, 1), (8, 12, 13))]
    return [(name, g, zy[i % len(zy)]) for i, (name, g) in enumerate(gt)]


GROUPS = ["pairs", "triples-and-all", "beside-larger"]


def _weights(pileup_weights, gb, zb):
    w = [np.array(a, dtype=np.float32, copy=True) for a in pileup_weights]
    w[GT_W][:] = 0; w[ZY_W][:] = 0
    w[GT_B][:] = gb; w[ZY_B][:] = zb
    return w


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tie_errors(prob, bias):
    """the hard precondition: classes of equal bias have bitwise-equal probabilities at EVERY site -> list of offending bias values"""
    bad = []
    pb = _bits(prob)
    for v in np.unique(bias):
        cols = np.flatnonzero(bias == v)
        if not (pb[:, cols] == pb[:, cols[:1]]).all():
            bad.append(float(v))
    return bad


def _check(prob, bias, arg, mx):
    """-> list of what is wrong with one head's (probabilities, argmax, max) for the bias pattern"""
    errs = []
    if prob.shape[0] != N_SITES or not np.isfinite(prob).all():
        return ["shape / non-finite probabilities"]
    bad = _tie_errors(prob, bias)
    if bad:
        return ["classes of bias %s are not bitwise equal at every site" % bad]
    first = int(np.flatnonzero(bias == bias.max())[0])              # min(tied classes of the maximum)
    if not (prob[:, first][:, None] >= prob).all() or ((prob[:, first][:, None] == prob).sum(1) != (bias == bias.max()).sum()).any():
        errs.append("the classes of the largest bias are not exactly the maxima")
    if not np.array_equal(arg, np.full(N_SITES, first)):
        errs.append("argmax %s, want %d everywhere" % (np.unique(arg).tolist(), first))
    if not np.array_equal(_bits(mx), _bits(prob[:, first])):
        errs.append("max is not the bits of class %d" % first)
    if not np.array_equal(arg, np.argmax(prob, 1)) or not np.array_equal(_bits(mx), _bits(np.max(prob, 1))):
        errs.append("differs from np.argmax / np.max of the returned probabilities")
    return errs


def _windows(seed=5):
    rng = np.random.default_rng(seed)
    m = 3000
    counts = rng.integers(-30, 40, (m, 18)).astype(np.int32)
    centers = rng.choice(np.arange(16, m - 16), N_SITES, replace=False).astype(np.int64)
    return counts, centers


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_probabilities_are_tied_bitwise_for_these_weights(pileup_weights, group):
    """the CPU oracle with the same weights: equal biases give bitwise-equal probabilities at every site (what the GPU tests below demand
    of every kernel path as a precondition), and np.argmax then takes the first of them"""
    from oracle import oracle
    counts, centers = _windows()
    x = np.stack([counts[c - 16:c + 17] for c in centers[:24]])
    for name, gb, zb in _patterns(group):
        gt, zy = oracle.pileup_forward(_weights(pileup_weights, gb, zb), x, nthreads=8)
        assert not _tie_errors(gt, gb) and not _tie_errors(zy, zb), name
        assert np.array_equal(np.argmax(gt, 1), np.full(24, np.flatnonzero(gb == gb.max())[0])), name
        assert np.array_equal(np.argmax(zy, 1), np.full(24, np.flatnonzero(zb == zb.max())[0])), name


# (options on top of the defaults, the call): every generation of heads kernel and both ways to the argmax
DEFAULTS = {"pileup_precision": 0, "head_split": 1, "l0_register_stationary": 2, "l1_register_stationary": 1}
PATHS = [("fp32 fused heads", {}, "calls"),
         ("fp32 one-wave heads", {"head_split": 0}, "calls"),
         ("fp32 LDS-image kernels", {"l0_register_stationary": 0, "l1_register_stationary": 0}, "calls"),
         ("f16x3", {"pileup_precision": 1}, "calls"),
         ("bf16x3", {"pileup_precision": 2}, "calls"),
         ("fp32 fused heads, pinned outputs", {}, "pinned"),
         ("forward + postprocess", {}, "two-call"),
         ("f16x3 forward + postprocess", {"pileup_precision": 1}, "two-call"),
         ("bf16x3 forward + postprocess", {"pileup_precision": 2}, "two-call")]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_ties_resolve_to_the_first_maximum_on_every_path(pileup_weights, group):
    """every pattern x every path, N = 130 random windows: first the precondition (tied bitwise at every site, nothing skipped), then
    gt_arg / zy_arg = the lowest tied class, gt_max / zy_max = its bits, all equal to np.argmax / np.max of the returned arrays.  One
    weight load per pattern, the paths looped inside; every failure is collected so that one run names them all."""
    import torch
    from nanosnp_amd import _lib
    counts_np, centers_np = _windows()
    c = _lib.Context(0)
    counts = torch.from_numpy(counts_np).cuda(); centers = torch.from_numpy(centers_np).cuda()
    pin = [torch.zeros(N_SITES, dtype=dt, pin_memory=True) for dt in (torch.uint8, torch.uint8, torch.float32, torch.float32)]
    failures = []
    for name, gb, zb in _patterns(group):
        c.pileup_load_weights(_weights(pileup_weights, gb, zb))
        for path, opts, call in PATHS:
            for k, v in {**DEFAULTS, **opts}.items():
                c.set_option(k, v)
            if call == "two-call":
                x = c.pileup_gather_windows(counts, centers)
                gt, zy = c.pileup_forward(x)
                ga, za, gm, zm, _ = c.pileup_postprocess(gt, zy, x)
            elif call == "pinned":
                for t in pin:
                    t.zero_()
                gt, zy, ga, za, gm, zm = c.pileup_forward_windows_calls(counts, centers, calls_out=tuple(pin))
            else:
                gt, zy, ga, za, gm, zm = c.pileup_forward_windows_calls(counts, centers)
            torch.cuda.synchronize()
            out = [t.cpu().numpy().copy() for t in (gt, zy, ga, za, gm, zm)]
            for head, errs in (("genotype", _check(out[0], gb, out[2], out[4])), ("zygosity", _check(out[1], zb, out[3], out[5]))):
                failures += ["%s | %s | %s: %s" % (name, path, head, e) for e in errs]
    for k, v in DEFAULTS.items():
        c.set_option(k, v)
    c.close()
    assert not failures, "%d failures, the first: %s" % (len(failures), failures[:12])
