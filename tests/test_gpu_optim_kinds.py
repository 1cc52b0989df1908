"""Novograd, LookaheadNovograd, SGD and Adadelta as one fused device step (nsnp_optim_step_kind, the kinds "Novograd", "LookaheadNovograd",
"sgd", "adadelta" of nanosnp_amd.train.DeviceOptimizer) against the float64 restatement tests/optim_kinds_rules.py, on the cases the
reference's own novograd.py / lookahead.py and torch's SGD / Adadelta ran (tests/golden/pileup_optim_kinds.npz).

Fixture parity, per case, recorded step and tensor: max |p_dev - p_f64| <= 4 x max(ref_abs_max, 2^-23 max |p|), ref_abs_max the reference's
OWN fp32 distance from float64 recorded in the fixture (tests/test_gpu_optim_step.py has the rule); the per-element states and the slow
buffers by the same rule on their own magnitudes and distances; Novograd's per-tensor v and the norms relative, 4 x max(the reference's own
relative distance, 2^-23).

Where there is no recorded reference (segments, 301 partials, ranges of two tiles: ONE Novograd step against float64) the bounds are counted
in fp32 roundings R = 2^-24 relative, on top of the counts of tests/test_gpu_optim_ranges.py for a range of `mult` tiles: a partial sum
mult + 11, the norm N = (mult + 11) / 2 + 1, the coefficient c = max_norm / (norm + 1e-6) N + 2.  Then
    n_t = (float)(c c seg_t)       the segment sum is float64 (nothing), c c carries 2 (N + 2), the partials mult + 11, the cast 1:
                                   V = 2 (N + 2) + mult + 12                                                    (32 at mult 1, 34 at mult 2)
    v_t' = beta2 v_t + (1 - beta2) n_t   |v' - v'_f64| <= R ((V + 2) (1 - beta2) n_t + 2 beta2 v_t + v_t'); from v_t = 0 it is n_t: R V n_t
    d = sqrt(v_t') + eps           half of v's count (taken at V + 2, the averaged form), the root (v_sqrt_f32: 1 ulp = 2), the sum: V / 2 + 4
    x = (g c) / d                  (N + 2) + 1 + (V / 2 + 4) + 1:  X = N + V / 2 + 8                             (31 at mult 1, 32.5 at mult 2)
    m = beta1 m + x                |m - m_f64| <= R (X max |x| + 2 max |beta1 m0| + max |m|)
A parameter moves by lr m, about 1e-3 of its magnitude here, so those relative errors reach it far below its own rounding: the floor alone,
4 x 2^-23 max |p|.

The shapes are the ones that can break the step: the eight SHAPES of the fixture (every tail, a two-range tensor); a four-range tensor
between two one-range tensors whose gradients are 2^12 larger and 2^12 smaller (a segment that takes a partial too many or too few misses
v_t by far more than a rounding); one tensor of 301 ranges (more partials than lanes); ranges of two tiles (a partial belongs to a range, not
to a tile); 64 tensors of one element (the table's limit, a segment of one partial each).

Distances measured on an MI355X: docs/rounds/r34.md."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_rules as er
from tests import optim_kinds_rules as okr
from tests import optim_rules as orl
from tests.test_gpu_optim_ranges import R, SETS, _cut, _flats, _state, norm_roundings
from tests.test_gpu_optim_step import _dev

pytestmark = pytest.mark.gpu
B1, B2, EPS = okr.BETAS[0], okr.BETAS[1], okr.NOVOGRAD_EPS


def v_roundings(mult):
    return 2 * (norm_roundings(mult) + 2) + mult + 12        # (the module docstring counts them)


def x_roundings(mult):
    return norm_roundings(mult) + v_roundings(mult) / 2 + 8


def _top(a):
    return float(np.abs(a).max())


@pytest.fixture(scope="module")
def fx():
    return okr.load_fixture()


@pytest.fixture(scope="module")
def f64(fx):
    """the float64 trajectories, computed once and shared"""
    return {name: okr.run(name, fx["p0"], c["grads"]) for name, c in fx["cases"].items()}


def _kind_args(**kw):
    from nanosnp_amd import _lib
    a = _lib.OptimKindArgs()
    vals = dict(kind=_lib.OPTIM_NOVOGRAD, lr=1e-3, beta1=B1, beta2=B2, eps=EPS, weight_decay=0.0, momentum=0.0, nesterov=0, rho=okr.RHO,
                alpha=0.5, max_norm=1.0, sync=0)
    vals.update(kw)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def _states_of(opt):
    """the per-element states of a DeviceOptimizer in the order of okr.STATES -> [flat, flat] (None where the kind has none)"""
    out = [orl.join([t.cpu().numpy() for t in getattr(opt, name)]) for name in opt.state_names]
    return out + [None] * (2 - len(out))


def _set_grads(params, gdev, s):
    o = 0
    for p, n in zip(params, orl.SIZES):
        p.grad = gdev[s - 1, o:o + n].view(p.shape)
        o += n


def _run_case(ctx, name, fx, first=1, last=orl.STEPS, opt=None, params=None):
    """steps first .. last of a case through DeviceOptimizer -> (dict as optim_kinds_rules.run returns it, the gradient tensors, the
    optimizer, the parameters)"""
    import torch
    from nanosnp_amd import train
    cfg, c = okr.CASES[name], fx["cases"][name]
    if params is None:
        params = [torch.nn.Parameter(_dev(a)) for a in orl.split(fx["p0"])]
    if opt is None:
        opt = train.DeviceOptimizer(params, ctx=ctx, **okr.optimizer_kwargs(cfg))
    gdev = _dev(c["grads"])                                             # [STEPS, TOTAL]: every step's gradients are views of one row
    out, norms = dict(p={}, v_at={}), []
    for s in range(first, last + 1):
        _set_grads(params, gdev, s)
        norms.append(opt.step(cfg["max_norm"]))
        if s in (2, 3) and opt.layer_v is not None:
            out["v_at"][s] = opt.layer_v.cpu().numpy().copy()
        if s in orl.RECORD:
            out["p"][s] = orl.join([p.detach().cpu().numpy() for p in params])
    torch.cuda.synchronize()
    out["norm"] = np.array([float(n) for n in norms])
    out["a"], out["b"] = _states_of(opt)
    out["v"] = opt.layer_v.cpu().numpy().copy() if opt.layer_v is not None else None
    out["slow"] = orl.join([t.cpu().numpy() for t in opt.slow]) if opt.slow is not None else None
    return out, gdev, opt, params


# ---- 1. the reference's own runs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(okr.CASES))
def test_fixture_parity(gpu_ctx, fx, f64, name):
    c, want = fx["cases"][name], f64[name]
    got, gdev, opt, _ = _run_case(gpu_ctx, name, fx)
    assert opt.global_step == 1 + orl.STEPS and opt.step_count == orl.STEPS
    # each kind owns the state it uses and nothing else
    owned = {q for q in ("exp_avg", "exp_avg_sq", "momentum_buffer", "square_avg", "acc_delta") if getattr(opt, q) is not None}
    assert owned == (set(okr.STATES[okr.RULE[opt.kind]]) if okr.CASES[name].get("momentum", 1.0) != 0 else set()), owned
    assert (opt.layer_v is not None) == (okr.RULE[opt.kind] == "novograd") and (opt.slow is not None) == (name == "la_novograd_wd")
    worst = {}
    for s in orl.RECORD:
        for i, (a, b) in enumerate(zip(orl.split(got["p"][s]), orl.split(want["p"][s]))):
            d, bd = float(np.abs(a - b).max()), orl.bound(c["ref_abs_max"]["p"], b)
            worst["p"] = max(worst.get("p", 0.0), d / bd)
            assert np.isfinite(a).all() and d <= bd, (name, "p", s, i, d, bd)
    for q in ("a", "b", "slow"):
        assert (got[q] is None) == (c[q] is None), (name, q)
        if c[q] is not None:
            for i, (a, b) in enumerate(zip(orl.split(got[q]), orl.split(want[q]))):
                d, bd = float(np.abs(a - b).max()), orl.bound(c["ref_abs_max"][q], b)
                worst[q] = max(worst.get(q, 0.0), d / bd)
                assert np.isfinite(a).all() and d <= bd, (name, q, i, d, bd)
    if c["v"] is not None:
        vb = orl.FACTOR * max(c["ref_v_rel"], orl.ULP)
        z = okr.ZERO_TENSOR
        for what, mine, ref in (("v14", got["v"], want["v"]), ("v2", got["v_at"][2], want["v_at"][2]), ("v3", got["v_at"][3], want["v_at"][3])):
            assert np.array_equal(mine == 0, ref == 0), (name, what, mine, ref)
            nz = ref != 0
            rel = float(np.abs(mine[nz] / ref[nz] - 1.0).max())
            worst["v"] = max(worst.get("v", 0.0), rel / vb)
            assert rel <= vb, (name, what, rel, vb)
        assert got["v_at"][2][z] == 0.0 and got["v_at"][3][z] > 0.0          # the copy branch at step 3, two steps behind its neighbours
    rel = float(np.abs(got["norm"] / c["norm"].astype(np.float64) - 1.0).max())
    nb = orl.FACTOR * max(c["ref_norm_rel"], orl.ULP)
    print(f"{name}: worst distance / bound " + " ".join(f"{q} {w:.3f}" for q, w in worst.items()) + f"; norm rel {rel:.2e} (bound {nb:.2e}); "
          f"max |p_dev - p_f64| {max(np.abs(got['p'][s] - want['p'][s]).max() for s in orl.RECORD):.2e}, ref_abs_max {c['ref_abs_max']['p']:.2e}")
    assert rel <= nb, (name, rel, nb)
    assert np.array_equal(gdev.cpu().numpy(), c["grads"])                 # the gradient buffers are bit-unchanged


# ---- 2. one Novograd step against float64: segments, partials, wide ranges ----------------------------------------------------------------------
def _novograd_step_against_float64(ctx, counts, mult, host, v_in, max_norm, wd, sync=0):
    """host: packed fp32 [p, g, m0(, slow)]; v_in fp32 [n_tensors].  One step of the raw entry from this state against KindRules."""
    import torch
    flats, lists, inside = _flats(counts, host)
    layer_in, layer_out = _dev(v_in), torch.full((len(counts),), -3.0, dtype=torch.float32, device="cuda")
    norm = torch.full((), -5.0, dtype=torch.float32, device="cuda")
    tensors = (lists[0], lists[1], lists[2], None, lists[3] if sync else None)
    ctx.optim_kind_step(tensors, _kind_args(max_norm=max_norm, weight_decay=wd, sync=sync), layer_in, layer_out, grad_norm_out=norm)
    torch.cuda.synchronize()
    p0, g, m0 = (_cut(a, counts) for a in host[:3])
    ref = okr.KindRules(p0, "LookaheadNovograd" if sync else "Novograd", lr=1e-3, weight_decay=wd, k=1)
    ref.a, ref.v, ref.t = list(m0), np.array(v_in, np.float64), 2
    if sync:
        ref.slow = _cut(host[3], counts)
    want_norm = ref.step(g, max_norm)
    assert want_norm > 4 * max_norm                          # clipped hard: a wrong total moves every x
    c = min(1.0, max_norm / (want_norm + 1e-6))
    rel = abs(float(norm) / want_norm - 1.0)
    assert rel <= norm_roundings(mult) * R, rel
    got_v = layer_out.cpu().numpy()
    worst = dict(v=0.0, m=0.0, p=0.0, slow=0.0)
    for i in range(len(counts)):
        n_t = float(((g[i] * c) ** 2).sum())
        vb = R * v_roundings(mult) * n_t if v_in[i] == 0 else R * ((v_roundings(mult) + 2) * (1 - B2) * n_t + 2 * B2 * float(v_in[i]) + ref.v[i])
        worst["v"] = max(worst["v"], abs(float(got_v[i]) - ref.v[i]) / vb)
        assert abs(float(got_v[i]) - ref.v[i]) <= vb, ("v", i, float(got_v[i]), ref.v[i], vb)
        x = ref.a[i] - B1 * m0[i]
        mb = R * (x_roundings(mult) * _top(x) + 2 * _top(B1 * m0[i]) + _top(ref.a[i]))
        checks = [("m", lists[2][i], ref.a[i], mb), ("p", lists[0][i], ref.p[i], orl.bound(0.0, ref.p[i]))]
        if sync:
            checks.append(("slow", lists[3][i], ref.slow[i], orl.bound(0.0, ref.slow[i])))
        for q, got, want, bd in checks:
            a = got.cpu().numpy()
            d = _top(a - want)
            worst[q] = max(worst[q], d / bd)
            assert np.isfinite(a).all() and d <= bd, (q, i, d, bd)
    assert np.array_equal(flats[1].cpu().numpy()[inside.cpu().numpy()], host[1])                 # the gradients are bit-unchanged
    assert np.array_equal(layer_in.cpu().numpy(), v_in)                                          # and so is what the step read
    for flat in flats:
        assert bool((flat[~inside] == 77.0).all())
    return worst, rel


def test_segment_bounds(gpu_ctx):
    """a tensor of 3 x 1024 + 1 floats (four ranges) between two one-range tensors whose gradients are 2^12 times larger (1 float) and 2^12
    times smaller (7 floats): per float n_t differs by 2^24 between neighbours, so one partial across a boundary is no rounding.  From
    v = 0 everywhere: every tensor copies its own n_t."""
    counts = (1, 3 * 1024 + 1, 7)
    assert orl.plan(counts) == (1, [0, 1, 5, 6])
    rng = np.random.default_rng([34, 1])
    total = sum(counts)
    scale = np.concatenate([np.full(n, s, np.float32) for n, s in zip(counts, (2.0 ** 12, 1.0, 2.0 ** -12))])
    g = (rng.uniform(0.5, 1.0, total) * rng.choice([-1.0, 1.0], total)).astype(np.float32) * scale
    p = (rng.uniform(0.05, 0.15, total) * rng.choice([-1.0, 1.0], total)).astype(np.float32)
    worst, rel = _novograd_step_against_float64(gpu_ctx, counts, 1, [p, g, np.zeros(total, np.float32)], np.zeros(3, np.float32), 1.0, 0.0)
    # (the least that one partial across a boundary would do, against the bound: the middle tensor without its last range, which holds
    # ONE float; the first tensor with the middle one's first range; the others are off by far more)
    n = [float((a.astype(np.float64) ** 2).sum()) for a in _cut(g, counts)]
    assert float(g[-8]) ** 2 / n[1] > 50 * R * v_roundings(1) and 1024 * 0.25 / n[0] > 4 * R * v_roundings(1)
    print("segments: worst distance / bound " + " ".join(f"{q} {r:.3f}" for q, r in worst.items()) + f"; norm rel {rel:.2e}")


@pytest.mark.parametrize("name", ["partials", "mult2"])
def test_more_partials_than_lanes_and_ranges_wider_than_a_tile(gpu_ctx, name):
    """partials: one tensor of 301 ranges (lanes 0 .. 44 add a second partial) - as the set stands it has no neighbours, so two small
    tensors are put around it.  mult2: a partial belongs to a range of two tiles.  Step 3 from non-trivial moments, v on the averaging
    branch except for the first tensor, whose v is 0: it copies.  With weight decay and a Lookahead sync."""
    counts, mult = SETS[name]["counts"], SETS[name]["mult"]
    packed = _state(name)
    if name == "partials":
        rng = np.random.default_rng([34, 2])
        extra = lambda n, s: (rng.standard_normal(n).astype(np.float32) * np.float32(s))
        counts = (3,) + tuple(counts) + (1025,)
        packed = [np.concatenate([extra(3, s), a, extra(1025, s)]) for a, s in zip(packed, (0.1, 0.05, 0.01, 1e-4, 0.1))]
        packed[0][:3] += np.float32(0.5)                     # (no parameter so small that a move of about lr outweighs its own rounding)
        assert orl.plan(counts) == (1, [0, 1, 302, 304])
    assert orl.plan(counts)[0] == mult
    host = [packed[0], packed[1], packed[2], packed[4]]
    g = _cut(packed[1], counts)
    v_in = np.array([0.0] + [0.5 * float((a ** 2).sum()) * 1e-3 for a in g[1:]], np.float32)
    worst, rel = _novograd_step_against_float64(gpu_ctx, counts, mult, host, v_in, 1.0, 1e-4, sync=1)
    print(f"{name}: worst distance / bound " + " ".join(f"{q} {r:.3f}" for q, r in worst.items()) + f"; norm rel {rel:.2e}")


def test_64_tensors_of_one_element(gpu_ctx):
    """one Novograd step, no weight decay, no clipping: every segment is one partial of one float, v_t = g^2 within ONE rounding (g g is
    rounded once, zeros are added, c = 1) and p moves by lr g / (|g| + eps)"""
    import torch
    from nanosnp_amd import train
    rng = np.random.default_rng(64)
    draw = lambda: (rng.uniform(0.5, 1.5, 1) * rng.choice([-1.0, 1.0])).astype(np.float32)
    p0, g = [draw() for _ in range(64)], [draw() for _ in range(64)]
    params = [torch.nn.Parameter(_dev(a)) for a in p0]
    for p, a in zip(params, g):
        p.grad = _dev(a)
    opt = train.DeviceOptimizer(params, kind="Novograd", lr=1e-2, ctx=gpu_ctx)
    norm = opt.step(None)
    want_norm = float(np.sqrt(sum(float(a[0]) ** 2 for a in g)))
    assert abs(float(norm) / want_norm - 1.0) <= orl.FACTOR * orl.ULP
    v = opt.layer_v.cpu().numpy()
    for i in range(64):
        gi, pi = float(g[i][0]), float(p0[i][0])
        assert abs(float(v[i]) / (gi * gi) - 1.0) <= R, (i, float(v[i]), gi * gi)
        want = pi - 1e-2 * gi / (abs(gi) + EPS)
        # one rounding of the stored parameter (2^-24 |p|) and the few roundings of m = +-1, scaled by lr: 2^-23 |p| holds both
        assert abs(float(params[i].detach()) - want) <= orl.ULP * abs(want), (i, float(params[i].detach()), want)
        # m = g / (sqrt(fl(g g)) + eps): half a rounding from v, the root (1 ulp: 2), the sum, the division
        assert abs(float(opt.exp_avg[i]) - gi / (abs(gi) + EPS)) <= 4.5 * R


# ---- 3. the same bits ----------------------------------------------------------------------------------------------------------------------------
def _kind_state(fx, kind):
    """host lists [p, g, a, b, slow] with non-trivial states (>= 0 where a root is taken) and Novograd's v"""
    rng = np.random.default_rng([34, 3, kind])
    p = orl.split(fx["p0"])
    g = orl.split(fx["cases"]["la_novograd_wd"]["grads"][2])
    a = [(rng.random(x.shape) * 1e-2).astype(np.float32) for x in p]
    b = [(rng.random(x.shape) * 1e-4).astype(np.float32) for x in p]
    slow = [(x + rng.standard_normal(x.shape).astype(np.float32) * 0.01).astype(np.float32) for x in p]
    v = (rng.random(len(p)) * 0.1).astype(np.float32)
    v[2] = 0.0
    return [p, g, a, b, slow], v


def _three_kind_steps(ctx, kind, lists, v):
    """no sync, the first sync, a sync, the layer arrays changing places behind each -> every tensor's bytes, the two layer arrays (the one
    that began as v, the one that began as zeros and is written last), the three norms"""
    import torch
    layer = [_dev(v), torch.zeros(len(v), dtype=torch.float32, device="cuda")]
    both = list(layer)
    norms = []
    for sync in (0, 2, 1):
        n = torch.zeros((), dtype=torch.float32, device="cuda")
        ctx.optim_kind_step(tuple(lists), _kind_args(kind=kind, sync=sync, weight_decay=1e-4, momentum=0.9, nesterov=1, eps=1e-6, lr=1e-2),
                            layer[0], layer[1], grad_norm_out=n)
        layer.reverse()
        norms.append(n)
    torch.cuda.synchronize()
    return [[t.cpu().numpy().copy() for t in ts] for ts in lists], np.stack([t.cpu().numpy() for t in both]), [float(n) for n in norms]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_views_at_an_odd_offset_give_the_same_bits(gpu_ctx, fx, kind):
    """tensors allocated on their own, and as views 1, 2 and 3 floats behind a 16-byte boundary of one flat buffer per list"""
    import torch
    from nanosnp_amd import _lib
    assert (_lib.OPTIM_NOVOGRAD, _lib.OPTIM_SGD, _lib.OPTIM_ADADELTA) == (0, 1, 2)
    host, v = _kind_state(fx, kind)
    want, want_v, want_norms = _three_kind_steps(gpu_ctx, kind, [[_dev(a) for a in ts] for ts in host], v)
    assert not np.array_equal(want[0][4], host[0][4]) and np.array_equal(want[1][4], host[1][4])         # p moved, g did not
    assert not np.array_equal(want[2][4], host[2][4]) and (kind == 2) == (not np.array_equal(want[3][4], host[3][4]))
    if kind == 0:
        assert bool((want_v > 0).all()) and not np.array_equal(want_v[0], v)                             # both were written
    else:
        assert np.array_equal(want_v[0], v) and not want_v[1].any()                                     # the other kinds leave them alone
    for off in (1, 2, 3):
        lists, flats = [], []
        for ts in host:
            starts, cur = [], 0
            for a in ts:
                cur = (cur + 3) // 4 * 4 + off
                starts.append(cur)
                cur += a.size
            flat = torch.full((cur + 8,), 77.0, dtype=torch.float32, device="cuda")
            assert flat.data_ptr() % 16 == 0
            views = [flat[o:o + a.size].view(a.shape) for o, a in zip(starts, ts)]
            for vw, a in zip(views, ts):
                vw.copy_(torch.from_numpy(a))
                assert vw.data_ptr() % 16 == 4 * off
            lists.append(views); flats.append((flat, starts, [a.size for a in ts]))
        got, got_v, norms = _three_kind_steps(gpu_ctx, kind, lists, v)
        assert norms == want_norms and np.array_equal(got_v.view(np.int32), want_v.view(np.int32)), off
        for ts_got, ts_want in zip(got, want):
            for i, (a, b) in enumerate(zip(ts_got, ts_want)):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (off, i)
        for flat, starts, sizes in flats:                            # and nothing between or behind the views was written
            keep = np.ones(flat.numel(), bool)
            for o, n in zip(starts, sizes):
                keep[o:o + n] = False
            assert (flat.cpu().numpy()[keep] == 77.0).all(), off


@pytest.mark.parametrize("name", ["la_novograd_wd", "sgd_nesterov", "adadelta_wd"])
def test_same_run_same_bits(gpu_ctx, fx, name):
    """the same 14 steps twice: the layer arrays change places 14 times and end where they began"""
    a, _, _, _ = _run_case(gpu_ctx, name, fx)
    b, _, _, _ = _run_case(gpu_ctx, name, fx)
    for s in orl.RECORD:
        assert np.array_equal(a["p"][s], b["p"][s])
    for q in ("a", "b", "v", "slow", "norm"):
        assert (a[q] is None) == (b[q] is None) and (a[q] is None or np.array_equal(a[q], b[q])), q


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_ctx, fx):
    import torch
    from nanosnp_amd import _lib
    ctx = gpu_ctx
    host, v = _kind_state(fx, 0)
    lists = [[_dev(a) for a in ts] for ts in host]
    n = len(host[0])
    ot = ctx.optim_tensors(*lists)
    scratch = torch.zeros(ot.scratch_floats, dtype=torch.float32, device="cuda")
    norm = torch.full((), -5.0, dtype=torch.float32, device="cuda")
    layer_in, layer_out = _dev(v), torch.full((n,), -3.0, dtype=torch.float32, device="cuda")
    lib, h, s = ctx.lib, ctx.handle, _lib._stream_ptr()
    sp, np_, li, lo = (C.c_void_p(t.data_ptr()) for t in (scratch, norm, layer_in, layer_out))
    NOVO, SGD, ADA = _lib.OPTIM_NOVOGRAD, _lib.OPTIM_SGD, _lib.OPTIM_ADADELTA

    def call(ctx_=h, n_=n, p=ot.params, g=ot.grads, a=ot.exp_avg, b=ot.exp_avg_sq, sl=ot.slow, cnt=ot.counts, args=_kind_args(sync=1), lin=li,
             lout=lo, scr=sp, nrm=np_):
        return lib.nsnp_optim_step_kind(ctx_, n_, p, g, a, b, sl, cnt, None if args is None else C.byref(args), lin, lout, scr, nrm, s)
    hole = (C.c_void_p * n)(*[None if i == 5 else t.data_ptr() for i, t in enumerate(lists[2])])
    odd = (C.c_void_p * n)(*[t.data_ptr() + (2 if i == 3 else 0) for i, t in enumerate(lists[0])])
    zero = (C.c_int64 * n)(*[0 if i == 6 else a.size for i, a in enumerate(host[0])])
    big = (C.c_void_p * 65)(*([lists[0][0].data_ptr()] * 65))
    big_n = (C.c_int64 * 65)(*([1] * 65))
    mom = dict(kind=SGD, momentum=0.9, sync=1)
    # null pointers: the tables every kind uses, and the state tables of the kind that uses them
    assert call(ctx_=None) == -1 and call(p=None) == -1 and call(g=None) == -1 and call(cnt=None) == -1 and call(args=None) == -1
    assert call(a=None) == -1 and call(sl=None) == -1 and call(a=hole) == -1
    assert call(a=None, args=_kind_args(**mom)) == -1 and call(a=None, args=_kind_args(kind=ADA)) == -1 and call(b=None, args=_kind_args(kind=ADA)) == -1
    assert call(b=hole, args=_kind_args(kind=ADA)) == -1
    # misaligned pointers, counts, the table's limit
    assert call(p=odd) == -1 and call(a=odd) == -1 and call(b=odd, args=_kind_args(kind=ADA)) == -1
    assert call(lin=C.c_void_p(layer_in.data_ptr() + 2)) == -1 and call(lout=C.c_void_p(layer_out.data_ptr() + 2)) == -1
    assert call(scr=C.c_void_p(scratch.data_ptr() + 2)) == -1 and call(nrm=C.c_void_p(norm.data_ptr() + 2)) == -1
    assert call(cnt=zero) == -1 and call(n_=0) == -1
    assert call(n_=65, p=big, g=big, a=big, b=big, sl=big, cnt=big_n) == -1
    # the scalars
    for bad in (dict(kind=3), dict(kind=-1), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(rho=1.0),
                dict(rho=-0.1), dict(momentum=1.0), dict(momentum=-0.1), dict(alpha=1.5), dict(alpha=-0.1), dict(sync=3), dict(nesterov=2),
                dict(kind=SGD, nesterov=1, momentum=0.0), dict(kind=NOVO, nesterov=1), dict(kind=ADA, rho=float("nan"))):
        assert call(args=_kind_args(**{"sync": 1, **bad})) == -1, bad
    # Novograd without scratch or without both layer arrays, and the two arrays being one
    assert call(scr=None) == -1 and call(lin=None) == -1 and call(lout=None) == -1 and call(lin=lo) == -1 and call(lout=li) == -1
    # the other kinds need scratch only for a norm
    assert call(scr=None, args=_kind_args(**mom)) == -1 and call(scr=None, nrm=None, args=_kind_args(**mom)) == -1       # (max_norm 1 clips)
    torch.cuda.synchronize()
    for ts, hs in zip(lists, host):
        assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(ts, hs))
    assert float(norm) == -5.0 and not bool(scratch.any()) and bool((layer_out == -3.0).all()) and np.array_equal(layer_in.cpu().numpy(), v)
    assert call() == 0                                                              # (and the same arguments do run)
    torch.cuda.synchronize()
    assert float(norm) > 0 and not np.array_equal(lists[0][4].cpu().numpy(), host[0][4]) and bool((layer_out > 0).all())
    assert np.array_equal(lists[3][4].cpu().numpy(), host[3][4])                    # Novograd does not touch a second state table
    # SGD without a momentum takes no buffer, no layer arrays and, with nothing to clip or report, no scratch
    before = lists[0][4].cpu().numpy().copy()
    assert call(a=None, b=None, sl=None, lin=None, lout=None, scr=None, nrm=None, args=_kind_args(kind=SGD, max_norm=0.0)) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(lists[0][4].cpu().numpy(), before)
    # the binding's own checks
    good = [[_dev(a) for a in ts] for ts in host]
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_kind_step((good[0], good[1], good[2], None), _kind_args(sync=1), layer_in, layer_out)      # a sync without slow buffers
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_kind_step((good[0], good[1], None, None), _kind_args(), layer_in, layer_out)               # Novograd without exp_avg
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_kind_step((good[0], good[1], good[2], None), _kind_args(kind=ADA))                         # Adadelta without acc_delta
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_kind_step((good[0], good[1], good[2], None), _kind_args(), layer_in, None)
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_kind_step((good[0], good[1], good[2], None), _kind_args(), layer_in[:3], layer_out)
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_kind_step((good[0], good[1], good[2], None), _lib.OptimArgs(), layer_in, layer_out)
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_step((good[0], good[1], good[2], None), _lib.OptimArgs())                                  # the Adam entry needs both moments
    assert all(np.array_equal(t.cpu().numpy(), a) for ts, hs in zip(good, host) for t, a in zip(ts, hs))


# ---- 5. checkpoints --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["la_novograd_wd", "novograd_plain", "sgd_nesterov", "sgd_plain", "adadelta_wd"])
def test_resume_is_bit_exact(gpu_ctx, fx, name, tmp_path):
    """14 straight steps = 7 steps, state_dict() through torch.save / torch.load, a fresh DeviceOptimizer over copies of the parameters plus
    load_state_dict, the other 7.  la_novograd_wd is cut between the first sync (step 6, which fills the slow buffers) and the second."""
    import torch
    from nanosnp_amd import train
    want, _, _, _ = _run_case(gpu_ctx, name, fx)
    _, _, opt, params = _run_case(gpu_ctx, name, fx, 1, 7)
    path = str(tmp_path / "opt.pt")
    torch.save({"optimizer": opt.state_dict(), "step": opt.global_step, "epoch": 3}, path)
    ck = torch.load(path)
    st = ck["optimizer"]["state"]
    if okr.RULE[opt.kind] == "novograd":
        assert sorted(st[0]) == ["exp_avg", "exp_avg_sq", "step"] and st[0]["exp_avg_sq"].dim() == 0 and st[0]["step"] == 7
    elif name == "sgd_nesterov":
        assert sorted(st[0]) == ["momentum_buffer"]
    elif name == "sgd_plain":
        assert st == {}
    else:
        assert sorted(st[0]) == ["acc_delta", "square_avg", "step"]
    assert bool(ck["optimizer"]["slow_state"]) == (name == "la_novograd_wd")
    fresh_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    fresh = train.DeviceOptimizer(fresh_params, ctx=gpu_ctx, **{**okr.optimizer_kwargs(okr.CASES[name]), "lr": 123.0, "weight_decay": 0.5})
    fresh.load_state_dict(ck["optimizer"], ck["step"], ck["epoch"])
    assert (fresh.lr, fresh.weight_decay) == (okr.CASES[name]["lr"], okr.CASES[name]["weight_decay"])
    assert fresh.global_step == 8 and fresh.current_epoch == 3
    got, _, _, _ = _run_case(gpu_ctx, name, fx, 8, orl.STEPS, opt=fresh, params=fresh_params)
    for s in orl.RECORD:
        if s >= 8:
            assert np.array_equal(got["p"][s].view(np.int32), want["p"][s].view(np.int32)), s
    for q in ("a", "b", "v", "slow"):
        assert (got[q] is None) == (want[q] is None) and (got[q] is None or np.array_equal(got[q].view(np.int32), want[q].view(np.int32))), q
    assert np.array_equal(got["norm"], want["norm"][7:])


def test_reference_layout_loads(gpu_ctx, fx):
    """hand-built dicts as the reference's utils.save_model leaves them in a checkpoint's ``optimizer`` entry: torch's layout, state keyed
    by parameter index, Novograd's exp_avg_sq a 0-d tensor, SGD's momentum_buffer without a step; a LookaheadNovograd's slow_state is keyed
    by id() and is ignored.  One step from the loaded state against the float64 rules."""
    import torch
    from nanosnp_amd import train
    rng = np.random.default_rng([34, 5])
    p0 = orl.split(fx["p0"])
    g = orl.split(fx["cases"]["la_novograd_wd"]["grads"][2])
    n = len(p0)
    m = [(rng.standard_normal(a.shape) * 0.1).astype(np.float32) for a in p0]
    v = (rng.random(n) * 0.1 + 0.01).astype(np.float32)
    for kind in ("LookaheadNovograd", "sgd"):
        params = [torch.nn.Parameter(_dev(a)) for a in p0]
        for p, a in zip(params, g):
            p.grad = _dev(a)
        if kind == "sgd":
            sd = {"state": {i: {"momentum_buffer": torch.from_numpy(m[i].copy())} for i in range(n)},
                  "param_groups": [{"lr": 1e-2, "momentum": 0.9, "dampening": 0, "weight_decay": 1e-4, "nesterov": True, "maximize": False,
                                    "foreach": None, "differentiable": False, "fused": None, "params": list(range(n))}]}
            opt = train.DeviceOptimizer(params, kind="sgd", momentum=0.5, ctx=gpu_ctx)
        else:
            sd = {"state": {i: {"step": 3, "exp_avg": torch.from_numpy(m[i].copy()), "exp_avg_sq": torch.tensor(float(v[i]))} for i in range(n)},
                  "slow_state": {140000000 + i: {"slow_buffer": torch.zeros(p0[i].shape)} for i in range(n)},
                  "param_groups": [{"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-4, "grad_averaging": False, "amsgrad": False,
                                    "lookahead_alpha": 0.5, "lookahead_k": 6, "lookahead_step": 3, "params": list(range(n))}]}
            opt = train.DeviceOptimizer(params, kind=kind, ctx=gpu_ctx)
        opt.load_state_dict(sd, global_step=4, current_epoch=1)
        assert opt.lr == 1e-2 and opt.weight_decay == 1e-4 and opt.global_step == 4 and opt.current_epoch == 1
        ref = okr.KindRules(p0, kind, lr=1e-2, weight_decay=1e-4, momentum=0.9, nesterov=True)
        ref.a, ref.t = [a.astype(np.float64) for a in m], 3
        if kind == "sgd":
            assert (opt.momentum, opt.nesterov) == (0.9, True) and all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(opt.momentum_buffer, m))
        else:
            assert opt.step_count == 3 and opt.lookahead_step == 3 and not opt.slow_ready
            assert np.array_equal(opt.layer_v.cpu().numpy(), v) and all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(opt.exp_avg, m))
            ref.v = v.astype(np.float64)
        opt.step(2.0)
        ref.step(g, 2.0)
        for i in range(n):
            # a and p carry the roundings of one step on top of exact loaded values: the counts of the module docstring at mult 1
            a = getattr(opt, opt.state_names[0])[i].cpu().numpy()
            x = ref.a[i] - (B1 if kind != "sgd" else 0.9) * m[i]
            assert _top(a - ref.a[i]) <= R * ((x_roundings(1) + 2) * _top(x) + 2 * _top(m[i]) + _top(ref.a[i])), (kind, i)
            assert _top(params[i].detach().cpu().numpy() - ref.p[i]) <= orl.bound(0.0, ref.p[i]) + 1e-2 * R * 40 * _top(ref.a[i]), (kind, i)


# ---- 6. through the trainer ------------------------------------------------------------------------------------------------------------------------
def test_through_the_trainer(tmp_path):
    """two passes of train_train_bins over tests/golden/train_g1.td.gz (138 rows, 14 batches of 10: a first and a real Lookahead sync per
    pass) with optimizer=DeviceOptimizer(trainer, kind="LookaheadNovograd"): the parameters move, stay finite, and the second pass's loss is
    below the first's"""
    import os
    from nanosnp_amd import train
    from tests.helpers import ROOT
    path = er.fixture_rows("train_g1", str(tmp_path))[0]
    tr = train.PileupTrainer.from_npz(os.path.join(ROOT, "nanosnp_amd", "data", "ont_pileup_weights.npz"), chunk_sites=64)
    start = [p.detach().cpu().numpy().copy() for p in tr.parameters()]
    opt = train.DeviceOptimizer(tr, kind="LookaheadNovograd", lr=1e-3)
    kw = dict(batch_size=10, dropout=0.0, max_grad_norm=20.0, seed=7)
    first = train.train_train_bins(tr, path, optimizer=opt, **kw)
    second = train.train_train_bins(tr, path, optimizer=opt, **kw)
    assert first["batches"] == second["batches"] == 14 and opt.step_count == 28 and opt.global_step == 29 and opt.slow_ready
    end = [p.detach().cpu().numpy() for p in tr.parameters()]
    assert len(end) == 24 and all(np.isfinite(a).all() for a in end) and np.isfinite(opt.layer_v.cpu().numpy()).all()
    assert all(not np.array_equal(a, b) for a, b in zip(end, start)) and bool((opt.layer_v > 0).all())
    print(f"LookaheadNovograd through train_train_bins: mean_loss {first['mean_loss']:.6f} -> {second['mean_loss']:.6f}")
    assert np.isfinite(first["mean_loss"]) and second["mean_loss"] < first["mean_loss"]
