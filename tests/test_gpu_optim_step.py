"""The fused optimiser step on the device (nsnp_optim_step, nanosnp_amd.train.DeviceOptimizer) against the float64 restatement
tests/optim_rules.py, on the cases the reference's own optimisers ran (tests/golden/pileup_optim.npz).

Parity bound, per case, recorded step and tensor: max |p_dev - p_f64| <= 4 x max(ref_abs_max, 2^-23 max |p|) - ref_abs_max is the reference's
OWN fp32 distance from float64 recorded in the fixture, the factor is the one tests/test_gpu_train.py grants, the floor is one rounding of a
stored parameter.  exp_avg, exp_avg_sq and the slow buffers: the same rule on their own magnitudes and their own recorded distances.  Norms:
relative to the recorded norm, 4 x max(the reference's own relative distance, 2^-23).

Where there is no recorded reference (64 one-element tensors, the 24 real shapes: ONE step from zero moments) the bounds are counted in fp32
roundings of 2^-24 relative each.  The norm is asserted within 4 x 2^-23 = 8 roundings; the clip coefficient max_norm / (norm + 1e-6) adds an
addition and a division: 10.  g' = g c + wd p: 12.  m = (1 - beta1) g' with the rounded constant: 14 roundings = 7 x 2^-23 -> M_ULPS 8.
v = ((1 - beta2) g') g': 2 x 12 + 3 = 27 roundings = 13.5 x 2^-23 -> V_ULPS 16.  A parameter moves by about lr, so those relative errors reach
it scaled by lr / |p| and its own rounding dominates: the floor alone, 4 x 2^-23 max |p|; the slow buffer is a copy of it.  All of them are
taken against the largest magnitude of the tensor.

The tensor counts are the ones that can break the range map: 1, 3, 7, 21 (partial 16-byte accesses), 1023 / 1024 / 1025 (one tile short,
exact, one over: a second workgroup), a 2-D tensor; 64 tensors (the table's limit); views at 1, 2, 3 floats off a 16-byte boundary.

Distances measured on an MI355X: docs/rounds/r27.md."""
import ctypes as C

import numpy as np
import pytest

from tests import optim_rules as orl

pytestmark = pytest.mark.gpu
M_ULPS, V_ULPS = 8, 16                                       # (the module docstring counts them)


def _one_step_bounds(ref, i):
    top = lambda a: float(np.abs(a).max())
    return {"p": orl.bound(0.0, ref.p[i]), "slow": orl.bound(0.0, ref.slow[i]), "m": M_ULPS * orl.ULP * top(ref.m[i]), "v": V_ULPS * orl.ULP * top(ref.v[i])}


@pytest.fixture(scope="module")
def fx():
    return orl.load_fixture()


@pytest.fixture(scope="module")
def f64(fx):
    """the float64 trajectories, computed once and shared"""
    return {name: orl.run(name, fx["p0"], c["grads"]) for name, c in fx["cases"].items()}


@pytest.fixture(scope="module")
def ctx():
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_case(ctx, name, fx):
    """the 14 steps of a case through DeviceOptimizer -> (dict as optim_rules.run returns it, the gradient tensors, their source)"""
    import torch
    from nanosnp_amd import train
    cfg, c = orl.CASES[name], fx["cases"][name]
    params = [torch.nn.Parameter(_dev(a)) for a in orl.split(fx["p0"])]
    opt = train.DeviceOptimizer(params, kind=cfg["kind"], lr=cfg["lr"], weight_decay=cfg["weight_decay"], alpha=cfg["alpha"], k=cfg["k"], ctx=ctx)
    gdev = _dev(c["grads"])                                             # [STEPS, TOTAL]: every step's gradients are views of one row
    out, norms = dict(p={}), []
    for s in range(1, orl.STEPS + 1):
        o = 0
        for p, n in zip(params, orl.SIZES):
            p.grad = gdev[s - 1, o:o + n].view(p.shape)
            o += n
        norms.append(opt.step(cfg["max_norm"]))
        if s in orl.RECORD:
            out["p"][s] = orl.join([p.detach().cpu().numpy() for p in params])
    torch.cuda.synchronize()
    out["norm"] = np.array([float(n) for n in norms])
    out["m"], out["v"] = orl.join([t.cpu().numpy() for t in opt.exp_avg]), orl.join([t.cpu().numpy() for t in opt.exp_avg_sq])
    out["slow"] = orl.join([t.cpu().numpy() for t in opt.slow]) if opt.slow is not None else None
    assert opt.global_step == 1 + orl.STEPS and opt.step_count == orl.STEPS
    return out, gdev, c["grads"]


@pytest.mark.parametrize("name", list(orl.CASES))
def test_fixture_parity(ctx, fx, f64, name):
    c, want = fx["cases"][name], f64[name]
    got, gdev, gsrc = _run_case(ctx, name, fx)
    worst = {}
    for s in orl.RECORD:
        for i, (a, b) in enumerate(zip(orl.split(got["p"][s]), orl.split(want["p"][s]))):
            d, bd = float(np.abs(a - b).max()), orl.bound(c["ref_abs_max"]["p"], b)
            worst["p"] = max(worst.get("p", 0.0), d / bd)
            assert np.isfinite(a).all() and d <= bd, (name, "p", s, i, d, bd)
    for q in ("m", "v", "slow"):
        assert (got[q] is None) == (want[q] is None)
        if want[q] is not None:
            for i, (a, b) in enumerate(zip(orl.split(got[q]), orl.split(want[q]))):
                d, bd = float(np.abs(a - b).max()), orl.bound(c["ref_abs_max"][q], b)
                worst[q] = max(worst.get(q, 0.0), d / bd)
                assert np.isfinite(a).all() and d <= bd, (name, q, i, d, bd)
    rel = float(np.abs(got["norm"] / c["norm"].astype(np.float64) - 1.0).max())
    nb = orl.FACTOR * max(c["ref_norm_rel"], orl.ULP)
    print(f"{name}: worst distance / bound " + " ".join(f"{q} {w:.3f}" for q, w in worst.items()) + f"; norm rel {rel:.2e} (bound {nb:.2e}); "
          f"max |p_dev - p_f64| {max(np.abs(got['p'][s] - want['p'][s]).max() for s in orl.RECORD):.2e}, ref_abs_max {c['ref_abs_max']['p']:.2e}")
    assert rel <= nb, (name, rel, nb)
    assert np.array_equal(gdev.cpu().numpy(), gsrc)                     # the gradient buffers are bit-unchanged


def test_same_run_same_bits(ctx, fx):
    a, _, _ = _run_case(ctx, "la_adam_wd", fx)
    b, _, _ = _run_case(ctx, "la_adam_wd", fx)
    for s in orl.RECORD:
        assert np.array_equal(a["p"][s], b["p"][s])
    assert all(np.array_equal(a[q], b[q]) for q in ("m", "v", "slow", "norm"))


def _args(**kw):
    from nanosnp_amd import _lib
    a = _lib.OptimArgs()
    vals = dict(max_norm=2.0, weight_decay=1e-4, decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8, a=1e-2, b=1.5, alpha=0.5, wd_mode=1, form=0, sync=0)
    vals.update(kw)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def _state(fx, case="la_adam_wd", seed=3):
    """five lists of host tensors: p, g, and non-trivial m, v (>= 0), slow"""
    rng = np.random.default_rng(seed)
    p = orl.split(fx["p0"])
    g = orl.split(fx["cases"][case]["grads"][0])
    m = [(rng.standard_normal(a.shape) * 0.01).astype(np.float32) for a in p]
    v = [(rng.random(a.shape) * 1e-4).astype(np.float32) for a in p]
    slow = [(a + rng.standard_normal(a.shape).astype(np.float32) * 0.01).astype(np.float32) for a in p]
    return [p, g, m, v, slow]


def _three_steps(ctx, lists):
    """no sync, the first sync, a sync - with the norm out each time -> every tensor's bytes and the three norms"""
    import torch
    norms = []
    for sync in (0, 2, 1):
        n = torch.zeros((), dtype=torch.float32, device="cuda")
        ctx.optim_step(tuple(lists), _args(sync=sync), grad_norm_out=n)
        norms.append(n)
    torch.cuda.synchronize()
    return [[t.cpu().numpy().copy() for t in ts] for ts in lists], [float(n) for n in norms]


def test_views_off_a_16_byte_boundary_give_the_same_bits(ctx, fx):
    import torch
    host = _state(fx)
    want, want_norms = _three_steps(ctx, [[_dev(a) for a in ts] for ts in host])
    assert not np.array_equal(want[0][4], host[0][4]) and np.array_equal(want[1][4], host[1][4])         # p moved, g did not
    for off in (1, 2, 3):
        lists, flats = [], []
        for ts in host:
            starts, cur = [], 0
            for a in ts:
                cur = (cur + 3) // 4 * 4 + off                       # `off` floats behind a 16-byte boundary of the flat buffer
                starts.append(cur)
                cur += a.size
            flat = torch.full((cur + 8,), 77.0, dtype=torch.float32, device="cuda")
            assert flat.data_ptr() % 16 == 0
            views = [flat[o:o + a.size].view(a.shape) for o, a in zip(starts, ts)]
            for vw, a in zip(views, ts):
                vw.copy_(torch.from_numpy(a))
                assert vw.data_ptr() % 16 == 4 * off
            lists.append(views); flats.append((flat, starts, [a.size for a in ts]))
        got, norms = _three_steps(ctx, lists)
        assert norms == want_norms, off
        for ts_got, ts_want in zip(got, want):
            for i, (a, b) in enumerate(zip(ts_got, ts_want)):
                assert np.array_equal(a, b), (off, i)
        for flat, starts, sizes in flats:                            # and nothing between or behind the views was written
            keep = np.ones(flat.numel(), bool)
            for o, n in zip(starts, sizes):
                keep[o:o + n] = False
            assert (flat.cpu().numpy()[keep] == 77.0).all(), off


def test_64_tensors_of_one_element(ctx):
    import torch
    from nanosnp_amd import _lib, train
    rng = np.random.default_rng(64)
    draw = lambda: (rng.uniform(0.5, 1.5, 1) * rng.choice([-1.0, 1.0])).astype(np.float32)     # every tensor is its own largest magnitude: none near 0
    p0, g = [draw() for _ in range(64)], [draw() for _ in range(64)]
    params = [torch.nn.Parameter(_dev(a)) for a in p0]
    for p, a in zip(params, g):
        p.grad = _dev(a)
    opt = train.DeviceOptimizer(params, kind="LookaheadAdam", lr=1e-2, k=1, ctx=ctx)
    norm = opt.step(1.0)
    ref = orl.Rules(p0, "LookaheadAdam", lr=1e-2, k=1)
    want_norm = ref.step(g, 1.0)
    assert want_norm > 1.0 and abs(float(norm) / want_norm - 1.0) <= orl.FACTOR * orl.ULP
    for i in range(64):
        bd = _one_step_bounds(ref, i)
        for what, got, want in (("p", params[i], ref.p[i]), ("m", opt.exp_avg[i], ref.m[i]), ("v", opt.exp_avg_sq[i], ref.v[i]),
                                ("slow", opt.slow[i], ref.slow[i])):
            assert np.abs(got.detach().cpu().numpy() - want).max() <= bd[what], (i, what)
    extra = torch.nn.Parameter(_dev(p0[0]))
    extra.grad = _dev(g[0])
    with pytest.raises(_lib.NanoSNPError, match="1..64 tensors"):
        train.DeviceOptimizer(params + [extra], ctx=ctx).step()


def test_zero_gradients(ctx, fx):
    """norm 0, coefficient min(1, max_norm / 1e-6) = 1, moments stay 0 and 0 / (0 + eps) moves nothing"""
    import torch
    from nanosnp_amd import train
    params = [torch.nn.Parameter(_dev(a)) for a in orl.split(fx["p0"])]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = train.DeviceOptimizer(params, kind="Adam", ctx=ctx)
    norm = opt.step(20.0)
    assert float(norm) == 0.0
    for p, a, m, v in zip(params, orl.split(fx["p0"]), opt.exp_avg, opt.exp_avg_sq):
        assert np.array_equal(p.detach().cpu().numpy(), a) and not bool(m.any()) and not bool(v.any())


def test_norm_without_clipping_and_no_norm_at_all(ctx, fx):
    import torch
    host = _state(fx)
    runs = []
    for max_norm, with_norm in ((1e30, True), (0.0, True), (-1.0, True), (-1.0, False)):
        lists = [[_dev(a) for a in ts] for ts in host]
        n = torch.full((), -5.0, dtype=torch.float32, device="cuda") if with_norm else None
        ctx.optim_step(tuple(lists), _args(max_norm=max_norm, sync=1), grad_norm_out=n)          # (scratch made by the binding only when needed)
        torch.cuda.synchronize()
        runs.append(([t.cpu().numpy() for ts in lists for t in ts], None if n is None else float(n)))
    want = float(np.sqrt(sum((a.astype(np.float64) ** 2).sum() for a in host[1])))
    assert want > 2.0                                                 # (max_norm 2 would have clipped)
    for tensors, norm in runs:
        assert norm is None or abs(norm / want - 1.0) <= orl.FACTOR * orl.ULP
        assert all(np.array_equal(a, b) for a, b in zip(tensors, runs[0][0]))
    assert runs[1][1] == runs[0][1] == runs[2][1]
    clipped = [[_dev(a) for a in ts] for ts in host]
    ctx.optim_step(tuple(clipped), _args(sync=1))
    assert not np.array_equal(clipped[0][4].cpu().numpy(), runs[0][0][4])                        # and clipping at 2 does change the step


def test_refusals_change_nothing(ctx, fx):
    import torch
    from nanosnp_amd import _lib
    host = _state(fx)
    lists = [[_dev(a) for a in ts] for ts in host]
    n = len(host[0])
    ot = ctx.optim_tensors(*lists)
    scratch = torch.zeros(ot.scratch_floats, dtype=torch.float32, device="cuda")
    norm = torch.full((), -5.0, dtype=torch.float32, device="cuda")
    lib, h, s = ctx.lib, ctx.handle, _lib._stream_ptr()
    sp, np_ = C.c_void_p(scratch.data_ptr()), C.c_void_p(norm.data_ptr())

    def call(ctx_=h, n_=n, p=ot.params, g=ot.grads, m=ot.exp_avg, v=ot.exp_avg_sq, sl=ot.slow, cnt=ot.counts, args=_args(sync=1), scr=sp):
        return lib.nsnp_optim_step(ctx_, n_, p, g, m, v, sl, cnt, None if args is None else C.byref(args), scr, np_, s)
    hole = (C.c_void_p * n)(*[None if i == 5 else t.data_ptr() for i, t in enumerate(lists[2])])
    odd = (C.c_void_p * n)(*[t.data_ptr() + (2 if i == 3 else 0) for i, t in enumerate(lists[0])])
    zero = (C.c_int64 * n)(*[0 if i == 6 else a.size for i, a in enumerate(host[0])])
    big = (C.c_void_p * 65)(*([lists[0][0].data_ptr()] * 65))
    big_n = (C.c_int64 * 65)(*([1] * 65))
    assert call(ctx_=None) == -1 and call(p=None) == -1 and call(g=None) == -1 and call(m=None) == -1 and call(v=None) == -1
    assert call(sl=None) == -1 and call(cnt=None) == -1 and call(args=None) == -1 and call(scr=None) == -1
    assert call(m=hole) == -1 and call(p=odd) == -1 and call(cnt=zero) == -1 and call(n_=0) == -1
    assert call(n_=65, p=big, g=big, m=big, v=big, sl=big, cnt=big_n) == -1
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(alpha=1.5), dict(alpha=-0.1), dict(form=2),
                dict(wd_mode=3), dict(sync=3)):
        assert call(args=_args(**{"sync": 1, **bad})) == -1, bad
    torch.cuda.synchronize()
    for ts, hs in zip(lists, host):
        assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(ts, hs))
    assert float(norm) == -5.0 and not bool(scratch.any())
    assert call() == 0                                                              # (and the same arguments do run)
    torch.cuda.synchronize()
    assert float(norm) > 0 and not np.array_equal(lists[0][4].cpu().numpy(), host[0][4])
    # the binding's own checks
    good = [[_dev(a) for a in ts] for ts in host]
    for k, wrong in ((1, good[1][4].double()), (2, good[2][4][:-1]), (3, good[3][4].cpu()), (4, good[4][7].t())):
        broken = [list(ts) for ts in good]
        broken[k][7 if k == 4 else 4] = wrong
        with pytest.raises(_lib.NanoSNPError):
            ctx.optim_tensors(*broken)
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_step(tuple(good[:4]), _args(sync=1))                               # a sync without slow buffers
    with pytest.raises(_lib.NanoSNPError):
        ctx.optim_step(tuple(good), _args(), scratch=torch.zeros(2, dtype=torch.float32, device="cuda"))


def test_real_shapes_one_step(ctx):
    """the 24 tensors of the PileupModel (198,040 floats, 205 workgroups): one clipped Adam step with weight decay and the first
    Lookahead sync (k = 1), against float64"""
    import torch
    from nanosnp_amd import _lib, train
    rng = np.random.default_rng(24)
    p0 = [(rng.standard_normal(s) * 0.1).astype(np.float32) for s in _lib.Context.TRAIN_SHAPES]
    g = [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in _lib.Context.TRAIN_SHAPES]
    params = [torch.nn.Parameter(_dev(a)) for a in p0]
    for p, a in zip(params, g):
        p.grad = _dev(a)
    opt = train.DeviceOptimizer(params, kind="LookaheadAdam", lr=1e-3, weight_decay=1e-4, k=1, ctx=ctx)
    norm = opt.step(20.0)
    ref = orl.Rules(p0, "LookaheadAdam", lr=1e-3, weight_decay=1e-4, k=1)
    want_norm = ref.step(g, 20.0)
    assert want_norm > 20.0 and abs(float(norm) / want_norm - 1.0) <= orl.FACTOR * orl.ULP
    for i in range(24):
        bd = _one_step_bounds(ref, i)
        for what, got, want in (("p", params[i], ref.p[i]), ("m", opt.exp_avg[i], ref.m[i]), ("v", opt.exp_avg_sq[i], ref.v[i]),
                                ("slow", opt.slow[i], ref.slow[i])):
            assert np.abs(got.detach().cpu().numpy() - want).max() <= bd[what], (i, what)
        assert np.array_equal(params[i].grad.cpu().numpy(), g[i]), i
