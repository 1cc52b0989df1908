"""nsnp_optim_step where a range is wider than a tile and where a workgroup adds more than 256 partial sums: the iterations of
optim_step.hip that tests/test_gpu_optim_step.py never reaches (its largest set is 205 workgroups at mult = 1).  Against the float64
restatement tests/optim_rules.py; the range map itself is restated there too (plan, owner, first_float_of) and compared with the
library's in tests/test_optim_rules.py, which also asserts every figure of this table:

    set        tensors (floats, in table order)                                              floats      mult  grid   five buffers
    mult2      1, 1023, 1024, 1025, FILLER 2,089,989, 2047, 2048, 2049, 3073                 2,102,279   2     1,031  42.0 MB
    mult4      1, 1023, 1024, 1025, FILLER 4,192,261, 3073, 4095, 4096, 4097, 6145           4,216,840   4     1,035  84.3 MB
    partials   307,205                                                                       307,205     1     301    6.1 MB

mult2 needs 2,058 workgroups at mult = 1, mult4 2,065 at mult = 2: both one step past the limit of 2,048.  The small tensors are, in
units of a range (2,048 / 4,096 floats): less than a tile (1, 1023), a tile (1024), one float into the second tile (1025), one float
into the LAST tile (3073, mult4), one float short of a range (2047 / 4095), a range, one float into a second workgroup (2049 / 4097), a
range and a half (3073 / 6145).  The fillers end 1,029 and 2,053 floats into their last range: a full tile, then a tile of five floats
that all but two lanes leave by the `break`.  Every grid is above 257: lane t of k_opt_update adds partial t + 256 as well (lanes
0 .. 44 of the partials set; every lane of the other two, lanes 0 .. 6 of mult2 and 0 .. 10 of mult4 a fifth one).

Bounds, in fp32 roundings of 2^-24 relative each, counted as the docstring of tests/test_gpu_optim_step.py counts them.  A partial sum:
the squares (1), (g0^2 + g1^2) + (g2^2 + g3^2) (2), mult - 1 additions of further tiles, six butterfly steps, three wave additions:
mult + 11 on a sum of non-negative terms.  The partials are added in float64 (nothing at this scale); the square root halves the count,
the conversion of the norm to fp32 adds one: N = (mult + 11) / 2 + 1.  Then as for mult = 1: the coefficient max_norm / (norm + 1e-6)
adds an addition and a division, g' = g c + wd p two more, m = (1 - beta1) g' the rounded constant and the product, v = ((1 - beta2) g') g'
is twice g' and three.

    mult   partial   norm N   coefficient   g'      m (N + 6)   v (2 N + 11)
    1      12        7        9             11      13          25
    2      13        7.5      9.5           11.5    13.5        26
    4      15        8.5      10.5          12.5    14.5        28

4 x 2^-23 = 8 roundings, which tests/test_gpu_optim_step.py grants the norm, holds the count at mult 1 and 2 and NOT at mult 4: the
norm is asserted within N roundings of its own mult here.  With moments that are not zero, beta1 m0 is rounded twice (the constant,
the product) and the sum once more:  |m - m_f64| <= 2^-24 ((N + 6) max |(1 - beta1) g'| + 2 max |beta1 m0| + max |m|), and v likewise with
2 N + 11, beta2 v0 and v; each maximum over the tensor (over the one element, for the one-hot test).  A parameter and its slow buffer move
by about lr, so those errors reach them scaled by lr / |p|: the floor alone, 4 x 2^-23 max |p|, as for mult = 1.  After TWO steps
(test_device_optimizer_two_steps) the error of the first step is carried into the second with factors below one (beta1, beta2, 1 - alpha)
and the second adds its own: twice the one-step allowances taken at the second step.

Distances measured on an MI355X: docs/rounds/r28.md."""
import numpy as np
import pytest

from tests import optim_rules as orl
from tests.test_gpu_optim_step import _args, _dev

pytestmark = pytest.mark.gpu
SETS = orl.RANGE_SETS
R = 2.0 ** -24                                               # one fp32 rounding, relative
B1, B2 = 0.9, 0.999


def norm_roundings(mult):
    return (mult + 11) / 2 + 1                               # (the module docstring counts them)


def _top(a):
    return float(np.abs(a).max())


def _allowances(mult, ref, i, p0, g, m0, v0, norm, max_norm, wd_l2):
    """the one-step allowances of tensor i (module docstring).  ref: the float64 rules AFTER the step; p0, g, m0, v0: float64 arrays of the
    tensor before it; norm: the float64 norm of the whole set; wd_l2: the weight decay where it enters the gradient (Adam), else 0"""
    n = norm_roundings(mult)
    x = g * min(1.0, max_norm / (norm + 1e-6)) + wd_l2 * p0
    return {"p": orl.bound(0.0, ref.p[i]), "slow": orl.bound(0.0, ref.slow[i]) if ref.slow is not None else None,
            "m": R * ((n + 6) * _top((1 - B1) * x) + 2 * _top(B1 * m0) + (_top(ref.m[i]) if np.any(m0) else 0.0)),
            "v": R * ((2 * n + 11) * _top((1 - B2) * x * x) + 2 * _top(B2 * v0) + (_top(ref.v[i]) if np.any(v0) else 0.0))}


def _rule_args(radam, t, lr, wd, **kw):
    """the arguments DeviceOptimizer gives step t of Adam / RAdam (train.step_scalars: tests/test_optim_rules.py checks them)"""
    from nanosnp_amd import train
    return _args(**{**train.step_scalars(radam, t, lr, B1, B2, wd), "weight_decay": wd, **kw})


def _layout(counts, off=0):
    """every tensor `off` floats behind a 16-byte boundary of a flat buffer -> (starts, floats of the buffer)"""
    starts, cur = [], 0
    for n in counts:
        cur = (cur + 3) // 4 * 4 + off
        starts.append(cur)
        cur += n
    return starts, cur + 8


def _flats(counts, packed, off=0):
    """packed: host fp32 arrays [sum(counts)], the tensors back to back (p, g, m, v, slow) -> (the flat device buffers, filled with 77.0
    around the tensors; per buffer the list of views; the bool mask of the floats that belong to a tensor)"""
    import torch
    starts, size = _layout(counts, off)
    inside = torch.zeros(size, dtype=torch.bool, device="cuda")
    for s, n in zip(starts, counts):
        inside[s:s + n] = True
    flats, lists = [], []
    for a in packed:
        flat = torch.full((size,), 77.0, dtype=torch.float32, device="cuda")
        assert flat.data_ptr() % 16 == 0 and a.dtype == np.float32 and a.size == sum(counts)
        flat[inside] = _dev(a)
        views = [flat[s:s + n] for s, n in zip(starts, counts)]
        assert all(v.data_ptr() % 16 == 4 * off for v in views)
        flats.append(flat); lists.append(views)
    return flats, lists, inside


def _step(ctx, lists, args):
    import torch
    norm = torch.full((), -5.0, dtype=torch.float32, device="cuda")
    ctx.optim_step(tuple(lists), args, grad_norm_out=norm)
    return norm


def _cut(flat, counts):
    """a packed host array -> the tensors, float64"""
    out, o = [], 0
    for n in counts:
        out.append(np.asarray(flat[o:o + n], np.float64))
        o += n
    return out


def _bits(t):
    import torch
    return t.view(torch.int32)


_STATE = {}


def _state(name):
    """the random state of a set, drawn once and shared (nobody writes to it): p, g, and non-trivial m, v (>= 0), slow, packed"""
    if name not in _STATE:
        n = sum(SETS[name]["counts"])
        rng = np.random.default_rng([28, n])
        draw = lambda scale: (rng.standard_normal(n, dtype=np.float32) * np.float32(scale))
        p = draw(0.1)
        _STATE[name] = [p, draw(0.05), draw(0.01), rng.random(n, dtype=np.float32) * np.float32(1e-4), p + draw(0.01)]
    return _STATE[name]


# ---- 1. every float is visited exactly once ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_every_float_is_visited_once(gpu_ctx, name):
    """parameters and gradients 1.0, moments 0, no weight decay, the first sync, clipping at 1: the sum of squares is an integer below
    2^24 - every partial and the total are exact, the norm is the correctly rounded root - and every float of p, m, v and slow ends with
    the same bits.  A float visited twice or never differs by the whole step."""
    import torch
    counts, mult = SETS[name]["counts"], SETS[name]["mult"]
    total = sum(counts)
    assert total < 1 << 24
    ones, zeros = np.ones(total, np.float32), np.zeros(total, np.float32)
    flats, lists, inside = _flats(counts, [ones, ones, zeros, zeros, zeros])
    norm = _step(gpu_ctx, lists, _rule_args(False, 1, 1e-2, 0.0, sync=2, max_norm=1.0))
    torch.cuda.synchronize()
    assert norm.cpu().numpy().tobytes() == np.float32(np.sqrt(np.float64(total))).tobytes()
    ref = orl.Rules([np.ones(n) for n in counts], "LookaheadAdam", lr=1e-2, k=1)
    want_norm = ref.step([np.ones(n) for n in counts], 1.0)
    allow = _allowances(mult, ref, 0, np.ones(1), np.ones(1), np.zeros(1), np.zeros(1), want_norm, 1.0, 0.0)
    ratios = {}
    for what, flat, want in (("p", flats[0], ref.p), ("m", flats[2], ref.m), ("v", flats[3], ref.v), ("slow", flats[4], ref.slow)):
        values = torch.unique(_bits(flat[inside])).cpu().numpy().view(np.float32)
        assert values.size == 1, (name, what, values[:8])
        assert all(np.all(w == w[0]) and w[0] == want[0][0] for w in want)           # (the rules give one value too)
        ratios[what] = abs(float(values[0]) - want[0][0]) / allow[what]
        assert ratios[what] <= 1.0, (name, what, float(values[0]), want[0][0], allow[what])
        assert bool((flat[~inside] == 77.0).all()), (name, what)
    assert bool((flats[1] == torch.where(inside, 1.0, 77.0)).all())                  # the gradients are only read
    print(f"{name}: visited once; distance / bound " + " ".join(f"{q} {r:.3f}" for q, r in ratios.items()))


# ---- 2. a one-hot gradient -------------------------------------------------------------------------------------------------------------------
def _placements(name):
    """[(what, tensor, offset)] of the single 3.0"""
    s = SETS[name]
    counts, mult, f = s["counts"], s["mult"], s["filler"]
    span, grid = orl.TILE * mult, orl.plan(counts)[1][-1]
    out = [("the first float of the set", 0, 0), ("the last float of the set", len(counts) - 1, counts[-1] - 1),
           ("the last float of a range", f, 8 * span - 1), ("the first float of the next range", f, 8 * span)]
    if mult > 1:
        out += [("the first float of tile 1 of a range", f, 7 * span + orl.TILE), (f"the first float of tile {mult - 1} of a range", f, 7 * span + (mult - 1) * orl.TILE),
                ("the last float of the filler", f, counts[f] - 1)]
    for wg in (255, 256, 257, grid - 1):
        t, o = orl.first_float_of(counts, wg)
        o += min(517, counts[t] - 1 - o)                     # (inside the workgroup's range, off a lane's first float where there is room)
        assert orl.owner(counts, t, o)[0] == wg
        out.append((f"a float of workgroup {wg}", t, o))
    seen, uniq = set(), []
    for what, t, o in out:
        if (t, o) not in seen:
            seen.add((t, o)); uniq.append((what, t, o))
    return uniq


@pytest.mark.parametrize("name", list(SETS))
def test_one_hot_gradient(gpu_ctx, name):
    """every gradient 0 but a single 3.0: the norm is exactly 3, the one element moves as the rules say (clipped at 1: g' = 3 / (3 + 1e-6)),
    every other parameter keeps its bits and its moments stay exactly 0.  The parameters lie in 0.5 <= |p| < 1.5, so the floor of one
    element's allowance, 4 x 2^-23 |p|, holds the relative errors of a move of lr = 0.01 as it does for a whole tensor."""
    import torch
    counts, mult = SETS[name]["counts"], SETS[name]["mult"]
    total = sum(counts)
    rng = np.random.default_rng([2, total])
    p0 = (rng.uniform(0.5, 1.5, total) * rng.choice([-1.0, 1.0], total)).astype(np.float32)
    zeros = np.zeros(total, np.float32)
    (p, g, m, v), lists, inside = _flats(counts, [p0, zeros, zeros, zeros])
    p_init, m_init = p.clone(), m.clone()
    starts, _ = _layout(counts)
    args = _rule_args(False, 1, 1e-2, 0.0, sync=0, max_norm=1.0)
    places = _placements(name)
    assert len(places) >= 7 and {orl.owner(counts, t, o)[0] for _, t, o in places} >= {0, 255, 256, 257, SETS[name]["grid"] - 1}
    assert mult == 1 or {orl.owner(counts, t, o)[1] for _, t, o in places} >= {0, 1, mult - 1}
    worst = dict(p=0.0, m=0.0, v=0.0)
    for what, t, o in places:
        at = starts[t] + o
        p.copy_(p_init); m.copy_(m_init); v.copy_(m_init)
        g[at] = 3.0
        norm = _step(gpu_ctx, lists, args)
        got = [float(norm)] + [float(q[at]) for q in (p, m, v)]
        moved = [torch.nonzero(_bits(p) != _bits(p_init)).view(-1).tolist(), torch.nonzero((m != 0) & inside).view(-1).tolist(),
                 torch.nonzero((v != 0) & inside).view(-1).tolist()]
        g[at] = 0.0
        assert got[0] == 3.0, (name, what, got[0])
        assert moved == [[at], [at], [at]], (name, what, at, [x[:6] for x in moved])
        assert bool((m[~inside] == 77.0).all()) and bool((v[~inside] == 77.0).all()), (name, what)
        x0 = np.array([np.float64(p0[sum(counts[:t]) + o])])
        ref = orl.Rules([x0], "Adam", lr=1e-2)
        assert ref.step([np.array([3.0])], 1.0) == 3.0
        allow = _allowances(mult, ref, 0, x0, np.array([3.0]), np.zeros(1), np.zeros(1), 3.0, 1.0, 0.0)
        for q, value, want in (("p", got[1], ref.p[0][0]), ("m", got[2], ref.m[0][0]), ("v", got[3], ref.v[0][0])):
            worst[q] = max(worst[q], abs(value - want) / allow[q])
            assert abs(value - want) <= allow[q], (name, what, q, value, want, allow[q])
        assert abs(got[1] - float(x0[0])) > 0.009                                    # (it did move, by about lr)
    print(f"{name}: {len(places)} placements; worst distance / bound " + " ".join(f"{q} {r:.3f}" for q, r in worst.items()))


# ---- 3. float64 parity on random values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", list(SETS))
def test_random_values_against_float64(gpu_ctx, name, form):
    """one clipped step with weight decay and a Lookahead sync from non-trivial moments: step 3 of LookaheadAdam (form 0, the decay enters the
    gradient) and of LookaheadRadam (form 1 below N_sma 5, wd_mode 2: the decay shrinks the parameter)"""
    import torch
    counts, mult = SETS[name]["counts"], SETS[name]["mult"]
    host = _state(name)
    kind, radam, lr, wd = ("LookaheadAdam", False, 1e-3, 1e-4) if form == 0 else ("LookaheadRadam", True, 1e-3, 1e-4)
    args = _rule_args(radam, 3, lr, wd, sync=1, max_norm=1.0, alpha=0.5)
    assert (args.form, args.wd_mode) == ((0, 1) if form == 0 else (1, 2))
    flats, lists, inside = _flats(counts, host)
    norm = _step(gpu_ctx, lists, args)
    torch.cuda.synchronize()
    p0, g, m0, v0, s0 = (_cut(a, counts) for a in host)
    ref = orl.Rules(p0, kind, lr=lr, weight_decay=wd, alpha=0.5, k=1)
    ref.m, ref.v, ref.slow, ref.t = list(m0), list(v0), list(s0), 2
    want_norm = ref.step(g, 1.0)
    assert ref.t == 3 and want_norm > 10.0                   # clipped hard: a wrong total moves every g'
    assert min(_top(a) for a in p0) >= 0.01                  # (no tensor so small that a move of about lr outweighs its own rounding)
    rel = abs(float(norm) / want_norm - 1.0)
    worst = dict(p=0.0, m=0.0, v=0.0, slow=0.0)
    got = {q: [t.cpu().numpy() for t in lists[k]] for q, k in (("p", 0), ("m", 2), ("v", 3), ("slow", 4))}
    for i in range(len(counts)):
        allow = _allowances(mult, ref, i, p0[i], g[i], m0[i], v0[i], want_norm, 1.0, 0.0 if radam else wd)
        for q, want in (("p", ref.p), ("m", ref.m), ("v", ref.v), ("slow", ref.slow)):
            d = _top(got[q][i] - want[i])
            worst[q] = max(worst[q], d / allow[q])
            assert np.isfinite(got[q][i]).all() and d <= allow[q], (name, form, q, i, d, allow[q])
    print(f"{name} form {form}: norm rel {rel:.2e} / bound {norm_roundings(mult) * R:.2e} = {rel / (norm_roundings(mult) * R):.3f}; "
          "worst distance / bound " + " ".join(f"{q} {r:.3f}" for q, r in worst.items()))
    assert rel <= norm_roundings(mult) * R, (name, form, rel)
    assert np.array_equal(flats[1].cpu().numpy()[inside.cpu().numpy()], host[1])                 # the gradients are bit-unchanged
    for flat in flats:
        assert bool((flat[~inside] == 77.0).all())


# ---- 4. views give the same bits -------------------------------------------------------------------------------------------------------------
def _three_steps(ctx, lists):
    """no sync, the first sync, a sync - with the norm out each time -> the three norms (device scalars)"""
    return [_step(ctx, lists, _args(sync=sync, max_norm=1.0)) for sync in (0, 2, 1)]


def test_views_off_a_16_byte_boundary_give_the_same_bits(gpu_ctx):
    """the mult2 set as views 1, 2 and 3 floats behind a 16-byte boundary: the 4-byte accesses of every tile of a range give the bits of
    the 16-byte ones, and nothing outside the views is written"""
    import torch
    counts = SETS["mult2"]["counts"]
    host = _state("mult2")
    _, want, _ = _flats(counts, host)
    want_norms = _three_steps(gpu_ctx, want)
    assert not torch.equal(want[0][4], _dev(host[0][counts[0] + counts[1] + counts[2] + counts[3]:][:counts[4]]))         # p moved
    for off in (1, 2, 3):
        flats, lists, inside = _flats(counts, host, off)
        norms = _three_steps(gpu_ctx, lists)
        assert [float(a) for a in norms] == [float(b) for b in want_norms], off
        for k, (ts_got, ts_want) in enumerate(zip(lists, want)):
            for i, (a, b) in enumerate(zip(ts_got, ts_want)):
                assert torch.equal(_bits(a), _bits(b)), (off, k, i)
        for flat in flats:
            assert bool((flat[~inside] == 77.0).all()), off


# ---- 5. a non-finite gradient reaches the returned norm ------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_gradient_reaches_the_norm(gpu_ctx, value):
    """one NaN / +Inf among the five floats of the LAST workgroup (partial 300: lane 44's second trip): the norm a training loop gets back is
    NaN / +Inf.  What the step then makes of the parameters is not asserted."""
    counts = SETS["partials"]["counts"]
    host = [a.copy() for a in _state("partials")]
    assert orl.owner(counts, 0, counts[0] - 3) == (300, 0)
    host[1][counts[0] - 3] = value
    _, lists, _ = _flats(counts, host)
    norm = float(_step(gpu_ctx, lists, _args(sync=0, max_norm=1.0)))
    assert np.isnan(norm) if np.isnan(value) else norm == float("inf"), norm


# ---- 6. DeviceOptimizer over the mult = 4 set ------------------------------------------------------------------------------------------------
def test_device_optimizer_two_steps(gpu_ctx):
    """plain device tensors of the mult4 set through the binding, LookaheadAdam with k = 1: the first sync (step 1), a real one (step 2).
    After step 2 within TWICE the one-step allowances taken at step 2 (module docstring)."""
    import torch
    from nanosnp_amd import train
    counts, mult = SETS["mult4"]["counts"], SETS["mult4"]["mult"]
    host = _state("mult4")
    p0, g = _cut(host[0], counts), _cut(host[1], counts)
    params = [torch.nn.Parameter(_dev(a.astype(np.float32))) for a in p0]
    for p, a in zip(params, g):
        p.grad = _dev(a.astype(np.float32))
    opt = train.DeviceOptimizer(params, kind="LookaheadAdam", lr=1e-3, weight_decay=1e-4, k=1, ctx=gpu_ctx)
    assert opt.ctx.optim_scratch_floats(counts) == SETS["mult4"]["grid"]
    norms = [opt.step(1.0), opt.step(1.0)]
    torch.cuda.synchronize()
    ref = orl.Rules(p0, "LookaheadAdam", lr=1e-3, weight_decay=1e-4, k=1)
    want_norm = ref.step(g, 1.0)
    p1, m1, v1 = list(ref.p), list(ref.m), list(ref.v)
    assert ref.step(g, 1.0) == want_norm and want_norm > 10.0
    for n in norms:
        assert abs(float(n) / want_norm - 1.0) <= norm_roundings(mult) * R
    worst = dict(p=0.0, m=0.0, v=0.0, slow=0.0)
    for i in range(len(counts)):
        allow = _allowances(mult, ref, i, p1[i], g[i], m1[i], v1[i], want_norm, 1.0, 1e-4)
        for q, got, want in (("p", params[i], ref.p[i]), ("m", opt.exp_avg[i], ref.m[i]), ("v", opt.exp_avg_sq[i], ref.v[i]), ("slow", opt.slow[i], ref.slow[i])):
            d = _top(got.detach().cpu().numpy() - want)
            worst[q] = max(worst[q], d / (2 * allow[q]))
            assert d <= 2 * allow[q], (i, q, d, allow[q])
        assert torch.equal(params[i].grad, _dev(g[i].astype(np.float32))), i
    assert opt.step_count == 2 and opt.slow_ready
    print("mult4, two steps: worst distance / (2 x one-step bound) " + " ".join(f"{q} {r:.3f}" for q, r in worst.items()))
