"""HaplotypeModel forward at the model dimensions nsnp_hap_load_weights accepts (1 <= n_features <= 128, n_gt, n_zy >= 1, n_gt + n_zy <= 16)
beyond the shipped 105 / 10 + 3: the partial last feature chunk of k_hap_pack_input (F mod 16 lanes filled, the rest zero), the chunk count
ceil(F / 16) that sizes the workspace and the weight images, the 16-entry logit array of k_hap_heads.  Yardsticks: the reference module's
own outputs (tests/golden/hap_fwd_dims.npz) and the CPU oracle, which tests/test_oracle_golden.py pins against that fixture.  Tolerance:
PROB_ATOL in all three arithmetic modes (the inputs stay under 2048, where the f16x3 mode's documented bound is 1e-4 as well).

Every context sets "hap_pass_sites" 256 BEFORE it loads weights: the workspace is sized at load time (~195 KB per site of a pass)."""
import functools

import numpy as np
import pytest

from tests.helpers import HAP_DIMS_WEIGHTS, PROB_ATOL, hap_dims_cases, hap_dims_inputs, seeded_hap_weights

pytestmark = pytest.mark.gpu

PRECISIONS = [0, 2, 1]
PREC_IDS = ["fp32", "bf16x3", "f16x3"]


def _ctx(prec=0):
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    c.set_option("hap_pass_sites", 256)
    c.set_option("hap_precision", prec)
    return c


def _load(c, seed, F, n_gt, n_zy):
    ws = seeded_hap_weights(seed, F=F, n_gt=n_gt, n_zy=n_zy, **HAP_DIMS_WEIGHTS)
    c.hap_load_weights(ws, n_features=F, n_gt=n_gt, n_zy=n_zy)
    return ws


def _fwd(c, xp, xh):
    import torch
    gt, zy = c.hap_forward(torch.from_numpy(np.ascontiguousarray(xp)).cuda(), torch.from_numpy(np.ascontiguousarray(xh)).cuda())
    torch.cuda.synchronize()
    return gt.cpu().numpy(), zy.cpu().numpy()


@pytest.mark.parametrize("prec", PRECISIONS, ids=PREC_IDS)
def test_fixture_of_the_reference_module_at_every_dimension(prec):
    """hap_fwd_dims.npz, every case: probabilities within PROB_ATOL of model_dev.LSTMNetwork.predict, the same argmax"""
    for F, n_gt, n_zy, seed, xp, xh, gt_ref, zy_ref in hap_dims_cases():
        c = _ctx(prec)
        _load(c, seed, F, n_gt, n_zy)
        gt, zy = _fwd(c, xp, xh)
        c.close()
        assert gt.shape == gt_ref.shape and zy.shape == zy_ref.shape
        d = max(np.abs(gt - gt_ref).max(), np.abs(zy - zy_ref).max())
        print("F %d, classes %d + %d, hap_precision %d: max |dp| vs the reference = %.3g" % (F, n_gt, n_zy, prec, d))
        assert d < PROB_ATOL, (F, n_gt, n_zy)
        assert np.array_equal(gt.argmax(1), gt_ref.argmax(1)) and np.array_equal(zy.argmax(1), zy_ref.argmax(1)), (F, n_gt, n_zy)


SWEEP_F = [1, 2, 15, 16, 17, 31, 32, 33, 104, 105, 106, 112, 113, 127, 128]
SWEEP_CLASSES = [(10, 3), (1, 1), (15, 1), (1, 15), (13, 3)]
SWEEP_N = 300                   # two full 128-site tiles and a ragged one; two passes at "hap_pass_sites" 256


# every F with the class counts of the cycle; the three feature counts the cycle gives 1 + 1 classes - both heads are then the constant 1
# whatever the network computes - run with 10 + 3 as well, so that every F has a head whose output depends on its input
SWEEP_CASES = [(F,) + SWEEP_CLASSES[i % len(SWEEP_CLASSES)] for i, F in enumerate(SWEEP_F)]
SWEEP_CASES += [(F, 10, 3) for F, n_gt, n_zy in SWEEP_CASES if n_gt == 1 and n_zy == 1]
assert {F for F, n_gt, n_zy in SWEEP_CASES if max(n_gt, n_zy) > 1} == set(SWEEP_F)


@functools.lru_cache(maxsize=None)
def _sweep_case(F, n_gt, n_zy):
    from oracle import oracle
    seed = 700 + F + 1000 * n_gt
    ws = seeded_hap_weights(seed, F=F, n_gt=n_gt, n_zy=n_zy, **HAP_DIMS_WEIGHTS)
    xp, xh = hap_dims_inputs(seed, SWEEP_N, F)
    ogt, ozy = oracle.hap_forward(ws, xp, xh, n_gt=n_gt, n_zy=n_zy, nthreads=16)
    return seed, xp, xh, ogt, ozy


@pytest.mark.parametrize("prec", PRECISIONS, ids=PREC_IDS)
@pytest.mark.parametrize("F,n_gt,n_zy", SWEEP_CASES, ids=["F%d-%d+%d" % c for c in SWEEP_CASES])
def test_feature_count_sweep_vs_oracle(F, n_gt, n_zy, prec):
    """F around every multiple of 16 the ABI accepts, the class counts cycling through 10 + 3, 1 + 1, 15 + 1, 1 + 15, 13 + 3; N = 300"""
    seed, xp, xh, ogt, ozy = _sweep_case(F, n_gt, n_zy)
    # the yardstick's outputs differ from site to site, so a constant output cannot pass: asserted on the larger head of every case but
    # 1 + 1, where both heads are a softmax over one class (exactly 1) and the case pins the shapes and that 1 only
    if max(n_gt, n_zy) > 1:
        assert (ogt if n_gt >= n_zy else ozy).std(0).max() > 1e-3
    else:
        assert (ogt == 1).all() and (ozy == 1).all()
    c = _ctx(prec)
    _load(c, seed, F, n_gt, n_zy)
    gt, zy = _fwd(c, xp, xh)
    c.close()
    assert gt.shape == (SWEEP_N, n_gt) and zy.shape == (SWEEP_N, n_zy)
    d = max(np.abs(gt - ogt).max(), np.abs(zy - ozy).max())
    print("F %d, classes %d + %d, hap_precision %d: max |dp| vs the oracle = %.3g" % (F, n_gt, n_zy, prec, d))
    assert d < PROB_ATOL
    assert np.abs(gt.sum(1) - 1).max() < 1e-5 and np.abs(zy.sum(1) - 1).max() < 1e-5


@pytest.mark.parametrize("prec", PRECISIONS, ids=PREC_IDS)
def test_reloading_other_dimensions_leaves_nothing_behind(prec):
    """one context: F = 128, then F = 17 (two of the eight input chunks; the workspace keeps its larger size), then F = 128 with other
    weights - each result equals that of a context that never held anything else, bit for bit"""
    loads = [(128, 10, 3, 31), (17, 13, 3, 32), (128, 10, 3, 33)]
    n = 300
    c = _ctx(prec)
    for F, n_gt, n_zy, seed in loads:
        xp, xh = hap_dims_inputs(seed, n, F)
        _load(c, seed, F, n_gt, n_zy)
        got = _fwd(c, xp, xh)
        fresh = _ctx(prec)
        _load(fresh, seed, F, n_gt, n_zy)
        want = _fwd(fresh, xp, xh)
        fresh.close()
        assert want[0].std(0).max() > 1e-3
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (F, seed)
    c.close()


def test_dimensions_outside_the_accepted_range_are_refused_and_leave_the_model_alone():
    """n_features 0 and 129, n_gt 0, n_zy 0, n_gt + n_zy = 17: NSNP_ESHAPE; the context goes on with the model it holds, same bits"""
    from nanosnp_amd import _lib
    c = _ctx(0)
    F, n_gt, n_zy, seed = 33, 13, 3, 51
    ws = _load(c, seed, F, n_gt, n_zy)
    xp, xh = hap_dims_inputs(seed, 130, F)
    want = _fwd(c, xp, xh)
    assert want[0].std(0).max() > 1e-3
    for kw in (dict(n_features=0), dict(n_features=129), dict(n_gt=0), dict(n_zy=0), dict(n_gt=14, n_zy=3), dict(n_gt=1, n_zy=16)):
        args = dict(n_features=F, n_gt=n_gt, n_zy=n_zy)
        args.update(kw)
        with pytest.raises(_lib.NanoSNPError, match="unsupported model dimensions"):
            c.hap_load_weights(ws, **args)
        got = _fwd(c, xp, xh)
        assert got[0].shape == (130, n_gt) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kw
    c.close()


def test_model_class_refuses_unsupported_dimensions_at_construction():
    """nanosnp_amd.haplotype_model.LSTMNetwork(config): pileup_dim != haplotype_dim, or a dimension nsnp_hap_load_weights would refuse,
    raises when the object is made - not at the first load or forward; the ends of the range are accepted and run"""
    from nanosnp_amd import _lib
    from nanosnp_amd.haplotype_model import LSTMNetwork
    base = {"pileup_dim": 105, "haplotype_dim": 105, "pileup_length": 33, "haplotype_length": 11, "hidden_size": 256, "lstm_layers": 3,
            "gt_num_class": 10, "zy_num_class": 3, "dropout": 0.1}
    for kw in (dict(pileup_dim=104), dict(haplotype_dim=17), dict(pileup_dim=0, haplotype_dim=0), dict(pileup_dim=129, haplotype_dim=129),
               dict(gt_num_class=0), dict(zy_num_class=0), dict(gt_num_class=14), dict(gt_num_class=1, zy_num_class=16), dict(hidden_size=128),
               dict(lstm_layers=2)):
        with pytest.raises(_lib.NanoSNPError):
            LSTMNetwork({"model": dict(base, **kw)})
    import torch
    from oracle import oracle
    for F, n_gt, n_zy in ((1, 15, 1), (128, 1, 15)):
        c = _ctx(0)
        m = LSTMNetwork({"model": dict(base, pileup_dim=F, haplotype_dim=F, gt_num_class=n_gt, zy_num_class=n_zy)}, ctx=c)
        ws = seeded_hap_weights(60 + F, F=F, n_gt=n_gt, n_zy=n_zy, **HAP_DIMS_WEIGHTS)
        m.load_weight_list(ws)
        xp, xh = hap_dims_inputs(60 + F, 40, F)
        gt, zy = m.predict(torch.from_numpy(xp).cuda(), torch.from_numpy(xh).cuda())
        torch.cuda.synchronize()
        ogt, ozy = oracle.hap_forward(ws, xp, xh, n_gt=n_gt, n_zy=n_zy, nthreads=8)
        assert np.abs(gt.cpu().numpy() - ogt).max() < PROB_ATOL and np.abs(zy.cpu().numpy() - ozy).max() < PROB_ATOL
        c.close()
