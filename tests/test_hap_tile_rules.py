"""tests/hap_tile_rules.py at the numbers tests/test_gpu_hap_tile_kernels.py relies on: the schedule of a pass, the K-chunk counts per
feature count, and - for an MI355X's 256 CUs - which launches of every site count of the GPU file take the 256 x 256 kernel."""
import numpy as np
import pytest

from tests import hap_tile_rules as tr

N_CU = 256


def test_schedule_of_a_pass():
    for F in (1, 105, 128):
        l = tr.lstm_launches(F)
        assert len(l) == 83 and sum(1 for x in l if x[2] == 4) == 28 and sum(1 for x in l if x[2] == 2) == 55
        assert [sum(1 for x in l if x[0] == layer) for layer in range(3)] == [33, 33, 17]
        # layers 0 and 1: steps 0..10 with four slices; layer 2: steps 0..5
        assert [x[1] for x in l if x[0] == 0 and x[2] == 4] == list(range(11))
        assert [x[1] for x in l if x[0] == 1 and x[2] == 4] == list(range(11))
        assert [x[1] for x in l if x[0] == 2 and x[2] == 4] == list(range(6))
        assert [(x[0], x[1]) for x in l] == [(a, s) for a, n in ((0, 33), (1, 33), (2, 17)) for s in range(n)]


@pytest.mark.parametrize("F,first,want", [(1, 1, {1, 17, 32, 48}), (16, 1, {1, 17, 32, 48}), (17, 2, {2, 18, 32, 48}), (32, 2, {2, 18, 32, 48}),
                                          (33, 3, {3, 19, 32, 48}), (105, 7, {7, 23, 32, 48}), (128, 8, {8, 24, 32, 48})])
def test_chunk_counts_per_feature_count(F, first, want):
    l = tr.lstm_launches(F)
    assert {x[3] for x in l} == want
    assert l[0] == (0, 0, 4, first)                      # the first step of layer 0: the input chunks alone, h = 0
    assert {x[3] for x in l if x[0] == 0 and x[1] > 0} == {first + 16}
    assert {x[3] for x in l if x[0] > 0} == {32, 48} and [x[3] for x in l if x[1] == 0] == [first, 32, 32]
    # both kinds of launch run every chunk count: the hand-over regime splits them between the two kernels
    assert {x[3] for x in l if x[2] == 4} == want and {x[3] for x in l if x[2] == 2} == want - {first, 32}


def test_thresholds_at_256_cus():
    assert tr.tiles_all(N_CU) == 64 and tr.tiles_four(N_CU) == 32
    assert tr.takes_b3x(3969, 4, N_CU) and not tr.takes_b3x(3968, 4, N_CU)            # 32 tiles from 3,969 sites on
    assert tr.takes_b3x(8065, 2, N_CU) and not tr.takes_b3x(8064, 2, N_CU)
    assert not tr.takes_b3x(128 * 33, 4, N_CU) and not tr.takes_b3x(128 * 65, 2, N_CU)  # odd tile counts never


@pytest.mark.parametrize("n_cu", [32, 64, 128, 256, 304])
def test_thresholds_stay_consistent(n_cu):
    A, Q = tr.tiles_all(n_cu), tr.tiles_four(n_cu)
    assert A == 2 * Q and A % 2 == 0 and Q % 2 == 0
    assert tr.takes_b3x(128 * A, 2, n_cu) and not tr.takes_b3x(128 * (A - 2), 2, n_cu)
    assert tr.takes_b3x(128 * Q, 4, n_cu) and not tr.takes_b3x(128 * (Q - 2), 4, n_cu)
    assert tr.regime(128 * A, n_cu) == "all" and tr.regime(128 * Q, n_cu) == "four" and tr.regime(128 * (A - 1), n_cu) == "none"


def test_regime_of_every_site_count_of_the_gpu_file():
    """the site counts of tests/test_gpu_hap_tile_kernels.py (site_cases there, by name) at 256 CUs, pass 8,192"""
    from tests.test_gpu_hap_tile_kernels import site_cases
    cases = site_cases(N_CU)
    assert cases == {"all": (8192, ["all"]), "all_one_site_tile": (8065, ["all"]), "odd_control": (8064, ["none"]), "handover": (4096, ["four"]),
                     "handover_ragged": (4347, ["four"]), "two_passes": (8321, ["all", "none"])}
    every = tr.lstm_launches(105)
    for name, (n, regimes) in cases.items():
        sizes = tr.passes(n, 8192)
        assert [tr.regime(p, N_CU) for p in sizes] == regimes, name
        for p, r in zip(sizes, regimes):
            big = tr.big_kernel_launches(p, N_CU)
            assert len(big) == {"all": 83, "four": 28, "none": 0}[r]
            if r == "four":
                assert big == [l for l in every if l[2] == 4]
    assert tr.passes(8321, 8192) == [8192, 129] and tr.n_tiles(129) == 2 and tr.n_tiles(8065) == 64 and tr.n_tiles(4347) == 34


def test_ballast_regimes_at_256_cus():
    """fp32 / f16x3: hap_gemm.hpp's gemm_lds_ballast is non-zero for two and three workgroups per CU, zero from four on"""
    assert tr.gemm_lds_ballast(2 * N_CU, N_CU) == 14165 and tr.gemm_lds_ballast(3 * N_CU, N_CU) == 512 and tr.gemm_lds_ballast(4 * N_CU, N_CU) == 0
    assert tr.gemm_lds_ballast(1, N_CU) == 14165 and tr.gemm_lds_ballast(2 * N_CU + 1, N_CU) == 512 and tr.gemm_lds_ballast(3 * N_CU + 1, N_CU) == 0
    assert tr.ballast_sites(N_CU) == (2560, 4096, 8192)
    assert [(tr.ballast_per_cu(n, 4, N_CU), tr.ballast_per_cu(n, 2, N_CU)) for n in tr.ballast_sites(N_CU)] == [(3, 2), (0, 2), (0, 0)]
    assert (tr.ballast_per_cu(256, 4, N_CU), tr.ballast_per_cu(256, 2, N_CU)) == (2, 2)              # the pass size of the comparison run


def test_oracle_logits_are_what_its_softmaxes_see():
    """oracle.hap_forward_logits (the yardstick of the scoring comparison in the GPU file): its float64 softmax gives oracle.hap_forward's
    probabilities to fp32 rounding, and the logits lie within 1e-4 of the float64 restatement - at F = 17, 13 + 3 classes, the scaled weights"""
    from oracle import oracle
    from tests import hap_eval_rules as hr
    from tests.helpers import HAP_DIMS_WEIGHTS, hap_dims_inputs, seeded_hap_weights
    F, n_gt, n_zy = 17, 13, 3
    ws = seeded_hap_weights(5, F=F, n_gt=n_gt, n_zy=n_zy, **HAP_DIMS_WEIGHTS)
    xp, xh = hap_dims_inputs(5, 6, F)
    z = np.concatenate(oracle.hap_forward_logits(ws, xp, xh, n_gt=n_gt, n_zy=n_zy, nthreads=2), axis=1)
    gt, zy = oracle.hap_forward(ws, xp, xh, n_gt=n_gt, n_zy=n_zy, nthreads=2)
    assert z.shape == (6, 16) and z.dtype == np.float32 and z.std(0).max() > 1e-3
    for a, prob in ((z[:, :n_gt], gt), (z[:, n_gt:], zy)):
        e = np.exp(a.astype(np.float64) - a.max(1, keepdims=True))
        assert np.abs(e / e.sum(1, keepdims=True) - prob).max() <= 5e-7
    assert np.abs(z - hr.forward_logits_f64(ws, xp, xh)).max() <= 1e-4
