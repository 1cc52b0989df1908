"""The launch schedule of one HaplotypeModel pass and the rule by which a step launch of the bf16x3 arithmetic takes the 256 x 256 kernel
k_hap_lstm_b3x instead of k_hap_gemm<MODE_LSTM, 2>, restated in plain Python.  Test infrastructure only: the product never imports it.

    lstm_launches(F)      the 83 (layer, step, nz, nk) of hap_forward_t: nz slices (encoder x direction), nk = nk0 + nk1 K chunks of 16
    takes_b3x             the predicate of launch_hap_gemm
    tiles_four, tiles_all the smallest even tile counts at which the four-slice / the two-slice launches take the big kernel
    regime                which of the 83 launches of a pass take it: "all", "four" (exactly the four-slice ones) or "none"
    ballast_per_cu        fp32 / f16x3: the workgroups per CU the LDS ballast of k_hap_gemm holds a step launch to (0: no ballast)
"""
from __future__ import annotations

TS = 128                    # sites per tile (hap_gemm.hpp: TS)
BK = 16                     # K chunk (hap_gemm.hpp: BK)
H = 256                     # hidden size: 4 H / 128 = 8 row tiles per LSTM launch, H / 16 = 16 chunks of h
N_RT = 4 * H // 128
LP, LH = 33, 11             # steps of the pileup / the haplotype encoder (hap_forward.hip: Lp, Lh)


def n_tiles(n_sites):
    return -(-int(n_sites) // TS)


def lstm_launches(F):
    """hap_forward.hip, hap_forward_t: layers 0 and 1 run Lp = 33 steps, layer 2 runs Lp / 2 + 1 = 17; the haplotype encoder (Lh = 11, then
    6) rides along as two more slices while it has steps left.  Layer 0 reads ceil(F / 16) input chunks, the others the 2 H / 16 = 32 chunks
    [h_fwd ; h_bwd] of the layer below; every step but the first adds the H / 16 = 16 chunks of h_{t-1}."""
    nk_in0 = -(-int(F) // BK)
    out = []
    for layer in range(3):
        steps = (LP // 2 + 1, LH // 2 + 1) if layer == 2 else (LP, LH)
        for st in range(max(steps)):
            nz = 2 * sum(1 for s in steps if st < s)
            nk = (nk_in0 if layer == 0 else 2 * H // BK) + (H // BK if st else 0)
            out.append((layer, st, nz, nk))
    return out


def takes_b3x(n_sites, nz, n_cu):
    # nanosnp_amd/csrc/hap_gemm.hpp:660, launch_hap_gemm (with the option hap_b3x on; n_rt = 8 is even):
    #   n_tiles % 2 == 0 && n_rt % 2 == 0 && (n_tiles / 2) * (n_rt / 2) * nz >= n_cu
    t = n_tiles(n_sites)
    return t % 2 == 0 and N_RT % 2 == 0 and (t // 2) * (N_RT // 2) * nz >= n_cu


def _smallest_even_tiles(nz, n_cu):
    t = 2
    while not takes_b3x(TS * t, nz, n_cu):
        t += 2
    return t


def tiles_four(n_cu):
    return _smallest_even_tiles(4, n_cu)


def tiles_all(n_cu):
    return _smallest_even_tiles(2, n_cu)


def big_kernel_launches(n_sites, n_cu, F=105):
    """the launches of one pass of n_sites that take k_hap_lstm_b3x"""
    return [l for l in lstm_launches(F) if takes_b3x(n_sites, l[2], n_cu)]


def regime(n_sites, n_cu):
    """one pass of n_sites sites -> "all" | "four" | "none"; anything else is an error of these rules"""
    every = lstm_launches(105)
    big = big_kernel_launches(n_sites, n_cu)
    if len(big) == len(every):
        return "all"
    if not big:
        return "none"
    assert big == [l for l in every if l[2] == 4], (n_sites, n_cu)
    return "four"


def passes(n_sites, pass_sites):
    """the site counts of the passes of one forward (hap_forward_t: for n0 in 0, chunk, ...)"""
    return [min(pass_sites, n_sites - n0) for n0 in range(0, n_sites, pass_sites)]


def gemm_lds_ballast(wgs, n_cu):
    """nanosnp_amd/csrc/hap_gemm.hpp:88, gemm_lds_ballast: the dynamic LDS bytes added to a launch of `wgs` workgroups of k_hap_gemm"""
    k_static, k_cu = 2 * 2 * 128 * (BK + 4) * 4, 160 * 1024
    per = -(-wgs // n_cu) if n_cu > 0 else 4
    per = max(per, 2)
    if per >= 4:
        return 0
    b = k_cu // (per + 1) - k_static + 512
    return b if per * (k_static + b) <= k_cu else 0


def ballast_per_cu(n_sites, nz, n_cu):
    """fp32 and f16x3 step launch (n_tiles x 8 x nz workgroups): 2 or 3 workgroups per CU under a non-zero ballast, 0 without one"""
    wgs = n_tiles(n_sites) * N_RT * nz
    if gemm_lds_ballast(wgs, n_cu) == 0:
        return 0
    return max(-(-wgs // n_cu), 2)


def ballast_sites(n_cu):
    """the three site counts of the ballast test: (four-slice launches at three per CU and two-slice launches at two,
    four-slice launches without ballast and two-slice launches at two, no ballast in any step launch)"""
    return TS * (5 * n_cu // 64), TS * (n_cu // 8), TS * tiles_all(n_cu)
