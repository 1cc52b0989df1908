// nsnp_philox.hpp -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based
// generator behind the training sample draws (pileup_eval.hip, nsnp_hap_train_samples).  Stateless: four output words are a pure function of
// a 128-bit counter and a 64-bit key, so a draw is the same bits whichever lane, grid or run computes it.
//
// Plain C++ with no HIP built-ins: the same text compiles for the device and for the host (tests/helpers_native/philox_kat.cpp runs the
// known answers under the host sanitizers).  Known answers, counter / key -> output:
//   {0,0,0,0} / {0,0}                                                    6627e8d5 e169c58d bc57ac4c 9b00dbd8   (Random123's kat_vectors)
//   {ffffffff x 4} / {ffffffff x 2}                                      408f276d 41c83b0e a20bc7c6 6d5451fd
//   {243f6a88,85a308d3,13198a2e,03707344} / {a4093822,299f31d0}          d16cfe09 94fdcceb 5001e420 24126ea1
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NSNP_PHILOX_FN __host__ __device__ inline
#else
#define NSNP_PHILOX_FN inline
#endif

struct nsnp_philox4 { uint32_t v[4]; };

// ten rounds; between rounds the key words advance by the Weyl constants (nine bumps)
NSNP_PHILOX_FN nsnp_philox4 nsnp_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    const uint64_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = M0 * c0, p1 = M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;                                  // (unsigned: wraps; the bump behind round ten is unused)
    }
    nsnp_philox4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// an index in [0, n) from 32 random bits by multiply-shift: (r n) >> 32.  n < 2^32.  Every index gets floor(2^32 / n) or one more of the 2^32
// values of r, so no probability departs from 1 / n by more than 2^-32 and the total bias is below n / 2^32 (4e-6 at 16,384 variants).
NSNP_PHILOX_FN uint64_t nsnp_philox_index(uint32_t r, uint64_t n)
{
    return ((uint64_t)r * n) >> 32;
}
