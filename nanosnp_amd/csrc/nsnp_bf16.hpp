// nsnp_bf16.hpp -- the three-term bf16 split shared by the bf16x3 kernels (pileup_forward_bf16x3.hip) and the exact input block of
// the fp32 layer-0 kernel (pileup_forward.hip): v = v0 + v1 + v2, v0 = bf16(v), v1 = bf16(v - v0), v2 = bf16(v - v0 - v1), round to
// nearest even (8 + 8 + 8 significand bits and the fp32 exponent range: exact for every finite fp32 whose third term does not
// underflow, |v| > 2^-110).  Device split for operands computed in a kernel, host packer for weight images.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef __bf16 b2 __attribute__((ext_vector_type(2)));

namespace {

// hipcc emits v_cvt_pk_bf16_f32 for the casts (round to nearest even, NaN stays NaN)
__device__ __forceinline__ void split3(float v, __bf16& p0, __bf16& p1, __bf16& p2)
{
    p0 = (__bf16)v;
    const float r1 = v - (float)p0;
    p1 = (__bf16)r1;
    p2 = (__bf16)(r1 - (float)p1);
}

inline uint16_t bf16_rne(float v)
{
    uint32_t u; memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);     // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_f32(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float v; memcpy(&v, &u, 4); return v; }

// A-operand image of v_mfma_f32_16x16x32_bf16, three planes: img[tile][kb][plane][lane][j]  <-  split of
// f(row = 16 tile + (lane & 15), kb, q = lane >> 4, j), K position 32 kb + 8 q + j
template <typename F>
void pack_b3(uint16_t* img, int n_tiles, int n_kb, F f)
{
    for (int tile = 0; tile < n_tiles; ++tile)
        for (int kb = 0; kb < n_kb; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const float v = f(16 * tile + (lane & 15), kb, lane >> 4, j);
                    const uint16_t p0 = bf16_rne(v);
                    const float r1 = v - bf16_f32(p0);
                    const uint16_t p1 = bf16_rne(r1);
                    const uint16_t p2 = bf16_rne(r1 - bf16_f32(p1));
                    const size_t e = (((size_t)tile * n_kb + kb) * 3) * 64 + lane;
                    img[e * 8 + j] = p0;
                    img[(e + 64) * 8 + j] = p1;
                    img[(e + 128) * 8 + j] = p2;
                }
}

}  // namespace
