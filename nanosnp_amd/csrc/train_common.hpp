// train_common.hpp -- what the two training translation units (pileup_train.hip, hap_train.hip) share: the cell's activations, the
// two-level strides of a matrix operand, and the small elementwise / reduction kernels.  Everything has internal linkage.
#pragma once

#include "nsnp_common.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int TR_KCH = 1024;                                  // reduction rows per slice of a weight gradient

// the training cell's activations (nsnp_lstm_cell.hpp fuses them and never exposes a gate): v_exp_f32 + v_rcp_f32 each
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * x)); }
__device__ __forceinline__ float tanh_f(float x)
{
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((2.0f * LOG2E) * x)), 1.0f);
}

// ---- two-level strides ------------------------------------------------------------------------
// index i of a dimension -> (i / T) * so + (i % T) * si, T == 0: i * si.  A (site, step) row is T steps per site with the step stride
// negative where a direction walks the positions backwards.
struct TrDim { int T; int64_t so, si; };
TrDim lin(int64_t si) { return TrDim{0, 0, si}; }
TrDim two(int T, int64_t so, int64_t si) { return TrDim{T, so, si}; }
__device__ __forceinline__ int64_t tr_off(const TrDim& d, int64_t i)
{
    if (!d.T) return i * d.si;
    const uint32_t u = (uint32_t)i, o = u / (uint32_t)d.T;
    return (int64_t)o * d.so + (int64_t)(u - o * (uint32_t)d.T) * d.si;
}

// out = in * mask * scale over the first `live` floats (mask NULL: a copy), a copy behind them (the padding sites have no mask rows)
__global__ __launch_bounds__(256) void k_tr_mask(const float* in, float* out, const uint8_t* __restrict__ mask, float scale, int64_t live,
                                                 int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = in[i];
    if (mask && i < live) v *= (float)mask[i] * scale;
    out[i] = v;
}

__global__ __launch_bounds__(256) void k_tr_dtanh(float* __restrict__ dx, const float* __restrict__ y, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) dx[i] *= 1.0f - y[i] * y[i];
}

// out[i] = (add ? out[i] : 0) + part[0][i] + part[1][i] + ... in that order; out2 (may be null) receives the same value
__global__ __launch_bounds__(256) void k_tr_reduce(const float* __restrict__ part, int64_t count, int Zn, int add, float* __restrict__ out,
                                                   float* __restrict__ out2)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float s = part[i];
    for (int z = 1; z < Zn; ++z) s += part[(int64_t)z * count + i];
    if (add) s += out[i];
    out[i] = s;
    if (out2) out2[i] = s;
}

inline unsigned blocks(int64_t n) { return (unsigned)NSNP_CDIV(n, (int64_t)256); }

}  // namespace
