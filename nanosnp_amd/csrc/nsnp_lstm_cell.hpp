// nsnp_lstm_cell.hpp -- the ONE LSTM cell of every recurrence kernel (pileup_forward.hip, pileup_forward_bf16x3.hip, hap_gemm.hpp)
// and the gate-scale contract its weight packers follow.
//
// torch.nn.LSTM equations (PileupModel/model.py:34, HaplotypeModel/model_dev.py:33), gate order i f g o:
//   c' = sigmoid(f) c + sigmoid(i) tanh(g),   h' = sigmoid(o) tanh(c')
// with sigmoid(x) = 1 / (1 + e^-x), tanh(x) = (1 - e^-2x) / (1 + e^-2x): the two products share ONE reciprocal each,
//   sigmoid(i) tanh(g) = (1 - e^-2g) / ((1 + e^-i)(1 + e^-2g)),
// 5 v_exp_f32 + 3 v_rcp_f32 per unit and step instead of 5 + 5 (fp32 MFMAs and vector instructions share a SIMD's lanes: every
// instruction of the cell is matrix-pipe time).  The exponent of the tanh terms is capped at 2^64 so that 1 - e stays finite; an
// overflowing product of the denominators gives reciprocal 0, the correct limit.
//
// Contract with the packers: the four pre-activations arrive already multiplied by lstm_gate_scale(gate) - zi, zf, zo by -log2 e,
// zg by -2 log2 e (folded into the gate rows of W_ih, W_hh and the biases at pack time) - and the cell state is kept multiplied by
// -2 log2 e (it is only ever the argument of the next tanh): K c' = f (K c) + (K - K e_g) r.
#pragma once

namespace nsnp_cell {

constexpr float LOG2E = 1.4426950408889634f;

// factor folded into image row R of an LSTM weight image and its bias (image row R: unit R / 4, gate R % 4 in the order i f g o)
static inline float lstm_gate_scale(int R) { return (R & 3) == 2 ? -2.0f * LOG2E : -LOG2E; }

// min(z, 64) as ONE v_med3_f32 (fminf costs a canonicalising v_max_f32 beside its v_min_f32 where the operand is a computed value);
// the same bits for every z: below -3e38 the exponential is 0 either way
__device__ __forceinline__ float cap64(float z) { return __builtin_amdgcn_fmed3f(z, -3.0e38f, 64.0f); }

__device__ __forceinline__ float lstm_cell(float zi, float zf, float zg, float zo, float c_prev, float& c_new)
{
    const float ei = __builtin_amdgcn_exp2f(zi);
    const float ef = __builtin_amdgcn_exp2f(zf);
    const float eo = __builtin_amdgcn_exp2f(zo);
    const float eg = __builtin_amdgcn_exp2f(cap64(zg));
    constexpr float K = -2.0f * LOG2E;
    const float tg = 1.0f + eg;                                    // (1 + e_i)(1 + e_g) = e_i t + t
    const float ig = __builtin_fmaf(-K, eg, K) * __builtin_amdgcn_rcpf(__builtin_fmaf(ei, tg, tg));
    const float fg = __builtin_amdgcn_rcpf(1.0f + ef);
    const float cn = __builtin_fmaf(fg, c_prev, ig);
    const float ec = __builtin_amdgcn_exp2f(cap64(cn));
    c_new = cn;
    const float tc = 1.0f + ec;
    return (1.0f - ec) * __builtin_amdgcn_rcpf(__builtin_fmaf(eo, tc, tc));
}

// The same cell for FOUR units, one instruction at a time, for kernels that place the cell into the gaps of an MFMA burst by hand:
// slice I = 4 stage + unit, 20 stages per unit, 80 slices.  A stage is one instruction of lstm_cell above with the same operands in
// the same order, so the bits are lstm_cell's; consecutive slices belong to different units, a dependent instruction follows its
// operand four slices later.  z[u] holds the pre-activations (i f g o) of unit u, c[u] its state (updated by stage 12), h[u]
// receives h' (stage 19).
struct CellSlices { float ei[4], ef[4], eo[4], eg[4], t[4], d[4], m[4], fg[4]; };
constexpr int CELL_SLICES = 80;

template <int I, typename Z4>
__device__ __forceinline__ void lstm_cell_slice(CellSlices& w, const Z4 (&z)[4], float (&c)[4], Z4& h)
{
    static_assert(I >= 0 && I < CELL_SLICES, "slice index");
    constexpr int st = I >> 2, u = I & 3;
    constexpr float K = -2.0f * LOG2E;
    if constexpr (st == 0) w.ei[u] = __builtin_amdgcn_exp2f(z[u][0]);
    else if constexpr (st == 1) w.ef[u] = __builtin_amdgcn_exp2f(z[u][1]);
    else if constexpr (st == 2) w.eo[u] = __builtin_amdgcn_exp2f(z[u][3]);
    else if constexpr (st == 3) w.t[u] = cap64(z[u][2]);
    else if constexpr (st == 4) w.eg[u] = __builtin_amdgcn_exp2f(w.t[u]);
    else if constexpr (st == 5) w.t[u] = 1.0f + w.eg[u];                                   // tg
    else if constexpr (st == 6) w.d[u] = __builtin_fmaf(w.ei[u], w.t[u], w.t[u]);
    else if constexpr (st == 7) w.d[u] = __builtin_amdgcn_rcpf(w.d[u]);
    else if constexpr (st == 8) w.m[u] = __builtin_fmaf(-K, w.eg[u], K);
    else if constexpr (st == 9) w.m[u] = w.m[u] * w.d[u];                                  // ig
    else if constexpr (st == 10) w.fg[u] = 1.0f + w.ef[u];
    else if constexpr (st == 11) w.fg[u] = __builtin_amdgcn_rcpf(w.fg[u]);
    else if constexpr (st == 12) c[u] = __builtin_fmaf(w.fg[u], c[u], w.m[u]);             // cn
    else if constexpr (st == 13) w.t[u] = cap64(c[u]);
    else if constexpr (st == 14) w.eg[u] = __builtin_amdgcn_exp2f(w.t[u]);                 // ec
    else if constexpr (st == 15) w.t[u] = 1.0f + w.eg[u];                                  // tc
    else if constexpr (st == 16) w.d[u] = __builtin_fmaf(w.eo[u], w.t[u], w.t[u]);
    else if constexpr (st == 17) w.d[u] = __builtin_amdgcn_rcpf(w.d[u]);
    else if constexpr (st == 18) w.m[u] = 1.0f - w.eg[u];
    else h[u] = w.m[u] * w.d[u];
    // the result is made opaque where it is written: hipcc otherwise packs two units' slices into one v_pk_* instruction and sinks
    // the dependent chain to the end of the burst
    if constexpr (st == 0) asm volatile("" : "+v"(w.ei[u]));
    else if constexpr (st == 1) asm volatile("" : "+v"(w.ef[u]));
    else if constexpr (st == 2) asm volatile("" : "+v"(w.eo[u]));
    else if constexpr (st == 4 || st == 14) asm volatile("" : "+v"(w.eg[u]));
    else if constexpr (st == 3 || st == 5 || st == 13 || st == 15) asm volatile("" : "+v"(w.t[u]));
    else if constexpr (st == 6 || st == 7 || st == 16 || st == 17) asm volatile("" : "+v"(w.d[u]));
    else if constexpr (st == 8 || st == 9 || st == 18) asm volatile("" : "+v"(w.m[u]));
    else if constexpr (st == 10 || st == 11) asm volatile("" : "+v"(w.fg[u]));
    else if constexpr (st == 12) asm volatile("" : "+v"(c[u]));
    else { float v = h[u]; asm volatile("" : "+v"(v)); h[u] = v; }
}

}  // namespace nsnp_cell
