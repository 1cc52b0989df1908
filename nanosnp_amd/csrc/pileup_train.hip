// pileup_train.hip -- the loss gradients of a batch of labelled windows: what loss.backward() of PileupModel/train.py:60-75 computes.
//
// Replaces, for windows, classes and parameters that are already in HBM,
//   LSTMNetwork.forward in train() mode                        PileupModel/model.py:97-112 (BaseEncoder 31-39, ForwardLayer 66-73)
//   the inter-layer dropout of nn.LSTM(dropout=...)            model.py:18-25, as an explicit keep mask and scale
//   LabelSmoothingLoss.forward and its mean                    PileupModel/optim.py:137-144
//   autograd of loss = gt_loss + zy_loss                       model.py:109-110 (the indel heads get no gradient there either)
//
// fp32 only.  The parameters are the caller's 24 device tensors in plain state-dict layout (they change every step, so nothing is
// packed); the inference kernels, their weight images and launch_layers are not involved.  Everything works on groups of 16 sites: a
// chunk of n sites is padded to Np = 16 ceil(n / 16) sites whose counts are 0 and whose dz is 0, so no kernel behind the gather and the
// loss looks at n again and the padding adds exact zeros to every gradient.
//
// The schedule is the reduced one of the inference kernels (the loss reads position 16 only): layer 0 runs 33 steps per direction,
// layer 1 runs 17 (forward direction positions 0..16, reverse 32..16), the dense layers and heads run at position 16.
//
// Kernels
//   k_tr_gather    counts int32 (contiguous or through center_idx) -> X0 fp32 [Np,33,18], zeros behind site n.
//   k_tr_lstm_fwd  the recurrence of one layer: a workgroup of 4 waves per (16 sites, direction), W_hh as MFMA A fragments in 64 VGPRs
//                  per lane, h in LDS.  Wave w owns gate tiles w, w + 4, w + 8, w + 12, so a lane's four accumulators of one register
//                  index are i, f, g, o of ONE hidden unit 16 w + 4 q + r.  G arrives holding the input projections and leaves
//                  holding sigma(i), sigma(f), tanh(g), sigma(o) in place; the cell state c' is saved per step (tanh(c') is
//                  recomputed in the backward: the backward needs c of the previous step anyway), h per step.
//   k_tr_lstm_bwd  backpropagation through time of one layer, same workgroups and the same lane <-> unit map.  Per step the gate
//                  gradients replace the activations in G (in place) and go to LDS; dh of the previous step = W_hh^T dgates is 64
//                  MFMAs per wave whose accumulators land on the lanes that own those units, so only dgates crosses LDS.
//   k_tr_mask      x1 = h0 * mask * keep_scale (forward) and dx1 *= mask * keep_scale (backward); NULL mask: factor 1.
// Every product outside the recurrence (the input projections of both layers, output_proj, dense + tanh, the two heads, their
// transposes and every weight gradient in slices of TR_KCH rows) goes through k_tr_gemm; it, k_tr_loss, k_tr_colsum, k_tr_mask,
// k_tr_dtanh, k_tr_reduce and their launch helpers are train_common.hpp's, shared with hap_train.hip.
// No floating-point atomic anywhere: the same call gives the same bits twice.
#include "train_common.hpp"

namespace {

constexpr int TR_KCH = 1024;                                  // reduction rows per slice of a weight gradient
constexpr int64_t TR_MAX_SITES = (int64_t)1 << 20;

// floats per site of the workspace
constexpr int64_t F_X0 = 33 * 18, F_G0 = 2 * 33 * 256, F_H0 = 33 * 128, F_G1 = 2 * 17 * 256, F_H1 = 17 * 128;
constexpr int64_t F_SITE = F_X0 + F_G0 + 4 * F_H0 + F_G1 + 2 * F_H1 + 128 + 256 + 24 + 24 + 256 + 128 + 128;

struct TrWs {
    float *X0, *G0, *H0, *C0, *X1, *DX1, *G1, *H1, *C1, *Y1, *X2, *Z, *DZ, *DX2, *DY1, *DH1, *PART;
};
TrWs carve(float* base, int64_t cap)
{
    TrWs w; float* p = base;
    auto take = [&](int64_t per) { float* r = p; p += per * cap; return r; };
    w.X0 = take(F_X0); w.G0 = take(F_G0); w.H0 = take(F_H0); w.C0 = take(F_H0); w.X1 = take(F_H0); w.DX1 = take(F_H0);
    w.G1 = take(F_G1); w.H1 = take(F_H1); w.C1 = take(F_H1); w.Y1 = take(128); w.X2 = take(256); w.Z = take(24); w.DZ = take(24);
    w.DX2 = take(256); w.DY1 = take(128); w.DH1 = take(128);
    w.PART = p;
    return w;
}
int64_t part_floats(int64_t cap) { return NSNP_CDIV(cap * 33, (int64_t)TR_KCH) * 256 * 128; }

// ---- the recurrences --------------------------------------------------------------------------
// grid (Np / 16, 2 directions), 256 threads.  G of direction d: [Np][T][256] by STEP (gate rows i f g o as nn.LSTM orders them); H and Cs:
// [Np][rows][128], direction d in columns 64 d.., row = the step, or rows - 1 - step for the reverse direction with `flip` (layer 0: h0 by
// position).  Lane (site ns = lane & 15, q = lane >> 4) of wave w owns units u0 .. u0 + 3, u0 = 16 w + 4 q.
__global__ __launch_bounds__(256) void k_tr_lstm_fwd(float* __restrict__ G, const float* __restrict__ whh0, const float* __restrict__ whh1,
                                                     float* __restrict__ H, float* __restrict__ Cs, int T, int rows, int flip)
{
    __shared__ float hl[64][16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, ns = lane & 15, d = blockIdx.y;
    const int64_t site = (int64_t)blockIdx.x * 16 + ns;
    const int u0 = 16 * w + 4 * q;
    const float* __restrict__ whh = d ? whh1 : whh0;
    float W[4][16];
#pragma unroll
    for (int gate = 0; gate < 4; ++gate)
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) W[gate][kk] = whh[(64 * gate + 16 * w + ns) * 64 + 4 * kk + q];
    float* __restrict__ Gd = G + (int64_t)d * gridDim.x * 16 * T * 256;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) {
        const int row = (flip && d) ? rows - 1 - t : t;
        float* __restrict__ gp = Gd + (site * T + t) * 256 + u0;
        f32x4 acc[4];
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) acc[gate] = *reinterpret_cast<const f32x4*>(gp + 64 * gate);
        if (t > 0) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float b = hl[4 * kk + q][ns];
#pragma unroll
                for (int gate = 0; gate < 4; ++gate) acc[gate] = mfma4(W[gate][kk], b, acc[gate]);
            }
        }
        f32x4 hn, cn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ai = sigmoid_f(acc[0][e]), af = sigmoid_f(acc[1][e]), ag = tanh_f(acc[2][e]), ao = sigmoid_f(acc[3][e]);
            c[e] = af * c[e] + ai * ag;
            cn[e] = c[e];
            hn[e] = ao * tanh_f(c[e]);
            acc[0][e] = ai; acc[1][e] = af; acc[2][e] = ag; acc[3][e] = ao;
        }
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) *reinterpret_cast<f32x4*>(gp + 64 * gate) = acc[gate];
        const int64_t ho = (site * rows + row) * 128 + d * 64 + u0;
        *reinterpret_cast<f32x4*>(Cs + ho) = cn;
        *reinterpret_cast<f32x4*>(H + ho) = hn;
        __syncthreads();                                       // every wave has read the previous h
#pragma unroll
        for (int e = 0; e < 4; ++e) hl[u0 + e][ns] = hn[e];
        __syncthreads();
    }
}

// dH: the gradient that reaches h from outside the recurrence, [Np][rows][128] indexed as H, or with `last_only` [Np][128] applied at the
// last step alone (layer 1: the loss reads position 16, the last step of both directions).
__global__ __launch_bounds__(256) void k_tr_lstm_bwd(float* __restrict__ G, const float* __restrict__ whh0, const float* __restrict__ whh1,
                                                     const float* __restrict__ Cs, const float* __restrict__ dH, int T, int rows, int flip,
                                                     int last_only)
{
    __shared__ float dgl[256][16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, ns = lane & 15, d = blockIdx.y;
    const int64_t site = (int64_t)blockIdx.x * 16 + ns;
    const int u0 = 16 * w + 4 * q;
    const float* __restrict__ whh = d ? whh1 : whh0;
    float WT[64];                                              // A fragments of W_hh^T: A(m = unit 16 w + ns, k = gate row 4 kk + q)
#pragma unroll
    for (int kk = 0; kk < 64; ++kk) WT[kk] = whh[(4 * kk + q) * 64 + 16 * w + ns];
    float* __restrict__ Gd = G + (int64_t)d * gridDim.x * 16 * T * 256;
    f32x4 rec = {0.f, 0.f, 0.f, 0.f};
    float dc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = T - 1; t >= 0; --t) {
        const int row = (flip && d) ? rows - 1 - t : t;
        const int row_prev = (flip && d) ? row + 1 : row - 1;
        float* __restrict__ gp = Gd + (site * T + t) * 256 + u0;
        const int64_t col = d * 64 + u0;
        f32x4 dh = rec;
        if (!last_only) dh += *reinterpret_cast<const f32x4*>(dH + (site * rows + row) * 128 + col);
        else if (t == T - 1) dh += *reinterpret_cast<const f32x4*>(dH + site * 128 + col);
        f32x4 a[4];
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) a[gate] = *reinterpret_cast<const f32x4*>(gp + 64 * gate);
        const f32x4 cc = *reinterpret_cast<const f32x4*>(Cs + (site * rows + row) * 128 + col);
        f32x4 cp = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) cp = *reinterpret_cast<const f32x4*>(Cs + (site * rows + row_prev) * 128 + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ai = a[0][e], af = a[1][e], ag = a[2][e], ao = a[3][e];
            const float tc = tanh_f(cc[e]);
            const float d_o = dh[e] * tc * ao * (1.0f - ao);
            const float dct = dc[e] + dh[e] * ao * (1.0f - tc * tc);
            a[0][e] = dct * ag * ai * (1.0f - ai);
            a[1][e] = dct * cp[e] * af * (1.0f - af);
            a[2][e] = dct * ai * (1.0f - ag * ag);
            a[3][e] = d_o;
            dc[e] = dct * af;
        }
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) *reinterpret_cast<f32x4*>(gp + 64 * gate) = a[gate];
        if (t == 0) break;
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int e = 0; e < 4; ++e) dgl[64 * gate + u0 + e][ns] = a[gate][e];
        __syncthreads();
        rec = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 64; ++kk) rec = mfma4(WT[kk], dgl[4 * kk + q][ns], rec);
        __syncthreads();                                       // dgl is rewritten by the next step
    }
}

// ---- the gather (the other small kernels: train_common.hpp) -------------------------------------
__global__ __launch_bounds__(256) void k_tr_gather(const int32_t* __restrict__ counts, const int64_t* __restrict__ center_idx, int64_t n,
                                                   int64_t total, float* __restrict__ X0)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t site = i / (PW * PC), r = i - site * (PW * PC);
    float v = 0.f;
    if (site < n) v = (float)(center_idx ? counts[(center_idx[site] - PCENTER) * PC + r] : counts[i]);
    X0[i] = v;
}

// one chunk of n <= reservation sites; `add`: the gradients of earlier chunks are in grads already
void run_chunk(nsnp_ctx* ctx, const float* const* P, const int32_t* counts, const int64_t* center_idx, const uint8_t* cls, int64_t n,
               float inv_n, const uint8_t* mask, float scale, float* const* grads, int add, float* site_loss, uint8_t* pred, hipStream_t s)
{
    const int64_t np = NSNP_CDIV(n, (int64_t)16) * 16, cap = NSNP_CDIV(ctx->tr_sites, (int64_t)16) * 16;
    const TrWs w = carve((float*)ctx->tr_ws, cap);
    const unsigned groups = (unsigned)(np / 16);
    const int64_t S0 = np * 33, S1 = np * 17;
    {
        ScopedKernelTimer tm(ctx, NSNP_K_TRAIN_FWD, s);
        hipLaunchKernelGGL(k_tr_gather, dim3(blocks(np * F_X0)), dim3(256), 0, s, counts, center_idx, n, np * F_X0, w.X0);
        for (int d = 0; d < 2; ++d)             // layer 0 input projections: G0[d][site][step] = W_ih x(position of the step) + b_ih + b_hh
            gemm1(s, rows_gemm(P[4 * d], lin(18), lin(1), 256, 18, w.X0 + (d ? 32 * 18 : 0), lin(1), two(33, 33 * 18, d ? -18 : 18), S0,
                      w.G0 + d * S0 * 256, lin(256), P[4 * d + 2], P[4 * d + 3], 0));
        hipLaunchKernelGGL(k_tr_lstm_fwd, dim3(groups, 2), dim3(256), 0, s, w.G0, P[1], P[5], w.H0, w.C0, 33, 33, 1);
        hipLaunchKernelGGL(k_tr_mask, dim3(blocks(np * F_H0)), dim3(256), 0, s, (const float*)w.H0, w.X1, mask, scale, n * F_H0, np * F_H0);
        for (int d = 0; d < 2; ++d)             // layer 1: steps 0..16 are positions 0..16 (forward) and 32..16 (reverse)
            gemm1(s, rows_gemm(P[8 + 4 * d], lin(128), lin(1), 256, 128, w.X1 + (d ? 32 * 128 : 0), lin(1), two(17, 33 * 128, d ? -128 : 128), S1,
                      w.G1 + d * S1 * 256, lin(256), P[8 + 4 * d + 2], P[8 + 4 * d + 3], 0));
        hipLaunchKernelGGL(k_tr_lstm_fwd, dim3(groups, 2), dim3(256), 0, s, w.G1, P[9], P[13], w.H1, w.C1, 17, 17, 0);
        const float* h1c = w.H1 + 16 * 128;     // step 16 of both directions = position 16; one row per site, 17 * 128 apart
        gemm1(s, rows_gemm(P[16], lin(128), lin(1), 128, 128, h1c, lin(1), lin(17 * 128), np, w.Y1, lin(128), P[17], nullptr, 0));
        gemm1(s, rows_gemm(P[18], lin(128), lin(1), 256, 128, w.Y1, lin(1), lin(128), np, w.X2, lin(256), P[19], nullptr, 2));
        gemm1(s, rows_gemm(P[20], lin(256), lin(1), 21, 256, w.X2, lin(1), lin(256), np, w.Z, lin(24), P[21], nullptr, 0));
        gemm1(s, rows_gemm(P[22], lin(256), lin(1), 3, 256, w.X2, lin(1), lin(256), np, w.Z + 21, lin(24), P[23], nullptr, 0));
        hipLaunchKernelGGL(k_tr_loss, dim3(blocks(np)), dim3(256), 0, s, (const float*)w.Z, cls, n, np, 21, 3, 24, 4, inv_n, w.DZ, site_loss, pred);
    }
    {
        ScopedKernelTimer tm(ctx, NSNP_K_TRAIN_BWD, s);
        // heads^T, tanh', dense^T, output_proj^T
        gemm1(s, rows_gemm(P[20], lin(1), lin(256), 256, 21, w.DZ, lin(1), lin(24), np, w.DX2, lin(256), nullptr, nullptr, 0));
        gemm1(s, rows_gemm(P[22], lin(1), lin(256), 256, 3, w.DZ + 21, lin(1), lin(24), np, w.DX2, lin(256), nullptr, nullptr, 1));
        hipLaunchKernelGGL(k_tr_dtanh, dim3(blocks(np * 256)), dim3(256), 0, s, w.DX2, (const float*)w.X2, np * 256);
        gemm1(s, rows_gemm(P[18], lin(1), lin(128), 128, 256, w.DX2, lin(1), lin(256), np, w.DY1, lin(128), nullptr, nullptr, 0));
        gemm1(s, rows_gemm(P[16], lin(1), lin(128), 128, 128, w.DY1, lin(1), lin(128), np, w.DH1, lin(128), nullptr, nullptr, 0));
        hipLaunchKernelGGL(k_tr_lstm_bwd, dim3(groups, 2), dim3(256), 0, s, w.G1, P[9], P[13], (const float*)w.C1, (const float*)w.DH1, 17, 17, 0, 1);
        // dx1 = sum over the directions of W_ih^T dgates at the step's position; position 16 receives both
        (void)hipMemsetAsync(w.DX1, 0, (size_t)(np * F_H0) * sizeof(float), s);
        for (int d = 0; d < 2; ++d)
            gemm1(s, rows_gemm(P[8 + 4 * d], lin(1), lin(128), 128, 256, w.G1 + d * S1 * 256, lin(1), lin(256), S1, w.DX1 + (d ? 32 * 128 : 0),
                      two(17, 33 * 128, d ? -128 : 128), nullptr, nullptr, 1));
        if (mask) hipLaunchKernelGGL(k_tr_mask, dim3(blocks(np * F_H0)), dim3(256), 0, s, (const float*)w.DX1, w.DX1, mask, scale, n * F_H0, np * F_H0);
        hipLaunchKernelGGL(k_tr_lstm_bwd, dim3(groups, 2), dim3(256), 0, s, w.G0, P[1], P[5], (const float*)w.C0, (const float*)w.DX1, 33, 33, 1, 0);
    }
    {
        ScopedKernelTimer tm(ctx, NSNP_K_TRAIN_WGRAD, s);
        float* part = w.PART;
        for (int d = 0; d < 2; ++d) {
            const float* g0 = w.G0 + d * S0 * 256;
            wgrad(s, part, TR_KCH, g0, lin(256), 256, w.X0 + (d ? 32 * 18 : 0), two(33, 33 * 18, d ? -18 : 18), lin(1), 18, S0, grads[4 * d], add);
            // step t + 1 (t = 0..31) meets the h of step t: position t (forward), 32 - t (reverse)
            wgrad(s, part, TR_KCH, g0 + 256, two(32, 33 * 256, 256), 256, w.H0 + d * 64 + (d ? 32 * 128 : 0), two(32, 33 * 128, d ? -128 : 128), lin(1), 64,
                  np * 32, grads[4 * d + 1], add);
            bgrad(s, part, TR_KCH, g0, lin(256), 256, S0, grads[4 * d + 2], grads[4 * d + 3], add);
            const float* g1 = w.G1 + d * S1 * 256;
            wgrad(s, part, TR_KCH, g1, lin(256), 256, w.X1 + (d ? 32 * 128 : 0), two(17, 33 * 128, d ? -128 : 128), lin(1), 128, S1, grads[8 + 4 * d], add);
            wgrad(s, part, TR_KCH, g1 + 256, two(16, 17 * 256, 256), 256, w.H1 + d * 64, two(16, 17 * 128, 128), lin(1), 64, np * 16, grads[8 + 4 * d + 1], add);
            bgrad(s, part, TR_KCH, g1, lin(256), 256, S1, grads[8 + 4 * d + 2], grads[8 + 4 * d + 3], add);
        }
        wgrad(s, part, TR_KCH, w.DY1, lin(128), 128, w.H1 + 16 * 128, lin(17 * 128), lin(1), 128, np, grads[16], add);
        bgrad(s, part, TR_KCH, w.DY1, lin(128), 128, np, grads[17], nullptr, add);
        wgrad(s, part, TR_KCH, w.DX2, lin(256), 256, w.Y1, lin(128), lin(1), 128, np, grads[18], add);
        bgrad(s, part, TR_KCH, w.DX2, lin(256), 256, np, grads[19], nullptr, add);
        wgrad(s, part, TR_KCH, w.DZ, lin(24), 21, w.X2, lin(256), lin(1), 256, np, grads[20], add);
        bgrad(s, part, TR_KCH, w.DZ, lin(24), 21, np, grads[21], nullptr, add);
        wgrad(s, part, TR_KCH, w.DZ + 21, lin(24), 3, w.X2, lin(256), lin(1), 256, np, grads[22], add);
        bgrad(s, part, TR_KCH, w.DZ + 21, lin(24), 3, np, grads[23], nullptr, add);
    }
}

}  // namespace

void nsnp_train_free(nsnp_ctx* ctx)
{
    if (ctx->tr_ws) (void)hipFree(ctx->tr_ws);
    ctx->tr_ws = nullptr; ctx->tr_sites = 0;
}

extern "C" int nsnp_pileup_train_reserve(nsnp_ctx* ctx, int64_t max_sites)
{
    if (!ctx || max_sites <= 0 || max_sites > TR_MAX_SITES) return NSNP_EINVAL;
    if (ctx->tr_ws && ctx->tr_sites == max_sites) return NSNP_OK;
    const int64_t cap = NSNP_CDIV(max_sites, (int64_t)16) * 16;
    const int rc = reserve_ws(ctx, &ctx->tr_ws, (size_t)(cap * F_SITE + part_floats(cap)) * sizeof(float));
    if (rc != NSNP_OK) return rc;
    ctx->tr_sites = max_sites;
    return NSNP_OK;
}

extern "C" int nsnp_pileup_loss_grad(nsnp_ctx* ctx, const float* const* params, const int32_t* counts, const int64_t* center_idx,
                                     const uint8_t* cls, int64_t N, const uint8_t* keep_mask, float keep_scale, float* const* grads,
                                     float* site_loss, uint8_t* pred, void* stream)
{
    if (!ctx || N < 0) return NSNP_EINVAL;
    if (ctx->precision != 0) return NSNP_EINVAL;             // fp32 only
    if (N == 0) return NSNP_OK;
    if (!params || !counts || !cls || !grads) return NSNP_EINVAL;
    for (int i = 0; i < 24; ++i) if (!params[i] || !grads[i]) return NSNP_EINVAL;
    if (!ctx->tr_ws || ctx->tr_sites <= 0) return NSNP_EINVAL;     // nsnp_pileup_train_reserve first
    hipStream_t s = (hipStream_t)stream;
    const float inv_n = 1.0f / (float)N;                     // of the whole batch, whatever the chunks
    for (int64_t base = 0; base < N; base += ctx->tr_sites) {
        const int64_t n = N - base < ctx->tr_sites ? N - base : ctx->tr_sites;
        run_chunk(ctx, params, center_idx ? counts : counts + base * (PW * PC), center_idx ? center_idx + base : nullptr, cls + base * 4, n,
                  inv_n, keep_mask ? keep_mask + base * F_H0 : nullptr, keep_scale, grads, base > 0, site_loss ? site_loss + base * 2 : nullptr,
                  pred ? pred + base * 2 : nullptr, s);
    }
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
