// train_common.hpp -- what the two training translation units (pileup_train.hip, hap_train.hip) share: everything of a training step
// outside the recurrence.  The cell's fast activations, the two-level strides of a matrix operand, the matrix product with its launch
// helpers, the loss, the bias sums, the small elementwise / reduction kernels and the workspace reservation.  Everything has internal linkage.
//
//   k_tr_gemm      C(m, n) (+)= sum_k A(m, k) B(k, n) on v_mfma_f32_16x16x4_f32.  A workgroup of four waves owns a 64 x 64 tile of C, each wave
//                  32 x 32 of it (2 x 2 MFMA tiles); K streams through LDS in tiles of 16, the next tile's global loads in flight under the
//                  products of this one.  Every operand is addressed through two-level strides (TrDim), so that one kernel serves
//                    the input projections of a layer          (A = W_ih, B = the input rows of every (site, step), bias b_ih + b_hh)  -> G
//                    the haplotype step products               (A = W_hh, B = h of the previous step; C += : G_t)
//                    W_hh^T dgates_t and W_ih^T dgates         (A = W^T)
//                    output_proj, dense (+ tanh), the heads and their transposes
//                    every weight gradient                     (K = sites x steps, cut into slices of `kchunk` rows: slice blockIdx.y writes
//                                                               its own partial image, k_tr_reduce adds the images in order)
//                  blockIdx.z selects one of up to four problems of a launch.
//   k_tr_loss      per site: lp = z - logsumexp(z), the smoothed loss, the first maximum, dz = (softmax(z) - true_dist) / N; a head of one
//                  class: 0, 0, 0; a padding site: dz = 0.
//   k_tr_colsum    bias gradients: column sums per slice.
//   k_tr_mask, k_tr_dtanh, k_tr_reduce (adds the slices' images in a fixed order).
// No floating-point atomic anywhere: the same call gives the same bits twice.
#pragma once

#include "nsnp_common.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BM = 64, BN = 64, BK = 16, LDS_LD = 80;         // LDS_LD: the four k rows a wave reads at once start 16 banks apart

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

// ---- the tiled product --------------------------------------------------------------------------
struct TrGemm {
    const float* A; const float* B; float* C; const float* bias; const float* bias2;
    int M, N; int64_t K; int kchunk;
    TrDim am, ak, bk, bn, cm, cn;
    int64_t cz;                // floats between the images of two K slices
    int flags;                 // 1: C += , 2: tanh_f (the fast form), 4: tanhf (libm's)
    int a_kfast, b_kfast;      // the operand is contiguous along K: a wave's loads walk K first
};
struct TrBatch { TrGemm g[4]; };

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One operand's share of a K tile for one thread: 4 of the 64 x 16 elements.  kfast: element j is (row (tid >> 4) + 16 j, k tid & 15);
// otherwise (row tid & 63, k (tid >> 6) + 4 j).  Rows outside the matrix and k outside the slice are zeros and are never loaded.
struct HtStage {
    const float* p; TrDim dk; int kfast, kk0, row0; int64_t roff[4]; bool rok[4];
    __device__ __forceinline__ void init(const float* base, const TrDim& drow, const TrDim& dk_, int kfast_, int first_row, int rows, int tid)
    {
        p = base; dk = dk_; kfast = kfast_;
        kk0 = kfast ? (tid & 15) : (tid >> 6);
        row0 = kfast ? (tid >> 4) : (tid & 63);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = first_row + row0 + (kfast ? 16 * j : 0);
            rok[j] = r < rows;
            roff[j] = rok[j] ? tr_off(drow, r) : 0;
        }
    }
    __device__ __forceinline__ void load(int64_t kt, int64_t k1, float (&v)[4]) const
    {
        if (kfast) {
            const int64_t k = kt + kk0;
            const bool kok = k < k1;
            const int64_t ko = kok ? tr_off(dk, k) : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (kok && rok[j]) ? p[roff[j] + ko] : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t k = kt + kk0 + 4 * j;
                v[j] = (k < k1 && rok[0]) ? p[roff[0] + tr_off(dk, k)] : 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(float (*lds)[LDS_LD], const float (&v)[4]) const
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (kfast) lds[kk0][row0 + 16 * j] = v[j];
            else lds[kk0 + 4 * j][row0] = v[j];
        }
    }
};

// grid (tiles of the largest problem, K slices, problems).  MFMA operands: lane l gives A(m + (l & 15), k + (l >> 4)) and
// B(k + (l >> 4), n + (l & 15)); its accumulator register r is C(m + 4 (l >> 4) + r, n + (l & 15)).
__global__ __launch_bounds__(256) void k_tr_gemm(const TrBatch batch)
{
    __shared__ float As[BK][LDS_LD], Bs[BK][LDS_LD];
    const TrGemm& g = batch.g[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, r16 = lane & 15;
    const int tiles_m = NSNP_CDIV(g.M, BM), tiles_n = NSNP_CDIV(g.N, BN);
    if ((int64_t)blockIdx.x >= (int64_t)tiles_m * tiles_n) return;                    // (the whole workgroup)
    const int64_t k0 = (int64_t)blockIdx.y * g.kchunk, k1 = k0 + g.kchunk < g.K ? k0 + g.kchunk : g.K;
    if (k0 >= k1) return;
    const int m0 = (int)(blockIdx.x % tiles_m) * BM, n0 = (int)(blockIdx.x / tiles_m) * BN;
    HtStage sa, sb;
    sa.init(g.A, g.am, g.ak, g.a_kfast, m0, g.M, tid);
    sb.init(g.B, g.bn, g.bk, g.b_kfast, n0, g.N, tid);
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[4];
    sa.load(k0, k1, ra); sb.load(k0, k1, rb);
    for (int64_t kt = k0; kt < k1; kt += BK) {
        __syncthreads();                                       // every wave has finished with the previous tile
        sa.store(As, ra); sb.store(Bs, rb);
        __syncthreads();
        if (kt + BK < k1) { sa.load(kt + BK, k1, ra); sb.load(kt + BK, k1, rb); }
#pragma unroll
        for (int s = 0; s < BK / 4; ++s) {
            const int k = 4 * s + q;
            const float a0 = As[k][wm + r16], a1 = As[k][wm + 16 + r16];
            const float b0 = Bs[k][wn + r16], b1 = Bs[k][wn + 16 + r16];
            acc[0][0] = mfma4(a0, b0, acc[0][0]); acc[0][1] = mfma4(a0, b1, acc[0][1]);
            acc[1][0] = mfma4(a1, b0, acc[1][0]); acc[1][1] = mfma4(a1, b1, acc[1][1]);
        }
    }
    float* __restrict__ cbase = g.C + (int64_t)blockIdx.y * g.cz;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + 16 * j + r16;
        if (n >= g.N) continue;
        float* __restrict__ pc = cbase + tr_off(g.cn, n);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * q + r;
                if (m >= g.M) continue;
                float v = acc[i][j][r];
                if (g.bias) v += g.bias[m];
                if (g.bias2) v += g.bias2[m];
                if (g.flags & 6) v = (g.flags & 2) ? tanh_f(v) : tanhf(v);
                float* c = pc + tr_off(g.cm, m);
                if (g.flags & 1) v += *c;
                *c = v;
            }
    }
}

// ---- the small kernels ------------------------------------------------------------------------
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

// one lane per site.  Z, DZ: [np][ldz], genotype 0 .. n_gt - 1, zygosity behind it; cls: ldc bytes per site, genotype then zygosity.  The
// rules of nsnp_hap_eval's heads: a target outside its head counts as the head's last class, a head of one class has loss 0, pred 0 and
// gradient 0, pred is the first maximum.  A padding site (n <= site < np) gets a zero DZ row and nothing else.
__global__ __launch_bounds__(256) void k_tr_loss(const float* __restrict__ Z, const uint8_t* __restrict__ cls, int64_t n, int64_t np, int n_gt,
                                                 int n_zy, int ldz, int ldc, float inv_n, float* __restrict__ DZ,
                                                 float* __restrict__ site_loss, uint8_t* __restrict__ pred)
{
    const int64_t site = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (site >= np) return;
    if (site >= n) {
        for (int c = 0; c < ldz; ++c) DZ[site * ldz + c] = 0.f;
        return;
    }
    for (int h = 0; h < 2; ++h) {
        const int C = h ? n_zy : n_gt;
        const float* z = Z + site * ldz + (h ? n_gt : 0);
        float* dz = DZ + site * ldz + (h ? n_gt : 0);
        if (C == 1) {
            dz[0] = 0.f;
            if (site_loss) site_loss[site * 2 + h] = 0.f;
            if (pred) pred[site * 2 + h] = 0;
            continue;
        }
        float bv = z[0]; int bi = 0;
        for (int c = 1; c < C; ++c) if (z[c] > bv) { bv = z[c]; bi = c; }           // the first maximum
        float se = 0.f, sz = 0.f;
        for (int c = 0; c < C; ++c) { se += expf(z[c] - bv); sz += z[c]; }
        int t = cls[site * ldc + h];
        if (t >= C) t = C - 1;
        // lp = z - logsumexp(z); loss = -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t]))
        const float lse = bv + logf(se);
        const float lpt = z[t] - lse, slp = sz - (float)C * lse;
        const float off = 0.1f / (float)(C - 1);
        if (site_loss) site_loss[site * 2 + h] = -(0.9f * lpt + off * (slp - lpt));
        if (pred) pred[site * 2 + h] = (uint8_t)bi;
        for (int c = 0; c < C; ++c) dz[c] = (expf(z[c] - lse) - (c == t ? 0.9f : off)) * inv_n;
    }
}

// part[z][m] = sum of src[tr_off(rows, r) + m] over the kchunk rows r of slice z, in order; grid (slices, ceil(M / 256))
__global__ __launch_bounds__(256) void k_tr_colsum(const float* __restrict__ src, const TrDim rows, int M, int64_t R, int kchunk,
                                                   float* __restrict__ part)
{
    const int m = blockIdx.y * 256 + threadIdx.x;
    if (m >= M) return;
    const int64_t r0 = (int64_t)blockIdx.x * kchunk, r1 = r0 + kchunk < R ? r0 + kchunk : R;
    float s = 0.f;
    for (int64_t r = r0; r < r1; ++r) s += src[tr_off(rows, r) + m];
    part[(int64_t)blockIdx.x * M + m] = s;
}

// ---- launch helpers ---------------------------------------------------------------------------
inline unsigned blocks(int64_t n) { return (unsigned)NSNP_CDIV(n, (int64_t)256); }

void launch(hipStream_t s, const TrBatch& b, int count)
{
    int64_t tiles = 0, slices = 1;
    for (int i = 0; i < count; ++i) {
        const TrGemm& g = b.g[i];
        const int64_t t = (int64_t)NSNP_CDIV(g.M, BM) * NSNP_CDIV(g.N, BN), z = NSNP_CDIV(g.K, (int64_t)g.kchunk);
        if (t > tiles) tiles = t;
        if (z > slices) slices = z;
    }
    if (count < 1 || tiles < 1) return;
    hipLaunchKernelGGL(k_tr_gemm, dim3((unsigned)tiles, (unsigned)slices, (unsigned)count), dim3(256), 0, s, b);
}

// Y(m, sample) (+)= sum_k W(m, k) X(sample, k) (+ biases): K in one slice
TrGemm rows_gemm(const float* W, TrDim wm, TrDim wk, int M, int K, const float* X, TrDim xk, TrDim xs, int64_t S, float* Y, TrDim ys,
                 const float* b1, const float* b2, int flags)
{
    TrGemm g{};
    g.A = W; g.B = X; g.C = Y; g.bias = b1; g.bias2 = b2;
    g.M = M; g.N = (int)S; g.K = K; g.kchunk = K;
    g.am = wm; g.ak = wk; g.bk = xk; g.bn = xs; g.cm = lin(1); g.cn = ys; g.cz = 0; g.flags = flags;
    g.a_kfast = wk.T == 0 && wk.si == 1; g.b_kfast = xk.T == 0 && xk.si == 1;
    return g;
}
void gemm1(hipStream_t s, const TrGemm& g) { TrBatch b{}; b.g[0] = g; launch(s, b, 1); }

// dW[m][n] (+)= sum over rows r of DY(r, m) X(r, n): slices of kchunk rows, then the ordered sum
void wgrad(hipStream_t s, float* part, int kchunk, const float* DY, TrDim dyr, int M, const float* X, TrDim xr, TrDim xn, int N, int64_t R,
           float* out, int add)
{
    TrGemm g{};
    g.A = DY; g.B = X; g.C = part;
    g.M = M; g.N = N; g.K = R; g.kchunk = kchunk;
    g.am = lin(1); g.ak = dyr; g.bk = xr; g.bn = xn; g.cm = lin(N); g.cn = lin(1); g.cz = (int64_t)M * N; g.flags = 0;
    g.a_kfast = 0; g.b_kfast = 0;
    gemm1(s, g);
    hipLaunchKernelGGL(k_tr_reduce, dim3(blocks((int64_t)M * N)), dim3(256), 0, s, (const float*)part, (int64_t)M * N,
                       (int)NSNP_CDIV(R, (int64_t)kchunk), add, out, (float*)nullptr);
}

void bgrad(hipStream_t s, float* part, int kchunk, const float* src, TrDim rows, int M, int64_t R, float* out, float* out2, int add)
{
    const int Zn = (int)NSNP_CDIV(R, (int64_t)kchunk);
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)Zn, (unsigned)NSNP_CDIV(M, 256)), dim3(256), 0, s, src, rows, M, R, kchunk, part);
    hipLaunchKernelGGL(k_tr_reduce, dim3(blocks(M)), dim3(256), 0, s, (const float*)part, (int64_t)M, Zn, add, out, out2);
}

// a workspace of `bytes` in place of *ws; the previous reservation stays in force where the allocation fails
int reserve_ws(nsnp_ctx* ctx, void** ws, size_t bytes)
{
    NSNP_HIP(ctx, hipSetDevice(ctx->device));
    NSNP_HIP(ctx, hipDeviceSynchronize());
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->last_err = e;
        return e == hipErrorOutOfMemory ? NSNP_ENOMEM : NSNP_EHIP;
    }
    if (*ws) (void)hipFree(*ws);
    *ws = p;
    return NSNP_OK;
}

}  // namespace
