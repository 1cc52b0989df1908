// pileup_forward_f16x3.hip -- PileupModel forward with every fp32 matrix product evaluated as three
// fp16 MFMAs with fp32 accumulation ("f16x3"):
//
//     w = w_hi + w_lo,  x = x_hi + x_lo   (hi = fp16(v), lo = fp16(v - hi); 21-22 significant bits)
//     w.x  ~=  w_hi.x_hi + w_lo.x_hi + w_hi.x_lo          (dropped term w_lo.x_lo <= 2^-22 |w.x|)
//
// fp16 products are exact in the fp32 accumulator and v_mfma_f32_16x16x32_f16 honours fp16
// subnormals (probed on gfx950: tools/probes/denorm_probe.hip), so the result differs from the exact-fp32
// path (pileup_forward.hip) by ~1e-6 in the probabilities (measured; tolerance 1e-4) while the matrix
// pipe runs at the fp16 rate: 3 MFMAs of 16 cycles replace 8 of 32 cycles per 32-deep K block.
//
// Kernels in this file (same reference functions as the fp32 path):
//   K1r  k_pileup_l0_rs   layer 0, weights in VGPRs, h exchanged through LDS            default
//   K23r k_pileup_l1_rs   layer 1 projection + recurrence, weights in VGPRs           default
//   K4   k_pileup_head_h  output_proj, dense + tanh, heads, softmax                   default
//   K4e  k_pileup_head_eval_h  K4 up to the head product, then all 90 head rows as logits, loss / argmax / counts   scoring (eval_windows2)
//   K1   k_pileup_l0_h    layer 0 with LDS weight images, h in registers (the accumulator layout of tile i - lane = site +
//                         16*q holds unit 4*i+q - is packed straight into the next step's B fragments)   l0_register_stationary 0
//   K23  k_pileup_l1f_h   fused layer 1 with LDS images + a streamed ring             l1_register_stationary 0
//   K2 / K3               unfused layer-1 projection and recurrence                    fused_l1 0
#include "nsnp_common.hpp"
#include "nsnp_eval_tail.hpp"
#include <type_traits>

#ifndef NSNP_F16_PIN
#define NSNP_F16_PIN 1
#endif
#if NSNP_F16_PIN
#define PIN() __builtin_amdgcn_sched_barrier(0)
#else
#define PIN() do {} while (0)
#endif

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x4 mfma_h(h8 a, h8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float sigmoid_f(float x)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * x));
}
__device__ __forceinline__ float tanh_f(float x)
{
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((2.0f * LOG2E) * x)), 1.0f);
}
__device__ __forceinline__ void split1(float v, _Float16& hi, _Float16& lo)
{
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}
// Input counts: int32 in the ABI, below 2^11 in practice (mpileup depth cap 144, make_predict_data.sh:117) and then
// exact in the hi half alone.  Both halves saturate at the fp16 maximum instead of overflowing to infinity, so
// |x| <= 131008 is carried (to ~3e-5 relative beyond 67552) and larger magnitudes act as +-131008: every gate such an
// input reaches is saturated either way.  pileup_precision = 0 is exact for the whole int32 range.
__device__ __forceinline__ void split_count(float v, _Float16& hi, _Float16& lo)
{
    hi = (_Float16)__builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f);
    lo = (_Float16)__builtin_amdgcn_fmed3f(v - (float)hi, -65504.0f, 65504.0f);
}

// acc[t] += W(tile TB+t, K block kb) . b for t < NT, three MFMAs per (tile, block), walked in groups of
// G tiles term-major so that MFMAs on one accumulator are G issue slots apart.
// img: h8 elements [tile][kb][part][lane] with NKB blocks per tile.
template <int NT, int NKB, int KB0, int KBN, int TB, int G, typename WP>
__device__ __forceinline__ void wave_gemm_h(WP img, int lane, const h8* bh, const h8* bl, f32x4* acc)
{
#pragma unroll
    for (int kb = 0; kb < KBN; ++kb) {
#pragma unroll
        for (int ig = 0; ig < NT; ig += G) {
            h8 ah[G], al[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                ah[u] = img[(((TB + ig + u) * NKB + (KB0 + kb)) * 2 + 0) * 64 + lane];
                al[u] = img[(((TB + ig + u) * NKB + (KB0 + kb)) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int u = 0; u < G; ++u) acc[ig + u] = mfma_h(ah[u], bh[kb], acc[ig + u]);
#pragma unroll
            for (int u = 0; u < G; ++u) acc[ig + u] = mfma_h(al[u], bh[kb], acc[ig + u]);
#pragma unroll
            for (int u = 0; u < G; ++u) acc[ig + u] = mfma_h(ah[u], bl[kb], acc[ig + u]);
            PIN();
        }
    }
}

// LSTM cell for 8 units; the new h values become one K block of next step's B fragments
__device__ __forceinline__ void lstm_pointwise8_h(const f32x4* acc, float* c, h8& nh, h8& nl)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float ig = sigmoid_f(acc[i][0]);
        const float fg = sigmoid_f(acc[i][1]);
        const float gg = tanh_f(acc[i][2]);
        const float og = sigmoid_f(acc[i][3]);
        c[i] = __builtin_fmaf(fg, c[i], ig * gg);
        const float h = og * tanh_f(c[i]);
        _Float16 hi, lo;
        split1(h, hi, lo);
        nh[i] = hi; nl[i] = lo;
    }
}

// Same contraction as wave_gemm_h with the weight fragments of group g+1 requested before the MFMAs of
// group g are issued (G = 2 tiles per group), so the LDS latency hides behind the previous group's
// matrix work instead of in front of every group.
// PINMASK: which instruction classes may still cross the scheduling pins (0 = none; 0x1 = ALU incl. MFMA and
// VALU, so that independent sigmoid/tanh work of the previous quarter can be woven between the MFMAs while
// the LDS / global reads stay where they are).
template <int NT, int NKB, int KBN, int TB, int PINMASK = 0, typename WP>
__device__ __forceinline__ void wave_gemm_h_pipe(WP img, int lane, const h8* bh, const h8* bl, f32x4* acc)
{
    constexpr int G = 2;
    constexpr int NG = KBN * (NT / G);
    h8 ah[2][G], al[2][G];
    auto fetch = [&](int g, int buf) {
        const int kb = g / (NT / G), ig = (g % (NT / G)) * G;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            ah[buf][u] = img[(((TB + ig + u) * NKB + kb) * 2 + 0) * 64 + lane];
            al[buf][u] = img[(((TB + ig + u) * NKB + kb) * 2 + 1) * 64 + lane];
        }
    };
    fetch(0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int buf = g & 1;
        const int kb = g / (NT / G), ig = (g % (NT / G)) * G;
        if (g + 1 < NG) fetch(g + 1, buf ^ 1);
#pragma unroll
        for (int u = 0; u < G; ++u) acc[ig + u] = mfma_h(ah[buf][u], bh[kb], acc[ig + u]);
#pragma unroll
        for (int u = 0; u < G; ++u) acc[ig + u] = mfma_h(al[buf][u], bh[kb], acc[ig + u]);
#pragma unroll
        for (int u = 0; u < G; ++u) acc[ig + u] = mfma_h(ah[buf][u], bl[kb], acc[ig + u]);
        __builtin_amdgcn_sched_barrier(PINMASK);
    }
}

// LSTM cell for 4 units (a quarter pass); the new h values fill half of one K block of next step's B fragments
template <int J0>
__device__ __forceinline__ void lstm_pointwise4_h(const f32x4* acc, float* c, h8& nh, h8& nl)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float ig = sigmoid_f(acc[i][0]);
        const float fg = sigmoid_f(acc[i][1]);
        const float gg = tanh_f(acc[i][2]);
        const float og = sigmoid_f(acc[i][3]);
        c[i] = __builtin_fmaf(fg, c[i], ig * gg);
        const float h = og * tanh_f(c[i]);
        _Float16 hi, lo;
        split1(h, hi, lo);
        nh[J0 + i] = hi; nl[J0 + i] = lo;
    }
}

__device__ __forceinline__ void copy_to_lds_h(h8* dst, const _Float16* __restrict__ src, int n_h8, int tid, int nthreads)
{
    const h8* s8 = reinterpret_cast<const h8*>(src);
    for (int i = tid; i < n_h8; i += nthreads) dst[i] = s8[i];
}

// ---------------------------------------------------------------------------------------------
// K1: layer 0.  LDS: W_hh image (64 KB: [16][2][2][64] h8) + hi part of the W_ih image (16 KB) = 80 KB;
// the lo part of W_ih (16 KB) is read through L1.  H0 layout: [site][t][dir][q][16 hi | 16 lo] fp16.
// ---------------------------------------------------------------------------------------------
constexpr int HH_H8 = 16 * 2 * 2 * 64;       // h8 elements of a recurrent image
constexpr int IH_H8 = 16 * 64;               // one part of the input image
constexpr int L0H_LDS_BYTES = (HH_H8 + IH_H8) * 16;

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES, (WAVES >= 8 ? 4 : (WAVES == 4 ? 2 : 1))) void k_pileup_l0_h(
    const int32_t* __restrict__ x, const int64_t* __restrict__ center_idx, int64_t N,
    const _Float16* __restrict__ whh0, const _Float16* __restrict__ whh1,
    const _Float16* __restrict__ wih_hi0, const _Float16* __restrict__ wih_hi1,
    const _Float16* __restrict__ wih_lo0, const _Float16* __restrict__ wih_lo1,
    _Float16* __restrict__ H0)
{
    extern __shared__ h8 ldsh[];
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    copy_to_lds_h(ldsh, dir ? whh1 : whh0, HH_H8, tid, 64 * WAVES);
    copy_to_lds_h(ldsh + HH_H8, dir ? wih_hi1 : wih_hi0, IH_H8, tid, 64 * WAVES);
    const h8* __restrict__ wlo = reinterpret_cast<const h8*>(dir ? wih_lo1 : wih_lo0);
    __syncthreads();

    const int64_t site = (int64_t)blockIdx.x * (16 * WAVES) + wave * 16 + (lane & 15);
    const bool live = site < N;
    const int64_t sc = live ? site : N - 1;
    const int32_t* __restrict__ xs = center_idx ? x + (center_idx[sc] - PCENTER) * PC : x + sc * (PW * PC);
    _Float16* __restrict__ hout = H0 + ((sc * PW * 2 + dir) * 4 + q) * 32;

    float c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = 0.f;
    h8 bh[2], bl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) { bh[k][j] = (_Float16)0.f; bl[k][j] = (_Float16)0.f; }

    // lane q supplies channels 8q..8q+7 (q = 2: channels 16,17 and the constant 1 the bias rides on)
    int xi[8];
    auto load_x = [&](int t) {
        const int32_t* p = xs + t * PC;
        if (q < 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xi[j] = p[8 * q + j];
        } else {
            xi[0] = p[16]; xi[1] = p[17];
#pragma unroll
            for (int j = 2; j < 8; ++j) xi[j] = 0;
        }
    };
    load_x(dir ? PW - 1 : 0);
    for (int s = 0; s < PW; ++s) {
        const int t = dir ? PW - 1 - s : s;
        h8 xh, xl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = (float)xi[j];                       // predict.py:49 int -> float
            if (q == 2 && j == 2) v = 1.0f;
            if (q == 3) v = 0.0f;
            _Float16 hi, lo; split_count(v, hi, lo);
            xh[j] = hi; xl[j] = lo;
        }
        if (s + 1 < PW) load_x(dir ? t - 1 : t + 1);
        h8 nh[2], nl[2];
        // four quarter passes of 4 gate tiles.  Within a quarter the lo fragments of the input image (read
        // through L1) are requested first and consumed last, behind the LDS-fed recurrent MFMAs; the LSTM cell
        // of quarter q is issued together with the MFMAs of quarter q+1 (which only need the previous step's
        // h), inside one scheduling region whose inner pins let ALU work cross, so the matrix and the vector
        // pipe overlap inside a single wave.
#define QMFMA(QP, ACC)                                                                                     \
        {                                                                                                  \
            h8 ilo[4];                                                                                     \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) ilo[u] = wlo[((QP) * 4 + u) * 64 + lane];        \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) ACC[i] = f32x4{0.f, 0.f, 0.f, 0.f};             \
            wave_gemm_h_pipe<4, 2, 2, (QP) * 4, 0x1>(ldsh, lane, bh, bl, ACC); /* h = 0 at s = 0 */       \
            h8 ihi[4];                                                                                     \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) ihi[u] = ldsh[HH_H8 + ((QP) * 4 + u) * 64 + lane]; \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) ACC[u] = mfma_h(ihi[u], xh, ACC[u]);             \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) ACC[u] = mfma_h(ilo[u], xh, ACC[u]);             \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) ACC[u] = mfma_h(ihi[u], xl, ACC[u]);             \
        }
#define QPW(QP, ACC) lstm_pointwise4_h<((QP) & 1) * 4>(ACC, c + (QP) * 4, nh[(QP) >> 1], nl[(QP) >> 1]);
        f32x4 accA[4], accB[4];
        PIN(); QMFMA(0, accA)
        PIN(); QMFMA(1, accB) QPW(0, accA)
        PIN(); QMFMA(2, accA) QPW(1, accB)
        PIN(); QMFMA(3, accB) QPW(2, accA)
        PIN(); QPW(3, accB)
        PIN();
#undef QMFMA
#undef QPW
        bh[0] = nh[0]; bh[1] = nh[1]; bl[0] = nl[0]; bl[1] = nl[1];
        if (live) {
            h8* o = reinterpret_cast<h8*>(hout + (int64_t)t * (2 * 4 * 32));
            o[0] = bh[0]; o[1] = bh[1]; o[2] = bl[0]; o[3] = bl[1];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K1r: layer 0 with REGISTER-STATIONARY weights (default).  K1 above keeps one wave per 16 sites with all 16
// gate tiles and re-reads the 80 KB weight images from LDS every step: the LDS image pins one workgroup per CU
// (one wave per SIMD, nobody to fill MFMA / transcendental / LDS stalls: SQ counters showed 36 % matrix-pipe
// busy, 38 % issue stalls) and the LDS pipe is 40 % busy.  Here a workgroup is 4 waves x NSG groups of 16 sites;
// wave w owns gate tiles 4w..4w+3 (hidden units 16w..16w+15, all four gates) and holds their W_hh / W_ih hi+lo
// fragments in 96 VGPRs for the whole kernel.  Only h_t (and the staged x_t) cross waves, through a
// double-buffered LDS exchange (one workgroup barrier per step, 17 KB per buffer), so LDS traffic per site-step
// drops 5x, a workgroup needs 52 KB of LDS and 2-3 workgroups (independent barriers) share a CU.
//   exchange row of a site: 64 hi halves | 64 lo halves; K position p = 16w + 4q + u <-> unit 16w + 4u + q, the four
//   units lane (site, q) of wave w leaves the cell with (two 8-byte writes); a B fragment (K block kb, lane quarter kq)
//   is one 16-byte read per plane at position 32kb + 8kq - no register shuffles.
//   The per-step barrier waits for LDS only (s_waitcnt lgkmcnt(0); s_barrier): __syncthreads() would also drain
//   the H0 stores to HBM every step.
// H0 is written in the layout K1 writes (entries m = 4w+u of row q), so the layer-1 kernels are unchanged.
// ---------------------------------------------------------------------------------------------
constexpr int RS_HROW = 136;                 // halves per exchange row (256 B + 16 B pad: 16-byte accesses of 16 lanes hit distinct banks)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
constexpr float RS_K = 2.0f * LOG2E;         // scale of the cell state kept by K1r
constexpr int RS_XROW = 72;                  // halves per staged-input row: 32 hi | 32 lo | pad (144 B)
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

template <int NSG>
__global__ __launch_bounds__(256, 2) void k_pileup_l0_rs(
    const int32_t* __restrict__ x, const int64_t* __restrict__ center_idx, int64_t N,
    const _Float16* __restrict__ whh0, const _Float16* __restrict__ whh1,
    const _Float16* __restrict__ wih0, const _Float16* __restrict__ wih1,
    _Float16* __restrict__ H0 /* padded to a multiple of 64 sites: stores are unconditional */, int prio)
{
    if ((prio & 2) && (blockIdx.x & 1)) __builtin_amdgcn_s_setprio(1);
    __shared__ __attribute__((aligned(16))) _Float16 hx[2][16 * NSG][RS_HROW];
    __shared__ __attribute__((aligned(16))) _Float16 xx[2][16 * NSG][RS_XROW];
    __shared__ int xflag[2][4];
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;

    // ---- weights of this wave's four gate tiles -> registers -------------------------------------
    h8 Whh[4][2][2], Wih[4][2];
    {
        const h8* __restrict__ ghh = reinterpret_cast<const h8*>(dir ? whh1 : whh0);
        const h8* __restrict__ gih = reinterpret_cast<const h8*>(dir ? wih1 : wih0);       // [tile][part][lane]
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int part = 0; part < 2; ++part) Whh[u][kb][part] = ghh[(((4 * wave + u) * 2 + kb) * 2 + part) * 64 + lane];
            Wih[u][0] = gih[((4 * wave + u) * 2 + 0) * 64 + lane];
            Wih[u][1] = gih[((4 * wave + u) * 2 + 1) * 64 + lane];
        }
    }

    // ---- input staging: wave w (< NSG) converts x_t of site group w to fp16 hi/lo rows --------------
    const int64_t base_site = (int64_t)blockIdx.x * (16 * NSG);
    const bool stager = NSG >= 4 || wave < NSG;
    const int64_t xsite = base_site + wave * 16 + n;
    const int64_t xsc = (stager && xsite < N) ? xsite : N - 1;
    const int32_t* __restrict__ xs = center_idx ? x + (center_idx[xsc] - PCENTER) * PC : x + xsc * (PW * PC);
    int xi[8];
    auto load_x = [&](int t) {
        if (!stager) return;
        const int32_t* p = xs + t * PC;
        if (q < 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xi[j] = p[8 * q + j];
        } else {
            xi[0] = p[16]; xi[1] = p[17];
#pragma unroll
            for (int j = 2; j < 8; ++j) xi[j] = 0;
        }
    };
    auto stage_x = [&](int buf) {
        if (!stager) return;
        h8 xh, xl;
        bool big = false;                                  // counts are exact in one fp16 up to +-2048 (always, in practice)
#pragma unroll
        for (int j = 0; j < 8; ++j) big |= (unsigned)(xi[j] + 2048) > 4096u;
        bool any = __ballot(big) != 0ull;
        if (!any) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = (float)xi[j];                       // predict.py:49 int -> float
                if (q == 2 && j == 2) v = 1.0f;               // the bias column of the input image
                if (q == 3) v = 0.0f;
                xh[j] = (_Float16)v; xl[j] = (_Float16)0.f;
            }
        } else {
            bool nz = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = (float)xi[j];
                if (q == 2 && j == 2) v = 1.0f;
                if (q == 3) v = 0.0f;
                _Float16 hi, lo; split_count(v, hi, lo);
                xh[j] = hi; xl[j] = lo; nz |= lo != (_Float16)0.f;
            }
            any = __ballot(nz) != 0ull;
        }
        _Float16* row = &xx[buf][wave * 16 + n][0];
        *reinterpret_cast<h8*>(row + 8 * q) = xh;
        *reinterpret_cast<h8*>(row + 32 + 8 * q) = xl;
        if (lane == 0) xflag[buf][wave] = any;
    };
    if (tid < 8) xflag[tid >> 2][tid & 3] = 0;
    // h_{-1} = 0: the buffer step 0 reads
    for (int i = tid; i < 16 * NSG * RS_HROW / 8; i += 256) reinterpret_cast<h8*>(&hx[1][0][0])[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
    __syncthreads();
    load_x(dir ? PW - 1 : 0);
    stage_x(0);
    __syncthreads();

    float c[4 * NSG];
#pragma unroll
    for (int i = 0; i < 4 * NSG; ++i) c[i] = 0.f;
    // H0 rows leave through the exchange buffer one step late: thread (row = tid / 4, q' = tid % 4) gathers the
    // four chunks q', 4+q', 8+q', 12+q' of its site (hi and lo of units 4m + q', m = 0..15) and writes the
    // complete 64-byte row [16 hi | 16 lo] that K1 writes
    auto flush_h = [&](int buf, int t) {
        // with fewer than four site groups the waves that do not stage x rows do the flushing
        constexpr int FO = NSG < 4 ? 64 * NSG : 0;
        if (NSG < 4 && (tid < FO || tid >= FO + 64 * NSG)) return;
        const int row = (tid - FO) >> 2, qq = tid & 3;
        const _Float16* r = &hx[buf][row][4 * qq];                  // positions 16w + 4qq + u, w = 0..3: units 4m + qq, m = 4w + u
        h8* o = reinterpret_cast<h8*>(H0 + ((((base_site + row) * PW + t) * 2 + dir) * 4 + qq) * 32);
        h4 a0 = *reinterpret_cast<const h4*>(r), a1 = *reinterpret_cast<const h4*>(r + 16);
        h4 a2 = *reinterpret_cast<const h4*>(r + 32), a3 = *reinterpret_cast<const h4*>(r + 48);
        o[0] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
        o[1] = __builtin_shufflevector(a2, a3, 0, 1, 2, 3, 4, 5, 6, 7);
        a0 = *reinterpret_cast<const h4*>(r + 64); a1 = *reinterpret_cast<const h4*>(r + 80);
        a2 = *reinterpret_cast<const h4*>(r + 96); a3 = *reinterpret_cast<const h4*>(r + 112);
        o[2] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
        o[3] = __builtin_shufflevector(a2, a3, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    struct BFrag { h8 bh0, bh1, bl0, bl1, xh, xl; };
    auto step = [&](auto any_lo_tag, int t, int xb, int hw_) {
        constexpr bool ANYLO = decltype(any_lo_tag)::value;
        const int hr = hw_ ^ 1;
        auto load_b = [&](int sg, BFrag& f) {
            const _Float16* hrow = &hx[hr][16 * sg + n][8 * q];
            f.bh0 = *reinterpret_cast<const h8*>(hrow);            // positions 8q.. of K block 0 (hi plane)
            f.bh1 = *reinterpret_cast<const h8*>(hrow + 32);
            f.bl0 = *reinterpret_cast<const h8*>(hrow + 64);       // lo plane
            f.bl1 = *reinterpret_cast<const h8*>(hrow + 96);
            const _Float16* xrow = &xx[xb][16 * sg + n][0];
            f.xh = *reinterpret_cast<const h8*>(xrow + 8 * q);
            if (ANYLO) f.xl = *reinterpret_cast<const h8*>(xrow + 32 + 8 * q);
        };
        auto gemm = [&](const BFrag& f, f32x4* acc) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][0][0], f.bh0, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][0][1], f.bh0, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][0][0], f.bl0, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][1][0], f.bh1, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][1][1], f.bh1, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][1][0], f.bl1, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Wih[u][0], f.xh, acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Wih[u][1], f.xh, acc[u]);
            if (ANYLO) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Wih[u][0], f.xl, acc[u]);
            }
        };
        auto cell = [&](int sg, const f32x4* acc) {
            h4 nh, nl;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // gate rows are pre-scaled at pack time (i, f, o by -log2 e; g by 2 log2 e) and the cell state is kept
                // as c' = 2 log2(e) c, so every activation is exp2 -> add -> rcp on the accumulator itself
                const float ig = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][0]));
                const float fg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][1]));
                const float gk = __builtin_fmaf(-2.0f * RS_K, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][2])), RS_K);   // K tanh(g)
                const float og = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][3]));
                const float cn = __builtin_fmaf(fg, c[4 * sg + u], ig * gk);
                c[4 * sg + u] = cn;
                const float h = og * __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(cn)), 1.0f);
                _Float16 hi, lo; split1(h, hi, lo);
                nh[u] = hi; nl[u] = lo;
            }
            *reinterpret_cast<h4*>(&hx[hw_][16 * sg + n][16 * wave + 4 * q]) = nh;
            *reinterpret_cast<h4*>(&hx[hw_][16 * sg + n][64 + 16 * wave + 4 * q]) = nl;
        };
        // software pipeline over the site groups: the MFMAs of group g+1 are issued among the sigmoid / tanh
        // work of group g (one scheduling region; the matrix pipe runs while the vector ALU issues)
        BFrag fr[2];
        f32x4 acc[2][4];
        load_b(0, fr[0]);
        if (NSG > 1) load_b(1, fr[1]);
        __builtin_amdgcn_sched_barrier(0);
        gemm(fr[0], acc[0]);
#pragma unroll
        for (int sg = 0; sg < NSG; ++sg) {
            // the fragment reads of group sg+2 are pinned to the top of the phase (their LDS latency hides behind
            // the whole phase); gemm(sg) which last used these registers was issued in the previous phase
            __builtin_amdgcn_sched_barrier(0);
            if (sg + 2 < NSG) load_b(sg + 2, fr[sg & 1]);
            __builtin_amdgcn_sched_barrier(0);
            if (sg + 1 < NSG) gemm(fr[(sg + 1) & 1], acc[(sg + 1) & 1]);
            cell(sg, acc[sg & 1]);
            if (sg + 1 < NSG) {
#pragma unroll
                for (int i = 0; i < (ANYLO ? 36 : 32); ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
                    __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);      // one transcendental   (cell of the previous
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);      // two other VALU        group; cell_rate probe)
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    for (int s = 0; s < PW; ++s) {
        const int t = dir ? PW - 1 - s : s;
        const int xb = s & 1;
        if (s + 1 < PW) load_x(dir ? t - 1 : t + 1);
        const bool any_lo = (xflag[xb][0] | xflag[xb][1] | xflag[xb][2] | xflag[xb][3]) != 0;
        if (s > 0) flush_h((s & 1) ^ 1, dir ? t + 1 : t - 1);
        if (any_lo) step(std::true_type{}, t, xb, s & 1);
        else        step(std::false_type{}, t, xb, s & 1);
        if (s + 1 < PW) stage_x(xb ^ 1);
        lds_barrier();
    }
    flush_h((PW - 1) & 1, dir ? 0 : PW - 1);
}

// ---------------------------------------------------------------------------------------------
// K2: layer-1 input projection.  LDS: W_ih1 image 128 KB ([16][4][2][64] h8) + fp32 bias image 4 KB.
// ---------------------------------------------------------------------------------------------
constexpr int P1H_W_H8 = 16 * 4 * 2 * 64;
constexpr int P1H_LDS_BYTES = P1H_W_H8 * 16 + 16 * 64 * 16;

__global__ __launch_bounds__(1024, 4) void k_pileup_proj1_h(
    const _Float16* __restrict__ H0, int64_t N,
    const _Float16* __restrict__ w0, const _Float16* __restrict__ w1,
    const float* __restrict__ b0, const float* __restrict__ b1,
    float* __restrict__ Xp1)
{
    extern __shared__ h8 ldsh[];
    f32x4* lbias = reinterpret_cast<f32x4*>(ldsh + P1H_W_H8);
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    copy_to_lds_h(ldsh, dir ? w1 : w0, P1H_W_H8, tid, 1024);
    {
        const f32x4* sb = reinterpret_cast<const f32x4*>(dir ? b1 : b0);
        for (int i = tid; i < 16 * 64; i += 1024) lbias[i] = sb[i];
    }
    __syncthreads();
    const int64_t M = N * PSTEPS1;
    const int64_t n_rt = NSNP_CDIV(M, 16);
    float* __restrict__ out = Xp1 + (int64_t)dir * M * 256;
    for (int64_t rt = (int64_t)blockIdx.x * 16 + wave; rt < n_rt; rt += (int64_t)gridDim.x * 16) {
        const int64_t m = rt * 16 + (lane & 15);
        const bool live = m < M;
        const int64_t mc = live ? m : M - 1;
        const int64_t site = mc / PSTEPS1;
        const int u = (int)(mc - site * PSTEPS1);
        const int t = dir ? PW - 1 - u : u;
        // K block kb = (source direction d', half): hi at [d'][q][half*8..], lo 16 halfs further
        const h8* __restrict__ hin = reinterpret_cast<const h8*>(H0 + ((site * PW + t) * 2 * 4 + q) * 32);
        h8 bh[4], bl[4];
#pragma unroll
        for (int dp = 0; dp < 2; ++dp)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                bh[dp * 2 + half] = hin[dp * 16 + half];          // 4 q-blocks x 4 h8 per direction
                bl[dp * 2 + half] = hin[dp * 16 + 2 + half];
            }
        f32x4* o = reinterpret_cast<f32x4*>(out + mc * 256 + q * 4);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            f32x4 acc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = lbias[(hf * 8 + i) * 64 + lane];
            if (hf == 0) wave_gemm_h<8, 4, 0, 4, 0, 4>(ldsh, lane, bh, bl, acc);
            else         wave_gemm_h<8, 4, 0, 4, 8, 4>(ldsh, lane, bh, bl, acc);
            if (live) {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[(hf * 8 + i) * 4] = acc[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K3: layer-1 recurrence, 17 steps; LDS: W_hh1 image 64 KB.  H1c: [site][dir][q][16 hi | 16 lo] fp16.
// ---------------------------------------------------------------------------------------------
constexpr int L1H_LDS_BYTES = HH_H8 * 16;

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES, (WAVES >= 8 ? 4 : (WAVES == 4 ? 2 : 1))) void k_pileup_l1_h(
    const float* __restrict__ Xp1, int64_t N,
    const _Float16* __restrict__ whh0, const _Float16* __restrict__ whh1,
    _Float16* __restrict__ H1c)
{
    extern __shared__ h8 ldsh[];
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    copy_to_lds_h(ldsh, dir ? whh1 : whh0, HH_H8, tid, 64 * WAVES);
    __syncthreads();
    const int64_t site = (int64_t)blockIdx.x * (16 * WAVES) + wave * 16 + (lane & 15);
    const bool live = site < N;
    const int64_t sc = live ? site : N - 1;
    const int64_t M = N * PSTEPS1;
    const f32x4* __restrict__ xin =
        reinterpret_cast<const f32x4*>(Xp1 + ((int64_t)dir * M + sc * PSTEPS1) * 256 + q * 4);
    float c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = 0.f;
    h8 bh[2], bl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) { bh[k][j] = (_Float16)0.f; bl[k][j] = (_Float16)0.f; }
    for (int u = 0; u < PSTEPS1; ++u) {
        h8 nh[2], nl[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            f32x4 acc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = xin[(int64_t)u * 64 + (hf * 8 + i) * 4];
            if (u > 0) {
                if (hf == 0) wave_gemm_h<8, 2, 0, 2, 0, 2>(ldsh, lane, bh, bl, acc);
                else         wave_gemm_h<8, 2, 0, 2, 8, 2>(ldsh, lane, bh, bl, acc);
            }
            lstm_pointwise8_h(acc, c + hf * 8, nh[hf], nl[hf]);
        }
        bh[0] = nh[0]; bh[1] = nh[1]; bl[0] = nl[0]; bl[1] = nl[1];
    }
    if (live) {
        h8* o = reinterpret_cast<h8*>(H1c + ((site * 2 + dir) * 4 + q) * 32);
        o[0] = bh[0]; o[1] = bh[1]; o[2] = bl[0]; o[3] = bl[1];
    }
}

// ---------------------------------------------------------------------------------------------
// K23: layer-1 input projection FUSED into the layer-1 recurrence (no Xp1 round trip through HBM:
// 70 KB/site less traffic).  One 16-wave workgroup per CU keeps in LDS the recurrent image (64 KB), the
// hi half of the input image (64 KB) and a compact bias table (1 KB); the lo half of the input image
// (64 KB) is streamed from L2 through a two-slot LDS ring, 8 KB (two gate tiles) per chunk, one
// workgroup barrier per chunk.  Arithmetic and summation order are those of K2 followed by K3.
// ---------------------------------------------------------------------------------------------
constexpr int L1F_IHI_H8 = 16 * 4 * 64;                 // hi half of the input image  [tile][kb][lane]
constexpr int L1F_CHUNK_H8 = 2 * 4 * 64;                // one ring chunk: 2 tiles x 4 K blocks
constexpr int L1F_OFF_IHI = HH_H8;
constexpr int L1F_OFF_RING = HH_H8 + L1F_IHI_H8;
constexpr int L1F_OFF_BIAS = L1F_OFF_RING + 2 * L1F_CHUNK_H8;      // then 64 f32x4 of bias
constexpr int L1F_LDS_BYTES = (L1F_OFF_BIAS) * 16 + 64 * 16;

// WAVES = 4 / 8 / 12 waves of 16 sites per workgroup (one workgroup per CU by LDS), picked from the batch.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES, (WAVES + 3) / 4) void k_pileup_l1f_h(
    const _Float16* __restrict__ H0, int64_t N,
    const _Float16* __restrict__ whh0, const _Float16* __restrict__ whh1,
    const _Float16* __restrict__ ihi0, const _Float16* __restrict__ ihi1,
    const _Float16* __restrict__ ilo0, const _Float16* __restrict__ ilo1,
    const float* __restrict__ bias0, const float* __restrict__ bias1,
    _Float16* __restrict__ H1c)
{
    extern __shared__ h8 ldsh[];
    constexpr int NT = 64 * WAVES;
    constexpr int NP = (L1F_CHUNK_H8 + NT - 1) / NT;        // ring pieces (16 B) each thread moves per chunk
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    copy_to_lds_h(ldsh, dir ? whh1 : whh0, HH_H8, tid, NT);
    copy_to_lds_h(ldsh + L1F_OFF_IHI, dir ? ihi1 : ihi0, L1F_IHI_H8, tid, NT);
    const h8* __restrict__ ilo = reinterpret_cast<const h8*>(dir ? ilo1 : ilo0);       // [8 chunks][512] h8
    f32x4* lbias = reinterpret_cast<f32x4*>(ldsh + L1F_OFF_BIAS);                      // [tile][q]
    if (tid < 64) lbias[tid] = reinterpret_cast<const f32x4*>(dir ? bias1 : bias0)[tid];
    // ring: chunk c lives in slot c & 1.  The piece of chunk c+2 is requested at the start of chunk c, held in
    // registers across two chunks and written to LDS at the end of chunk c+1 (two chunks of latency hiding).
    h8 pc[2][NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int e = tid + k * NT;
        if (e < L1F_CHUNK_H8) { ldsh[L1F_OFF_RING + e] = ilo[e]; pc[1][k] = ilo[L1F_CHUNK_H8 + e]; }
    }
    __syncthreads();

    const int64_t site = (int64_t)blockIdx.x * (16 * WAVES) + wave * 16 + (lane & 15);
    const bool live = site < N;
    const int64_t sc = live ? site : N - 1;
    float c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = 0.f;
    h8 bh[2], bl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) { bh[k][j] = (_Float16)0.f; bl[k][j] = (_Float16)0.f; }

    for (int u = 0; u < PSTEPS1; ++u) {
        const int t = dir ? PW - 1 - u : u;
        const h8* __restrict__ hin = reinterpret_cast<const h8*>(H0 + ((sc * PW + t) * 2 * 4 + q) * 32);
        h8 gh[4], gl[4];
#pragma unroll
        for (int dp = 0; dp < 2; ++dp)
#pragma unroll
            for (int half = 0; half < 2; ++half) { gh[dp * 2 + half] = hin[dp * 16 + half]; gl[dp * 2 + half] = hin[dp * 16 + 2 + half]; }
        h8 nh[2], nl[2];
#define CHUNK(C)                                                                                                 \
        {                                                                                                        \
            PIN();                                                                                               \
            _Pragma("unroll") for (int k = 0; k < NP; ++k) {                                                     \
                const int e = tid + k * NT;                                                                      \
                if (e < L1F_CHUNK_H8) pc[(C) & 1][k] = ilo[(((C) + 2) & 7) * L1F_CHUNK_H8 + e];                  \
            }                                                                                                    \
            f32x4 acc[2];                                                                                        \
            acc[0] = lbias[(2 * (C)) * 4 + q]; acc[1] = lbias[(2 * (C) + 1) * 4 + q];                            \
            const h8* ring = ldsh + L1F_OFF_RING + ((C) & 1) * L1F_CHUNK_H8;                                     \
            h8 ah[2][2], al[2][2];                                                                               \
            _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) {                                                   \
                ah[0][tt] = ldsh[L1F_OFF_IHI + ((2 * (C) + tt) * 4 + 0) * 64 + lane];                            \
                al[0][tt] = ring[(tt * 4 + 0) * 64 + lane];                                                      \
            }                                                                                                    \
            _Pragma("unroll") for (int kb = 0; kb < 4; ++kb) {                                                   \
                if (kb + 1 < 4) {                                                                                \
                    _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) {                                           \
                        ah[(kb + 1) & 1][tt] = ldsh[L1F_OFF_IHI + ((2 * (C) + tt) * 4 + kb + 1) * 64 + lane];    \
                        al[(kb + 1) & 1][tt] = ring[(tt * 4 + kb + 1) * 64 + lane];                              \
                    }                                                                                            \
                }                                                                                                \
                _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) acc[tt] = mfma_h(ah[kb & 1][tt], gh[kb], acc[tt]); \
                _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) acc[tt] = mfma_h(al[kb & 1][tt], gh[kb], acc[tt]); \
                _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) acc[tt] = mfma_h(ah[kb & 1][tt], gl[kb], acc[tt]); \
                PIN();                                                                                           \
            }                                                                                                    \
            wave_gemm_h<2, 2, 0, 2, 2 * (C), 2>(ldsh, lane, bh, bl, acc); /* h = 0 at u = 0: adds nothing */   \
            _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) {                                                   \
                const int i = 2 * (C) + tt;                                                                      \
                const float ig = sigmoid_f(acc[tt][0]);                                                          \
                const float fg = sigmoid_f(acc[tt][1]);                                                          \
                const float gg = tanh_f(acc[tt][2]);                                                             \
                const float og = sigmoid_f(acc[tt][3]);                                                          \
                c[i] = __builtin_fmaf(fg, c[i], ig * gg);                                                        \
                const float h = og * tanh_f(c[i]);                                                               \
                _Float16 hi, lo;                                                                                 \
                split1(h, hi, lo);                                                                               \
                nh[i >> 3][i & 7] = hi; nl[i >> 3][i & 7] = lo;                                                  \
            }                                                                                                    \
            _Pragma("unroll") for (int k = 0; k < NP; ++k) {                                                     \
                const int e = tid + k * NT;                                                                      \
                if (e < L1F_CHUNK_H8) ldsh[L1F_OFF_RING + (((C) + 1) & 1) * L1F_CHUNK_H8 + e] = pc[((C) + 1) & 1][k]; \
            }                                                                                                    \
            lds_barrier();   /* LDS only: __syncthreads() would also drain the ring prefetch (vmcnt) */             \
        }
        CHUNK(0) CHUNK(1) CHUNK(2) CHUNK(3) CHUNK(4) CHUNK(5) CHUNK(6) CHUNK(7)
#undef CHUNK
        bh[0] = nh[0]; bh[1] = nh[1]; bl[0] = nl[0]; bl[1] = nl[1];
    }
    if (live) {
        h8* o = reinterpret_cast<h8*>(H1c + ((site * 2 + dir) * 4 + q) * 32);
        o[0] = bh[0]; o[1] = bh[1]; o[2] = bl[0]; o[3] = bl[1];
    }
}

// ---------------------------------------------------------------------------------------------
// K23r: layer 1 (input projection + recurrence) with REGISTER-STATIONARY weights, the counterpart of K1r.
// One workgroup = 8 waves x 64 sites; wave w owns gate tiles 2w, 2w+1 (hidden units 8w..8w+7, all four gates) and keeps
// their W_ih1 (K = 128) and W_hh1 (K = 64) hi+lo fragments in 96 VGPRs, so nothing is streamed through an LDS ring and
// a step needs ONE workgroup barrier instead of eight.  LDS holds only operands: h0_t of the 64 sites (512 B rows copied
// from H0 one step ahead, double-buffered) and the h1 exchange rows (64 hi | 64 lo halves; K position p = 8w + 2q + u
// <-> unit 4(2w+u) + q, the two units lane (site, q) of wave w leaves the cell with).  A step is 24 "pieces" per wave
// (4 site groups x (4 input + 2 recurrent K blocks)), each piece one hi and one lo fragment from LDS and 6 MFMAs,
// requested two pieces ahead.  Gate rows are pre-scaled by log2 e as in K1r.
// ---------------------------------------------------------------------------------------------
constexpr int R1_H0ROW = 264;                // halves per staged h0 row: [dir][q][16 hi | 16 lo] = 512 B + 16 B pad
constexpr int R1_HROW = 136;                 // halves per h1 exchange row: 64 hi | 64 lo | pad
constexpr int r1_lds_bytes(int nsg) { return 2 * 16 * nsg * R1_H0ROW * 2 + 2 * 16 * nsg * R1_HROW * 2; }

template <int NSG>          // 16-site groups per workgroup: 4 (64 sites) or 2 (32 sites, small batches)
__global__ __launch_bounds__(512, 2) void k_pileup_l1_rs(
    const _Float16* __restrict__ H0 /* padded to a multiple of 64 sites */, int64_t N,
    const _Float16* __restrict__ wih0, const _Float16* __restrict__ wih1,
    const _Float16* __restrict__ whh0, const _Float16* __restrict__ whh1,
    const float* __restrict__ bias0, const float* __restrict__ bias1,
    _Float16* __restrict__ H1c /* padded likewise */, int prio)
{
    extern __shared__ h8 ldsh[];
    _Float16* const h0s = reinterpret_cast<_Float16*>(ldsh);                       // [2][64][R1_H0ROW]
    constexpr int NS = 16 * NSG;                                                    // sites per workgroup
    _Float16* const h1x = h0s + 2 * NS * R1_H0ROW;                                 // [2][NS][R1_HROW]
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int64_t base_site = (int64_t)blockIdx.x * NS;
    if (prio && wave >= 4) __builtin_amdgcn_s_setprio(1);       // static priority for the younger half (MI355X_MICROARCH.md, 'Two waves per SIMD' item 4)

    // ---- this wave's two gate tiles -> registers ---------------------------------------------------
    h8 Wih[2][4][2], Whh[2][2][2];
    f32x4 bias[2];
    {
        const h8* __restrict__ gih = reinterpret_cast<const h8*>(dir ? wih1 : wih0);        // [tile][kb 4][part][lane]
        const h8* __restrict__ ghh = reinterpret_cast<const h8*>(dir ? whh1 : whh0);        // [tile][kb 2][part][lane]
        const f32x4* __restrict__ gb = reinterpret_cast<const f32x4*>(dir ? bias1 : bias0);  // [tile][q]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int part = 0; part < 2; ++part) Wih[u][kb][part] = gih[(((2 * wave + u) * 4 + kb) * 2 + part) * 64 + lane];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int part = 0; part < 2; ++part) Whh[u][kb][part] = ghh[(((2 * wave + u) * 2 + kb) * 2 + part) * 64 + lane];
            bias[u] = gb[(2 * wave + u) * 4 + q];
        }
    }

    // ---- h0 staging: 512 / NS threads per site row, each moves NS bytes (NS / 16 h8) of the 512-byte row ----
    constexpr int TPR = 512 / NS, SPT = NS / 16;                    // threads per row, h8 pieces per thread
    const int srow = tid / TPR, spiece = tid % TPR;
    const int64_t ssite = base_site + srow;                         // H0 is padded: rows beyond N hold garbage that only
    const h8* __restrict__ gsrc = reinterpret_cast<const h8*>(H0 + (ssite * PW) * (2 * 4 * 32)) + spiece * SPT;   // feeds dead sites
    h8 sreg[SPT];
    auto load_h0 = [&](int t) {
        const h8* p = gsrc + (int64_t)t * (2 * 4 * 32 / 8);
#pragma unroll
        for (int k = 0; k < SPT; ++k) sreg[k] = p[k];
    };
    auto store_h0 = [&](int buf) {
        h8* d = reinterpret_cast<h8*>(h0s + ((size_t)buf * NS + srow) * R1_H0ROW + spiece * SPT * 8);
#pragma unroll
        for (int k = 0; k < SPT; ++k) d[k] = sreg[k];
    };
    // h1_{-1} = 0 in the buffer step 0 reads
    for (int i = tid; i < NS * R1_HROW / 8; i += 512) reinterpret_cast<h8*>(h1x + (size_t)NS * R1_HROW)[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
    load_h0(dir ? PW - 1 : 0);
    store_h0(0);
    __syncthreads();

    float c[2 * NSG];
#pragma unroll
    for (int i = 0; i < 2 * NSG; ++i) c[i] = 0.f;
    h4 last_h[NSG];                                                   // [sg]: hi(u0,u1) lo(u0,u1) of the final step

    for (int s = 0; s < PSTEPS1; ++s) {
        const int t = dir ? PW - 1 - s : s;
        const int cur = s & 1;
        if (s + 1 < PSTEPS1) load_h0(dir ? t - 1 : t + 1);
        const _Float16* h0b = h0s + (size_t)cur * NS * R1_H0ROW;
        const _Float16* hrb = h1x + (size_t)(cur ^ 1) * NS * R1_HROW;      // h1_{s-1}
        _Float16* hwb = h1x + (size_t)cur * NS * R1_HROW;                  // h1_s

        // piece P = sg * 6 + k: k < 4 input K block k (dir = k >> 1, half = k & 1), k >= 4 recurrent K block k - 4
        h8 fh[3], fl[3];
        auto fetch = [&](int P, int slot) {
            const int sg = P / 6, k = P % 6;
            if (k < 4) {
                const _Float16* r = h0b + (size_t)(16 * sg + n) * R1_H0ROW + (k >> 1) * 128 + q * 32 + (k & 1) * 8;
                fh[slot] = *reinterpret_cast<const h8*>(r);
                fl[slot] = *reinterpret_cast<const h8*>(r + 16);
            } else {
                const _Float16* r = hrb + (size_t)(16 * sg + n) * R1_HROW + (k - 4) * 32 + q * 8;
                fh[slot] = *reinterpret_cast<const h8*>(r);
                fl[slot] = *reinterpret_cast<const h8*>(r + 64);
            }
        };
        fetch(0, 0);
        fetch(1, 1);
        f32x4 acc[2][2];
#pragma unroll
        for (int P = 0; P < 6 * NSG; ++P) {
            const int sg = P / 6, k = P % 6, slot = P % 3, ab = sg & 1;
            if (P + 2 < 6 * NSG) fetch(P + 2, (P + 2) % 3);
            if (k == 0) { acc[ab][0] = bias[0]; acc[ab][1] = bias[1]; }
            if (k < 4) {
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[ab][u] = mfma_h(Wih[u][k][0], fh[slot], acc[ab][u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[ab][u] = mfma_h(Wih[u][k][1], fh[slot], acc[ab][u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[ab][u] = mfma_h(Wih[u][k][0], fl[slot], acc[ab][u]);
            } else {
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[ab][u] = mfma_h(Whh[u][k - 4][0], fh[slot], acc[ab][u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[ab][u] = mfma_h(Whh[u][k - 4][1], fh[slot], acc[ab][u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[ab][u] = mfma_h(Whh[u][k - 4][0], fl[slot], acc[ab][u]);
            }
            if (k == 5) {
                // cell of site group sg: lane (n, q) holds units 4 (2 wave + u) + q, u = 0, 1
                _Float16 hi[2], lo[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float ig = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[ab][u][0]));
                    const float fg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[ab][u][1]));
                    const float gk = __builtin_fmaf(-2.0f * RS_K, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[ab][u][2])), RS_K);
                    const float og = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[ab][u][3]));
                    const float cn = __builtin_fmaf(fg, c[2 * sg + u], ig * gk);
                    c[2 * sg + u] = cn;
                    const float h = og * __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(cn)), 1.0f);
                    split1(h, hi[u], lo[u]);
                }
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                _Float16* w = hwb + (size_t)(16 * sg + n) * R1_HROW + 8 * wave + 2 * q;
                *reinterpret_cast<h2*>(w) = h2{hi[0], hi[1]};
                *reinterpret_cast<h2*>(w + 64) = h2{lo[0], lo[1]};
                last_h[sg] = h4{hi[0], hi[1], lo[0], lo[1]};
            }
        }
        if (s + 1 < PSTEPS1) store_h0(cur ^ 1);
        lds_barrier();
    }
    // H1c: [site][dir][q][16 hi | 16 lo], entries m = 2 wave + u of row q (the layout K3 / K23 write)
#pragma unroll
    for (int sg = 0; sg < NSG; ++sg) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        _Float16* o = H1c + (((base_site + 16 * sg + n) * 2 + dir) * 4 + q) * 32 + 2 * wave;
        *reinterpret_cast<h2*>(o) = h2{last_h[sg][0], last_h[sg][1]};
        *reinterpret_cast<h2*>(o + 16) = h2{last_h[sg][2], last_h[sg][3]};
    }
}

// ---------------------------------------------------------------------------------------------
// K23r4: the same layer-1 step with FOUR gate tiles per wave and four waves per workgroup (the shape of the fp32 kernel
// k_pileup_l1_rs4): wave w owns tiles 4w..4w+3, their W_ih1 and W_hh1 hi+lo fragments fill 192 VGPRs, a workgroup is one wave per
// SIMD and 16 sites, and the second wave of a SIMD belongs to ANOTHER workgroup with its own barrier - in the eight-wave kernel above
// both waves of a SIMD wait at the same barrier, and the matrix pipe idles 60 % of a step (39 % busy at N = 131072).  Every
// fragment read from LDS feeds 12 MFMAs instead of 6.  Same weight images, same exchange-row layout (K position 8 (T >> 1) + 2 q +
// (T & 1) <-> unit 4 T + q), same order of the six K blocks and three terms per accumulator: bit-identical results.
// ---------------------------------------------------------------------------------------------
constexpr int r1_lds_bytes4() { return 2 * 16 * R1_H0ROW * 2 + 2 * 16 * R1_HROW * 2 + 16 * 4 * 16; }

__global__ __launch_bounds__(256, 2) void k_pileup_l1_rs4_h(
    const _Float16* __restrict__ H0 /* padded to a multiple of 64 sites */, int64_t N,
    const _Float16* __restrict__ wih0, const _Float16* __restrict__ wih1,
    const _Float16* __restrict__ whh0, const _Float16* __restrict__ whh1,
    const float* __restrict__ bias0, const float* __restrict__ bias1,
    _Float16* __restrict__ H1c /* padded likewise */)
{
    extern __shared__ h8 ldsh[];
    constexpr int NS = 16;
    _Float16* const h0s = reinterpret_cast<_Float16*>(ldsh);                       // [2][16][R1_H0ROW]
    _Float16* const h1x = h0s + 2 * NS * R1_H0ROW;                                 // [2][16][R1_HROW]
    f32x4* const bls = reinterpret_cast<f32x4*>(h1x + 2 * NS * R1_HROW);           // [16 tiles][4 q] bias rows (registers are full)
    const int dir = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int64_t base_site = (int64_t)blockIdx.x * NS;

    h8 Wih[4][4][2], Whh[4][2][2];
    {
        const h8* __restrict__ gih = reinterpret_cast<const h8*>(dir ? wih1 : wih0);        // [tile][kb 4][part][lane]
        const h8* __restrict__ ghh = reinterpret_cast<const h8*>(dir ? whh1 : whh0);        // [tile][kb 2][part][lane]
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int part = 0; part < 2; ++part) Wih[u][kb][part] = gih[(((4 * wave + u) * 4 + kb) * 2 + part) * 64 + lane];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int part = 0; part < 2; ++part) Whh[u][kb][part] = ghh[(((4 * wave + u) * 2 + kb) * 2 + part) * 64 + lane];
        }
        if (tid < 64) bls[tid] = reinterpret_cast<const f32x4*>(dir ? bias1 : bias0)[tid];
    }
    const f32x4* const myb = bls + 16 * wave + q;                                   // + 4 u

    // h0 staging: 16 threads per site row, each moves 32 bytes of the 512-byte row
    constexpr int TPR = 256 / NS, SPT = 32 / TPR;
    const int srow = tid / TPR, spiece = tid % TPR;
    const int64_t ssite = base_site + srow;                         // H0 is padded: rows beyond N hold garbage that only feeds dead sites
    const h8* __restrict__ gsrc = reinterpret_cast<const h8*>(H0 + (ssite * PW) * (2 * 4 * 32)) + spiece * SPT;
    h8 sreg[SPT];
    auto load_h0 = [&](int t) {
        const h8* p = gsrc + (int64_t)t * (2 * 4 * 32 / 8);
#pragma unroll
        for (int k = 0; k < SPT; ++k) sreg[k] = p[k];
    };
    auto store_h0 = [&](int buf) {
        h8* d = reinterpret_cast<h8*>(h0s + ((size_t)buf * NS + srow) * R1_H0ROW + spiece * SPT * 8);
#pragma unroll
        for (int k = 0; k < SPT; ++k) d[k] = sreg[k];
    };
    for (int i = tid; i < NS * R1_HROW / 8; i += 256) reinterpret_cast<h8*>(h1x + (size_t)NS * R1_HROW)[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
    load_h0(dir ? PW - 1 : 0);
    store_h0(0);
    __syncthreads();

    float c[4] = {0.f, 0.f, 0.f, 0.f};
    h8 last_h = h8{0, 0, 0, 0, 0, 0, 0, 0};                            // hi(u0..u3) lo(u0..u3) of the final step

    for (int s = 0; s < PSTEPS1; ++s) {
        const int t = dir ? PW - 1 - s : s;
        const int cur = s & 1;
        if (s + 1 < PSTEPS1) load_h0(dir ? t - 1 : t + 1);
        const _Float16* h0r = h0s + ((size_t)cur * NS + n) * R1_H0ROW + q * 32;
        const _Float16* hrr = h1x + ((size_t)(cur ^ 1) * NS + n) * R1_HROW + q * 8;      // h1_{s-1}
        _Float16* hwr = h1x + ((size_t)cur * NS + n) * R1_HROW + 16 * wave + 2 * q;      // h1_s

        // piece k < 4: input K block k (dir = k >> 1, half = k & 1), k >= 4: recurrent K block k - 4; fetched one piece ahead
        h8 fh[2], fl[2];
        auto fetch = [&](int k, int slot) {
            if (k < 4) {
                const _Float16* r = h0r + (k >> 1) * 128 + (k & 1) * 8;
                fh[slot] = *reinterpret_cast<const h8*>(r);
                fl[slot] = *reinterpret_cast<const h8*>(r + 16);
            } else {
                const _Float16* r = hrr + (k - 4) * 32;
                fh[slot] = *reinterpret_cast<const h8*>(r);
                fl[slot] = *reinterpret_cast<const h8*>(r + 64);
            }
        };
        fetch(0, 0);
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = myb[4 * u];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int slot = k & 1;
            if (k + 1 < 6) fetch(k + 1, slot ^ 1);
            if (k < 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Wih[u][k][0], fh[slot], acc[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Wih[u][k][1], fh[slot], acc[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Wih[u][k][0], fl[slot], acc[u]);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][k - 4][0], fh[slot], acc[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][k - 4][1], fh[slot], acc[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma_h(Whh[u][k - 4][0], fl[slot], acc[u]);
            }
        }
        // cell: lane (n, q) holds units 4 (4 wave + u) + q, u = 0..3
        _Float16 hi[4], lo[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float ig = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][0]));
            const float fg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][1]));
            const float gk = __builtin_fmaf(-2.0f * RS_K, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][2])), RS_K);
            const float og = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[u][3]));
            const float cn = __builtin_fmaf(fg, c[u], ig * gk);
            c[u] = cn;
            const float h = og * __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(cn)), 1.0f);
            split1(h, hi[u], lo[u]);
        }
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<h2*>(hwr) = h2{hi[0], hi[1]};                     // tiles 4w, 4w+1: positions 16 w + 2 q + {0, 1}
        *reinterpret_cast<h2*>(hwr + 8) = h2{hi[2], hi[3]};                 // tiles 4w+2, 4w+3: positions 16 w + 8 + 2 q + {0, 1}
        *reinterpret_cast<h2*>(hwr + 64) = h2{lo[0], lo[1]};
        *reinterpret_cast<h2*>(hwr + 72) = h2{lo[2], lo[3]};
        last_h = h8{hi[0], hi[1], hi[2], hi[3], lo[0], lo[1], lo[2], lo[3]};
        if (s + 1 < PSTEPS1) store_h0(cur ^ 1);
        lds_barrier();
    }
    // H1c: [site][dir][q][16 hi | 16 lo], entries m = 4 wave + u of row q
    {
        _Float16* o = H1c + (((base_site + n) * 2 + dir) * 4 + q) * 32 + 4 * wave;
        *reinterpret_cast<h4*>(o) = h4{last_h[0], last_h[1], last_h[2], last_h[3]};
        *reinterpret_cast<h4*>(o + 16) = h4{last_h[4], last_h[5], last_h[6], last_h[7]};
    }
}

// ---------------------------------------------------------------------------------------------
// K4: heads, weights from L2 as fp16 hi/lo images.
// ---------------------------------------------------------------------------------------------
// HW waves of 16 sites per workgroup share every weight image through one 64 KB LDS stage (proj, dense rows 0-127,
// dense rows 128-255, heads): the images leave L2 once per workgroup instead of once per wave.
constexpr int HEAD_WAVES = 8;
constexpr int HEAD_STAGE_H8 = 8 * 4 * 2 * 64;           // 64 KB: 8 gate tiles x 4 K blocks x (hi, lo)
__global__ __launch_bounds__(64 * HEAD_WAVES) void k_pileup_head_h(
    const _Float16* __restrict__ H1c, int64_t N,
    const _Float16* __restrict__ proj_w, const float* __restrict__ proj_b,
    const _Float16* __restrict__ dense_w, const float* __restrict__ dense_b,
    const _Float16* __restrict__ head_w, const float* __restrict__ head_b,
    float* __restrict__ gt_prob, float* __restrict__ zy_prob)
{
    __shared__ h8 wst[HEAD_STAGE_H8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    const int64_t site = ((int64_t)blockIdx.x * HEAD_WAVES + wave) * 16 + (lane & 15);
    const bool live = site < N;
    const int64_t sc = live ? site : N - 1;
    auto stage = [&](const _Float16* src, int n_h8) {
        __syncthreads();                                   // everyone is done with the previous image
        copy_to_lds_h(wst, src, n_h8, tid, 64 * HEAD_WAVES);
        __syncthreads();
    };
    const h8* __restrict__ hin = reinterpret_cast<const h8*>(H1c + (sc * 2 * 4 + q) * 32);
    h8 bh[4], bl[4];
#pragma unroll
    for (int dp = 0; dp < 2; ++dp)
#pragma unroll
        for (int half = 0; half < 2; ++half) { bh[dp * 2 + half] = hin[dp * 16 + half]; bl[dp * 2 + half] = hin[dp * 16 + 2 + half]; }
    // output_proj 128 -> 128
    f32x4 ap[8];
    {
        const f32x4* pb = reinterpret_cast<const f32x4*>(proj_b);
#pragma unroll
        for (int i = 0; i < 8; ++i) ap[i] = pb[i * 64 + lane];
        stage(proj_w, 8 * 4 * 2 * 64);
        wave_gemm_h<8, 4, 0, 4, 0, 4>(wst, lane, bh, bl, ap);
    }
    // dense 128 -> 256 + tanh: K position (kb, q, j) <-> proj feature 16*(2kb + (j>>2)) + 4q + (j&3)
    h8 dh[4], dl[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) { _Float16 hi, lo; split1(ap[2 * kb + (j >> 2)][j & 3], hi, lo); dh[kb][j] = hi; dl[kb][j] = lo; }
    f32x4 ad[16];
    {
        const f32x4* db = reinterpret_cast<const f32x4*>(dense_b);
#pragma unroll
        for (int i = 0; i < 16; ++i) ad[i] = db[i * 64 + lane];
        stage(dense_w, 8 * 4 * 2 * 64);
        wave_gemm_h<8, 4, 0, 4, 0, 4>(wst, lane, dh, dl, ad);
        stage(dense_w + (size_t)8 * 4 * 2 * 64 * 8, 8 * 4 * 2 * 64);
        wave_gemm_h<8, 4, 0, 4, 0, 4>(wst, lane, dh, dl, ad + 8);
    }
    h8 eh[8], el[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) { _Float16 hi, lo; split1(tanh_f(ad[2 * kb + (j >> 2)][j & 3]), hi, lo); eh[kb][j] = hi; el[kb][j] = lo; }
    f32x4 ah[2];
    {
        const f32x4* hb = reinterpret_cast<const f32x4*>(head_b);
        ah[0] = hb[lane]; ah[1] = hb[64 + lane];
        stage(head_w, 2 * 8 * 2 * 64);
        wave_gemm_h<2, 8, 0, 8, 0, 2>(wst, lane, eh, el, ah);
    }
    const float NEG = -3.0e38f;
    float g0[4], g1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        g0[g] = ah[0][g];
        const bool is_gt = (q == 0) || (q == 1 && g == 0);
        g1[g] = is_gt ? ah[1][g] : NEG;
    }
    float mx = fmaxf(fmaxf(fmaxf(g0[0], g0[1]), fmaxf(g0[2], g0[3])), fmaxf(fmaxf(g1[0], g1[1]), fmaxf(g1[2], g1[3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float e0[4], e1[4], sum = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        e0[g] = __expf(g0[g] - mx);
        e1[g] = g1[g] > -1.0e38f ? __expf(g1[g] - mx) : 0.f;
        sum += e0[g] + e1[g];
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float z1 = ah[1][1], z2 = ah[1][2], z3 = ah[1][3];
    const float zm = fmaxf(z1, fmaxf(z2, z3));
    const float ez1 = __expf(z1 - zm), ez2 = __expf(z2 - zm), ez3 = __expf(z3 - zm);
    const float zs = ez1 + ez2 + ez3;
    if (live) {
        float* gp = gt_prob + site * NSNP_GT_CLASSES;
#pragma unroll
        for (int g = 0; g < 4; ++g) gp[4 * q + g] = e0[g] / sum;
        if (q == 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) gp[16 + g] = e1[g] / sum;
        }
        if (q == 1) {
            gp[20] = e1[0] / sum;
            float* zp = zy_prob + site * NSNP_ZY_CLASSES;
            zp[0] = ez1 / zs; zp[1] = ez2 / zs; zp[2] = ez3 / zs;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K4e: scoring heads.  k_pileup_head_h up to its last product (restated: the same H1c, splits, staged images, K order and MFMA
// chains), then the head product over the six tiles of the 90-row image instead of two.  The image is 96 KB and the stage 64 KB, so it
// comes in two pieces (tiles 0..3, tiles 4..5); every accumulator runs kb = 0..7 with the three products of wave_gemm_h<2, 8, .., 2>, so
// tiles 0 and 1 hold the bits k_pileup_head_h takes its softmax from.  The 90 logits of a wave's 16 sites then meet in LDS (the stage,
// free behind a barrier: 51.5 KB) and the tail is k_pileup_head_eval's (nsnp_eval_tail.hpp).
// LDS: the 64 KB stage + 10.5 KB of 32-bit confusion counters that leave once per workgroup.
// ---------------------------------------------------------------------------------------------
constexpr int HEAD_EVAL_LDS_BYTES = HEAD_STAGE_H8 * 16 + nsnp_eval::COUNTERS * 4;
static_assert(HEAD_WAVES * nsnp_eval::Z_WAVE * 4 <= HEAD_STAGE_H8 * 16, "the logit exchange fits the stage");

__global__ __launch_bounds__(64 * HEAD_WAVES) void k_pileup_head_eval_h(
    const _Float16* __restrict__ H1c, int64_t N,
    const _Float16* __restrict__ proj_w, const float* __restrict__ proj_b,
    const _Float16* __restrict__ dense_w, const float* __restrict__ dense_b,
    const _Float16* __restrict__ head6_w, const float* __restrict__ head6_b,
    const uint8_t* __restrict__ cls, float* __restrict__ site_loss, uint8_t* __restrict__ pred,
    unsigned long long* __restrict__ counters, float* __restrict__ logits)
{
    extern __shared__ h8 lds_he[];
    h8* const wst = lds_he;
    unsigned int* const cnt = reinterpret_cast<unsigned int*>(lds_he + HEAD_STAGE_H8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t site0 = ((int64_t)blockIdx.x * HEAD_WAVES + wave) * 16;
    const int64_t site = site0 + (lane & 15);
    const int64_t sc = site < N ? site : N - 1;
    for (int i = tid; i < nsnp_eval::COUNTERS; i += 64 * HEAD_WAVES) cnt[i] = 0;       // (first read behind the barriers below)
    const int q = lane >> 4;
    // ---- k_pileup_head_h to the letter up to the head product ----
    auto stage = [&](const _Float16* src, int n_h8) {
        __syncthreads();                                   // everyone is done with the previous image
        copy_to_lds_h(wst, src, n_h8, tid, 64 * HEAD_WAVES);
        __syncthreads();
    };
    const h8* __restrict__ hin = reinterpret_cast<const h8*>(H1c + (sc * 2 * 4 + q) * 32);
    h8 bh[4], bl[4];
#pragma unroll
    for (int dp = 0; dp < 2; ++dp)
#pragma unroll
        for (int half = 0; half < 2; ++half) { bh[dp * 2 + half] = hin[dp * 16 + half]; bl[dp * 2 + half] = hin[dp * 16 + 2 + half]; }
    // output_proj 128 -> 128
    f32x4 ap[8];
    {
        const f32x4* pb = reinterpret_cast<const f32x4*>(proj_b);
#pragma unroll
        for (int i = 0; i < 8; ++i) ap[i] = pb[i * 64 + lane];
        stage(proj_w, 8 * 4 * 2 * 64);
        wave_gemm_h<8, 4, 0, 4, 0, 4>(wst, lane, bh, bl, ap);
    }
    // dense 128 -> 256 + tanh: K position (kb, q, j) <-> proj feature 16*(2kb + (j>>2)) + 4q + (j&3)
    h8 dh[4], dl[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) { _Float16 hi, lo; split1(ap[2 * kb + (j >> 2)][j & 3], hi, lo); dh[kb][j] = hi; dl[kb][j] = lo; }
    f32x4 ad[16];
    {
        const f32x4* db = reinterpret_cast<const f32x4*>(dense_b);
#pragma unroll
        for (int i = 0; i < 16; ++i) ad[i] = db[i * 64 + lane];
        stage(dense_w, 8 * 4 * 2 * 64);
        wave_gemm_h<8, 4, 0, 4, 0, 4>(wst, lane, dh, dl, ad);
        stage(dense_w + (size_t)8 * 4 * 2 * 64 * 8, 8 * 4 * 2 * 64);
        wave_gemm_h<8, 4, 0, 4, 0, 4>(wst, lane, dh, dl, ad + 8);
    }
    h8 eh[8], el[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) { _Float16 hi, lo; split1(tanh_f(ad[2 * kb + (j >> 2)][j & 3]), hi, lo); eh[kb][j] = hi; el[kb][j] = lo; }
    f32x4 ah[6];
    {
        const f32x4* hb = reinterpret_cast<const f32x4*>(head6_b);     // [tile][lane], the accumulator image of the fp32 family
#pragma unroll
        for (int t = 0; t < 6; ++t) ah[t] = hb[t * 64 + lane];
        constexpr int PAIR_H8 = 2 * 8 * 2 * 64;                        // two tiles: the whole image of k_pileup_head_h
        stage(head6_w, 2 * PAIR_H8);
        wave_gemm_h<2, 8, 0, 8, 0, 2>(wst, lane, eh, el, ah);
        wave_gemm_h<2, 8, 0, 8, 2, 2>(wst, lane, eh, el, ah + 2);
        stage(head6_w + (size_t)2 * PAIR_H8 * 8, PAIR_H8);
        wave_gemm_h<2, 8, 0, 8, 0, 2>(wst, lane, eh, el, ah + 4);
    }
    __syncthreads();                                       // everyone is done with the weights: the stage becomes the logit exchange
    float* const zw = reinterpret_cast<float*>(wst) + wave * nsnp_eval::Z_WAVE;
    nsnp_eval::put_logits(zw, lane, ah);
    __syncthreads();
    nsnp_eval::wave_tail(zw, lane, site0, N, cls, site_loss, pred, cnt, logits);
    if (cls) {
        __syncthreads();
        nsnp_eval::flush_counters(cnt, counters, tid, 64 * HEAD_WAVES);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side: fp16 hi/lo weight images
// ---------------------------------------------------------------------------------------------
namespace {

inline int gate_row(int row) { const int i = row >> 4, r = row & 15; return (r & 3) * PH + 4 * i + (r >> 2); }

// img[tile][kb][part][lane][j]  <-  f(row = 16*tile + (lane & 15), kb, q = lane >> 4, j)
template <typename F>
void pack_h(_Float16* img, int n_tiles, int n_kb, F f)
{
    for (int tile = 0; tile < n_tiles; ++tile)
        for (int kb = 0; kb < n_kb; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const float v = f(16 * tile + (lane & 15), kb, lane >> 4, j);
                    const _Float16 hi = (_Float16)v;
                    const _Float16 lo = (_Float16)(v - (float)hi);
                    const size_t e = (((size_t)tile * n_kb + kb) * 2) * 64 + lane;
                    img[e * 8 + j] = hi;
                    img[(e + 64) * 8 + j] = lo;
                }
}

}  // namespace

int nsnp_pileup_pack_weights_f16(nsnp_ctx* ctx, const float* const* w)
{
    PileupWeightsF16& pw = ctx->pw16;
    const size_t n_hh = (size_t)HH_H8 * 8, n_ih = (size_t)IH_H8 * 8 * 2, n_p1 = (size_t)P1H_W_H8 * 8;
    const size_t n_proj = (size_t)8 * 4 * 2 * 64 * 8, n_dense = (size_t)16 * 4 * 2 * 64 * 8, n_head = (size_t)2 * 8 * 2 * 64 * 8;
    const size_t n_fhi = (size_t)L1F_IHI_H8 * 8, n_flo = (size_t)8 * L1F_CHUNK_H8 * 8;     // fused-kernel images
    const size_t total = 2 * (n_hh + n_ih + n_p1 + n_hh + n_fhi + n_flo + n_hh + n_ih + n_p1 + n_hh) + n_proj + n_dense + n_head;
    std::vector<_Float16> host(total);
    size_t off = 0;
    auto take = [&](size_t n) { _Float16* p = host.data() + off; off += n; return p; };
    _Float16 *l0_hh[2], *l0_ih[2], *l1_ih[2], *l1_hh[2];
    _Float16 *f_hi[2], *f_lo[2], *l0_rs[2], *l0_rs_ih[2], *l1_rs_ih[2], *l1_rs_hh[2];
    for (int d = 0; d < 2; ++d) { l0_rs[d] = take(n_hh); l0_rs_ih[d] = take(n_ih); l1_rs_ih[d] = take(n_p1); l1_rs_hh[d] = take(n_hh); l0_hh[d] = take(n_hh); l0_ih[d] = take(n_ih); l1_ih[d] = take(n_p1); l1_hh[d] = take(n_hh); f_hi[d] = take(n_fhi); f_lo[d] = take(n_flo); }
    _Float16* proj = take(n_proj); _Float16* dense = take(n_dense); _Float16* head = take(n_head);
    auto rec_feat = [](int kb, int q, int j) { return 4 * (8 * kb + j) + q; };                     // hidden unit
    auto h0_feat = [](int kb, int q, int j) { return (kb >> 1) * 64 + 4 * (8 * (kb & 1) + j) + q; };   // [fwd;bwd] feature
    auto acc_feat = [](int kb, int q, int j) { return 16 * (2 * kb + (j >> 2)) + 4 * q + (j & 3); };
    // register-stationary layer 0: B fragment (kb, q, j) = exchange position p = 32kb + 8q + j <-> unit 16 (p >> 4) + 4 (p & 3) + ((p >> 2) & 3)
    auto rs_feat = [](int kb, int q, int j) { const int p = 32 * kb + 8 * q + j; return 16 * (p >> 4) + 4 * (p & 3) + ((p >> 2) & 3); };
    for (int d = 0; d < 2; ++d) {
        const float* const* l0 = w + d * 4;
        const float* const* l1 = w + 8 + d * 4;
        // K1r images: gate rows pre-scaled so that the cell applies exp2 directly (image row r: gate r & 3)
        auto gscale = [](int row) { return (row & 3) == 2 ? 2.0f * LOG2E : -LOG2E; };
        pack_h(l0_rs[d], 16, 2, [&](int row, int kb, int q, int j) { return gscale(row) * l0[1][gate_row(row) * PH + rs_feat(kb, q, j)]; });
        pack_h(l0_rs_ih[d], 16, 1, [&](int row, int, int q, int j) {
            const int tr = gate_row(row);
            if (q < 2) return gscale(row) * l0[0][tr * PC + 8 * q + j];
            if (q == 2) { if (j < 2) return gscale(row) * l0[0][tr * PC + 16 + j]; if (j == 2) return gscale(row) * (l0[2][tr] + l0[3][tr]); }
            return 0.f;
        });
        pack_h(l0_hh[d], 16, 2, [&](int row, int kb, int q, int j) { return l0[1][gate_row(row) * PH + rec_feat(kb, q, j)]; });
        // input image: [tile][part][lane] (one K block): split the generic [tile][kb=1][part] layout
        pack_h(l0_ih[d], 16, 1, [&](int row, int, int q, int j) {
            const int tr = gate_row(row);
            if (q < 2) return l0[0][tr * PC + 8 * q + j];
            if (q == 2) { if (j < 2) return l0[0][tr * PC + 16 + j]; if (j == 2) return l0[2][tr] + l0[3][tr]; }
            return 0.f;
        });
        pack_h(l1_ih[d], 16, 4, [&](int row, int kb, int q, int j) { return l1[0][gate_row(row) * 2 * PH + h0_feat(kb, q, j)]; });
        // K23r images: the same input image and a recurrent image in the K order of its exchange rows, both pre-scaled
        auto r1_feat = [](int kb, int q, int j) { const int p = 32 * kb + 8 * q + j; return 4 * (2 * (p >> 3) + (p & 1)) + ((p >> 1) & 3); };
        pack_h(l1_rs_ih[d], 16, 4, [&](int row, int kb, int q, int j) { return gscale(row) * l1[0][gate_row(row) * 2 * PH + h0_feat(kb, q, j)]; });
        pack_h(l1_rs_hh[d], 16, 2, [&](int row, int kb, int q, int j) { return gscale(row) * l1[1][gate_row(row) * PH + r1_feat(kb, q, j)]; });
        pack_h(l1_hh[d], 16, 2, [&](int row, int kb, int q, int j) { return l1[1][gate_row(row) * PH + rec_feat(kb, q, j)]; });
    }
    pack_h(proj, 8, 4, [&](int row, int kb, int q, int j) { return w[16][row * 128 + h0_feat(kb, q, j)]; });
    pack_h(dense, 16, 4, [&](int row, int kb, int q, int j) { return w[18][row * 128 + acc_feat(kb, q, j)]; });
    pack_h(head, 2, 8, [&](int row, int kb, int q, int j) {
        const int f = acc_feat(kb, q, j);
        if (row < 21) return w[20][row * 256 + f];
        if (row < 24) return w[22][(row - 21) * 256 + f];
        return 0.f;
    });
    // the layer-0 input image is consumed as two separate [tile][lane] part images (hi in LDS, lo via L1)
    std::vector<_Float16> ih_split(2 * n_ih);
    for (int d = 0; d < 2; ++d)
        for (int tile = 0; tile < 16; ++tile)
            for (int part = 0; part < 2; ++part)
                memcpy(ih_split.data() + ((size_t)d * 2 + part) * (n_ih / 2) + (size_t)tile * 64 * 8,
                       l0_ih[d] + ((size_t)tile * 2 + part) * 64 * 8, sizeof(_Float16) * 64 * 8);
    for (int d = 0; d < 2; ++d) memcpy(l0_ih[d], ih_split.data() + (size_t)d * n_ih, sizeof(_Float16) * n_ih);

    // fused layer-1 kernel: hi half as [tile][kb][lane], lo half chunk-major [chunk][tile in chunk][kb][lane]
    for (int d = 0; d < 2; ++d)
        for (int tile = 0; tile < 16; ++tile)
            for (int kb = 0; kb < 4; ++kb) {
                const _Float16* src = l1_ih[d] + (((size_t)tile * 4 + kb) * 2) * 64 * 8;      // [tile][kb][part][lane][8]
                memcpy(f_hi[d] + ((size_t)tile * 4 + kb) * 64 * 8, src, sizeof(_Float16) * 64 * 8);
                memcpy(f_lo[d] + ((((size_t)(tile >> 1) * 2 + (tile & 1)) * 4 + kb) * 64) * 8, src + 64 * 8, sizeof(_Float16) * 64 * 8);
            }
    const size_t bytes = total * sizeof(_Float16);
    if (pw.arena && pw.arena_bytes != bytes) { (void)hipFree(pw.arena); pw.arena = nullptr; }
    if (!pw.arena) { NSNP_HIP(ctx, hipMalloc((void**)&pw.arena, bytes)); pw.arena_bytes = bytes; }
    NSNP_HIP(ctx, hipMemcpy(pw.arena, host.data(), bytes, hipMemcpyHostToDevice));
    auto dev = [&](const _Float16* hp) { return (void*)((char*)pw.arena + (hp - host.data()) * sizeof(_Float16)); };
    for (int d = 0; d < 2; ++d) {
        pw.l0_whh[d] = dev(l0_hh[d]); pw.l0_wih_hi[d] = dev(l0_ih[d]); pw.l0_wih_lo[d] = dev(l0_ih[d] + n_ih / 2);
        pw.l1_wih[d] = dev(l1_ih[d]); pw.l1_whh[d] = dev(l1_hh[d]);
        pw.l1f_hi[d] = dev(f_hi[d]); pw.l1f_lo[d] = dev(f_lo[d]);
        pw.l0_whh_rs[d] = dev(l0_rs[d]); pw.l0_wih_rs[d] = dev(l0_rs_ih[d]);
        pw.l1_wih_rs[d] = dev(l1_rs_ih[d]); pw.l1_whh_rs[d] = dev(l1_rs_hh[d]);
    }
    pw.proj_w = dev(proj); pw.dense_w = dev(dense); pw.head_w = dev(head);
    {
        float hb[4][64 * 4];                       // [0..1]: plain, [2..3]: pre-scaled by log2 e for K23r
        for (int d = 0; d < 2; ++d) {
            const float* const* l1 = w + 8 + d * 4;
            for (int tile = 0; tile < 16; ++tile) for (int qq = 0; qq < 4; ++qq) for (int g = 0; g < 4; ++g) {
                const int tr = gate_row(16 * tile + 4 * qq + g);
                hb[d][(tile * 4 + qq) * 4 + g] = l1[2][tr] + l1[3][tr];
                hb[2 + d][(tile * 4 + qq) * 4 + g] = (g == 2 ? 2.0f * LOG2E : -LOG2E) * (l1[2][tr] + l1[3][tr]);
            }
        }
        if (!pw.l1f_bias) NSNP_HIP(ctx, hipMalloc((void**)&pw.l1f_bias, sizeof hb));
        NSNP_HIP(ctx, hipMemcpy(pw.l1f_bias, hb, sizeof hb, hipMemcpyHostToDevice));
    }
    pw.loaded = true;
    return NSNP_OK;
}

// nsnp_pileup_load_indel_heads, fp16 hi/lo image of all 90 head rows.  Rows 0..23 (tile 0, and the lanes of tile 1 whose row is below 24)
// are read back from the two-tile image nsnp_pileup_pack_weights_f16 uploaded - the very bits k_pileup_head_h multiplies; rows 24..89 are
// split from the indel tensors w = {indel1 W, b, indel2 W, b} like every other weight, rows 90..95 are 0.  The biases are pw.head6_b.
int nsnp_pileup_pack_indel_heads_f16(nsnp_ctx* ctx, const float* const* w)
{
    PileupWeightsF16& pw = ctx->pw16;
    if (!pw.loaded) return NSNP_ENOWEIGHTS;
    constexpr size_t n_tile = (size_t)8 * 2 * 64 * 8;       // fp16 per tile
    std::vector<_Float16> img(6 * n_tile), old_w(2 * n_tile);
    NSNP_HIP(ctx, hipDeviceSynchronize());
    NSNP_HIP(ctx, hipMemcpy(old_w.data(), pw.head_w, old_w.size() * sizeof(_Float16), hipMemcpyDeviceToHost));
    auto acc_feat = [](int kb, int q, int j) { return 16 * (2 * kb + (j >> 2)) + 4 * q + (j & 3); };
    pack_h(img.data(), 6, 8, [&](int row, int kb, int q, int j) {
        const int f = acc_feat(kb, q, j);
        if (row >= 24 && row < 57) return w[0][(row - 24) * 256 + f];
        if (row >= 57 && row < 90) return w[2][(row - 57) * 256 + f];
        return 0.f;
    });
    for (int tile = 0; tile < 2; ++tile) for (int kp = 0; kp < 8 * 2; ++kp) for (int lane = 0; lane < 64; ++lane)
        if (16 * tile + (lane & 15) < 24) {
            const size_t e = (((size_t)tile * 16 + kp) * 64 + lane) * 8;
            memcpy(&img[e], &old_w[e], 8 * sizeof(_Float16));
        }
    if (!pw.head6_w) NSNP_HIP(ctx, hipMalloc(&pw.head6_w, img.size() * sizeof(_Float16)));
    NSNP_HIP(ctx, hipMemcpy(pw.head6_w, img.data(), img.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    return NSNP_OK;
}

static int set_lds_attr_f16(nsnp_ctx* ctx)
{
    if (ctx->attr_set_f16) return NSNP_OK;
#define SET(K, B) NSNP_HIP(ctx, hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, B))
    SET(k_pileup_l0_h<8>, L0H_LDS_BYTES); SET(k_pileup_l0_h<4>, L0H_LDS_BYTES); SET(k_pileup_l0_h<2>, L0H_LDS_BYTES); SET(k_pileup_l0_h<1>, L0H_LDS_BYTES);
    SET(k_pileup_proj1_h, P1H_LDS_BYTES);
    SET(k_pileup_l1_rs<4>, r1_lds_bytes(4)); SET(k_pileup_l1_rs<2>, r1_lds_bytes(2));
    SET(k_pileup_l1f_h<4>, L1F_LDS_BYTES); SET(k_pileup_l1f_h<8>, L1F_LDS_BYTES); SET(k_pileup_l1f_h<12>, L1F_LDS_BYTES);
    SET(k_pileup_head_eval_h, HEAD_EVAL_LDS_BYTES);
    SET(k_pileup_l1_h<8>, L1H_LDS_BYTES); SET(k_pileup_l1_h<4>, L1H_LDS_BYTES); SET(k_pileup_l1_h<2>, L1H_LDS_BYTES); SET(k_pileup_l1_h<1>, L1H_LDS_BYTES);
#undef SET
    ctx->attr_set_f16 = true;
    return NSNP_OK;
}

// The chunk loop and layers 0 and 1 of an f16x3 pass under the context's options, ending in the caller's heads launch heads(base, n) on
// the chunk's H1c: the ONE place these launches are made - the probability forward and the scoring forward below differ in their heads
// kernel only.  (H0 and H1c have the bytes per site of the fp32 layout, so any reserved workspace serves.)
template <typename HeadsFn>
static int forward_f16x3_t(nsnp_ctx* ctx, const int32_t* x, const int64_t* center_idx, int64_t N, hipStream_t s, HeadsFn heads)
{
    if (N == 0) return NSNP_OK;
    int rc = set_lds_attr_f16(ctx);
    if (rc) return rc;
    if (!ctx->ws_h0) { rc = nsnp_ctx_reserve(ctx, ctx->chunk_sites); if (rc) return rc; }
    const PileupWeightsF16& pw = ctx->pw16;
    const PileupWeightsDev& p32 = ctx->pw;            // fp32 bias images are shared with the fp32 path
    _Float16* H0 = reinterpret_cast<_Float16*>(ctx->ws_h0);       // same bytes per site as the fp32 layout
    _Float16* H1c = reinterpret_cast<_Float16*>(ctx->ws_h1c);
    for (int64_t base = 0; base < N; base += ctx->chunk_sites) {
        const int64_t n = (N - base < ctx->chunk_sites) ? N - base : ctx->chunk_sites;
        const int32_t* xc = center_idx ? x : x + base * (PW * PC);
        const int64_t* cc = center_idx ? center_idx + base : nullptr;
        // 4 waves per recurrence workgroup at most: the 8-wave variant has to fit 128 VGPRs and spills
        // (measured 2.4 ms vs 1.6 ms for layer 0 at 131072 sites); fewer for small batches as in the fp32 path
        const int64_t waves_total = NSNP_CDIV(n, 16) * 2;
        int wpb = 4;
        while (wpb > 1 && waves_total / wpb < (int64_t)ctx->n_cu / 2) wpb >>= 1;
        if (ctx->force_wpb) wpb = ctx->force_wpb;
        const dim3 g_rec((unsigned)NSNP_CDIV(n, 16 * wpb), 2);
        if (ctx->l0_rs) {
            ScopedKernelTimer tm(ctx, NSNP_K_L0, s);
            // 64 sites per workgroup when that still gives every CU two workgroups, else 32 or 16
            int nsg = 4;
            while (nsg > 1 && NSNP_CDIV(n, 16 * nsg) * 2 < 2 * (int64_t)ctx->n_cu) nsg >>= 1;
            if (ctx->l0_rs_groups) nsg = ctx->l0_rs_groups;
#define LAUNCH_RS(G) hipLaunchKernelGGL(k_pileup_l0_rs<G>, dim3((unsigned)NSNP_CDIV(n, 16 * G), 2), dim3(256), 0, s, xc, cc, n, \
            (const _Float16*)pw.l0_whh_rs[0], (const _Float16*)pw.l0_whh_rs[1], (const _Float16*)pw.l0_wih_rs[0], (const _Float16*)pw.l0_wih_rs[1], H0, ctx->rs_prio)
            if (nsg == 4) LAUNCH_RS(4); else if (nsg == 2) LAUNCH_RS(2); else LAUNCH_RS(1);
#undef LAUNCH_RS
        } else
        { ScopedKernelTimer tm(ctx, NSNP_K_L0, s);
#define LAUNCH_L0(W) hipLaunchKernelGGL(k_pileup_l0_h<W>, g_rec, dim3(64 * W), L0H_LDS_BYTES, s, xc, cc, n, \
            (const _Float16*)pw.l0_whh[0], (const _Float16*)pw.l0_whh[1], (const _Float16*)pw.l0_wih_hi[0], (const _Float16*)pw.l0_wih_hi[1], \
            (const _Float16*)pw.l0_wih_lo[0], (const _Float16*)pw.l0_wih_lo[1], H0)
        if (wpb == 8) LAUNCH_L0(8); else if (wpb == 4) LAUNCH_L0(4); else if (wpb == 2) LAUNCH_L0(2); else LAUNCH_L0(1);
#undef LAUNCH_L0
        }
        if (ctx->fused_l1 && ctx->l1_rs) {
            ScopedKernelTimer tm(ctx, NSNP_K_L1, s);
            // 64 sites per workgroup when that still gives every CU a workgroup, else 32
            int g1 = NSNP_CDIV(n, 64) * 2 >= (int64_t)ctx->n_cu ? 4 : 2;
            if (ctx->l1_rs_groups) g1 = ctx->l1_rs_groups;
#define LAUNCH_R1(G) hipLaunchKernelGGL(k_pileup_l1_rs<G>, dim3((unsigned)NSNP_CDIV(n, 16 * G), 2), dim3(512), r1_lds_bytes(G), s, H0, n, \
                               (const _Float16*)pw.l1_wih_rs[0], (const _Float16*)pw.l1_wih_rs[1], \
                               (const _Float16*)pw.l1_whh_rs[0], (const _Float16*)pw.l1_whh_rs[1], \
                               (const float*)pw.l1f_bias + 512, (const float*)pw.l1f_bias + 768, H1c, ctx->rs_prio)
            if (ctx->l1_rs == 1 && !ctx->l1_rs_groups) {      // default: four waves x four tiles, 16 sites per workgroup
                hipLaunchKernelGGL(k_pileup_l1_rs4_h, dim3((unsigned)NSNP_CDIV(n, 16), 2), dim3(256), r1_lds_bytes4(), s, H0, n,
                                   (const _Float16*)pw.l1_wih_rs[0], (const _Float16*)pw.l1_wih_rs[1],
                                   (const _Float16*)pw.l1_whh_rs[0], (const _Float16*)pw.l1_whh_rs[1],
                                   (const float*)pw.l1f_bias + 512, (const float*)pw.l1f_bias + 768, H1c);
            } else if (g1 == 4) LAUNCH_R1(4); else LAUNCH_R1(2);
#undef LAUNCH_R1
        } else if (ctx->fused_l1) {
            ScopedKernelTimer tm(ctx, NSNP_K_L1, s);
            // one workgroup per CU: 12 waves when the batch fills the chip that way, else 8 or 4
            // (the 12-wave build has to fit 168 VGPRs and spills: 1.84 ms vs 1.49 ms at 131072 sites)
            int fw = 8;
            if (NSNP_CDIV(n, 128) * 2 < ctx->n_cu) fw = 4;
            if (ctx->fused_waves) fw = ctx->fused_waves;
#define LAUNCH_F(W) hipLaunchKernelGGL(k_pileup_l1f_h<W>, dim3((unsigned)NSNP_CDIV(n, 16 * W), 2), dim3(64 * W), L1F_LDS_BYTES, s, H0, n, \
                               (const _Float16*)pw.l1_whh[0], (const _Float16*)pw.l1_whh[1], \
                               (const _Float16*)pw.l1f_hi[0], (const _Float16*)pw.l1f_hi[1], \
                               (const _Float16*)pw.l1f_lo[0], (const _Float16*)pw.l1f_lo[1], \
                               (const float*)pw.l1f_bias, (const float*)pw.l1f_bias + 256, H1c)
            if (fw == 12) LAUNCH_F(12); else if (fw == 8) LAUNCH_F(8); else LAUNCH_F(4);
#undef LAUNCH_F
        } else {
        { const int rx = nsnp_ctx_need_xp1(ctx); if (rx) return rx; }
        const int64_t n_rt = NSNP_CDIV(n * PSTEPS1, 16);
        // persistent workgroups: each loads the 128 KB weight image once and then walks
        // proj1_tiles 16-row tiles per wave, so the load is amortised even at small batches
        int64_t gp = NSNP_CDIV(n_rt, 16 * (int64_t)ctx->proj1_tiles);
        if (gp > ctx->n_cu) gp = ctx->n_cu;
        if (gp < 1) gp = 1;
        { ScopedKernelTimer tm(ctx, NSNP_K_PROJ1, s);
        hipLaunchKernelGGL(k_pileup_proj1_h, dim3((unsigned)gp, 2), dim3(1024), P1H_LDS_BYTES, s, H0, n,
                           (const _Float16*)pw.l1_wih[0], (const _Float16*)pw.l1_wih[1], p32.l1_bias_raw[0], p32.l1_bias_raw[1], ctx->ws_xp1); }
        { ScopedKernelTimer tm(ctx, NSNP_K_L1, s);
#define LAUNCH_L1(W) hipLaunchKernelGGL(k_pileup_l1_h<W>, g_rec, dim3(64 * W), L1H_LDS_BYTES, s, ctx->ws_xp1, n, \
            (const _Float16*)pw.l1_whh[0], (const _Float16*)pw.l1_whh[1], H1c)
        if (wpb == 8) LAUNCH_L1(8); else if (wpb == 4) LAUNCH_L1(4); else if (wpb == 2) LAUNCH_L1(2); else LAUNCH_L1(1);
#undef LAUNCH_L1
        }
        }
        ScopedKernelTimer tm_head(ctx, NSNP_K_HEAD, s);
        heads(base, n);
    }
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

int nsnp_pileup_forward_f16x3(nsnp_ctx* ctx, const int32_t* x, const int64_t* center_idx,
                              int64_t N, float* gt, float* zy, hipStream_t s)
{
    if (!ctx->pw16.loaded || !ctx->pw.loaded) return NSNP_ENOWEIGHTS;
    const PileupWeightsF16& pw = ctx->pw16;
    const PileupWeightsDev& p32 = ctx->pw;
    return forward_f16x3_t(ctx, x, center_idx, N, s, [&](int64_t base, int64_t n) {
        hipLaunchKernelGGL(k_pileup_head_h, dim3((unsigned)NSNP_CDIV(n, 16 * HEAD_WAVES)), dim3(64 * HEAD_WAVES), 0, s,
                           reinterpret_cast<const _Float16*>(ctx->ws_h1c), n,
                           (const _Float16*)pw.proj_w, p32.proj_b, (const _Float16*)pw.dense_w, p32.dense_b,
                           (const _Float16*)pw.head_w, p32.head_b, gt + base * NSNP_GT_CLASSES, zy + base * NSNP_ZY_CLASSES);
    });
}

// nsnp_pileup_forward_stage at precision 1 (N <= chunk_sites: one pass): the un-tiling launch stands where the heads launch stands
int nsnp_pileup_stage_f16x3(nsnp_ctx* ctx, const int32_t* x, const int64_t* center_idx, int64_t N, const PileupTap& tap, hipStream_t s)
{
    if (!ctx->pw16.loaded || !ctx->pw.loaded) return NSNP_ENOWEIGHTS;
    return forward_f16x3_t(ctx, x, center_idx, N, s, [&](int64_t, int64_t n) { nsnp_pileup_untile_launch(ctx, 1, tap, n, s); });
}

// nsnp_pileup_forward_logits2 / nsnp_pileup_eval_windows2 at precision 1.  cls NULL: logits only (site_loss, pred, counters unused)
int nsnp_pileup_eval_f16x3(nsnp_ctx* ctx, const int32_t* x, const int64_t* center_idx, const uint8_t* cls, int64_t N, float* site_loss,
                           uint8_t* pred, int64_t* counters, float* logits, hipStream_t s)
{
    if (!ctx->pw16.loaded || !ctx->pw.loaded || !ctx->pw.indel_loaded) return NSNP_ENOWEIGHTS;
    const PileupWeightsF16& pw = ctx->pw16;
    const PileupWeightsDev& p32 = ctx->pw;
    return forward_f16x3_t(ctx, x, center_idx, N, s, [&](int64_t base, int64_t n) {
        hipLaunchKernelGGL(k_pileup_head_eval_h, dim3((unsigned)NSNP_CDIV(n, 16 * HEAD_WAVES)), dim3(64 * HEAD_WAVES), HEAD_EVAL_LDS_BYTES, s,
                           reinterpret_cast<const _Float16*>(ctx->ws_h1c), n,
                           (const _Float16*)pw.proj_w, p32.proj_b, (const _Float16*)pw.dense_w, p32.dense_b,
                           (const _Float16*)pw.head6_w, p32.head6_b, cls ? cls + base * 4 : nullptr, cls ? site_loss + base * 4 : nullptr,
                           cls ? pred + base * 4 : nullptr, reinterpret_cast<unsigned long long*>(counters),
                           logits ? logits + base * NSNP_LABEL_WIDTH : nullptr);
    });
}
