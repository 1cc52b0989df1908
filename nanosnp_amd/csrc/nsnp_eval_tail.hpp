// nsnp_eval_tail.hpp -- the scoring tail of the split-precision heads kernels (k_pileup_head_eval_b3, k_pileup_head_eval_h): what
// k_pileup_head_eval (pileup_eval.hip) does behind its logit exchange, operation for operation, for ONE wave that holds the 90 logits
// of its own 16 sites.  There a workgroup shares one group of 16 sites and wave h finishes head h; here a wave owns its sites (as in the
// probability kernels these two end), so it walks the four heads itself.
//
// Row map (the same in every kernel family): head row r = 16 tile + 4 q + g is register g of accumulator `tile` in lane (site n, q) = n + 16 q
// and lands at z[n][r].  Lane (n, q) then reads classes c = q, q + 4, ... of a head; maximum / first argmax / sum of exponentials / sum of
// logits meet over the four q lanes of a site by two butterfly steps whose operands commute, so the four lanes hold the same bits.  Lane
// q = 0 stores loss and argmax and counts [target][predicted] in a 32-bit LDS counter (integer adds: order-free); the counters leave once,
// as 64-bit integer adds.  No float is ever added atomically.
#pragma once

#include "nsnp_common.hpp"

namespace nsnp_eval {

constexpr int W = NSNP_LABEL_WIDTH;                          // 90 head rows = 21 + 3 + 33 + 33
// floats per site of the logit exchange.  Lane (n, q) WRITES z[n][16 t + 4 q + g] and READS z[n][row0 + q + 4 i]; a 32-bit LDS access is
// served in two halves of 32 lanes (q = 0, 1 and q = 2, 3), so a half is conflict-free when the 32 values of (ZLD n + 4 q) mod 64 - the
// stores - and of (ZLD n + q) mod 64 - the loads - are distinct.  103 is the smallest stride >= 90 with both properties (the fp32 kernel's
// 97 clears the loads only: its 16 + 16 store addresses fall on 20 banks); computed from the bank rule, not measured with counters.
constexpr int ZLD = 103;
constexpr int COUNTERS = NSNP_EVAL_COUNTERS;
constexpr int Z_WAVE = 16 * ZLD;                             // floats of one wave's exchange
__device__ __forceinline__ int head_row0(int h) { return h == 0 ? 0 : (h == 1 ? 21 : (h == 2 ? 24 : 57)); }
__device__ __forceinline__ int head_classes(int h) { return h == 0 ? 21 : (h == 1 ? 3 : 33); }
__device__ __forceinline__ int head_counter0(int h) { return h == 0 ? 0 : (h == 1 ? 441 : (h == 2 ? 450 : 1539)); }
static_assert(441 + 9 + 1089 + 1089 == COUNTERS, "four confusion matrices");

// the six accumulator tiles of a lane -> the wave's exchange
__device__ __forceinline__ void put_logits(float* zw, int lane, const f32x4* ah)
{
    const int q = lane >> 4;
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) zw[(lane & 15) * ZLD + 16 * t + 4 * q + g] = ah[t][g];
}

// behind a barrier that follows put_logits: logits out, then loss / argmax / counts of the four heads.  site0: the wave's first site.
__device__ __forceinline__ void wave_tail(const float* zw, int lane, int64_t site0, int64_t N, const uint8_t* __restrict__ cls,
                                          float* __restrict__ site_loss, uint8_t* __restrict__ pred, unsigned int* cnt,
                                          float* __restrict__ logits)
{
    const int q = lane >> 4;
    const int64_t site = site0 + (lane & 15);
    const bool live = site < N;
    if (logits)
        for (int i = lane; i < 16 * W; i += 64) {
            const int n = i / W, r = i - n * W;
            if (site0 + n < N) logits[(site0 + n) * W + r] = zw[n * ZLD + r];
        }
    if (!cls) return;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int C = head_classes(h);
        const float* zr = zw + (lane & 15) * ZLD + head_row0(h);
        const float NEG = -3.0e38f;
        float v[9], bv = NEG;
        int bi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int c = q + 4 * i;
            v[i] = c < C ? zr[c] : NEG;
            if (c < C && v[i] > bv) { bv = v[i]; bi = c; }          // ascending classes within a lane: the first maximum
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        float se = 0.f, sz = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const bool ok = q + 4 * i < C;
            se += ok ? expf(v[i] - bv) : 0.f;
            sz += ok ? v[i] : 0.f;
        }
        se += __shfl_xor(se, 16); se += __shfl_xor(se, 32);
        sz += __shfl_xor(sz, 16); sz += __shfl_xor(sz, 32);
        if (live && q == 0) {
            int t = cls[site * 4 + h];
            if (t >= C) t = C - 1;
            if (bi >= C) bi = 0;                                   // (no maximum among NaN logits: class 0, as np.argmax of a NaN at 0)
            // lp = z - logsumexp(z); loss = -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t]))      optim.py:138-144
            const float lse = bv + logf(se);
            const float lpt = zr[t] - lse;
            const float slp = sz - (float)C * lse;
            site_loss[site * 4 + h] = -(0.9f * lpt + (0.1f / (float)(C - 1)) * (slp - lpt));
            pred[site * 4 + h] = (uint8_t)bi;
            atomicAdd(&cnt[head_counter0(h) + t * C + bi], 1u);
        }
    }
}

// the workgroup's counters leave once (behind a barrier that follows every wave_tail)
__device__ __forceinline__ void flush_counters(const unsigned int* cnt, unsigned long long* __restrict__ counters, int tid, int nthreads)
{
    for (int i = tid; i < COUNTERS; i += nthreads)
        if (cnt[i]) atomicAdd(counters + i, (unsigned long long)cnt[i]);
}

}  // namespace nsnp_eval
