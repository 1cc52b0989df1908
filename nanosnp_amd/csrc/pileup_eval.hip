// pileup_eval.hip -- scoring a checkpoint on labelled windows (<chr>.td.bin): what PileupModel/train.py:93-150, its eval(), computes.
//
// Replaces, for windows and label rows that are already in HBM,
//   the label decode and the variant filter of TrainDataset(for_evaluate=True)   PileupModel/dataset.py:78-82,98-104
//   ForwardLayer.forward with all four heads as raw logits                       PileupModel/model.py:66-73
//   LabelSmoothingLoss.forward before its mean                                   PileupModel/optim.py:137-144
//   the argmax behind torchmetrics' Accuracy / ConfusionMatrix updates           PileupModel/train.py:125-134
//
// nsnp_pileup_label_classes, three launches:
//   k_evl_flags    one lane per label row: the first maximum of each family, whether the row is one-hot, whether it is kept  -> scratch
//   k_evl_scan     exclusive prefix sums of the kept flags, int64, by ONE workgroup of 1024 lanes.  Levels: a lane sums its own run of
//                  ceil(N / 1024) consecutive rows serially; the 1024 run sums are scanned in LDS (Hillis-Steele, 10 rounds); each lane
//                  then writes the running offsets of its rows.  There is no carry between workgroups because there is one workgroup,
//                  so the scan is exact for any N and no workgroup waits for another.  The same lanes count the malformed rows; meta.
//   k_evl_compact  the kept rows' classes and centres, in order                                                              -> cls, center_idx
// k_pileup_head_eval: the heads kernel (below).  k_evl_batch_loss: float64 sums of the per-site losses of a batch, one workgroup each.
//
// The HaplotypeModel's scoring (HaplotypeModel/evaluate_dev.py:16-86) shares the scan, the scratch and the batch sums:
//   nsnp_hap_label_classes   k_hapl_flags (LabelField + the target rule, dataset_dev.py:174-187,320), k_evl_scan, k_hapl_compact
//   nsnp_hap_batch_loss      k_evl_batch_loss over rows of two heads
// Its heads kernel, k_hap_head_eval, lives beside the forward it ends (hap_forward.hip).
//
// The HaplotypeModel's training samples (TrainingDataset.__init__, HaplotypeModel/dataset_dev.py:190-230) start from that label pass's cls:
//   nsnp_hap_train_samples   k_haps_flags, k_evl_scan, k_haps_lists, one host wait for the two counts, k_haps_place (nsnp_philox.hpp)
//
// The PileupModel's balanced training samples (balance_dataset, PileupModel/dataset.py:32-66) start from nsnp_pileup_label_classes' cls:
//   nsnp_pileup_balance_samples   k_bal_count, k_bal_scan, k_bal_lists (a counting sort with 64 bins), one host wait for M, k_bal_place
#include "nsnp_common.hpp"
#include "nsnp_philox.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// the two device functions of pileup_forward.hip the heads use, restated: the accumulators of rows 0..23 must be the bits of k_pileup_head_rs
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float tanh_f(float x)
{
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((2.0f * LOG2E) * x)), 1.0f);
}

constexpr int EV_W = NSNP_LABEL_WIDTH;                       // 90 head rows = 21 + 3 + 33 + 33
constexpr int EV_ZLD = 97;                                   // floats per site of the logit exchange (odd: 16 sites hit 16 banks)
constexpr int EV_COUNTERS = NSNP_EVAL_COUNTERS;
__device__ __forceinline__ int head_row0(int h) { return h == 0 ? 0 : (h == 1 ? 21 : (h == 2 ? 24 : 57)); }
__device__ __forceinline__ int head_classes(int h) { return h == 0 ? 21 : (h == 1 ? 3 : 33); }
__device__ __forceinline__ int head_counter0(int h) { return h == 0 ? 0 : (h == 1 ? 441 : (h == 2 ? 450 : 1539)); }
static_assert(441 + 9 + 1089 + 1089 == EV_COUNTERS, "four confusion matrices");

// ---------------------------------------------------------------------------------------------
// K4e: k_pileup_head_rs with all 90 head rows, raw logits, and the loss / argmax / confusion counts of a scoring pass.
// 512 threads, a persistent loop over groups of 16 sites; wave w owns output_proj tile w and dense tiles 2w, 2w+1 with their weights in
// VGPRs across the loop - the code of k_pileup_head_rs to the letter up to x2.  Then waves 0..5 each own one head tile (64 VGPRs of
// weights, as waves 0 and 1 there), and the K order, the bias start and the MFMA chain of every accumulator are those of k_pileup_head_rs.
//
// Row map.  Head row r (0..20 genotype, 21..23 zygosity, 24..56 indel1, 57..89 indel2, 90..95 zero padding) is accumulator
//   tile r / 16  (= the wave that computes it),  lane (site n, q = (r % 16) / 4) = n + 16 q,  register g = r % 4,
// and lands in LDS at z[n][r] (6.1 KB, 97 floats per site).  Heads straddle tiles: genotype = tile 0 + tile 1 rows 16..20, zygosity = tile 1
// rows 21..23, indel1 = tile 1 rows 24..31 + tiles 2, 3 rows 32..56 (q = 0, 1 and g = 0 of q = 2), indel2 = tile 3 rows 57..63 + tiles 4, 5.
// Behind one barrier wave h (0..3) finishes head h for the 16 sites: lane (n, q) reads classes c = q, q + 4, ... of z[n][row0(h) + c];
// maximum / first argmax / sum of exponentials / sum of logits meet over the four q lanes of a site (16 lanes apart) by two butterfly
// steps whose operands commute, so the four lanes hold the same bits.  Lane q = 0 stores loss and argmax and counts [target][predicted]
// in a 32-bit LDS counter (10.5 KB per workgroup, integer adds: order-free); the counters leave once, behind the loop, as 64-bit adds.
// No float is ever added atomically.  With `logits` all 512 lanes copy z (1,440 contiguous floats of a full group) to HBM.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void k_pileup_head_eval(
    const float* __restrict__ H1c, int64_t N,
    const float* __restrict__ proj_w, const float* __restrict__ proj_b,
    const float* __restrict__ dense_w, const float* __restrict__ dense_b,
    const float* __restrict__ head_w, const float* __restrict__ head_b,
    const uint8_t* __restrict__ cls, float* __restrict__ site_loss, uint8_t* __restrict__ pred,
    unsigned long long* __restrict__ counters, float* __restrict__ logits)
{
    __shared__ float x1[32][64];          // output_proj results as dense K-steps
    __shared__ float x2[64][64];          // tanh(dense) as head K-steps
    __shared__ float z[16][EV_ZLD];       // the 90 logits of the group's 16 sites
    __shared__ unsigned int cnt[EV_COUNTERS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    for (int i = tid; i < EV_COUNTERS; i += 512) cnt[i] = 0;
    // weights of this wave
    f32x4 Wp[8], Wd[2][8], Wh[16], bp, bd[2], bh;
    {
        const f32x4* pw = reinterpret_cast<const f32x4*>(proj_w);      // [8 tiles][8 j4][lane]
        const f32x4* dw = reinterpret_cast<const f32x4*>(dense_w);     // [16][8][lane]
        const f32x4* hw = reinterpret_cast<const f32x4*>(head_w);      // [6][16][lane]
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Wp[j] = pw[(wave * 8 + j) * 64 + lane];
            Wd[0][j] = dw[((2 * wave) * 8 + j) * 64 + lane];
            Wd[1][j] = dw[((2 * wave + 1) * 8 + j) * 64 + lane];
        }
        bp = reinterpret_cast<const f32x4*>(proj_b)[wave * 64 + lane];
        bd[0] = reinterpret_cast<const f32x4*>(dense_b)[(2 * wave) * 64 + lane];
        bd[1] = reinterpret_cast<const f32x4*>(dense_b)[(2 * wave + 1) * 64 + lane];
        if (wave < 6) {
#pragma unroll
            for (int j = 0; j < 16; ++j) Wh[j] = hw[(wave * 16 + j) * 64 + lane];
            bh = reinterpret_cast<const f32x4*>(head_b)[wave * 64 + lane];
        }
    }
    const int64_t n_groups = NSNP_CDIV(N, 16);
    for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int64_t site = grp * 16 + (lane & 15);
        const bool live = site < N;
        const int64_t sc = live ? site : N - 1;
        const f32x4* __restrict__ hin = reinterpret_cast<const f32x4*>(H1c + sc * 128 + q * 16);
        // output_proj 128 -> 128 (model.py:37): tile `wave`
        f32x4 ap = bp;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f32x4 b4 = hin[(j >> 2) * 16 + (j & 3)];            // fwd half, then reverse half (+64 floats)
#pragma unroll
            for (int e = 0; e < 4; ++e) ap = mfma4(Wp[j][e], b4[e], ap);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) x1[4 * wave + g][lane] = ap[g];
        __syncthreads();
        // dense 128 -> 256 + tanh (model.py:67): tiles 2 wave, 2 wave + 1
        f32x4 ad[2] = {bd[0], bd[1]};
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float b = x1[4 * j + e][lane];
                ad[0] = mfma4(Wd[0][j][e], b, ad[0]);
                ad[1] = mfma4(Wd[1][j][e], b, ad[1]);
            }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) x2[4 * (2 * wave + u) + g][lane] = tanh_f(ad[u][g]);
        __syncthreads();
        // the four heads (model.py:69-72): tile `wave` of the 90-row image in waves 0..5
        if (wave < 6) {
            f32x4 ah = bh;
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) ah = mfma4(Wh[j][e], x2[4 * j + e][lane], ah);
#pragma unroll
            for (int g = 0; g < 4; ++g) z[lane & 15][16 * wave + 4 * q + g] = ah[g];
        }
        __syncthreads();
        if (logits)
            for (int i = tid; i < 16 * EV_W; i += 512) {
                const int n = i / EV_W, r = i - n * EV_W;
                if (grp * 16 + n < N) logits[(grp * 16 + n) * EV_W + r] = z[n][r];
            }
        if (cls && wave < 4) {
            const int C = head_classes(wave);
            const float* zr = &z[lane & 15][head_row0(wave)];
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
                int t = cls[site * 4 + wave];
                if (t >= C) t = C - 1;
                if (bi >= C) bi = 0;                                   // (no maximum among NaN logits: class 0, as np.argmax of a NaN at 0)
                // lp = z - logsumexp(z); loss = -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t]))      optim.py:138-144
                const float lse = bv + logf(se);
                const float lpt = zr[t] - lse;
                const float slp = sz - (float)C * lse;
                site_loss[site * 4 + wave] = -(0.9f * lpt + (0.1f / (float)(C - 1)) * (slp - lpt));
                pred[site * 4 + wave] = (uint8_t)bi;
                atomicAdd(&cnt[head_counter0(wave) + t * C + bi], 1u);
            }
        }
        // (x1 / x2 / z of this group are not touched again before the next group's first / second / third barrier)
    }
    if (cls) {
        __syncthreads();
        for (int i = tid; i < EV_COUNTERS; i += 512)
            if (cnt[i]) atomicAdd(counters + i, (unsigned long long)cnt[i]);
    }
}

// ---- label rows -> classes --------------------------------------------------------------------
constexpr int EVL_BLOCK = 256;
constexpr uint32_t EVL_BAD = 0x80u;                          // beside the genotype class (0..20) in byte 0 of a row's scratch word

__global__ __launch_bounds__(EVL_BLOCK) void k_evl_flags(const int32_t* __restrict__ label, int64_t N, int variants_only,
                                                         int64_t* __restrict__ keep, uint32_t* __restrict__ word)
{
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int32_t* y = label + n * EV_W;
    uint32_t w = 0;
    bool bad = false;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int r0 = head_row0(h), C = head_classes(h);
        int best = y[r0], bi = 0, ones = best == 1, nonzero = best != 0;
        for (int c = 1; c < C; ++c) {
            const int v = y[r0 + c];
            if (v > best) { best = v; bi = c; }              // the first maximum, as np.argmax
            ones += v == 1; nonzero += v != 0;
        }
        bad |= ones != 1 || nonzero != 1;
        w |= (uint32_t)bi << (8 * h);
    }
    keep[n] = (!variants_only || ((w >> 8) & 0xff) > 0) ? 1 : 0;
    word[n] = w | (bad ? EVL_BAD : 0u);
}

// (shared with nsnp_hap_label_classes, whose words carry two more flags to count: EVL_M2 / EVL_M3 -> meta[2] / meta[3].  The label rows of a
// .td.bin never set them - byte 1 of their word is the zygosity class, 0..2 - so those two stay 0 there.)
constexpr uint32_t EVL_M2 = 0x4000u, EVL_M3 = 0x8000u;
__global__ __launch_bounds__(1024) void k_evl_scan(int64_t* __restrict__ keep, const uint32_t* __restrict__ word, int64_t N, int64_t* __restrict__ meta)
{
    __shared__ int64_t part[1024];
    __shared__ unsigned long long n_bad, n_m2, n_m3;
    const int tid = threadIdx.x;
    if (tid == 0) { n_bad = 0; n_m2 = 0; n_m3 = 0; }
    const int64_t per = NSNP_CDIV(N, (int64_t)1024);
    const int64_t n0 = tid * per < N ? tid * per : N, n1 = n0 + per < N ? n0 + per : N;
    int64_t s = 0, b = 0, m2 = 0, m3 = 0;
    for (int64_t n = n0; n < n1; ++n) {
        const uint32_t w = word[n];
        s += keep[n]; b += (w & EVL_BAD) ? 1 : 0; m2 += (w & EVL_M2) ? 1 : 0; m3 += (w & EVL_M3) ? 1 : 0;
    }
    part[tid] = s;
    __syncthreads();
    if (b) atomicAdd(&n_bad, (unsigned long long)b);
    if (m2) atomicAdd(&n_m2, (unsigned long long)m2);
    if (m3) atomicAdd(&n_m3, (unsigned long long)m3);
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = tid ? part[tid - 1] : 0;
    for (int64_t n = n0; n < n1; ++n) { const int64_t v = keep[n]; keep[n] = run; run += v; }
    if (tid == 1023) {
        keep[N] = part[1023];
        meta[0] = part[1023]; meta[1] = (int64_t)n_bad; meta[2] = (int64_t)n_m2; meta[3] = (int64_t)n_m3;
    }
}

// ---- HaplotypeModel: candidate_labels rows {confident, gt21, zygosity} -> classes (LabelField, HaplotypeModel/dataset_dev.py:174-187,320) ----
// word of a row: gt in byte 0 (with EVL_BAD: kept by the filter but not scorable by the loaded model), max(zy, 0) in byte 1 with EVL_M2 for a
// kept refcall and EVL_M3 for a kept variant.  The scan and its meta are k_evl_scan's.
__global__ __launch_bounds__(EVL_BLOCK) void k_hapl_flags(const int32_t* __restrict__ label, int64_t N, int n_gt, int n_zy,
                                                          int64_t* __restrict__ keep, uint32_t* __restrict__ word)
{
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int32_t cf = label[n * 3], gt = label[n * 3 + 1], zy = label[n * 3 + 2];
    const bool refcall = cf == 1 && zy == -1 && gt < 10;            // dataset_dev.py:185
    const bool variant = cf == 1 && zy > 0 && zy < 10 && gt < 10;   // :180,187 (zy == 0 passes valid_idx and is in neither list)
    const bool scorable = gt >= 0 && gt < n_gt && zy < n_zy;        // (what scatter_ of the smoothed loss accepts)
    const bool kept = (refcall || variant) && scorable;
    uint32_t w = 0;
    if (kept) w = (uint32_t)gt | (uint32_t)(zy > 0 ? zy : 0) << 8 | (refcall ? EVL_M2 : EVL_M3);
    else if (refcall || variant) w = EVL_BAD;
    keep[n] = kept ? 1 : 0;
    word[n] = w;
}

__global__ __launch_bounds__(EVL_BLOCK) void k_hapl_compact(const int64_t* __restrict__ scan, const uint32_t* __restrict__ word, int64_t N,
                                                            uint8_t* __restrict__ cls, int64_t* __restrict__ rows)
{
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int64_t o = scan[n];
    if (scan[n + 1] == o || o < 0 || o >= N) return;         // (o lies in [0, N) by construction)
    const uint32_t w = word[n];
    cls[o * 2] = (uint8_t)(w & 0x7fu);
    cls[o * 2 + 1] = (uint8_t)((w >> 8) & 0x3fu);
    rows[o] = n;
}

// ---- HaplotypeModel training: the sample list of a pass under pn_value upsampling (TrainingDataset.__init__, dataset_dev.py:190-230) ----
// Input: cls of the kept rows (byte 1 is 0 exactly for a refcall).  k_haps_flags marks the refcalls for k_evl_scan (keep = refcall; the word
// carries EVL_M2 / EVL_M3, so the scan's meta is {refcalls, 0, refcalls, variants}).  A kept row is a refcall or a variant, so ONE scan ranks
// both: row n is refcall number scan[n] or variant number n - scan[n].  k_haps_lists writes list = {refcalls in order, variants in order}.
// k_haps_place: a lane per output entry.  Block b of HAPS_REFS refcalls starts at b * (HAPS_REFS + q_full) - closed form, no scan over blocks
// - and holds its refcalls and then its draws; draw j of block b is Philox4x32-10 word 0 at counter {j, b, draw, 0} under the key
// {seed low, seed high}, turned into a variant by multiply-shift (nsnp_philox.hpp).  Nothing is accumulated and no lane reads another's output.
constexpr int64_t HAPS_REFS = 1000;                          // block_size of dataset_dev.py:204

__global__ __launch_bounds__(EVL_BLOCK) void k_haps_flags(const uint8_t* __restrict__ cls, int64_t N, int64_t* __restrict__ keep, uint32_t* __restrict__ word)
{
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (n >= N) return;
    const bool refcall = cls[n * 2 + 1] == 0;
    keep[n] = refcall ? 1 : 0;
    word[n] = refcall ? EVL_M2 : EVL_M3;
}

__global__ __launch_bounds__(EVL_BLOCK) void k_haps_lists(const int64_t* __restrict__ scan, int64_t N, int64_t* __restrict__ list)
{
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int64_t o = scan[n], n_ref = scan[N];
    const int64_t at = scan[n + 1] != o ? o : n_ref + (n - o);           // (refcalls fill [0, n_ref), variants [n_ref, N): in [0, N) by construction)
    if (at < 0 || at >= N) return;
    list[at] = n;
}

__global__ __launch_bounds__(EVL_BLOCK) void k_haps_place(const int64_t* __restrict__ list, int64_t n_ref, int64_t n_var, int64_t M, int64_t q_full,
                                                          uint32_t key0, uint32_t key1, uint32_t draw, int64_t* __restrict__ samples,
                                                          int64_t* __restrict__ meta)
{
    const int64_t i = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (i == 0) { meta[0] = M; meta[1] = n_ref; meta[2] = n_var; meta[3] = NSNP_CDIV(n_ref, HAPS_REFS); }
    if (i >= M) return;
    const int64_t stride = HAPS_REFS + q_full;
    const int64_t b = i / stride, w = i - b * stride;
    const int64_t left = n_ref - b * HAPS_REFS, len = left < HAPS_REFS ? left : HAPS_REFS;
    int64_t at;
    if (w < len) at = b * HAPS_REFS + w;
    else at = n_ref + (int64_t)nsnp_philox_index(nsnp_philox4x32_10((uint32_t)(w - len), (uint32_t)b, draw, 0u, key0, key1).v[0], (uint64_t)n_var);
    samples[i] = list[at];
}

// ---- PileupModel training: the sample list of a pass under balance_dataset upsampling (PileupModel/dataset.py:32-66) ----------------------
// Input: cls [N,4] of a label pass; the category of a row is c = 3 gt + zy (0..62), bin 63 takes the rows in no category (gt >= 21 or
// zy >= 3).  A one-pass counting sort with 64 bins ranks every row inside its category, stably, in row order:
//   k_bal_count   a workgroup per block of EVL_BLOCK rows: the block's rows per bin                                   -> cnt[block][64]
//   k_bal_scan    ONE workgroup of 1024 lanes = 16 segments x 64 bins.  A lane sums its bin over its segment's run of ceil(blocks / 16)
//                 consecutive blocks serially, the 16 segment sums of a bin meet in LDS, the lane then rewrites its run as running offsets:
//                 cnt becomes base[block][bin], exact for any number of blocks, no workgroup waits for another.  Segment 0 (one wave, a lane
//                 per bin) makes the plan: size, the exclusive scan off over the bins, max / K / U / M and nz[k], the k-th nonempty category.
//   k_bal_lists   a workgroup per block again: the peers of a lane - the lanes of its wave in the same bin - are the AND over the six bits of
//                 c of the ballot of that bit or its complement; rank = the peers below it; the waves of a block meet in a [4][64] table in
//                 LDS written by each peer group's first lane.  list[off[c] + base[block][c] + rank] = row: every position is a function of
//                 the rows alone.
//   k_bal_place   a lane per sample m: Philox words v at counter {m low, m high, draw, 0}; category nz[index(v[0], K)], slot r =
//                 index(v[1], max); slot r < size is the category's r-th row, slot r >= size the row index(w[0], size) with w at counter
//                 {r - size, c, draw, 1}.  Lane 0.. of the first workgroup also copy the plan's meta and sizes out: nothing reaches the
//                 caller's memory before the entry has held cap against M.
// The only atomics are k_bal_count's 32-bit integer adds in LDS, whose sums do not depend on their order.
constexpr int BAL_BINS = 64, BAL_NONE = 63;
constexpr int BAL_WAVES = EVL_BLOCK / 64;
constexpr int BAL_SEGS = 16;                                 // segments of k_bal_scan: 16 x 64 bins = 1024 lanes
constexpr int BAL_SIZE = 0, BAL_OFF = 64, BAL_NZ = 128, BAL_META = 192, BAL_PLAN = 200;      // the plan: int64 words

__device__ __forceinline__ int bal_bin(const uint8_t* __restrict__ cls, int64_t n)
{
    const int gt = cls[n * 4], zy = cls[n * 4 + 1];
    return gt < 21 && zy < 3 ? 3 * gt + zy : BAL_NONE;
}

__global__ __launch_bounds__(EVL_BLOCK) void k_bal_count(const uint8_t* __restrict__ cls, int64_t N, uint32_t* __restrict__ cnt)
{
    __shared__ unsigned int h[BAL_BINS];
    const int tid = threadIdx.x;
    if (tid < BAL_BINS) h[tid] = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + tid;
    if (n < N) atomicAdd(&h[bal_bin(cls, n)], 1u);
    __syncthreads();
    if (tid < BAL_BINS) cnt[(int64_t)blockIdx.x * BAL_BINS + tid] = h[tid];
}

__global__ __launch_bounds__(BAL_SEGS * BAL_BINS) void k_bal_scan(uint32_t* __restrict__ cnt, int64_t n_blocks, int64_t* __restrict__ plan)
{
    __shared__ long long part[BAL_SEGS][BAL_BINS];
    const int c = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int64_t per = NSNP_CDIV(n_blocks, (int64_t)BAL_SEGS);
    const int64_t b0 = seg * per < n_blocks ? seg * per : n_blocks, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    long long s = 0;
    for (int64_t b = b0; b < b1; ++b) s += cnt[b * BAL_BINS + c];
    part[seg][c] = s;
    __syncthreads();
    long long run = 0, size = 0;
    for (int g = 0; g < BAL_SEGS; ++g) {
        const long long v = part[g][c];
        run += g < seg ? v : 0;
        size += v;
    }
    for (int64_t b = b0; b < b1; ++b) { const uint32_t v = cnt[b * BAL_BINS + c]; cnt[b * BAL_BINS + c] = (uint32_t)run; run += v; }
    if (seg != 0) return;
    // the plan, by one wave with a lane per bin
    long long mx = c < BAL_NONE ? size : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long v = __shfl_xor(mx, o); mx = v > mx ? v : mx; }
    const bool nonempty = c < BAL_NONE && size > 0;
    const unsigned long long ne = __ballot(nonempty), under = __ballot(nonempty && size < mx);
    const int K = __popcll(ne), U = __popcll(under);
    long long inc = size;                                    // (bin 63 is the last lane: off[63] = the rows in a category)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long v = __shfl_up(inc, o); inc += c >= o ? v : 0; }
    const long long none = __shfl(size, BAL_NONE);
    plan[BAL_SIZE + c] = size;
    plan[BAL_OFF + c] = inc - size;
    if (nonempty) plan[BAL_NZ + __popcll(ne & ((1ull << c) - 1ull))] = c;
    if (c >= K) plan[BAL_NZ + c] = 0;                        // (behind the K entries; never followed)
    if (c < 8) {
        const long long L = (long long)K * mx;               // below 2^38: K <= 63, max < 2^32
        const long long M = U ? L / U : 0;                   // int(L / U) of dataset.py:65
        plan[BAL_META + c] = c == 0 ? M : c == 1 ? K : c == 2 ? U : c == 3 ? mx : c == 4 ? none : c == 5 ? (U ? 0 : 1) : 0;
    }
}

__global__ __launch_bounds__(EVL_BLOCK) void k_bal_lists(const uint8_t* __restrict__ cls, int64_t N, const uint32_t* __restrict__ base,
                                                         const int64_t* __restrict__ plan, uint32_t* __restrict__ list)
{
    __shared__ unsigned int wtab[BAL_WAVES][BAL_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    wtab[wave][lane] = 0;
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + tid;
    const bool live = n < N;
    const int c = live ? bal_bin(cls, n) : BAL_NONE;
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int bit = 0; bit < 6; ++bit) {
        const bool set = (c >> bit) & 1;
        const unsigned long long b = __ballot(set);
        peers &= set ? b : ~b;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    __syncthreads();
    if (live && rank == 0) wtab[wave][c] = (unsigned int)__popcll(peers);
    __syncthreads();
    if (!live || c == BAL_NONE) return;
    int64_t at = plan[BAL_OFF + c] + base[(int64_t)blockIdx.x * BAL_BINS + c] + rank;
    for (int w = 0; w < wave; ++w) at += wtab[w][c];
    if (at < 0 || at >= N) return;                           // (at lies in [0, N) by construction)
    list[at] = (uint32_t)n;
}

__global__ __launch_bounds__(EVL_BLOCK) void k_bal_place(const uint32_t* __restrict__ list, const int64_t* __restrict__ plan, int64_t N, int64_t M,
                                                         uint32_t key0, uint32_t key1, uint32_t draw, int64_t* __restrict__ samples,
                                                         int64_t* __restrict__ sizes, int64_t* __restrict__ meta)
{
    const int64_t m = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (m < 8) meta[m] = plan[BAL_META + m];
    if (sizes && m < BAL_NONE) sizes[m] = plan[BAL_SIZE + m];
    if (m >= M) return;
    const int64_t K = plan[BAL_META + 1], mx = plan[BAL_META + 3];
    if (K < 1 || K > BAL_NONE || mx < 1 || N < 1) return;
    const nsnp_philox4 v = nsnp_philox4x32_10((uint32_t)m, (uint32_t)((uint64_t)m >> 32), draw, 0u, key0, key1);
    int64_t k = (int64_t)nsnp_philox_index(v.v[0], (uint64_t)K);
    k = k < K ? k : K - 1;
    int64_t c = plan[BAL_NZ + k];
    c = c < 0 ? 0 : (c < BAL_NONE ? c : BAL_NONE - 1);
    const int64_t size = plan[BAL_SIZE + c];
    if (size < 1) return;                                    // (a nonempty category by construction)
    int64_t r = (int64_t)nsnp_philox_index(v.v[1], (uint64_t)mx);
    if (r >= size) r = (int64_t)nsnp_philox_index(nsnp_philox4x32_10((uint32_t)(r - size), (uint32_t)c, draw, 1u, key0, key1).v[0], (uint64_t)size);
    r = r < size ? r : size - 1;
    int64_t at = plan[BAL_OFF + c] + r;
    at = at < 0 ? 0 : (at < N ? at : N - 1);
    samples[m] = (int64_t)list[at];
}

__global__ __launch_bounds__(EVL_BLOCK) void k_evl_compact(const int64_t* __restrict__ scan, const uint32_t* __restrict__ word, int64_t N,
                                                           uint32_t* __restrict__ cls, int64_t* __restrict__ center_idx)
{
    const int64_t n = (int64_t)blockIdx.x * EVL_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int64_t o = scan[n];
    if (scan[n + 1] == o || o < 0 || o >= N) return;         // (o lies in [0, N) by construction)
    cls[o] = word[n] & ~EVL_BAD;                             // bytes gt, zy, id1, id2 of row o
    center_idx[o] = (int64_t)NSNP_PILEUP_WINDOW * n + 16;
}

// ---- per-batch loss sums ----------------------------------------------------------------------
// one workgroup of 256 lanes per batch: lane t adds rows t, t + 256, ... of the batch in that order (float64), then the 256 partial sums of
// each head meet in a fixed binary tree in LDS.  Nothing depends on the grid or on timing.
// W: the heads of a row - 4 for the PileupModel (rows of 16 bytes), 2 for the HaplotypeModel (rows of 8 bytes); a row is one vector load.
template <int W>
__global__ __launch_bounds__(256) void k_evl_batch_loss(const float* __restrict__ site_loss, int64_t N, int64_t B, double* __restrict__ batch_sum)
{
    typedef float __attribute__((ext_vector_type(W))) row_t;
    __shared__ double part[W][256];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * B, r1 = r0 + B < N ? r0 + B : N;
    double s[W];
#pragma unroll
    for (int h = 0; h < W; ++h) s[h] = 0.0;
    for (int64_t r = r0 + tid; r < r1; r += 256) {
        const row_t v = *reinterpret_cast<const row_t*>(site_loss + r * W);
#pragma unroll
        for (int h = 0; h < W; ++h) s[h] += (double)v[h];
    }
#pragma unroll
    for (int h = 0; h < W; ++h) part[h][tid] = s[h];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int h = 0; h < W; ++h) part[h][tid] += part[h][tid + o];
        }
        __syncthreads();
    }
    if (tid < W) batch_sum[(int64_t)blockIdx.x * W + tid] = part[tid][0];
}

template <int W>
int batch_loss(nsnp_ctx* ctx, const float* site_loss, int64_t N, int64_t batch_size, double* batch_sum, void* stream)
{
    if (!ctx || N < 0 || batch_size < 1 || (N > 0 && (!site_loss || !batch_sum))) return NSNP_EINVAL;
    if (reinterpret_cast<uintptr_t>(site_loss) & (W * sizeof(float) - 1)) return NSNP_EINVAL;
    if (N == 0) return NSNP_OK;
    const int64_t nb = NSNP_CDIV(N, batch_size);
    if (nb > 0x7fffffffll) return NSNP_EINVAL;
    hipLaunchKernelGGL(k_evl_batch_loss<W>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, site_loss, N, batch_size, batch_sum);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

// scratch of a label pass: the int64 scan (N + 1 entries) and one word per row; grown behind a stream synchronisation
int label_scratch(nsnp_ctx* ctx, int64_t N, hipStream_t s, int64_t** scan, uint32_t** word)
{
    const size_t scan_bytes = (((size_t)N + 1) * sizeof(int64_t) + 15) & ~(size_t)15;
    const size_t need = scan_bytes + (size_t)N * sizeof(uint32_t) + 16;
    if (int rc = nsnp_scratch_reserve(ctx, &ctx->evl_tmp, &ctx->evl_tmp_bytes, need, need / 4, s)) return rc;
    *scan = (int64_t*)ctx->evl_tmp;
    *word = (uint32_t*)((uint8_t*)ctx->evl_tmp + scan_bytes);
    return NSNP_OK;
}

// scratch of a sample list (the same buffer): the scan, the two lists (N entries together), the scan's four counts, one word per row
int sample_scratch(nsnp_ctx* ctx, int64_t N, hipStream_t s, int64_t** scan, int64_t** list, int64_t** counts, uint32_t** word)
{
    const size_t scan_bytes = (((size_t)N + 1) * sizeof(int64_t) + 15) & ~(size_t)15;
    const size_t list_bytes = ((size_t)N + 4) * sizeof(int64_t);
    const size_t need = scan_bytes + list_bytes + (size_t)N * sizeof(uint32_t) + 16;
    if (int rc = nsnp_scratch_reserve(ctx, &ctx->evl_tmp, &ctx->evl_tmp_bytes, need, need / 4, s)) return rc;
    *scan = (int64_t*)ctx->evl_tmp;
    *list = (int64_t*)((uint8_t*)ctx->evl_tmp + scan_bytes);
    *counts = *list + N;
    *word = (uint32_t*)((uint8_t*)ctx->evl_tmp + scan_bytes + list_bytes);
    return NSNP_OK;
}

// scratch of a balanced sample list (the same buffer): the plan, cnt / base [blocks][64], the list (N rows, 32 bits each: N < 2^32)
int balance_scratch(nsnp_ctx* ctx, int64_t N, hipStream_t s, int64_t** plan, uint32_t** cnt, uint32_t** list)
{
    const size_t plan_bytes = (size_t)BAL_PLAN * sizeof(int64_t);
    const size_t cnt_bytes = (size_t)NSNP_CDIV(N, (int64_t)EVL_BLOCK) * BAL_BINS * sizeof(uint32_t);
    const size_t need = plan_bytes + cnt_bytes + (size_t)N * sizeof(uint32_t) + 16;
    if (int rc = nsnp_scratch_reserve(ctx, &ctx->evl_tmp, &ctx->evl_tmp_bytes, need, need / 4, s)) return rc;
    *plan = (int64_t*)ctx->evl_tmp;
    *cnt = (uint32_t*)((uint8_t*)ctx->evl_tmp + plan_bytes);
    *list = (uint32_t*)((uint8_t*)ctx->evl_tmp + plan_bytes + cnt_bytes);
    return NSNP_OK;
}

}  // namespace

void nsnp_pileup_eval_heads_launch(nsnp_ctx* ctx, int64_t n, const uint8_t* cls, float* site_loss, uint8_t* pred, int64_t* counters,
                                   float* logits, hipStream_t s)
{
    const PileupWeightsDev& pw = ctx->pw;
    int64_t gh = NSNP_CDIV(n, 16);
    if (gh > 2 * (int64_t)ctx->n_cu) gh = 2 * (int64_t)ctx->n_cu;          // persistent, as k_pileup_head_rs
    hipLaunchKernelGGL(k_pileup_head_eval, dim3((unsigned)gh), dim3(512), 0, s, ctx->ws_h1c, n, pw.proj_w, pw.proj_b, pw.dense_w, pw.dense_b,
                       pw.head6_w, pw.head6_b, cls, site_loss, pred, reinterpret_cast<unsigned long long*>(counters), logits);
}

extern "C" int nsnp_pileup_label_classes(nsnp_ctx* ctx, const int32_t* label, int64_t N, int variants_only, uint8_t* cls, int64_t* center_idx,
                                         int64_t* meta, void* stream)
{
    if (!ctx || !meta || N < 0 || (N > 0 && (!label || !cls || !center_idx))) return NSNP_EINVAL;
    if (reinterpret_cast<uintptr_t>(cls) & 3) return NSNP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int64_t* scan; uint32_t* word;
    if (const int rc = label_scratch(ctx, N, s, &scan, &word)) return rc;
    const unsigned grid = (unsigned)NSNP_CDIV(N, (int64_t)EVL_BLOCK);
    if (N > 0) hipLaunchKernelGGL(k_evl_flags, dim3(grid), dim3(EVL_BLOCK), 0, s, label, N, variants_only, scan, word);
    hipLaunchKernelGGL(k_evl_scan, dim3(1), dim3(1024), 0, s, scan, (const uint32_t*)word, N, meta);
    if (N > 0)
        hipLaunchKernelGGL(k_evl_compact, dim3(grid), dim3(EVL_BLOCK), 0, s, (const int64_t*)scan, (const uint32_t*)word, N,
                           reinterpret_cast<uint32_t*>(cls), center_idx);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

extern "C" int nsnp_pileup_batch_loss(nsnp_ctx* ctx, const float* site_loss, int64_t N, int64_t batch_size, double* batch_sum, void* stream)
{
    return batch_loss<4>(ctx, site_loss, N, batch_size, batch_sum, stream);
}

// ---- HaplotypeModel (include/nanosnp.h) --------------------------------------------------------
extern "C" int nsnp_hap_label_classes(nsnp_ctx* ctx, const int32_t* label, int64_t N, uint8_t* cls, int64_t* rows, int64_t* meta, void* stream)
{
    if (!ctx || !meta || N < 0 || (N > 0 && (!label || !cls || !rows))) return NSNP_EINVAL;
    int n_gt = 0, n_zy = 0;
    if (const int rc = nsnp_hap_dims(ctx, &n_gt, &n_zy)) return rc;           // (what is scorable depends on the loaded heads)
    hipStream_t s = (hipStream_t)stream;
    int64_t* scan; uint32_t* word;
    if (const int rc = label_scratch(ctx, N, s, &scan, &word)) return rc;
    const unsigned grid = (unsigned)NSNP_CDIV(N, (int64_t)EVL_BLOCK);
    if (N > 0) hipLaunchKernelGGL(k_hapl_flags, dim3(grid), dim3(EVL_BLOCK), 0, s, label, N, n_gt, n_zy, scan, word);
    hipLaunchKernelGGL(k_evl_scan, dim3(1), dim3(1024), 0, s, scan, (const uint32_t*)word, N, meta);
    if (N > 0) hipLaunchKernelGGL(k_hapl_compact, dim3(grid), dim3(EVL_BLOCK), 0, s, (const int64_t*)scan, (const uint32_t*)word, N, cls, rows);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

extern "C" int nsnp_hap_batch_loss(nsnp_ctx* ctx, const float* site_loss, int64_t N, int64_t batch_size, double* batch_sum, void* stream)
{
    return batch_loss<2>(ctx, site_loss, N, batch_size, batch_sum, stream);
}

// ---- HaplotypeModel training: the sample list of a pass (include/nanosnp.h) ---------------------------------------------------------------
extern "C" int nsnp_hap_train_samples(nsnp_ctx* ctx, const uint8_t* cls, int64_t kept, double pn_value, uint64_t seed, uint32_t draw,
                                      int64_t* samples, int64_t cap, int64_t* meta, void* stream)
{
    if (!ctx || !meta || kept < 0 || kept > 0xffffffffll || (kept > 0 && !cls)) return NSNP_EINVAL;
    if (!(pn_value >= 0.0) || !(pn_value <= NSNP_HAP_PN_VALUE_MAX)) return NSNP_EINVAL;          // (NaN fails both; a draw index is 32 bits)
    hipStream_t s = (hipStream_t)stream;
    int64_t n_ref = 0, n_var = 0;
    int64_t* list = nullptr;
    if (kept > 0) {
        int64_t *scan, *counts; uint32_t* word;
        if (const int rc = sample_scratch(ctx, kept, s, &scan, &list, &counts, &word)) return rc;
        const unsigned grid = (unsigned)NSNP_CDIV(kept, (int64_t)EVL_BLOCK);
        hipLaunchKernelGGL(k_haps_flags, dim3(grid), dim3(EVL_BLOCK), 0, s, cls, kept, scan, word);
        hipLaunchKernelGGL(k_evl_scan, dim3(1), dim3(1024), 0, s, scan, (const uint32_t*)word, kept, counts);
        hipLaunchKernelGGL(k_haps_lists, dim3(grid), dim3(EVL_BLOCK), 0, s, (const int64_t*)scan, kept, list);
        NSNP_HIP(ctx, hipGetLastError());
        int64_t host[4];                                      // the one wait of the entry: `cap` cannot be held against M without the counts
        NSNP_HIP(ctx, hipMemcpyAsync(host, counts, sizeof(host), hipMemcpyDeviceToHost, s));
        NSNP_HIP(ctx, hipStreamSynchronize(s));
        n_ref = host[2]; n_var = host[3];
        if (n_ref < 0 || n_var < 0 || n_ref + n_var != kept) return NSNP_EINVAL;
    }
    // int(len * pn_value) in float64, truncated, as Python computes it (dataset_dev.py:214,224); no draws without a variant (the except: branch)
    const int64_t blocks = NSNP_CDIV(n_ref, HAPS_REFS);
    const int64_t q_full = n_var > 0 ? (int64_t)((double)HAPS_REFS * pn_value) : 0;
    const int64_t q_tail = n_var > 0 && blocks > 0 ? (int64_t)((double)(n_ref - (blocks - 1) * HAPS_REFS) * pn_value) : 0;
    const int64_t M = blocks > 0 ? n_ref + (blocks - 1) * q_full + q_tail : 0;
    if (cap < M || (M > 0 && !samples)) return NSNP_EINVAL;
    const int64_t grid = NSNP_CDIV(M > 0 ? M : 1, (int64_t)EVL_BLOCK);
    if (grid > 0x7fffffffll) return NSNP_EINVAL;
    hipLaunchKernelGGL(k_haps_place, dim3((unsigned)grid), dim3(EVL_BLOCK), 0, s, (const int64_t*)list, n_ref, n_var, M, q_full,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw, samples, meta);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

// ---- PileupModel training: the balanced sample list of a pass (include/nanosnp.h) ----------------------------------------------------------
extern "C" int nsnp_pileup_balance_samples(nsnp_ctx* ctx, const uint8_t* cls, int64_t N, uint64_t seed, uint32_t draw, int64_t* samples,
                                           int64_t cap, int64_t* sizes, int64_t* meta, void* stream)
{
    if (!ctx || !meta || N < 0 || N > 0xffffffffll || (N > 0 && !cls)) return NSNP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int64_t* plan; uint32_t *cnt, *list;
    if (const int rc = balance_scratch(ctx, N, s, &plan, &cnt, &list)) return rc;
    const int64_t n_blocks = NSNP_CDIV(N, (int64_t)EVL_BLOCK);
    if (N > 0) hipLaunchKernelGGL(k_bal_count, dim3((unsigned)n_blocks), dim3(EVL_BLOCK), 0, s, cls, N, cnt);
    hipLaunchKernelGGL(k_bal_scan, dim3(1), dim3(BAL_SEGS * BAL_BINS), 0, s, cnt, n_blocks, plan);
    int64_t M = 0;
    if (N > 0) {
        hipLaunchKernelGGL(k_bal_lists, dim3((unsigned)n_blocks), dim3(EVL_BLOCK), 0, s, cls, N, (const uint32_t*)cnt, (const int64_t*)plan, list);
        NSNP_HIP(ctx, hipGetLastError());
        int64_t host[8];                                      // the one wait of the entry: `cap` cannot be held against M without the counts
        NSNP_HIP(ctx, hipMemcpyAsync(host, plan + BAL_META, sizeof(host), hipMemcpyDeviceToHost, s));
        NSNP_HIP(ctx, hipStreamSynchronize(s));
        M = host[0];
        if (M < 0 || M > 2 * N) return NSNP_EINVAL;           // (M <= 2 N by the rule)
    }
    if (cap < M || (M > 0 && !samples)) return NSNP_EINVAL;
    const int64_t grid = NSNP_CDIV(M > 0 ? M : 1, (int64_t)EVL_BLOCK);
    if (grid > 0x7fffffffll) return NSNP_EINVAL;              // (as nsnp_hap_train_samples; M <= 2 N < 2^33 gives at most 2^25 workgroups)
    hipLaunchKernelGGL(k_bal_place, dim3((unsigned)grid), dim3(EVL_BLOCK), 0, s, (const uint32_t*)list, (const int64_t*)plan, N, M,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw, samples, sizes, meta);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
