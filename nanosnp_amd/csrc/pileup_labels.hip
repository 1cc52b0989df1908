// pileup_labels.hip -- the training label of every selected site of a chunk, and the subsample of its non-variant sites (<chr>.td.bin).
//
// Replaces, for sites that are already selected in HBM,
//   the Y map lookup + output_labels_from_reference   dna_sv_tensor/src/make_train_data/main.cpp:287-317, common/genotype.cpp:282-304
//   the draw against non_variant_subsample_ratio      dna_sv_tensor/src/make_train_data/main.cpp:289
//   the count of calc_non_variant_subsample_ratio     dna_sv_tensor/src/make_train_data/main.cpp:143-153
// The truth VCF itself is read on the host (nanosnp_amd/truth.py: a few million rows, once): what arrives here is its sorted keys and one
// packed label code per key.
//
// nsnp_pileup_label_sites_keys, four launches:
//   k_label_sites    one lane per site: binary search of its key, its code and whether it is kept   -> scratch; count mode: the counters
//   k_label_scan     exclusive prefix sums of the kept flags (one block), the sums, meta            -> scratch, meta
//   k_label_compact  the kept centres and their codes, in order                                     -> out_center_idx, scratch
//   k_label_write    the one-hot rows, flat: a thread owns 16 bytes of the output whatever row they belong to (the label may be pinned
//                    host memory); the number of rows is read from the device
// The subsample is a function of the key and the seed alone (integer arithmetic): the kept set does not depend on the chunk layout.
#include "nsnp_common.hpp"

namespace {

constexpr int LAB_BLOCK = 256;
constexpr int LAB_W = NSNP_LABEL_WIDTH;                      // 90 = 21 + 3 + 33 + 33
constexpr int64_t LAB_POS_MASK = (1ll << NSNP_TOK_KEY_SHIFT) - 1;
constexpr uint32_t LAB_TRUTH = 1u << 30, LAB_BAD = 1u << 31;  // beside the code in the scratch word of a site
constexpr uint32_t LAB_CODE_MASK = 0x3f3f031fu;              // gt21 | zygosity << 8 | length 1 << 16 | length 2 << 24

// the label of a site no truth row names: homozygous reference of its base (output_labels_from_reference), lengths 0 + 16
__device__ __forceinline__ uint32_t reference_code(int base, bool& bad)
{
    const int b = base & ~0x20;                              // (toupper for the letters that count)
    int gt = 0;
    if (b == 'A') gt = 0; else if (b == 'C') gt = 4; else if (b == 'G') gt = 7; else if (b == 'T') gt = 9; else bad = true;
    return (uint32_t)gt | (16u << 16) | (16u << 24);
}

__device__ __forceinline__ uint64_t label_hash(int64_t key, uint64_t seed)
{
    uint64_t z = (uint64_t)key + seed * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__global__ __launch_bounds__(LAB_BLOCK) void k_label_sites(const int64_t* __restrict__ key, int64_t M, const int64_t* __restrict__ center_idx, int64_t N,
                                                           const uint8_t* __restrict__ genome, const int64_t* __restrict__ seq_off, int64_t n_contigs,
                                                           const int64_t* __restrict__ truth_key, const uint32_t* __restrict__ truth_code, int64_t T,
                                                           const uint64_t* __restrict__ thr, uint64_t seed, int64_t* __restrict__ keep,
                                                           uint32_t* __restrict__ info, int64_t* __restrict__ counts)
{
    // count mode: the sites of a block nearly always share one contig - its two counters are summed in LDS, the others go straight out
    __shared__ unsigned long long blk[2];
    __shared__ int64_t blk_cid;
    const int64_t n = (int64_t)blockIdx.x * LAB_BLOCK + threadIdx.x;
    if (counts && threadIdx.x == 0) { blk[0] = 0; blk[1] = 0; blk_cid = -1; }
    bool bad = false;
    int64_t cid = -1;
    uint32_t word = 0;
    if (n < N) {
        int64_t c = center_idx[n];
        if (c < 0 || c >= M) { c = c < 0 ? 0 : M - 1; bad = true; }          // (a centre outside the columns: clamped, never followed)
        const int64_t k = key[c];
        cid = k >> NSNP_TOK_KEY_SHIFT;
        int64_t p = k & LAB_POS_MASK;
        if (k < 0 || cid >= n_contigs) { cid = 0; p = 1; bad = true; }       // (a filler key or a contig outside the table)
        const int64_t o = seq_off[cid], len = seq_off[cid + 1] - o;
        int base = 'A';
        if (p < 1 || p > len) bad = true;                                    // (outside the site's own contig: no base is read)
        else base = genome[o + p - 1];
        // lower bound of the key among the truth keys
        int64_t lo = 0, hi = T;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (truth_key[mid] < k) lo = mid + 1; else hi = mid;
        }
        const bool hit = !bad && lo < T && truth_key[lo] == k;
        bool ref_bad = false;
        const uint32_t ref = reference_code(base, ref_bad);
        // (a site is only ever emitted at A/C/G/T, make_candidate_snp_tensor/main.cpp:196: any other byte is reported, for a truth site too)
        bad |= ref_bad;
        word = hit ? (truth_code[lo] & LAB_CODE_MASK) | LAB_TRUTH : ref;
        if (bad) word |= LAB_BAD;
        const bool kept = hit || !thr || (label_hash(k, seed) >> 11) < thr[cid];
        keep[n] = kept ? 1 : 0;
        info[n] = word;
    }
    if (counts) {
        __syncthreads();
        if (n < N && threadIdx.x == 0) blk_cid = cid;
        __syncthreads();
        if (n < N) {
            const int which = (word & LAB_TRUTH) ? 0 : 1;
            if (cid == blk_cid) atomicAdd(&blk[which], 1ull);
            else atomicAdd(reinterpret_cast<unsigned long long*>(counts) + 2 * cid + which, 1ull);
        }
        __syncthreads();
        if (threadIdx.x < 2 && blk_cid >= 0 && blk[threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long*>(counts) + 2 * blk_cid + threadIdx.x, blk[threadIdx.x]);
    }
}

// exclusive scan of the kept flags by one block, in place (k_alt_scan's scheme); meta = { kept, truth sites, other sites, status }
__global__ __launch_bounds__(1024) void k_label_scan(int64_t* __restrict__ keep, const uint32_t* __restrict__ info, int64_t N, int64_t* __restrict__ meta)
{
    __shared__ int64_t part[1024];
    __shared__ unsigned long long n_truth;
    __shared__ int any_bad;
    const int tid = threadIdx.x;
    if (tid == 0) { n_truth = 0; any_bad = 0; }
    const int64_t per = NSNP_CDIV(N, (int64_t)1024);
    const int64_t n0 = tid * per < N ? tid * per : N, n1 = n0 + per < N ? n0 + per : N;
    int64_t s = 0, t = 0;
    bool bad = false;
    for (int64_t n = n0; n < n1; ++n) { s += keep[n]; const uint32_t w = info[n]; t += (w & LAB_TRUTH) ? 1 : 0; bad |= (w & LAB_BAD) != 0; }
    part[tid] = s;
    __syncthreads();
    if (t) atomicAdd(&n_truth, (unsigned long long)t);
    if (bad) atomicOr(&any_bad, 1);
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
        meta[0] = part[1023]; meta[1] = (int64_t)n_truth; meta[2] = N - (int64_t)n_truth; meta[3] = any_bad;
    }
}

__global__ __launch_bounds__(LAB_BLOCK) void k_label_compact(const int64_t* __restrict__ scan, const uint32_t* __restrict__ info,
                                                             const int64_t* __restrict__ center_idx, int64_t N, int64_t* __restrict__ out_center_idx,
                                                             uint32_t* __restrict__ kept_code)
{
    const int64_t n = (int64_t)blockIdx.x * LAB_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int64_t o = scan[n];
    if (scan[n + 1] == o || o < 0 || o >= N) return;         // (o lies in [0, N) by construction)
    out_center_idx[o] = center_idx[n];
    kept_code[o] = info[n];
}

__device__ __forceinline__ int one_hot(uint32_t code, int c)
{
    const int gt = code & 0x1f, zy = (code >> 8) & 3, l1 = (code >> 16) & 0x3f, l2 = (code >> 24) & 0x3f;
    return (c == gt) | (c == 21 + zy) | (c == 24 + l1) | (c == 57 + l2);
}

__global__ __launch_bounds__(LAB_BLOCK) void k_label_write(const uint32_t* __restrict__ kept_code, const int64_t* __restrict__ total_p, int64_t N,
                                                           int32_t* __restrict__ label)
{
    int64_t rows = *total_p;
    if (rows > N) rows = N;                                  // (never beyond what the caller's buffer holds)
    const int64_t total = rows * LAB_W;
    for (int64_t e = ((int64_t)blockIdx.x * LAB_BLOCK + threadIdx.x) * 4; e < total; e += (int64_t)gridDim.x * LAB_BLOCK * 4) {
        int64_t r = e / LAB_W;
        int c = (int)(e - r * LAB_W);
        uint32_t code = kept_code[r];
        i32x4 v;
        int w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = e + j < total ? one_hot(code, c) : 0;
            if (++c == LAB_W && r + 1 < rows) { c = 0; ++r; code = kept_code[r]; }
        }
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        if (e + 4 <= total) *reinterpret_cast<i32x4*>(label + e) = v;
        else for (int j = 0; j < 4; ++j) if (e + j < total) label[e + j] = w[j];
    }
}

}  // namespace

extern "C" int nsnp_pileup_label_sites_keys(nsnp_ctx* ctx, const int64_t* key, int64_t M, const int64_t* center_idx, int64_t N, const uint8_t* genome,
                                            const int64_t* seq_off, int64_t n_contigs, const int64_t* truth_key, const uint32_t* truth_code, int64_t T,
                                            const uint64_t* keep_thr, uint64_t seed, int64_t* out_center_idx, int32_t* label, int64_t* counts,
                                            int64_t* meta, void* stream)
{
    if (!ctx || !meta || N < 0 || M < 0 || T < 0 || n_contigs < 0 || n_contigs > NSNP_TOK_MAX_CONTIGS) return NSNP_EINVAL;
    if (N > 0 && (!key || !center_idx || M < 1 || n_contigs < 1 || !genome || !seq_off || (T > 0 && (!truth_key || !truth_code)))) return NSNP_EINVAL;
    if (label && !out_center_idx) return NSNP_EINVAL;
    if (reinterpret_cast<uintptr_t>(label) & 15) return NSNP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // scratch of its own (this entry may run on another stream than nsnp_pileup_alt_info): N + 1 scanned flags, then two words per site
    const size_t scan_bytes = (((size_t)N + 1) * sizeof(int64_t) + 15) & ~(size_t)15;
    const size_t word_bytes = ((size_t)N * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t need = scan_bytes + 2 * word_bytes + 16;
    if (int rc = nsnp_scratch_reserve(ctx, &ctx->lab_tmp, &ctx->lab_tmp_bytes, need, need / 4, s)) return rc;
    int64_t* scan = (int64_t*)ctx->lab_tmp;
    uint32_t* info = (uint32_t*)((uint8_t*)ctx->lab_tmp + scan_bytes);
    uint32_t* kept_code = (uint32_t*)((uint8_t*)ctx->lab_tmp + scan_bytes + word_bytes);
    const unsigned grid = (unsigned)NSNP_CDIV(N, (int64_t)LAB_BLOCK);
    if (N > 0)
        hipLaunchKernelGGL(k_label_sites, dim3(grid), dim3(LAB_BLOCK), 0, s, key, M, center_idx, N, genome, seq_off, n_contigs, truth_key, truth_code, T,
                           keep_thr, seed, scan, info, counts);
    hipLaunchKernelGGL(k_label_scan, dim3(1), dim3(1024), 0, s, scan, (const uint32_t*)info, N, meta);
    if (N > 0 && out_center_idx) {
        hipLaunchKernelGGL(k_label_compact, dim3(grid), dim3(LAB_BLOCK), 0, s, (const int64_t*)scan, (const uint32_t*)info, center_idx, N, out_center_idx,
                           kept_code);
        if (label) {
            int64_t blocks = NSNP_CDIV(N * LAB_W, (int64_t)LAB_BLOCK * 4);
            if (blocks > 4096) blocks = 4096;
            hipLaunchKernelGGL(k_label_write, dim3((unsigned)blocks), dim3(LAB_BLOCK), 0, s, (const uint32_t*)kept_code, (const int64_t*)(scan + N), N, label);
        }
    }
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
