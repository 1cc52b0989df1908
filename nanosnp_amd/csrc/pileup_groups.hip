// pileup_groups.hip -- the stage-4 site groups from the pileup call rows, on the device.
//
// Restates select_hetesnp_homosnp.py:82-104,180-230 (every low-quality site with its `adjacent_size` nearest confident heterozygous
// neighbours on each side) over the [N,13] float64 call rows of nsnp_pileup_call_rows instead of the pileup.vcf the row writer formats
// from them (nsnp_vcf.c format_rows -> merge.parse_vcf_for_groups / merge.select_groups).  Integers and comparisons only: a QUAL
// threshold arrives as the float32 probability at which the host's own score first reaches it (merge.group_cuts), so no logarithm is
// evaluated here and none can disagree with glibc's in its last bit.
//
//   k_group_flags      one thread per row: is it written at all (predict.py:66-194 with the gt_output[ti] IndexError of short batches),
//                      is it in the dictionary, a candidate, a support -> one flag byte, the support bit as int32; keys that do not
//                      ascend inside a run -> status (64-bit atomicMin of the row: the smallest wins whatever the order of arrival)
//   k_gscan_*          three-launch exclusive int32 prefix sum (this unit's copy of the scan of hap_reads.hip)
//   k_support_compact  the flagged rows' indices, in order: the supports S[T], later the valid candidates V[G]
//   k_group_valid      one thread per row: a candidate with A supports on each side inside its own run
//   k_group_emit       one thread per (group, slot): row index and key of S[k - A .. k - 1], the candidate, S[k2 .. k2 + A - 1]
//   k_group_meta       {groups found, status, first offending row, supports}
// Every output cell has one writer.
#include "nsnp_common.hpp"

namespace {

constexpr int GR_BLOCK = 256;
constexpr int GS_PER = 8;                                  // elements per thread of the scan kernels
constexpr int GS_TILE = GR_BLOCK * GS_PER;                 // 2048
constexpr int ROW_DOUBLES = 13;
constexpr int64_t GR_MAX = 0x7FFFFFF0ll;                   // rows are indexed with int32

enum : uint8_t { F_WRITTEN = NSNP_GROUPS_WRITTEN, F_DICT = NSNP_GROUPS_DICT, F_CAND = NSNP_GROUPS_CANDIDATE, F_SUPPORT = NSNP_GROUPS_SUPPORT,
                 F_VALID = NSNP_GROUPS_GROUP };

// the cut table of merge.group_cuts as bit patterns: a non-negative float32 orders as its bits do
struct Cuts { uint32_t quality, support, lo, hi, neg_zero; };

__device__ __forceinline__ Cuts load_cuts(const float* __restrict__ cuts)
{
    Cuts c;
    c.quality = __float_as_uint(cuts[0]); c.support = __float_as_uint(cuts[1]);
    c.lo = __float_as_uint(cuts[2]); c.hi = __float_as_uint(cuts[3]); c.neg_zero = __float_as_uint(cuts[4]);
    return c;
}

// the bits of a probability as the comparisons take them: -0.0 counts as 0.0 where the host scores it so (score_mode 1); every other
// negative value and every NaN has bits above any cut's and above `hi`
__device__ __forceinline__ uint32_t prob_bits(double v, const Cuts& c)
{
    const uint32_t b = __float_as_uint((float)v);
    return (b == 0x80000000u && c.neg_zero) ? 0u : b;
}
__device__ __forceinline__ bool has_score(uint32_t b, const Cuts& c) { return b >= c.lo && b <= c.hi; }

// the run [lo, hi) that holds row i: run_off ascends from 0 to N; whatever it holds, lo <= i < hi <= N comes back
__device__ __forceinline__ void run_of(const int64_t* __restrict__ run_off, int n_runs, int64_t i, int64_t N, int64_t* lo, int64_t* hi)
{
    int a = 0, b = n_runs;                                 // first run whose end lies behind i
    while (a < b) { const int m = a + ((b - a) >> 1); if (run_off[m + 1] <= i) a = m + 1; else b = m; }
    if (a >= n_runs) a = n_runs - 1;
    int64_t l = run_off[a], h = run_off[a + 1];
    if (l < 0) l = 0;
    if (l > i) l = i;
    if (h > N) h = N;
    if (h < i + 1) h = i + 1;
    *lo = l; *hi = h;
}

__global__ __launch_bounds__(GR_BLOCK) void k_group_flags(
    const double* __restrict__ rows, const uint8_t* __restrict__ ref_base, int64_t N, const int64_t* __restrict__ run_off, int n_runs,
    int64_t batch_size, const float* __restrict__ cuts, uint8_t* __restrict__ flag, int32_t* __restrict__ support,
    unsigned long long* __restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (i >= N) return;
    const Cuts c = load_cuts(cuts);
    const double* r = rows + i * ROW_DOUBLES;
    int64_t lo, hi;
    run_of(run_off, n_runs, i, N, &lo, &hi);
    if (i > lo && !((int64_t)r[0] > (int64_t)r[0 - ROW_DOUBLES])) atomicMin(key, (unsigned long long)i);

    uint8_t f = 0;
    const double gd = r[1], zd = r[2];
    if (gd >= 0.0 && gd < 10.0 && zd >= 0.0 && zd <= 2.0) {                       // predict.py:68-69 (a NaN fails every comparison)
        const int g = (int)gd, z = (int)zd;
        const uint32_t gb = prob_bits(r[3], c), zb = prob_bits(r[4], c);
        // GT_LABELS[g], g < 10: the pairs of ACGT in order -> the two letters as indices
        const int l0 = g < 4 ? 0 : g < 7 ? 1 : g < 9 ? 2 : 3;
        const int l1 = g < 4 ? g : g < 7 ? g - 3 : g < 9 ? g - 5 : 3;
        const uint32_t sref = ref_base[i] & 0xDFu;                               // upper case
        const int si = sref == 'A' ? 0 : sref == 'C' ? 1 : sref == 'G' ? 2 : sref == 'T' ? 3 : -1;
        const int al = (l0 != si) + (l1 != si);
        bool written = has_score(gb, c) && has_score(zb, c);
        if (written && al == 0 && z != 0) {                                      // the gt_output[ti] search: IndexError in a short batch
            const int64_t at = i - lo, start = at - at % batch_size;
            const int64_t B = (hi - lo) - start < batch_size ? (hi - lo) - start : batch_size;
            const int64_t need = z == 2 ? 8 : (si == 3 ? 7 : 9);                 // the largest index the search reads
            if (B <= need) written = false;
        }
        if (written) {
            const bool two_alts = al == 2 && l0 != l1;
            const bool hom = z != 2 && !two_alts;                                // genotype text 0/0 or 1/1 ('1/2' otherwise, '0/1' for z == 2)
            const bool use_zy = al == 0 && z != 0, use_gt = al > 0 && z == 0;    // QUAL = zy_qual, gt_qual, else the smaller of both
            const bool q_hi = use_zy ? zb >= c.quality : use_gt ? gb >= c.quality : (gb >= c.quality && zb >= c.quality);
            const bool q_sup = use_zy ? zb >= c.support : use_gt ? gb >= c.support : (gb >= c.support && zb >= c.support);
            f = F_WRITTEN;
            if (!(hom && q_hi)) {
                f |= F_DICT;
                if (!q_hi) f |= F_CAND;
                if (z == 2 && q_sup) f |= F_SUPPORT;
            }
        }
    }
    flag[i] = f;
    support[i] = (f & F_SUPPORT) ? 1 : 0;
}

// ---- int32 exclusive prefix sum over n elements in three launches ----------------------------------------------------------------
__device__ __forceinline__ int block_exclusive_i32(int v, int* total, int32_t* sh /* [4] */)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    __syncthreads();                                        // (sh may still be read from an earlier call)
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int q = 0; q < GR_BLOCK / 64; ++q) { const int t = sh[q]; if (q < w) before += t; all += t; }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(GR_BLOCK) void k_gscan_tile_sums(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ sums)
{
    __shared__ int32_t sh[GR_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * GS_TILE;
    int v = 0;
    for (int j = 0; j < GS_PER; ++j) { const int64_t i = base + (int64_t)j * GR_BLOCK + threadIdx.x; if (i < n) v += in[i]; }
    int total;
    (void)block_exclusive_i32(v, &total, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nb) -> their exclusive prefix in place, the grand total widened in *total64
__global__ __launch_bounds__(GR_BLOCK) void k_gscan_sums(int32_t* __restrict__ sums, int64_t nb, int64_t* __restrict__ total64)
{
    __shared__ int32_t sh[GR_BLOCK / 64];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += GR_BLOCK) {
        const int64_t i = b0 + threadIdx.x;
        const int v = i < nb ? sums[i] : 0;
        int total;
        const int ex = block_exclusive_i32(v, &total, sh);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total64 = carry;
}

// io[i] = the sum of the elements in front of i (in place: a thread reads its eight elements before it writes them)
__global__ __launch_bounds__(GR_BLOCK) void k_gscan_apply(int32_t* io, int64_t n, const int32_t* __restrict__ sums)
{
    __shared__ int32_t sh[GR_BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * GS_TILE + (int64_t)threadIdx.x * GS_PER;
    int v[GS_PER], s = 0;
    for (int j = 0; j < GS_PER; ++j) { v[j] = base + j < n ? io[base + j] : 0; s += v[j]; }
    int total;
    int run = sums[blockIdx.x] + block_exclusive_i32(s, &total, sh);
    for (int j = 0; j < GS_PER; ++j) {
        if (base + j < n) io[base + j] = run;
        run += v[j];
    }
}

// the rows with `mask` in their flag byte, in row order: prefix[i] of them lie in front of row i
__global__ __launch_bounds__(GR_BLOCK) void k_support_compact(const uint8_t* __restrict__ flag, uint8_t mask,
                                                              const int32_t* __restrict__ prefix, int64_t N, int32_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (i < N && (flag[i] & mask)) out[prefix[i]] = (int32_t)i;              // prefix[i] < the count <= N
}

__global__ __launch_bounds__(GR_BLOCK) void k_group_valid(
    uint8_t* __restrict__ flag, const int32_t* __restrict__ prefix, const int32_t* __restrict__ S, const int64_t* __restrict__ n_support,
    int64_t N, const int64_t* __restrict__ run_off, int n_runs, int A, int32_t* __restrict__ valid)
{
    const int64_t i = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (i >= N) return;
    const uint8_t f = flag[i];
    int ok = 0;
    if (f & F_CAND) {
        const int64_t T = *n_support;
        const int64_t k = prefix[i], k2 = k + ((f & F_SUPPORT) ? 1 : 0);         // supports strictly left of i: S[0 .. k); right: S[k2 ..)
        if (k >= A && k2 + A <= T) {
            int64_t lo, hi;
            run_of(run_off, n_runs, i, N, &lo, &hi);
            ok = S[k - A] >= lo && S[k2 + A - 1] < hi;
        }
    }
    valid[i] = ok;
    if (ok) flag[i] = f | F_VALID;
}

__global__ __launch_bounds__(GR_BLOCK) void k_group_emit(
    const double* __restrict__ rows, const uint8_t* __restrict__ flag, const int32_t* __restrict__ prefix, const int32_t* __restrict__ S,
    const int32_t* __restrict__ V, const int64_t* __restrict__ n_groups, int64_t cap_groups, int A,
    int32_t* __restrict__ group_rows, int64_t* __restrict__ group_keys)
{
    const int W = 2 * A + 1;
    const int64_t t = (int64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    const int64_t G = *n_groups < cap_groups ? *n_groups : cap_groups;
    const int64_t gi = t / W;
    if (gi >= G) return;
    const int slot = (int)(t - gi * W);
    const int32_t i = V[gi];
    const int64_t k = prefix[i], k2 = k + ((flag[i] & F_SUPPORT) ? 1 : 0);
    const int32_t src = slot < A ? S[k - A + slot] : slot == A ? i : S[k2 + (slot - A - 1)];
    group_rows[t] = src;
    group_keys[t] = (int64_t)rows[(int64_t)src * ROW_DOUBLES];
}

// all null: no row, nothing found and nothing looked at
__global__ void k_group_meta(const int64_t* __restrict__ n_groups, const int64_t* __restrict__ n_support,
                             const unsigned long long* __restrict__ key, int64_t* __restrict__ meta)
{
    if (threadIdx.x || blockIdx.x) return;
    if (!key) { meta[0] = 0; meta[1] = 0; meta[2] = 0; meta[3] = 0; return; }
    const unsigned long long k = *key;
    meta[0] = *n_groups;
    meta[1] = k == ~0ull ? NSNP_GROUPS_OK : NSNP_GROUPS_KEY_ORDER;
    meta[2] = k == ~0ull ? -1 : (int64_t)k;
    meta[3] = *n_support;
}

// ---- scratch layout -----------------------------------------------------------------------------------------------------------------
struct GroupScratch {
    unsigned long long* key;
    int64_t *n_support, *n_groups;
    int32_t *pre, *S, *gpre, *V, *sums;
    uint8_t* flag;
    size_t bytes;
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

GroupScratch group_scratch(void* base, int64_t N)
{
    GroupScratch s;
    char* p = (char*)base;
    size_t o = 0;
    const size_t nb = (size_t)NSNP_CDIV(N, (int64_t)GS_TILE);
    s.flag = (uint8_t*)(p + o); o += align16((size_t)N);                  // first: the caller may read the flag bytes (include/nanosnp.h)
    s.key = (unsigned long long*)(p + o); s.n_support = (int64_t*)(p + o + 8); s.n_groups = (int64_t*)(p + o + 16); o += 32;
    s.pre = (int32_t*)(p + o); o += align16((size_t)N * 4);
    s.S = (int32_t*)(p + o); o += align16((size_t)N * 4);
    s.gpre = (int32_t*)(p + o); o += align16((size_t)N * 4);
    s.V = (int32_t*)(p + o); o += align16((size_t)N * 4);
    s.sums = (int32_t*)(p + o); o += align16((nb + 1) * 4);
    s.bytes = o;
    return s;
}

void scan_exclusive_i32(int32_t* io, int64_t n, int32_t* sums, int64_t* total64, hipStream_t s)
{
    const int64_t nb = NSNP_CDIV(n, (int64_t)GS_TILE);
    hipLaunchKernelGGL(k_gscan_tile_sums, dim3((unsigned)nb), dim3(GR_BLOCK), 0, s, (const int32_t*)io, n, sums);
    hipLaunchKernelGGL(k_gscan_sums, dim3(1), dim3(GR_BLOCK), 0, s, sums, nb, total64);
    hipLaunchKernelGGL(k_gscan_apply, dim3((unsigned)nb), dim3(GR_BLOCK), 0, s, io, n, (const int32_t*)sums);
}

}  // namespace

extern "C" size_t nsnp_pileup_groups_scratch_bytes(int64_t N)
{
    if (N < 0 || N > GR_MAX) return 0;
    return group_scratch(nullptr, N).bytes;
}

extern "C" int nsnp_pileup_select_groups(nsnp_ctx* ctx, const double* rows, const uint8_t* ref_base, int64_t N, const int64_t* run_off,
                                         int n_runs, int64_t batch_size, int adjacent_size, const float* cuts, int32_t* group_rows,
                                         int64_t* group_keys, int64_t cap_groups, int64_t* meta, void* scratch, void* stream)
{
    if (!ctx || N < 0 || adjacent_size < 1 || adjacent_size > 32 || batch_size < 1 || n_runs < 0 || cap_groups < 0) return NSNP_EINVAL;
    if (N > GR_MAX) return NSNP_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (meta) {
            hipLaunchKernelGGL(k_group_meta, dim3(1), dim3(64), 0, s, (const int64_t*)nullptr, (const int64_t*)nullptr,
                               (const unsigned long long*)nullptr, meta);
            NSNP_HIP(ctx, hipGetLastError());
        }
        return NSNP_OK;
    }
    if (!rows || !ref_base || !run_off || !cuts || !meta || !scratch || n_runs < 1) return NSNP_EINVAL;   // (no run: no row has a contig)
    if (cap_groups > 0 && (!group_rows || !group_keys)) return NSNP_EINVAL;
    const int W = 2 * adjacent_size + 1;
    if (cap_groups > GR_MAX / W) cap_groups = GR_MAX / W;                                   // (more groups than rows cannot be)
    const GroupScratch sc = group_scratch(scratch, N);
    const unsigned row_blocks = (unsigned)NSNP_CDIV(N, (int64_t)GR_BLOCK);
    NSNP_HIP(ctx, hipMemsetAsync(sc.key, 0xFF, 8, s));
    hipLaunchKernelGGL(k_group_flags, dim3(row_blocks), dim3(GR_BLOCK), 0, s, rows, ref_base, N, run_off, n_runs, batch_size, cuts,
                       sc.flag, sc.pre, sc.key);
    scan_exclusive_i32(sc.pre, N, sc.sums, sc.n_support, s);
    hipLaunchKernelGGL(k_support_compact, dim3(row_blocks), dim3(GR_BLOCK), 0, s, (const uint8_t*)sc.flag, (uint8_t)F_SUPPORT,
                       (const int32_t*)sc.pre, N, sc.S);
    hipLaunchKernelGGL(k_group_valid, dim3(row_blocks), dim3(GR_BLOCK), 0, s, sc.flag, (const int32_t*)sc.pre, (const int32_t*)sc.S,
                       (const int64_t*)sc.n_support, N, run_off, n_runs, adjacent_size, sc.gpre);
    scan_exclusive_i32(sc.gpre, N, sc.sums, sc.n_groups, s);
    hipLaunchKernelGGL(k_support_compact, dim3(row_blocks), dim3(GR_BLOCK), 0, s, (const uint8_t*)sc.flag, (uint8_t)F_VALID,
                       (const int32_t*)sc.gpre, N, sc.V);
    const int64_t slots = (cap_groups < N ? cap_groups : N) * W;                            // a thread per slot the outputs can hold
    if (slots > 0) {
        hipLaunchKernelGGL(k_group_emit, dim3((unsigned)NSNP_CDIV(slots, (int64_t)GR_BLOCK)), dim3(GR_BLOCK), 0, s, rows,
                           (const uint8_t*)sc.flag, (const int32_t*)sc.pre, (const int32_t*)sc.S, (const int32_t*)sc.V,
                           (const int64_t*)sc.n_groups, cap_groups, adjacent_size, group_rows, group_keys);
    }
    hipLaunchKernelGGL(k_group_meta, dim3(1), dim3(64), 0, s, (const int64_t*)sc.n_groups, (const int64_t*)sc.n_support,
                       (const unsigned long long*)sc.key, meta);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
