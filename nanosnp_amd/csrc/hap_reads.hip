// hap_reads.hip -- the stage-4 read matrices from decoded alignment records.
//
// Replaces the two pileup passes of single_group_pileup_haplotype_feature (HaplotypeModel/create_pileup_haplotype.py:39-60 the
// coverage filter, :89-134 one row per read over the wanted columns) for records that are already in memory as a struct of arrays
// (readmatrix.AlignmentRecords: start, mapq, hp, BAM-encoded CIGARs, bases, qualities, in coordinate order).  Integers only.
//
//   k_read_spans        one wave per record: the reference length of its CIGAR -> its span [a, b]; the index range [lo, hi) of the
//                       sorted wanted columns inside the span (two binary searches); +1 / -1 into a difference array over the
//                       columns (integer atomics: the sums do not depend on the order); flag = the record covers a column
//   k_scan_*            three-launch int32 prefix sum (tile sums, one-workgroup scan of the sums, rescan with the offset): the
//                       difference array -> depth per column, the flags -> row of every record (rows are a prefix count because the
//                       starts are sorted) and the row count
//   k_read_depth_check  a column deeper than max_coverage -> status
//   k_read_fill         one workgroup per covering record: its row of the four matrices, every cell written once (zeros outside
//                       [lo, hi) included).  The CIGAR is taken in tiles of 1024 ops: reference / query prefix sums of the tile in
//                       LDS, carried across tiles; the wanted columns that fall into the tile's reference range are a contiguous
//                       run of [lo, hi), one lane per column searches the tile's prefix for the op that holds it.
//   k_read_meta         {rows, status, record, column}
//
// The first offence is the smallest key (column index, record + 1 or 0 for a deep column, kind), the order in which the host
// function meets them: found with a 64-bit atomicMin, so it does not depend on the order of arrival either.
#include "nsnp_common.hpp"

namespace {

constexpr int RD_BLOCK = 256;
constexpr int RD_TILE = 1024;                              // CIGAR ops per tile of k_read_fill: 4 per thread
constexpr int SC_PER = 8;                                  // elements per thread of the scan kernels
constexpr int SC_TILE = RD_BLOCK * SC_PER;                 // 2048

// BAM ops MIDNSHP=X = 0..8: M, D, N, =, X consume the reference; M, I, S, =, X consume the query
__device__ __forceinline__ bool op_ref(uint32_t code) { return (0x18Du >> code) & 1u; }      // bits 0, 2, 3, 7, 8
__device__ __forceinline__ bool op_query(uint32_t code) { return (0x193u >> code) & 1u; }    // bits 0, 1, 4, 7, 8
__device__ __forceinline__ bool op_match(uint32_t code) { return (0x181u >> code) & 1u; }    // bits 0, 7, 8

__device__ __forceinline__ unsigned long long offence_key(int c, int64_t rec_plus_1, int kind)
{
    return ((unsigned long long)c << 33) | ((unsigned long long)rec_plus_1 << 2) | (unsigned long long)kind;
}

// first index in [lo, hi) with cols[i] >= v
__device__ __forceinline__ int lower_bound_cols(const int64_t* __restrict__ cols, int lo, int hi, int64_t v)
{
    while (lo < hi) {
        const int m = lo + ((hi - lo) >> 1);
        if (cols[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(RD_BLOCK) void k_read_spans(
    const int64_t* __restrict__ start, const uint32_t* __restrict__ cigar, const int64_t* __restrict__ cigar_off, int64_t R,
    const int64_t* __restrict__ cols, int P, int32_t* __restrict__ lo_out, int32_t* __restrict__ hi_out, int32_t* __restrict__ flag,
    int32_t* __restrict__ diff)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (RD_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t o0 = cigar_off[r], o1 = cigar_off[r + 1];
    int64_t len = 0;
    for (int64_t i = o0 + lane; i < o1; i += 64) {
        const uint32_t op = cigar[i];
        len += op_ref(op & 15u) ? (int64_t)(op >> 4) : 0;
    }
    len = wave_sum(len);
    if (lane == 0) {
        const int64_t a = start[r];
        const int lo = lower_bound_cols(cols, 0, P, a);
        const int hi = len > 0 ? lower_bound_cols(cols, lo, P, a + len) : lo;      // columns <= b = a + len - 1
        lo_out[r] = lo; hi_out[r] = hi; flag[r] = hi > lo;
        if (hi > lo) { atomicAdd(&diff[lo], 1); atomicAdd(&diff[hi], -1); }         // diff has P + 1 entries
    }
}

// ---- int32 prefix sum over n elements in three launches --------------------------------------------------------------------------
__device__ __forceinline__ int block_exclusive_i32(int v, int* total, int32_t* sh /* [5] */)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    __syncthreads();                                        // (sh may still be read from an earlier call)
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int q = 0; q < RD_BLOCK / 64; ++q) { const int t = sh[q]; if (q < w) before += t; all += t; }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(RD_BLOCK) void k_scan_tile_sums(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ sums)
{
    __shared__ int32_t sh[5];
    const int64_t base = (int64_t)blockIdx.x * SC_TILE;
    int v = 0;
    for (int j = 0; j < SC_PER; ++j) { const int64_t i = base + (int64_t)j * RD_BLOCK + threadIdx.x; if (i < n) v += in[i]; }
    int total;
    (void)block_exclusive_i32(v, &total, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nb) -> their exclusive prefix in place, the grand total in sums[nb] and, widened, in *total64 (optional)
__global__ __launch_bounds__(RD_BLOCK) void k_scan_sums(int32_t* __restrict__ sums, int64_t nb, int64_t* __restrict__ total64)
{
    __shared__ int32_t sh[5];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += RD_BLOCK) {
        const int64_t i = b0 + threadIdx.x;
        const int v = i < nb ? sums[i] : 0;
        int total;
        const int ex = block_exclusive_i32(v, &total, sh);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { sums[nb] = carry; if (total64) *total64 = carry; }
}

// out[i] = the prefix sum of in up to and with (inclusive) or without (exclusive) element i; out may be in
__global__ __launch_bounds__(RD_BLOCK) void k_scan_apply(const int32_t* in, int64_t n, const int32_t* __restrict__ sums, int inclusive,
                                                         int32_t* out)
{
    __shared__ int32_t sh[5];
    const int64_t base = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_PER;
    int v[SC_PER], s = 0;
    for (int j = 0; j < SC_PER; ++j) { v[j] = base + j < n ? in[base + j] : 0; s += v[j]; }
    int total;
    int run = sums[blockIdx.x] + block_exclusive_i32(s, &total, sh);
    for (int j = 0; j < SC_PER; ++j) {
        if (base + j < n) out[base + j] = inclusive ? run + v[j] : run;
        run += v[j];
    }
}

__global__ __launch_bounds__(RD_BLOCK) void k_read_depth_check(const int32_t* __restrict__ depth, int P, int max_coverage,
                                                               unsigned long long* __restrict__ key)
{
    const int64_t c = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (c < P && depth[c] > 0 && depth[c] > max_coverage) atomicMin(key, offence_key((int)c, 0, NSNP_READS_TOO_DEEP));
}

__global__ __launch_bounds__(RD_BLOCK) void k_read_fill(
    const int64_t* __restrict__ start, const uint8_t* __restrict__ mapq, const int32_t* __restrict__ hp,
    const uint32_t* __restrict__ cigar, const int64_t* __restrict__ cigar_off, const uint8_t* __restrict__ seq,
    const uint8_t* __restrict__ qual, const int64_t* __restrict__ seq_off, const int64_t* __restrict__ cols, int P,
    const int32_t* __restrict__ lo_in, const int32_t* __restrict__ hi_in, const int32_t* __restrict__ row_of, int64_t cap_rows,
    int32_t* __restrict__ oseq, int32_t* __restrict__ ohap, int32_t* __restrict__ obq, int32_t* __restrict__ omq,
    int64_t* __restrict__ row_record, unsigned long long* __restrict__ key)
{
    __shared__ __attribute__((aligned(16))) uint32_t ops[RD_TILE];
    __shared__ int64_t rinc[RD_TILE];                      // reference bases of the tile up to and with op i
    __shared__ int64_t qexc[RD_TILE];                      // query bases of the tile in front of op i
    __shared__ int64_t wsum[2 * (RD_BLOCK / 64)];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c0 = lo_in[r], c1 = hi_in[r];
    if (c1 <= c0) return;                                  // covers no wanted column: no row
    const int64_t row = row_of[r];
    if (row >= cap_rows) return;                           // (the launcher refuses such a call; never write behind the outputs)
    const int32_t raw_tag = hp[r];
    const int32_t tag = raw_tag == -1 ? 3 : raw_tag;       // create_pileup_haplotype.py:103
    const int32_t mq = mapq[r];
    if (tid == 0) {
        row_record[row] = r;
        if (tag < 1 || tag > 3) atomicMin(key, offence_key(c0, r + 1, NSNP_READS_BAD_HP));
    }
    const size_t obase = (size_t)row * (size_t)P;
    for (int c = tid; c < c0; c += RD_BLOCK) { oseq[obase + c] = 0; ohap[obase + c] = 0; obq[obase + c] = 0; omq[obase + c] = 0; }
    for (int c = c1 + tid; c < P; c += RD_BLOCK) { oseq[obase + c] = 0; ohap[obase + c] = 0; obq[obase + c] = 0; omq[obase + c] = 0; }

    const int64_t a = start[r], o0 = cigar_off[r], n_ops = cigar_off[r + 1] - o0;
    const int64_t s0 = seq_off[r], q_len = seq_off[r + 1] - s0;
    int64_t ref_carry = 0, q_carry = 0;
    int cb = c0;
    for (int64_t t0 = 0; t0 < n_ops && cb < c1; t0 += RD_TILE) {
        const int n = (int)(n_ops - t0 < RD_TILE ? n_ops - t0 : RD_TILE);
        for (int i = tid; i < RD_TILE; i += RD_BLOCK) ops[i] = i < n ? cigar[o0 + t0 + i] : 0x6u;      // P of length 0: consumes nothing
        __syncthreads();
        // ---- prefix sums of the tile: four consecutive ops per thread, a wave scan of the thread sums, the wave sums through LDS ----
        const uint4 my = *reinterpret_cast<const uint4*>(&ops[4 * tid]);
        const uint32_t o4[4] = {my.x, my.y, my.z, my.w};
        int64_t rl[4], ql[4], rs = 0, qs = 0;
        for (int j = 0; j < 4; ++j) {
            const uint32_t code = o4[j] & 15u;
            rl[j] = op_ref(code) ? (int64_t)(o4[j] >> 4) : 0; ql[j] = op_query(code) ? (int64_t)(o4[j] >> 4) : 0;
            rs += rl[j]; qs += ql[j];
        }
        int64_t ri = rs, qi = qs;
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t tr = __shfl_up(ri, o), tq = __shfl_up(qi, o);
            if (lane >= o) { ri += tr; qi += tq; }
        }
        if (lane == 63) { wsum[2 * w] = ri; wsum[2 * w + 1] = qi; }
        __syncthreads();
        int64_t rbefore = 0, qbefore = 0, rall = 0, qall = 0;
        for (int q = 0; q < RD_BLOCK / 64; ++q) {
            const int64_t tr = wsum[2 * q], tq = wsum[2 * q + 1];
            if (q < w) { rbefore += tr; qbefore += tq; }
            rall += tr; qall += tq;
        }
        int64_t rrun = rbefore + ri - rs, qrun = qbefore + qi - qs;
        for (int j = 0; j < 4; ++j) {
            qexc[4 * tid + j] = qrun; rrun += rl[j]; qrun += ql[j]; rinc[4 * tid + j] = rrun;
        }
        __syncthreads();
        // ---- the wanted columns inside this tile's reference range [a + ref_carry, a + ref_carry + rall): cols[cb .. ce) ----
        const int ce = rall > 0 ? lower_bound_cols(cols, cb, c1, a + ref_carry + rall) : cb;
        for (int c = cb + tid; c < ce; c += RD_BLOCK) {
            const int64_t off = cols[c] - a - ref_carry;   // 0 <= off < rall
            int k0 = 0, k1 = n;                            // first op with rinc > off: it consumes the reference and holds the column
            while (k0 < k1) { const int m = (k0 + k1) >> 1; if (rinc[m] <= off) k0 = m + 1; else k1 = m; }
            const int k = k0 < n ? k0 : n - 1;
            const uint32_t code = ops[k] & 15u;
            int32_t vs = 0, vh = 0, vb = 0, vm = 0;
            if (op_match(code)) {
                const int64_t rex = k > 0 ? rinc[k - 1] : 0;
                const int64_t qpos = q_carry + qexc[k] + (off - rex);
                int32_t base = 0;
                if (qpos >= 0 && qpos < q_len) {
                    const uint32_t ch = seq[s0 + qpos] & 0xDFu;   // upper case
                    base = ch == 'A' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : ch == 'T' ? 4 : 0;
                    vb = qual[s0 + qpos];
                }
                if (base == 0) { atomicMin(key, offence_key(c, r + 1, NSNP_READS_FOREIGN_BASE)); vb = 0; }
                vs = base; vh = tag; vm = mq;
            } else if (code == 2u) {                        // D
                vs = -1; vh = tag; vm = mq;
            }                                               // N: the read sits in the column and leaves it empty
            oseq[obase + c] = vs; ohap[obase + c] = vh; obq[obase + c] = vb; omq[obase + c] = vm;
        }
        cb = ce; ref_carry += rall; q_carry += qall;
        __syncthreads();                                    // the tile's LDS is rewritten by the next trip
    }
    // (spans and fill add the same lengths: every column of [c0, c1) lies inside the CIGAR's reference range and was written above)
}

// rows / key null: no record or no column, nothing can offend
__global__ void k_read_meta(const int64_t* __restrict__ rows, const unsigned long long* __restrict__ key,
                            const int64_t* __restrict__ cols, int64_t* __restrict__ meta)
{
    if (threadIdx.x || blockIdx.x) return;
    const unsigned long long k = key ? *key : ~0ull;
    meta[0] = rows ? *rows : 0;
    if (k == ~0ull) { meta[1] = NSNP_READS_OK; meta[2] = -1; meta[3] = -1; return; }
    meta[1] = (int64_t)(k & 3ull);
    meta[2] = (int64_t)((k >> 2) & 0x7FFFFFFFull) - 1;     // -1 for a deep column: no single record
    meta[3] = cols[k >> 33];
}

// ---- scratch layout -------------------------------------------------------------------------------------------------------------------
struct ReadScratch {
    int32_t *lo, *hi, *row, *diff, *sums;
    unsigned long long* key;
    int64_t* rows;
    size_t bytes;
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

ReadScratch read_scratch(void* base, int64_t R, int64_t P)
{
    ReadScratch s;
    char* p = (char*)base;
    size_t o = 0;
    const int64_t nmax = R > P + 1 ? R : P + 1;
    const size_t nb = (size_t)NSNP_CDIV(nmax, (int64_t)SC_TILE);
    s.key = (unsigned long long*)(p + o); s.rows = (int64_t*)(p + o + 8); o += 16;
    s.lo = (int32_t*)(p + o); o += align16((size_t)R * 4);
    s.hi = (int32_t*)(p + o); o += align16((size_t)R * 4);
    s.row = (int32_t*)(p + o); o += align16((size_t)R * 4);
    s.diff = (int32_t*)(p + o); o += align16((size_t)(P + 1) * 4);
    s.sums = (int32_t*)(p + o); o += align16((nb + 1) * 4);
    s.bytes = o;
    return s;
}

void scan_i32(const int32_t* in, int64_t n, int inclusive, int32_t* out, int32_t* sums, int64_t* total64, hipStream_t s)
{
    const int64_t nb = NSNP_CDIV(n, (int64_t)SC_TILE);
    hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)nb), dim3(RD_BLOCK), 0, s, in, n, sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(RD_BLOCK), 0, s, sums, nb, total64);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(RD_BLOCK), 0, s, in, n, sums, inclusive, out);
}

constexpr int64_t RD_MAX = 0x7FFFFFF0ll;                   // records and columns are indexed with int32

// spans, depth per column (left in sc.diff), the row of every record (sc.row) and the row count (*sc.rows); R > 0, P > 0
int read_spans_depths(nsnp_ctx* ctx, const int64_t* start, const uint32_t* cigar, const int64_t* cigar_off, int64_t R,
                      const int64_t* cols, int64_t P, const ReadScratch& sc, hipStream_t s)
{
    NSNP_HIP(ctx, hipMemsetAsync(sc.diff, 0, (size_t)(P + 1) * 4, s));
    NSNP_HIP(ctx, hipMemsetAsync(sc.key, 0xFF, 8, s));
    hipLaunchKernelGGL(k_read_spans, dim3((unsigned)NSNP_CDIV(R, (int64_t)(RD_BLOCK / 64))), dim3(RD_BLOCK), 0, s, start, cigar,
                       cigar_off, R, cols, (int)P, sc.lo, sc.hi, sc.row, sc.diff);
    scan_i32(sc.row, R, 0, sc.row, sc.sums, sc.rows, s);               // flags -> rows (the tile sums are reused by the next scan)
    scan_i32(sc.diff, P, 1, sc.diff, sc.sums, nullptr, s);             // difference array -> depth
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

}  // namespace

extern "C" size_t nsnp_hap_read_scratch_bytes(int64_t R, int64_t P)
{
    if (R < 0 || P < 0 || R > RD_MAX || P > RD_MAX) return 0;
    return read_scratch(nullptr, R, P).bytes;
}

extern "C" int nsnp_hap_read_depths(nsnp_ctx* ctx, const int64_t* start, const uint32_t* cigar, const int64_t* cigar_off, int64_t R,
                                    const int64_t* cols, int64_t P, int32_t* depth, int64_t* rows, void* scratch, void* stream)
{
    if (!ctx || R < 0 || P < 0) return NSNP_EINVAL;
    if (R > RD_MAX || P > RD_MAX) return NSNP_ESHAPE;
    if (P > 0 && (!cols || !depth)) return NSNP_EINVAL;
    if (R > 0 && (!start || !cigar_off)) return NSNP_EINVAL;           // (cigar may be null when no record has an op)
    hipStream_t s = (hipStream_t)stream;
    if (R == 0 || P == 0) {
        if (P > 0) NSNP_HIP(ctx, hipMemsetAsync(depth, 0, (size_t)P * 4, s));
        if (rows) NSNP_HIP(ctx, hipMemsetAsync(rows, 0, 8, s));
        return NSNP_OK;
    }
    if (!scratch) return NSNP_EINVAL;
    const ReadScratch sc = read_scratch(scratch, R, P);
    const int rc = read_spans_depths(ctx, start, cigar, cigar_off, R, cols, P, sc, s);
    if (rc) return rc;
    NSNP_HIP(ctx, hipMemcpyAsync(depth, sc.diff, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
    if (rows) NSNP_HIP(ctx, hipMemcpyAsync(rows, sc.rows, 8, hipMemcpyDeviceToDevice, s));
    return NSNP_OK;
}

extern "C" int nsnp_hap_read_matrices(nsnp_ctx* ctx, const int64_t* start, const uint8_t* mapq, const int32_t* hp,
                                      const uint32_t* cigar, const int64_t* cigar_off, const uint8_t* seq, const uint8_t* qual,
                                      const int64_t* seq_off, int64_t R, const int64_t* cols, int64_t P, int64_t max_coverage,
                                      int32_t* oseq, int32_t* ohap, int32_t* obq, int32_t* omq, int64_t cap_rows, int64_t* row_record,
                                      int64_t* meta, void* scratch, void* stream)
{
    if (!ctx || R < 0 || P < 0 || cap_rows < 0 || !meta) return NSNP_EINVAL;
    if (R > RD_MAX || P > RD_MAX) return NSNP_ESHAPE;
    if (P > 0 && !cols) return NSNP_EINVAL;
    if (R > 0 && (!start || !mapq || !hp || !cigar_off || !seq_off)) return NSNP_EINVAL;
    if (cap_rows > 0 && P > 0 && (!oseq || !ohap || !obq || !omq || !row_record)) return NSNP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (R == 0 || P == 0) {                                  // no record covers a column: no rows, nothing can offend
        hipLaunchKernelGGL(k_read_meta, dim3(1), dim3(64), 0, s, (const int64_t*)nullptr, (const unsigned long long*)nullptr, cols, meta);
        NSNP_HIP(ctx, hipGetLastError());
        return NSNP_OK;
    }
    if (!scratch) return NSNP_EINVAL;
    const ReadScratch sc = read_scratch(scratch, R, P);
    const int rc = read_spans_depths(ctx, start, cigar, cigar_off, R, cols, P, sc, s);
    if (rc) return rc;
    // the one host visit of the call: the row count against the caller's outputs, before anything is written to them
    int64_t rows = 0;
    NSNP_HIP(ctx, hipMemcpyAsync(&rows, sc.rows, 8, hipMemcpyDeviceToHost, s));
    NSNP_HIP(ctx, hipStreamSynchronize(s));
    if (rows > cap_rows) return NSNP_EINVAL;
    const int max_cov = (int)(max_coverage > 0x7FFFFFFFll ? 0x7FFFFFFFll : max_coverage < -1 ? -1 : max_coverage);
    hipLaunchKernelGGL(k_read_depth_check, dim3((unsigned)NSNP_CDIV(P, (int64_t)RD_BLOCK)), dim3(RD_BLOCK), 0, s, sc.diff, (int)P,
                       max_cov, sc.key);
    if (rows > 0) {                                          // (seq / qual may be null when no record has a base: nothing is read then)
        hipLaunchKernelGGL(k_read_fill, dim3((unsigned)R), dim3(RD_BLOCK), 0, s, start, mapq, hp, cigar, cigar_off, seq, qual,
                           seq_off, cols, (int)P, sc.lo, sc.hi, sc.row, cap_rows, oseq, ohap, obq, omq, row_record, sc.key);
    }
    hipLaunchKernelGGL(k_read_meta, dim3(1), dim3(64), 0, s, (const int64_t*)sc.rows, (const unsigned long long*)sc.key, cols, meta);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
