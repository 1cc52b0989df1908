// pileup_records.hip -- the records of a stage-1 window file (<chr>.pd.bin) for the selected sites of a chunk of columns.
//
// Replaces, for columns that are already encoded and selected in HBM,
//   make_predict_array              dna_sv_tensor/src/make_predict_data/main.cpp:76-127    window matrix + "ctg:pos:REF33"
//   the alt_dict of make_tensor     dna_sv_tensor/src/make_candidate_snp_tensor/tensor_maker.cpp:83-169, main.cpp:220-251
//   the right-trim of the text      dna_sv_tensor/src/make_predict_data/main.cpp:88
// (restated in oracle/pileup_encode_oracle.c: orc_make_tensor's alt_info branch, orc_mpileup_to_pd2).
//
// nsnp_pileup_window_records: the window matrix is a flat gather - a thread owns 16 bytes of the output, whatever site they belong to, so
// every store is a whole 16-byte store although a site's 1,188 (int16) or 2,376 (int32) bytes start on 4-byte boundaries only; the
// position strings likewise, 4 bytes per thread with the digits worked out per byte.  Both outputs may be pinned host memory.
//
// nsnp_pileup_alt_info: one LANE per selected site walks its column byte by byte (the grammar is sequential), three launches:
//   k_alt_sizes   the length of every site's text            -> scratch
//   k_alt_scan    exclusive prefix sums (one block), meta    -> scratch, offsets[N], meta
//   k_alt_write   the text itself                            -> a device staging blob, offsets[0..N)
//   k_alt_copy    staging -> the caller's blob in 16-byte stores (the blob may be pinned host memory: byte stores would each cross the bus)
// The text needs the column's distinct keys merged and in byte order.  No list of keys is kept anywhere: deletions are keyed by their
// declared length alone (a 64-bit mask, one more walk per length present), mismatches are four counters, and the insertion alleles
// are ENUMERATED in order - every walk finds the smallest upper-cased allele above the one written last, and counts it - so the
// kernel is exact for any column (any number of distinct alleles, any length) in registers alone, at one walk per distinct key.
// Only selected sites are visited (3-4 % of the columns) and nearly all of them hold a handful of keys.
#include "nsnp_common.hpp"

namespace {

constexpr int REC_BLOCK = 256;
constexpr int REC_W = PW * PC;                    // 594 values per site
constexpr int POSW = NSNP_POSITION_WIDTH;         // 83
constexpr int REC_NAME_MAX = POSW - 1 - 11 - 1 - PW;   // 37: name ':' 11 digits ':' 33 bases
constexpr int ALT_BLOCK = 64;
constexpr int MAX_INDEL = 60;                     // kMaxIndelSize, tensor_maker.cpp:5

struct RecName { uint8_t b[40]; int len; };

__global__ void k_records_meta(int64_t N, int64_t* __restrict__ meta)
{
    if (threadIdx.x < 4) meta[threadIdx.x] = threadIdx.x == 0 ? N : 0;
}

// centre of site n, kept inside [16, M - 17] (a centre outside is reported in meta[2], never followed)
__device__ __forceinline__ int64_t safe_center(const int64_t* __restrict__ center_idx, int64_t n, int64_t M, bool& bad)
{
    int64_t c = center_idx[n];
    if (c < PCENTER) { c = PCENTER; bad = true; }
    if (c > M - PCENTER - 1) { c = M - PCENTER - 1; bad = true; }
    return c;
}

template <typename T>
__global__ __launch_bounds__(REC_BLOCK) void k_window_matrix(const int32_t* __restrict__ counts, const int64_t* __restrict__ center_idx,
                                                             int64_t N, int64_t M, T* __restrict__ out, int64_t* __restrict__ meta)
{
    constexpr int PER = 16 / (int)sizeof(T);
    const int64_t total = N * REC_W;
    const int64_t e0 = ((int64_t)blockIdx.x * REC_BLOCK + threadIdx.x) * PER;
    if (e0 >= total) return;
    int64_t n = e0 / REC_W;
    int r = (int)(e0 - n * REC_W);
    bool bad = false, wide = false;
    const int32_t* src = counts + (safe_center(center_idx, n, M, bad) - PCENTER) * PC;
    int32_t v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        v[j] = 0;
        if (e0 + j < total) {
            v[j] = src[r];
            if (++r == REC_W && n + 1 < N) { r = 0; ++n; src = counts + (safe_center(center_idx, n, M, bad) - PCENTER) * PC; }
        }
        if (sizeof(T) == 2) wide = wide || v[j] < -32768 || v[j] > 32767;
    }
    if (e0 + PER <= total) {
        i32x4 w;
        if (sizeof(T) == 2) {
            w.x = (v[0] & 0xffff) | (int)((unsigned)v[1 % PER] << 16); w.y = (v[2 % PER] & 0xffff) | (int)((unsigned)v[3 % PER] << 16);
            w.z = (v[4 % PER] & 0xffff) | (int)((unsigned)v[5 % PER] << 16); w.w = (v[6 % PER] & 0xffff) | (int)((unsigned)v[7 % PER] << 16);
        } else {
            w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
        }
        *reinterpret_cast<i32x4*>(out + e0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) if (e0 + j < total) out[e0 + j] = (T)v[j];
    }
    if (wide) meta[1] = 1;                                   // (every writer stores the same word)
    if (bad) meta[2] = 1;
}

// byte b behind "name:" of the position string of one site: decimal(pos) ':' REF33 zeros, the bases from chr_seq[0, chr_len) (chr_len >= 1)
__device__ __forceinline__ int position_tail(int64_t p, int b, const uint8_t* __restrict__ chr_seq, int64_t chr_len, bool& bad)
{
    if (p < 0) { p = 0; bad = true; }
    if (p > 99999999999ll) { p = 99999999999ll; bad = true; }
    int nd = 1;
    for (int64_t q = 10; q <= p; q *= 10) ++nd;
    if (b < nd) {
        int64_t div = 1;
        for (int k = b + 1; k < nd; ++k) div *= 10;
        return '0' + (int)((p / div) % 10);
    }
    if (b == nd) return ':';
    b -= nd + 1;
    if (b >= PW) return 0;
    int64_t i = p - PCENTER - 1 + b;                         // 0-based index of position p - 16 + b
    if (i < 0) { i = 0; bad = true; }
    if (i >= chr_len) { i = chr_len - 1; bad = true; }
    const int c = chr_seq[i];
    return (c >= 'a' && c <= 'z') ? c - 32 : c;              // toupper in the C locale
}

// ---- where a site's position, name and sequence come from ----------------------------------------------------------------------------
// The position strings have ONE body; its template parameter answers, for a centre column, what the string is made of.  RecPos
// (nsnp_pileup_window_records2): a chunk of one contig, pos[c] a position, the caller's one sequence, the one name by value.  RecKey
// (nsnp_pileup_window_records_keys): a chunk that holds SEVERAL contigs, a site's contig comes out of its key ((cid << NSNP_TOK_KEY_SHIFT) |
// pos, as nsnp_mpileup_tokenise_contigs leaves it): its reference bases out of the resident genome, bounded by the contig's OWN length, its
// name out of the table's names.
constexpr int64_t KEY_POS_MASK = (1ll << NSNP_TOK_KEY_SHIFT) - 1;

// contig and position of a key; a filler key (negative) or a contig outside the table: contig -1, position 0
__device__ __forceinline__ int64_t key_contig(int64_t key, int64_t n_contigs, int64_t& p)
{
    const int64_t cid = key >> NSNP_TOK_KEY_SHIFT;
    if (key < 0 || cid >= n_contigs) { p = 0; return -1; }
    p = key & KEY_POS_MASK;
    return cid;
}

struct RecSite {                                             // what the position string of one site is made of
    const uint8_t* nm; int nlen;                             // its name (nm null: the source's one name), or the emitting line's own token
    const uint8_t* seq; int64_t len;                         // its contig's sequence
    int64_t p, key;
};

struct RecPos {
    const int64_t* __restrict__ pos; const uint8_t* __restrict__ seq; int64_t len; const RecName& name;      // (the kernel's own argument)
    static constexpr int64_t cap_names = 0x7fffffff;         // (the table's size is not known here: only the "no room" entry is refused)
    __device__ __forceinline__ RecSite site(int64_t c, bool&) const { return RecSite{nullptr, name.len, seq, len, pos[c], 0}; }
    __device__ __forceinline__ int name_byte(const RecSite& s, int b) const { return s.nm ? s.nm[b] : name.b[b]; }
    __device__ __forceinline__ void first_byte(int64_t, const RecSite&) const {}
};

struct RecKey {
    const int64_t* __restrict__ key; const uint8_t* __restrict__ names_blob; const int64_t* __restrict__ name_off;
    const uint8_t* __restrict__ genome; const int64_t* __restrict__ seq_off; int64_t n_contigs, cap_names;
    int64_t* __restrict__ site_key;
    __device__ __forceinline__ RecSite site(int64_t c, bool& bad) const
    {
        RecSite s;
        s.key = key[c];
        int64_t cid = key_contig(s.key, n_contigs, s.p);
        if (cid < 0) { cid = 0; bad = true; }                // (a filler or a contig outside the table: contig 0 at position 0, which clamps)
        const int64_t o = seq_off[cid];
        s.seq = genome + o; s.len = seq_off[cid + 1] - o;
        if (s.len < 1) { s.seq = genome; s.len = 1; bad = true; }      // (an empty contig holds no site: the genome's first byte stands in)
        const int64_t no = name_off[cid];
        s.nm = names_blob + no; s.nlen = (int)(name_off[cid + 1] - no);
        if (s.nlen < 0 || s.nlen > REC_NAME_MAX) { bad = true; s.nlen = s.nlen < 0 ? 0 : REC_NAME_MAX; }
        return s;
    }
    __device__ __forceinline__ int name_byte(const RecSite& s, int b) const { return s.nm[b]; }
    // (the thread that owns a site's first byte: one 8-byte store per site)
    __device__ __forceinline__ void first_byte(int64_t n, const RecSite& s) const { site_key[n] = s.key; }
};

// the position strings: name ':' decimal(pos) ':' REF33 zeros, 4 bytes per thread across the sites' boundaries
template <typename Src>
__device__ __forceinline__ void position_strings_body(const Src& src, const int64_t* __restrict__ center_idx, int64_t N, int64_t M,
                                                      const int32_t* __restrict__ line_idx, const uint8_t* __restrict__ names,
                                                      uint8_t* __restrict__ out, int64_t* __restrict__ meta)
{
    bool bad = false;
    auto site = [&](int64_t n) -> RecSite {
        const int64_t c = safe_center(center_idx, n, M, bad);
        RecSite s = src.site(c, bad);
        // the name of a site is column 0 of the line that EMITS it (main.cpp:248: the line at centre + 16); line_idx[line] < 0: the source's
        if (line_idx) {
            const int32_t e = line_idx[c + PCENTER];
            if (e == 0x7fffffff || (int64_t)e >= src.cap_names) bad = true;      // (an entry the table had no room for, or one outside it: not followed)
            else if (e >= 0) {
                // NSNP_NAME_ENTRY bytes: 40 name bytes, then the length as int32
                s.nm = names + (int64_t)e * NSNP_NAME_ENTRY;
                s.nlen = *reinterpret_cast<const int32_t*>(s.nm + 40);
                if (s.nlen < 1 || s.nlen > REC_NAME_MAX) { bad = true; s.nlen = s.nlen < 1 ? 1 : REC_NAME_MAX; }      // (no room for 11 digits and the bases behind it)
            }
        }
        return s;
    };
    const int64_t total = N * POSW;
    const int64_t e0 = ((int64_t)blockIdx.x * REC_BLOCK + threadIdx.x) * 4;
    if (e0 >= total) return;
    int64_t n = e0 / POSW;
    int b = (int)(e0 - n * POSW);
    RecSite s = site(n);
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (e0 + j < total) {
            if (b == 0) src.first_byte(n, s);
            const int v = b < s.nlen ? src.name_byte(s, b) : b == s.nlen ? ':' : position_tail(s.p, b - s.nlen - 1, s.seq, s.len, bad);
            w |= (unsigned)v << (8 * j);
            if (++b == POSW && n + 1 < N) { b = 0; ++n; s = site(n); }
        }
    }
    if (e0 + 4 <= total) *reinterpret_cast<unsigned*>(out + e0) = w;
    else for (int j = 0; j < 4; ++j) if (e0 + j < total) out[e0 + j] = (uint8_t)(w >> (8 * j));
    if (bad) meta[2] = 1;
}

// (a source reaches its kernel as the arguments the kernel always had - every pointer a __restrict__ argument of its own - and is put
// together there: handed over as one struct its pointers are no __restrict__ arguments any more and the ISA moves away from what it was)
__global__ __launch_bounds__(REC_BLOCK) void k_position_strings(const int64_t* __restrict__ center_idx, const int64_t* __restrict__ pos, int64_t N, int64_t M,
                                                                const uint8_t* __restrict__ chr_seq, int64_t chr_len, RecName name,
                                                                const int32_t* __restrict__ line_idx, const uint8_t* __restrict__ names,
                                                                uint8_t* __restrict__ out, int64_t* __restrict__ meta)
{
    position_strings_body(RecPos{pos, chr_seq, chr_len, name}, center_idx, N, M, line_idx, names, out, meta);
}

__global__ __launch_bounds__(REC_BLOCK) void k_position_strings_keys(const int64_t* __restrict__ center_idx, const int64_t* __restrict__ key, int64_t N, int64_t M,
                                                                     const uint8_t* __restrict__ names_blob, const int64_t* __restrict__ name_off,
                                                                     const uint8_t* __restrict__ genome, const int64_t* __restrict__ seq_off, int64_t n_contigs,
                                                                     const int32_t* __restrict__ line_idx, const uint8_t* __restrict__ names, int64_t cap_names,
                                                                     uint8_t* __restrict__ out, int64_t* __restrict__ site_key, int64_t* __restrict__ meta)
{
    position_strings_body(RecKey{key, names_blob, name_off, genome, seq_off, n_contigs, cap_names, site_key}, center_idx, N, M, line_idx, names, out, meta);
}

// ---- column 0 of every line --------------------------------------------------------------------------------------------------------
// DNA_CreateCanSnpTensor prints pileup_components[0] of the line that emits a site, not its contig argument (main.cpp:248).  Nearly every
// text holds the contig's name there; where a line holds another token, the position string must carry that one.  Three launches over the
// text of a chunk (the tokeniser's own line order: a line starts at offset 0 and behind every '\n'; the tokeniser refuses empty lines, so
// the ordinal of a line is the number of '\n' in front of it): newlines per tile, exclusive scan by one block, then every line start
// compares its first tab-delimited token (split_line: leading tabs are skipped) with the name - line_idx[line] = -1 when equal, else the
// index of an entry of `names` the token was copied to (entries are handed out by an atomic counter in device memory: their order means
// nothing, the index is what is kept).
constexpr int NM_PER = 16, NM_TILE = REC_BLOCK * NM_PER;

__device__ __forceinline__ int nm_newlines(const uint8_t* __restrict__ text, int64_t i0, int64_t len)
{
    int n = 0;
#pragma unroll
    for (int j = 0; j < NM_PER; ++j) n += (i0 + j < len && text[i0 + j] == '\n');
    return n;
}

__global__ __launch_bounds__(REC_BLOCK) void k_names_count(const uint8_t* __restrict__ text, int64_t len, int64_t* __restrict__ blk)
{
    __shared__ int wsum[REC_BLOCK / 64];
    int n = nm_newlines(text, ((int64_t)blockIdx.x * REC_BLOCK + threadIdx.x) * NM_PER, len);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) { int s = 0; for (int w = 0; w < REC_BLOCK / 64; ++w) s += wsum[w]; blk[blockIdx.x] = s; }
}

// exclusive scan of v[0, n) in place by the 1,024 threads of one block: a strip of ceil(n / 1024) entries per thread, a Hillis-Steele scan
// of the strips' sums in part[1024] (LDS), the strips written back; part[1023] holds the total afterwards
__device__ __forceinline__ void block_scan_in_place(int64_t* __restrict__ v, int64_t n, int64_t* part)
{
    const int tid = threadIdx.x;
    const int64_t per = NSNP_CDIV(n, (int64_t)1024);
    const int64_t i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    int64_t s = 0;
    for (int64_t i = i0; i < i1; ++i) s += v[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t t = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    int64_t run = tid ? part[tid - 1] : 0;
    for (int64_t i = i0; i < i1; ++i) { const int64_t t = v[i]; v[i] = run; run += t; }
}

__global__ __launch_bounds__(1024) void k_names_scan(int64_t* __restrict__ blk, int64_t n_blocks, unsigned long long* __restrict__ counter)
{
    __shared__ int64_t part[1024];
    block_scan_in_place(blk, n_blocks, part);
    if (threadIdx.x == 0) *counter = 0;
}

// The name a line is compared with, the template parameter of k_names_emit: name_of(line, o, nl) = false for a line that is not compared
// (it keeps -1 and takes no entry), else byte(o, k) for k < nl are the name's bytes.  LinePos (nsnp_mpileup_line_names): the one name, every
// line.  LineKey (nsnp_mpileup_line_names_contigs): the table's name of cid[line] (the contig tokeniser's, for the same text); a line of no
// wanted contig (cid outside [0, n_contigs)) never emits a site.
struct LinePos {
    const RecName& name;
    __device__ __forceinline__ bool name_of(int64_t, int64_t& o, int64_t& nl) const { o = 0; nl = name.len; return true; }
    __device__ __forceinline__ int byte(int64_t, int64_t k) const { return name.b[k]; }
};
struct LineKey {
    const int32_t* __restrict__ cid; const uint8_t* __restrict__ names_blob; const int64_t* __restrict__ name_off; int64_t n_contigs;
    __device__ __forceinline__ bool name_of(int64_t line, int64_t& o, int64_t& nl) const
    {
        const int64_t c = cid[line];
        if (c < 0 || c >= n_contigs) return false;
        o = name_off[c]; nl = name_off[c + 1] - o;
        return true;
    }
    __device__ __forceinline__ int byte(int64_t o, int64_t k) const { return names_blob[o + k]; }
};

template <typename Src>
__device__ __forceinline__ void names_emit_body(const Src& src, const uint8_t* __restrict__ text, int64_t len, const int64_t* __restrict__ blk,
                                                int64_t cap_lines, int32_t* __restrict__ line_idx, uint8_t* __restrict__ names, int64_t cap_names,
                                                unsigned long long* __restrict__ counter)
{
    __shared__ int wsum[REC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = ((int64_t)blockIdx.x * REC_BLOCK + tid) * NM_PER;
    const int mine = nm_newlines(text, i0, len);
    int inc = mine;                                          // inclusive scan over the wave
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (lane >= o) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t line = blk[blockIdx.x] + inc - mine;             // newlines in front of byte i0
    for (int w = 0; w < wave; ++w) line += wsum[w];
    for (int j = 0; j < NM_PER; ++j) {
        const int64_t i = i0 + j;
        if (i >= len) break;
        if ((i == 0 || text[i - 1] == '\n') && line < cap_lines) {
            int32_t idx = -1;
            int64_t no, nl;
            if (src.name_of(line, no, nl)) {
                int64_t a = i;
                while (a < len && text[a] == '\t') ++a;
                int64_t e = a;
                while (e < len && text[e] != '\t' && text[e] != '\n') ++e;
                const int64_t tl = e - a;
                bool same = tl == nl;
                for (int64_t k = 0; same && k < nl; ++k) same = text[a + k] == src.byte(no, k);
                if (!same) {
                    const unsigned long long slot = atomicAdd(counter, 1ull);
                    idx = slot < (unsigned long long)cap_names ? (int32_t)slot : 0x7fffffff;      // (beyond the table: the caller sees the count and runs again)
                    if (slot < (unsigned long long)cap_names) {
                        uint8_t* dst = names + (int64_t)slot * NSNP_NAME_ENTRY;
                        for (int k = 0; k < 40; ++k) dst[k] = k < tl ? text[a + k] : 0;
                        *reinterpret_cast<int32_t*>(dst + 40) = (int32_t)(tl > 0x7fffffff ? 0x7fffffff : tl);
                    }
                }
            }
            line_idx[line] = idx;
        }
        line += text[i] == '\n';
    }
}

__global__ __launch_bounds__(REC_BLOCK) void k_names_emit(const uint8_t* __restrict__ text, int64_t len, const int64_t* __restrict__ blk, RecName name,
                                                          int64_t cap_lines, int32_t* __restrict__ line_idx, uint8_t* __restrict__ names, int64_t cap_names,
                                                          unsigned long long* __restrict__ counter)
{
    names_emit_body(LinePos{name}, text, len, blk, cap_lines, line_idx, names, cap_names, counter);
}

__global__ __launch_bounds__(REC_BLOCK) void k_names_emit_contigs(const uint8_t* __restrict__ text, int64_t len, const int64_t* __restrict__ blk,
                                                                  const int32_t* __restrict__ cid, const uint8_t* __restrict__ names_blob,
                                                                  const int64_t* __restrict__ name_off, int64_t n_contigs,
                                                                  int64_t cap_lines, int32_t* __restrict__ line_idx, uint8_t* __restrict__ names, int64_t cap_names,
                                                                  unsigned long long* __restrict__ counter)
{
    names_emit_body(LineKey{cid, names_blob, name_off, n_contigs}, text, len, blk, cap_lines, line_idx, names, cap_names, counter);
}

__global__ void k_names_meta(const unsigned long long* __restrict__ counter, int64_t cap_names, int64_t* __restrict__ meta)
{
    if (threadIdx.x == 0) { const int64_t n = (int64_t)*counter; meta[0] = n; meta[1] = n > cap_names ? NSNP_TOK_ERANGE : 0; meta[2] = 0; meta[3] = 0; }
}

// ---- alt_info ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int upper(int c) { return (c >= 'a' && c <= 'z') ? c - 32 : c; }
__device__ __forceinline__ bool is_space(int c) { return c == ' ' || (c >= 9 && c <= 13); }     // isspace in the C locale
__device__ __forceinline__ int acgt(int c)        // index of an upper-case base, -1 for anything else
{
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

// The scan of tensor_maker.cpp:83-114 over bases[i, end): f(sign, off, len, adv) for every '+' / '-' construct (adv the declared length,
// [off, off + len) the allele bytes the column still holds: len < adv only for the last construct of a column), g(byte) for every other
// byte that is looked at; '^' swallows the byte behind it.  A declared length beyond 10^9 stays there: it is longer than any column.
template <typename F, typename G>
__device__ __forceinline__ void walk_column(const uint8_t* __restrict__ s, int64_t i, const int64_t end, F f, G g)
{
    while (i < end) {
        const int b = s[i];
        if (b == '+' || b == '-') {
            ++i;
            int64_t adv = 0;
            while (i < end && s[i] >= '0' && s[i] <= '9') { adv = adv >= 1000000000 ? adv : adv * 10 + (s[i] - '0'); ++i; }
            const int64_t avail = end - i;
            f(b, i, (int)(adv < avail ? adv : avail), adv);
            i = adv < avail ? i + adv : end;
        } else if (b == '^') {
            i += 2;
        } else {
            g(b);
            ++i;
        }
    }
}

// order of two insertion keys (upper-cased allele bytes, then the shorter first, then the complete one in front of the cut one)
__device__ __forceinline__ int ins_cmp(const uint8_t* __restrict__ s, int64_t ao, int al, bool ac, int64_t bo, int bl, bool bc)
{
    const int n = al < bl ? al : bl;
    for (int k = 0; k < n; ++k) {
        const int x = upper(s[ao + k]), y = upper(s[bo + k]);
        if (x != y) return x < y ? -1 : 1;
    }
    if (al != bl) return al < bl ? -1 : 1;
    return (int)ac - (int)bc;
}

struct CountSink {                                           // length of the text once right-trimmed
    int64_t n, keep;
    __device__ __forceinline__ void put(int b) { ++n; if (!is_space(b)) keep = n; }
};
struct WriteSink {                                           // lim: the right-trimmed length the first pass found
    uint8_t* p; int64_t n, lim;
    __device__ __forceinline__ void put(int b) { if (n < lim) p[n] = (uint8_t)b; ++n; }
};

template <typename Sink>
__device__ __forceinline__ void put_dec(Sink& out, int64_t v)
{
    if (v < 0) { out.put('-'); v = -v; }
    int64_t div = 1;
    while (v / div >= 10) div *= 10;
    for (; div > 0; div /= 10) out.put('0' + (int)((v / div) % 10));
}

template <typename Sink>
__device__ __forceinline__ void put_count(Sink& out, int64_t cnt) { out.put(' '); put_dec(out, cnt); out.put(' '); }

// the third field of a .pd line for the column bases[b0, b1) at 1-based position p
template <typename Sink>
__device__ __forceinline__ void alt_text(const uint8_t* __restrict__ s, const int64_t b0, const int64_t b1, int ref_raw, int64_t p, int depth,
                                         const uint8_t* __restrict__ chr_seq, int64_t chr_len, Sink& out)
{
    const int ub = upper(ref_raw);
    const int chr_base = acgt(ub) >= 0 ? ub : 'A';           // tensor_maker.hpp:37-44, tensor_maker.cpp:77-78
    put_dec(out, depth);
    out.put('-');
    int xa = 0, xc = 0, xg = 0, xt = 0, n_ins = 0;
    unsigned long long dmask = 0;
    walk_column(s, b0, b1,
                [&](int sign, int64_t, int, int64_t adv) {
                    if (adv > MAX_INDEL) return;
                    if (sign == '+') ++n_ins; else dmask |= 1ull << adv;
                },
                [&](int b) { const int k = acgt(upper(b)); xa += k == 0; xc += k == 1; xg += k == 2; xt += k == 3; });
    // 'D' + the d reference bytes behind the position, raw; a byte past the contig's end is the NUL that ends the text
    for (int d = 0; d <= MAX_INDEL && dmask; ++d) {
        if (!((dmask >> d) & 1ull)) continue;
        dmask &= ~(1ull << d);
        int cnt = 0;
        walk_column(s, b0, b1, [&](int sign, int64_t, int, int64_t adv) { cnt += sign == '-' && adv == d; }, [](int) {});
        out.put('D');
        for (int q = 0; q < d; ++q) {
            const int c = p + q < chr_len ? chr_seq[p + q] : 0;
            if (c == 0) return;
            out.put(c);
        }
        put_count(out, cnt);
    }
    // 'I' + chr_base + upper(allele), in order: each walk finds the smallest key above the last one written and counts it
    int64_t po = 0; int pl = -1; bool pc = false;            // the key written last (pl < 0: none yet)
    while (n_ins > 0) {
        int64_t bo = 0; int bl = -1, cnt = 0; bool bc = false;
        walk_column(s, b0, b1,
                    [&](int sign, int64_t off, int len, int64_t adv) {
                        if (sign != '+' || adv > MAX_INDEL) return;
                        const bool cut = adv > len;
                        if (pl >= 0 && ins_cmp(s, off, len, cut, po, pl, pc) <= 0) return;
                        const int c = bl < 0 ? -1 : ins_cmp(s, off, len, cut, bo, bl, bc);
                        if (c < 0) { bo = off; bl = len; bc = cut; cnt = 1; }
                        else if (c == 0) ++cnt;
                    },
                    [](int) {});
        if (bl < 0) break;
        out.put('I'); out.put(chr_base);
        for (int k = 0; k < bl; ++k) out.put(upper(s[bo + k]));
        if (bc) return;                                      // the cut allele's key holds the column string's NUL
        put_count(out, cnt);
        po = bo; pl = bl; pc = bc; n_ins -= cnt;
    }
    if (chr_base != 'A' && xa) { out.put('X'); out.put('A'); put_count(out, xa); }
    if (chr_base != 'C' && xc) { out.put('X'); out.put('C'); put_count(out, xc); }
    if (chr_base != 'G' && xg) { out.put('X'); out.put('G'); put_count(out, xg); }
    if (chr_base != 'T' && xt) { out.put('X'); out.put('T'); put_count(out, xt); }
}

// column of site n, or false when its centre lies outside the columns (reported in meta[1] by k_alt_scan's caller: size 0)
__device__ __forceinline__ bool alt_column(const int64_t* __restrict__ center_idx, int64_t n, int64_t M, const int64_t* __restrict__ col_off, int64_t n_bytes,
                                           int64_t& c, int64_t& b0, int64_t& b1)
{
    c = center_idx[n];
    if (c < 0 || c >= M) return false;
    b0 = col_off[c]; b1 = col_off[c + 1];
    return b0 >= 0 && b0 <= b1 && b1 <= n_bytes;
}

// Where the 'D' keys of column c read their reference bytes, the template parameter of k_alt_sizes / k_alt_write: site(c, p, seq, len) =
// false when the column's entry cannot be followed (keyed: k_alt_write then reports NSNP_TOK_EPOS).  AltPos (nsnp_pileup_alt_info): pos[c]
// clamped at 0 in the caller's one sequence (len 0 is allowed).  AltKey (nsnp_pileup_alt_info_keys): the site's OWN contig out of the
// resident genome, so the keys meet NUL at ITS end (the next contig's bases lie right behind it); a filler key or a contig outside the
// table is a contig of length 0.
struct AltPos {
    static constexpr bool keyed = false;
    const int64_t* __restrict__ pos; const uint8_t* __restrict__ chr_seq; int64_t chr_len;
    __device__ __forceinline__ bool site(int64_t c, int64_t& p, const uint8_t*& seq, int64_t& len) const
    {
        p = pos[c] < 0 ? 0 : pos[c];
        seq = chr_seq; len = chr_len;
        return true;
    }
};
struct AltKey {
    static constexpr bool keyed = true;
    const int64_t* __restrict__ key; const uint8_t* __restrict__ genome; const int64_t* __restrict__ seq_off; int64_t n_contigs;
    __device__ __forceinline__ bool site(int64_t c, int64_t& p, const uint8_t*& seq, int64_t& len) const
    {
        const int64_t cid = key_contig(key[c], n_contigs, p);
        seq = genome; len = 0;
        if (cid < 0) return false;
        const int64_t o = seq_off[cid];
        seq = genome + o; len = seq_off[cid + 1] - o;
        return true;
    }
};

template <typename Src>
__device__ __forceinline__ void alt_sizes_body(const Src& src, const uint8_t* __restrict__ bases, int64_t n_bytes, const int64_t* __restrict__ col_off,
                                               const uint8_t* __restrict__ ref, const int32_t* __restrict__ depth, int64_t M,
                                               const int64_t* __restrict__ center_idx, int64_t N, int64_t* __restrict__ sizes)
{
    const int64_t n = (int64_t)blockIdx.x * ALT_BLOCK + threadIdx.x;
    if (n >= N) return;
    int64_t c, b0, b1;
    CountSink out{0, 0};
    if (alt_column(center_idx, n, M, col_off, n_bytes, c, b0, b1)) {
        int64_t p, len; const uint8_t* seq;
        src.site(c, p, seq, len);
        alt_text(bases, b0, b1, ref[c], p, depth[c], seq, len, out);
    }
    sizes[n] = out.keep;
}

// exclusive scan of the sizes by one block, in place; the total behind them, into offsets[N] and meta
__global__ __launch_bounds__(1024) void k_alt_scan(int64_t* __restrict__ sizes, int64_t N, int64_t cap, int64_t* __restrict__ offsets, int64_t* __restrict__ meta)
{
    __shared__ int64_t part[1024];
    block_scan_in_place(sizes, N, part);
    if (threadIdx.x == 1023) {
        const int64_t total = part[1023];
        sizes[N] = total; offsets[N] = total;
        meta[0] = total; meta[1] = total > cap ? NSNP_TOK_ERANGE : 0; meta[2] = 0; meta[3] = 0;
    }
}

template <typename Src>
__device__ __forceinline__ void alt_write_body(const Src& src, const uint8_t* __restrict__ bases, int64_t n_bytes, const int64_t* __restrict__ col_off,
                                               const uint8_t* __restrict__ ref, const int32_t* __restrict__ depth, int64_t M,
                                               const int64_t* __restrict__ center_idx, int64_t N, const int64_t* __restrict__ scan, int64_t cap,
                                               uint8_t* __restrict__ stage, int64_t* __restrict__ offsets, int64_t* __restrict__ meta)
{
    const int64_t n = (int64_t)blockIdx.x * ALT_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int64_t o = scan[n], lim = scan[n + 1] - o;
    offsets[n] = o;
    int64_t c, b0, b1;
    if (!Src::keyed && (scan[N] > cap || lim <= 0)) return;  // (nothing to report: a text that is not written does not look at its column)
    if (!alt_column(center_idx, n, M, col_off, n_bytes, c, b0, b1)) return;
    int64_t p, len; const uint8_t* seq;
    if (!src.site(c, p, seq, len))                           // (keyed: reported although the blob overflows - this test stands in front of that one)
        meta[1] = (scan[N] > cap ? NSNP_TOK_ERANGE : 0) | NSNP_TOK_EPOS;      // (behind k_alt_scan's word; every writer stores the same one)
    if (Src::keyed && (scan[N] > cap || lim <= 0)) return;
    WriteSink out{stage + o, 0, lim};
    alt_text(bases, b0, b1, ref[c], p, depth[c], seq, len, out);
}

#define ALT_COLUMNS const uint8_t* __restrict__ bases, int64_t n_bytes, const int64_t* __restrict__ col_off, const uint8_t* __restrict__ ref
#define ALT_SITES const int32_t* __restrict__ depth, int64_t M, const int64_t* __restrict__ center_idx, int64_t N
__global__ __launch_bounds__(ALT_BLOCK) void k_alt_sizes(ALT_COLUMNS, const int64_t* __restrict__ pos, ALT_SITES, const uint8_t* __restrict__ chr_seq,
                                                         int64_t chr_len, int64_t* __restrict__ sizes)
{
    alt_sizes_body(AltPos{pos, chr_seq, chr_len}, bases, n_bytes, col_off, ref, depth, M, center_idx, N, sizes);
}

__global__ __launch_bounds__(ALT_BLOCK) void k_alt_sizes_keys(ALT_COLUMNS, const int64_t* __restrict__ key, ALT_SITES, const uint8_t* __restrict__ genome,
                                                              const int64_t* __restrict__ seq_off, int64_t n_contigs, int64_t* __restrict__ sizes)
{
    alt_sizes_body(AltKey{key, genome, seq_off, n_contigs}, bases, n_bytes, col_off, ref, depth, M, center_idx, N, sizes);
}

__global__ __launch_bounds__(ALT_BLOCK) void k_alt_write(ALT_COLUMNS, const int64_t* __restrict__ pos, ALT_SITES, const uint8_t* __restrict__ chr_seq,
                                                         int64_t chr_len, const int64_t* __restrict__ scan, int64_t cap, uint8_t* __restrict__ stage,
                                                         int64_t* __restrict__ offsets)
{
    alt_write_body(AltPos{pos, chr_seq, chr_len}, bases, n_bytes, col_off, ref, depth, M, center_idx, N, scan, cap, stage, offsets, nullptr);
}

__global__ __launch_bounds__(ALT_BLOCK) void k_alt_write_keys(ALT_COLUMNS, const int64_t* __restrict__ key, ALT_SITES, const uint8_t* __restrict__ genome,
                                                              const int64_t* __restrict__ seq_off, int64_t n_contigs, const int64_t* __restrict__ scan,
                                                              int64_t cap, uint8_t* __restrict__ stage, int64_t* __restrict__ offsets, int64_t* __restrict__ meta)
{
    alt_write_body(AltKey{key, genome, seq_off, n_contigs}, bases, n_bytes, col_off, ref, depth, M, center_idx, N, scan, cap, stage, offsets, meta);
}
#undef ALT_COLUMNS
#undef ALT_SITES

// staging -> blob: whole 16-byte stores where the blob is aligned for them, the total read from the device
__global__ __launch_bounds__(REC_BLOCK) void k_alt_copy(const uint8_t* __restrict__ stage, const int64_t* __restrict__ total_p, int64_t cap,
                                                        uint8_t* __restrict__ blob)
{
    const int64_t total = *total_p;
    if (total > cap) return;
    const bool vec = (reinterpret_cast<uintptr_t>(blob) & 15) == 0;      // (the staging blob is 16-byte aligned by its allocation)
    for (int64_t e = ((int64_t)blockIdx.x * REC_BLOCK + threadIdx.x) * 16; e < total; e += (int64_t)gridDim.x * REC_BLOCK * 16) {
        if (vec && e + 16 <= total) *reinterpret_cast<i32x4*>(blob + e) = *reinterpret_cast<const i32x4*>(stage + e);
        else for (int j = 0; j < 16 && e + j < total; ++j) blob[e + j] = stage[e + j];
    }
}

}  // namespace
// ---- the launches of a pair of entries (the arguments are checked by the entries: their conditions differ; an entry hands over the
// launch of its own kernel, `strings(grid, s)` and the like, with the source's arguments in it) ------------------------------------------
template <typename Strings>
static int window_records_launch(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, int64_t M, int64_t N, int elem, void* position_matrix,
                                 int64_t* meta, void* stream, Strings strings)
{
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_records_meta, dim3(1), dim3(64), 0, s, N, meta);
    if (N > 0) {
        const int64_t units = NSNP_CDIV(N * REC_W * elem, (int64_t)16);
        if (elem == 2)
            hipLaunchKernelGGL(k_window_matrix<int16_t>, dim3((unsigned)NSNP_CDIV(units, (int64_t)REC_BLOCK)), dim3(REC_BLOCK), 0, s, counts, center_idx, N, M,
                               (int16_t*)position_matrix, meta);
        else
            hipLaunchKernelGGL(k_window_matrix<int32_t>, dim3((unsigned)NSNP_CDIV(units, (int64_t)REC_BLOCK)), dim3(REC_BLOCK), 0, s, counts, center_idx, N, M,
                               (int32_t*)position_matrix, meta);
        const int64_t words = NSNP_CDIV(N * POSW, (int64_t)4);
        strings(dim3((unsigned)NSNP_CDIV(words, (int64_t)REC_BLOCK)), s);
    }
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

template <typename Emit>
static int line_names_launch(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, int64_t cap_names, int64_t* meta, void* stream, Emit emit)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_blocks = NSNP_CDIV(text_len, (int64_t)NM_TILE);
    const size_t need = ((size_t)n_blocks + 2) * sizeof(int64_t);
    if (int rc = nsnp_scratch_reserve(ctx, &ctx->rec_tmp, &ctx->rec_tmp_bytes, need, need / 4, s)) return rc;
    int64_t* blk = (int64_t*)ctx->rec_tmp;
    unsigned long long* counter = (unsigned long long*)(blk + n_blocks);
    if (n_blocks > 0) hipLaunchKernelGGL(k_names_count, dim3((unsigned)n_blocks), dim3(REC_BLOCK), 0, s, text, text_len, blk);
    hipLaunchKernelGGL(k_names_scan, dim3(1), dim3(1024), 0, s, blk, n_blocks, counter);
    if (n_blocks > 0) emit(dim3((unsigned)n_blocks), s, (const int64_t*)blk, counter);
    hipLaunchKernelGGL(k_names_meta, dim3(1), dim3(64), 0, s, (const unsigned long long*)counter, cap_names, meta);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

template <typename Sizes, typename Write>
static int alt_info_launch(nsnp_ctx* ctx, int64_t N, uint8_t* blob, int64_t cap, int64_t* offsets, int64_t* meta, void* stream, Sizes sizes, Write write)
{
    hipStream_t s = (hipStream_t)stream;
    // scratch: N + 1 scanned sizes, then the staging blob (16-byte aligned)
    const size_t scan_bytes = (((size_t)N + 1) * sizeof(int64_t) + 15) & ~(size_t)15;
    const size_t need = scan_bytes + (size_t)cap + 16;
    if (int rc = nsnp_scratch_reserve(ctx, &ctx->rec_tmp, &ctx->rec_tmp_bytes, need, need / 4, s)) return rc;
    int64_t* scan = (int64_t*)ctx->rec_tmp;
    uint8_t* stage = (uint8_t*)ctx->rec_tmp + scan_bytes;
    const unsigned grid = (unsigned)NSNP_CDIV(N, (int64_t)ALT_BLOCK);
    if (N > 0) sizes(dim3(grid), s, scan);
    hipLaunchKernelGGL(k_alt_scan, dim3(1), dim3(1024), 0, s, scan, N, cap, offsets, meta);
    if (N > 0) {
        write(dim3(grid), s, (const int64_t*)scan, stage);
        if (cap > 0) {
            int64_t blocks = NSNP_CDIV(cap, (int64_t)REC_BLOCK * 16);
            if (blocks > 1024) blocks = 1024;
            hipLaunchKernelGGL(k_alt_copy, dim3((unsigned)blocks), dim3(REC_BLOCK), 0, s, (const uint8_t*)stage, (const int64_t*)(scan + N), cap, blob);
        }
    }
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

static RecName rec_name(const uint8_t* name, int name_len)
{
    RecName nm; memset(&nm, 0, sizeof nm);
    memcpy(nm.b, name, (size_t)name_len); nm.len = name_len;
    return nm;
}

extern "C" int nsnp_pileup_window_records2(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* pos, int64_t M, int64_t N,
                                           const uint8_t* chr_seq, int64_t chr_len, const uint8_t* name, int name_len, int elem,
                                           const int32_t* line_idx, const uint8_t* names,
                                           void* position_matrix, uint8_t* position, int64_t* meta, void* stream)
{
    if (line_idx && !names) return NSNP_EINVAL;
    if (!ctx || !meta || N < 0 || M < 0 || (elem != 2 && elem != 4) || !name || name_len < 1 || name_len > REC_NAME_MAX) return NSNP_EINVAL;
    if (memchr(name, 0, (size_t)name_len)) return NSNP_EINVAL;
    if (N > 0 && (!counts || !center_idx || !pos || !chr_seq || !position_matrix || !position || M < PW || chr_len < 1)) return NSNP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(position_matrix) & 15) || (reinterpret_cast<uintptr_t>(position) & 3)) return NSNP_EINVAL;
    const RecName nm = rec_name(name, name_len);
    return window_records_launch(ctx, counts, center_idx, M, N, elem, position_matrix, meta, stream, [&](dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(k_position_strings, grid, dim3(REC_BLOCK), 0, s, center_idx, pos, N, M, chr_seq, chr_len, nm, line_idx, names, position, meta);
    });
}

extern "C" int nsnp_pileup_window_records(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* pos, int64_t M, int64_t N,
                                          const uint8_t* chr_seq, int64_t chr_len, const uint8_t* name, int name_len, int elem,
                                          void* position_matrix, uint8_t* position, int64_t* meta, void* stream)
{
    return nsnp_pileup_window_records2(ctx, counts, center_idx, pos, M, N, chr_seq, chr_len, name, name_len, elem, nullptr, nullptr, position_matrix,
                                       position, meta, stream);
}

extern "C" int nsnp_pileup_window_records_keys(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* key, int64_t M, int64_t N,
                                               const uint8_t* names_blob, const int64_t* name_off, const uint8_t* genome, const int64_t* seq_off,
                                               int64_t n_contigs, int elem, const int32_t* line_idx, const uint8_t* names, int64_t cap_names,
                                               void* position_matrix, uint8_t* position, int64_t* site_key, int64_t* meta, void* stream)
{
    if (line_idx && (!names || cap_names < 1)) return NSNP_EINVAL;
    if (!ctx || !meta || N < 0 || M < 0 || (elem != 2 && elem != 4) || cap_names < 0 || n_contigs < 0 || n_contigs > NSNP_TOK_MAX_CONTIGS) return NSNP_EINVAL;
    if (N > 0 && (!counts || !center_idx || !key || !names_blob || !name_off || !genome || !seq_off || n_contigs < 1 || !position_matrix || !position ||
                  !site_key || M < PW))
        return NSNP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(position_matrix) & 15) || (reinterpret_cast<uintptr_t>(position) & 3) || (reinterpret_cast<uintptr_t>(site_key) & 7))
        return NSNP_EINVAL;
    return window_records_launch(ctx, counts, center_idx, M, N, elem, position_matrix, meta, stream, [&](dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(k_position_strings_keys, grid, dim3(REC_BLOCK), 0, s, center_idx, key, N, M, names_blob, name_off, genome, seq_off, n_contigs,
                           line_idx, names, cap_names, position, site_key, meta);
    });
}

extern "C" int nsnp_mpileup_line_names(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, const uint8_t* name, int name_len, int64_t cap_lines,
                                       int32_t* line_idx, uint8_t* names, int64_t cap_names, int64_t* meta, void* stream)
{
    if (!ctx || !meta || text_len < 0 || cap_lines < 0 || cap_names < 0 || cap_names > 0x7ffffff0 || !name || name_len < 1 || name_len > REC_NAME_MAX) return NSNP_EINVAL;
    if (memchr(name, 0, (size_t)name_len) || (text_len > 0 && (!text || !line_idx)) || (cap_names > 0 && !names)) return NSNP_EINVAL;
    const RecName nm = rec_name(name, name_len);
    return line_names_launch(ctx, text, text_len, cap_names, meta, stream, [&](dim3 grid, hipStream_t s, const int64_t* blk, unsigned long long* counter) {
        hipLaunchKernelGGL(k_names_emit, grid, dim3(REC_BLOCK), 0, s, text, text_len, blk, nm, cap_lines, line_idx, names, cap_names, counter);
    });
}

extern "C" int nsnp_mpileup_line_names_contigs(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, const int32_t* cid, const uint8_t* names_blob,
                                               const int64_t* name_off, int64_t n_contigs, int64_t cap_lines, int32_t* line_idx, uint8_t* names,
                                               int64_t cap_names, int64_t* meta, void* stream)
{
    if (!ctx || !meta || text_len < 0 || cap_lines < 0 || cap_names < 0 || cap_names > 0x7ffffff0 || n_contigs < 0 || n_contigs > NSNP_TOK_MAX_CONTIGS)
        return NSNP_EINVAL;
    if ((text_len > 0 && (!text || !line_idx || !cid)) || (cap_names > 0 && !names) || (n_contigs > 0 && (!names_blob || !name_off))) return NSNP_EINVAL;
    return line_names_launch(ctx, text, text_len, cap_names, meta, stream, [&](dim3 grid, hipStream_t s, const int64_t* blk, unsigned long long* counter) {
        hipLaunchKernelGGL(k_names_emit_contigs, grid, dim3(REC_BLOCK), 0, s, text, text_len, blk, cid, names_blob, name_off, n_contigs, cap_lines, line_idx,
                           names, cap_names, counter);
    });
}

extern "C" int nsnp_pileup_alt_info(nsnp_ctx* ctx, const uint8_t* bases, int64_t n_bytes, const int64_t* col_off, const uint8_t* ref, const int64_t* pos,
                                    const int32_t* depth, int64_t M, const int64_t* center_idx, int64_t N, const uint8_t* chr_seq, int64_t chr_len,
                                    uint8_t* blob, int64_t cap, int64_t* offsets, int64_t* meta, void* stream)
{
    if (!ctx || !meta || !offsets || N < 0 || M < 0 || cap < 0 || n_bytes < 0 || chr_len < 0 || (cap > 0 && !blob)) return NSNP_EINVAL;
    if (N > 0 && (!col_off || !ref || !pos || !depth || !center_idx || (n_bytes > 0 && !bases) || (chr_len > 0 && !chr_seq))) return NSNP_EINVAL;
    return alt_info_launch(
        ctx, N, blob, cap, offsets, meta, stream,
        [&](dim3 grid, hipStream_t s, int64_t* scan) {
            hipLaunchKernelGGL(k_alt_sizes, grid, dim3(ALT_BLOCK), 0, s, bases, n_bytes, col_off, ref, pos, depth, M, center_idx, N, chr_seq, chr_len, scan);
        },
        [&](dim3 grid, hipStream_t s, const int64_t* scan, uint8_t* stage) {
            hipLaunchKernelGGL(k_alt_write, grid, dim3(ALT_BLOCK), 0, s, bases, n_bytes, col_off, ref, pos, depth, M, center_idx, N, chr_seq, chr_len, scan, cap,
                               stage, offsets);
        });
}

extern "C" int nsnp_pileup_alt_info_keys(nsnp_ctx* ctx, const uint8_t* bases, int64_t n_bytes, const int64_t* col_off, const uint8_t* ref, const int64_t* key,
                                         const int32_t* depth, int64_t M, const int64_t* center_idx, int64_t N, const uint8_t* genome,
                                         const int64_t* seq_off, int64_t n_contigs, uint8_t* blob, int64_t cap, int64_t* offsets, int64_t* meta, void* stream)
{
    if (!ctx || !meta || !offsets || N < 0 || M < 0 || cap < 0 || n_bytes < 0 || n_contigs < 0 || n_contigs > NSNP_TOK_MAX_CONTIGS || (cap > 0 && !blob))
        return NSNP_EINVAL;
    if (N > 0 && (!col_off || !ref || !key || !depth || !center_idx || (n_bytes > 0 && !bases) || (n_contigs > 0 && (!genome || !seq_off)))) return NSNP_EINVAL;
    return alt_info_launch(
        ctx, N, blob, cap, offsets, meta, stream,
        [&](dim3 grid, hipStream_t s, int64_t* scan) {
            hipLaunchKernelGGL(k_alt_sizes_keys, grid, dim3(ALT_BLOCK), 0, s, bases, n_bytes, col_off, ref, key, depth, M, center_idx, N, genome, seq_off,
                               n_contigs, scan);
        },
        [&](dim3 grid, hipStream_t s, const int64_t* scan, uint8_t* stage) {
            hipLaunchKernelGGL(k_alt_write_keys, grid, dim3(ALT_BLOCK), 0, s, bases, n_bytes, col_off, ref, key, depth, M, center_idx, N, genome, seq_off,
                               n_contigs, scan, cap, stage, offsets, meta);
        });
}
