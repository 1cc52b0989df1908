// optim_step.hip -- the optimiser step of a training iteration on up to 64 fp32 tensors, in two launches.
//
// Replaces, for gradients that are already in HBM (nsnp_pileup_loss_grad leaves them there),
//   torch.nn.utils.clip_grad_norm_(parameters, max_norm)                          PileupModel/train.py:61
//   torch.optim.Adam.step (L2 weight decay) / RAdam.step (decoupled weight decay) PileupModel/optim.py:67-84, radam.py:16-81
//   Lookahead.update_slow on a sync step                                          PileupModel/lookahead.py:34-58
//
// Range map.  Tensor i of n_i floats is cut into ceil(n_i / span) ranges of span = 1,024 * mult floats (mult = the smallest power of two
// that keeps the grid at 2,048 workgroups or fewer; 1 for anything below two million floats).  Workgroup b serves one range: the table in
// the kernel arguments holds the five pointers and the count of every tensor and first[i], the first workgroup of tensor i, so b finds its
// tensor by a binary search over at most 65 words of scalar memory.  A range is visited in tiles of 1,024 floats, lane t owning floats
// 4 t .. 4 t + 3 of a tile: one 16-byte access where every pointer of the tensor is 16-byte aligned and the four floats exist, four 4-byte
// accesses otherwise.  Both forms feed the same arithmetic in the same order, so a tensor that is a view at an odd offset of a flat buffer
// gets the bits of one allocated on its own.
//
//   k_opt_sqsum    a lane adds g * g of its floats in visiting order ((g0^2 + g1^2) + (g2^2 + g3^2) per tile), the 64 lanes of a wave meet
//                  by six butterfly steps (operands commute: every lane holds the same bits), the four waves are added in wave order.
//                  One fp32 partial per workgroup -> scratch[b].
//   k_opt_update   every workgroup adds ALL partials itself: lane t takes partials t, t + 256, ... in float64, then the same wave and
//                  workgroup tree in float64.  Every workgroup therefore holds the same bits of the total, no workgroup waits for
//                  another and there is no third launch.  norm = (float) sqrt(total); c = min(1, max_norm / (norm + 1e-6)), torch's
//                  coefficient.  Then per float, fp32, no contraction (the library is built with -ffp-contract=off):
//                      g' = g * c                                    (the gradient buffer is only read)
//                      g' = g' + wd * p                              wd_mode 1, torch Adam's L2 form
//                      p  = p + decay * p                            wd_mode 2, radam.py:69-70, decay = -wd * lr
//                      m  = beta1 * m + (1 - beta1) * g'
//                      v  = beta2 * v + ((1 - beta2) * g') * g'
//                      p  = p - a * (m / (sqrt(v) * b + eps))        form 0
//                      p  = p - a * m                                form 1 (RAdam below N_sma 5)
//                      slow = slow + alpha * (p - slow); p = slow    sync 1
//                      slow = p                                      sync 2 (the first sync of lookahead.py:39-41: the buffer is created as a copy)
//                  Workgroup 0, lane 0 stores norm to grad_norm_out.
// No floating-point atomics anywhere: the same call on the same bits gives the same bits.  The division is the IEEE sequence (no
// fast-math); sqrt(v) compiles to v_sqrt_f32 with the denormal scaling around it (1 ulp, which reaches p scaled by lr: far below its
// rounding).
//
// nsnp_optim_step_kind: Novograd (PileupModel/novograd.py:197-221, and behind Lookahead lookahead.py:111-113), torch.optim.SGD (dampening 0)
// and torch.optim.Adadelta (optim.py:51-66, 85-96) on the same range map, the same k_opt_sqsum and the same two launches.
//   k_opt_update_kind<KIND>   the total and c as k_opt_update has them.  Novograd's second moment is ONE scalar per tensor, the squared norm
//                  of that tensor's clipped gradient, so no float of tensor t can move before all of t's gradients were seen - and they were:
//                  ranges never cross tensors, so partials first[t] .. first[t + 1] - 1 are tensor t's own.  In the pass that adds all
//                  partials a lane adds those of them that lie in that segment a second time, into a float64 of their own (lane l: partials
//                  l, l + 256, ... in rising order), and the segment sum seg_t goes through the same float64 wave and workgroup tree:
//                      n_t  = (float)(((double)c * (double)c) * seg_t)          (no second pass over the gradients)
//                      v_t' = (v_t == 0) ? n_t : beta2 * v_t + (1 - beta2) * n_t     v_t = layer_in[t]; the test holds at EVERY step
//                      d    = sqrt(v_t') + eps
//                  Every workgroup of tensor t computes v_t' itself, from the same words in the same order: the same bits.  The first
//                  workgroup of t, lane 0, stores it to layer_out[t]; the caller swaps layer_in and layer_out behind every step.  No
//                  workgroup reads a word that another workgroup writes in the same launch (partials and layer_in are read only, layer_out,
//                  p and the states are written by their one owner): this is why there is no third launch and nothing to wait for.
//                  Then per float, fp32, no contraction, x = g * c (the gradient buffer is only read, where novograd.py:214 divides it in place):
//                      Novograd   x = x / d;  x = x + wd * p (wd != 0);  m = beta1 * m + x;  p = p - lr * m            (no bias correction)
//                      SGD        x = x + wd * p (wd != 0);  momentum != 0: buf = mu * buf + x,  x = nesterov ? x + mu * buf : buf;
//                                 p = p - lr * x                           (a zero-filled buf gives torch's first-step buf = x exactly)
//                      Adadelta   x = x + wd * p (wd != 0);  sq = rho * sq + ((1 - rho) * x) * x;  std = sqrt(sq + eps);
//                                 delta = (sqrt(acc + eps) / std) * x;  acc = rho * acc + ((1 - rho) * delta) * delta;  p = p - lr * delta
//                  and the Lookahead sync 1 / 2 of k_opt_update behind any of them.  Novograd has no per-element second moment: it reads p, g, m
//                  and writes p, m.
#include "nsnp_common.hpp"

namespace {

constexpr int OPT_MAX = NSNP_OPTIM_MAX_TENSORS;
constexpr int OPT_BLOCK = 256;
constexpr int OPT_TILE = 4 * OPT_BLOCK;                     // floats of a tile
constexpr int64_t OPT_MAX_GRID = 2048;

struct OptTable {                                            // 3.3 KB of kernel arguments
    float* p[OPT_MAX];
    const float* g[OPT_MAX];
    float* m[OPT_MAX];
    float* v[OPT_MAX];
    float* slow[OPT_MAX];
    int64_t n[OPT_MAX];
    int first[OPT_MAX + 1];                                  // first[i]: the first workgroup of tensor i; first[n_tensors]: the grid
    int n_tensors;
    int mult;                                                // tiles per range
};
static_assert(sizeof(OptTable) <= 3584, "the table and the scalars share 4 KB of kernel arguments");

struct OptScalars {
    float beta1, omb1, beta2, omb2, eps, wd, decay, a, b, alpha, max_norm;
    int form, wd_mode, sync, clip, n_partials;
};

__device__ __forceinline__ int opt_tensor_of(const OptTable& tb, int blk)
{
    int lo = 0, hi = tb.n_tensors - 1;                       // the last i with first[i] <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb.first[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ f32x4 opt_load4(const float* __restrict__ q, int64_t i, int64_t n, bool vec)
{
    if (vec && i + 4 <= n) return *reinterpret_cast<const f32x4*>(q + i);
    f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i + e < n) r[e] = q[i + e];
    return r;
}

__device__ __forceinline__ void opt_store4(float* __restrict__ q, int64_t i, int64_t n, bool vec, f32x4 r)
{
    if (vec && i + 4 <= n) { *reinterpret_cast<f32x4*>(q + i) = r; return; }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i + e < n) q[i + e] = r[e];
}

__device__ __forceinline__ bool opt_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the sum of x over the workgroup's 256 lanes, the same bits in every lane: butterfly inside a wave, the four waves in wave order
template <typename T>
__device__ __forceinline__ T opt_block_sum(T x, T* sh)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += __shfl_xor(x, d, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wave] = x;
    __syncthreads();
    const T r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(OPT_BLOCK) void k_opt_sqsum(const OptTable tb, float* __restrict__ partial)
{
    __shared__ float sh[4];
    const int blk = blockIdx.x, t = opt_tensor_of(tb, blk);
    const float* __restrict__ g = tb.g[t];
    const int64_t n = tb.n[t];
    const bool vec = opt_al16(g);
    const int64_t r0 = (int64_t)(blk - tb.first[t]) * tb.mult * OPT_TILE;
    float s = 0.0f;
    for (int k = 0; k < tb.mult; ++k) {
        const int64_t i = r0 + (int64_t)k * OPT_TILE + 4 * threadIdx.x;
        if (i >= n) break;
        const f32x4 x = opt_load4(g, i, n, vec);
        s += (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
    }
    s = opt_block_sum(s, sh);
    if (threadIdx.x == 0) partial[blk] = s;
}

__global__ __launch_bounds__(OPT_BLOCK) void k_opt_update(const OptTable tb, const OptScalars sc, const float* __restrict__ partial,
                                                          float* __restrict__ grad_norm_out)
{
    __shared__ double shd[4];
    float c = 1.0f;
    if (sc.n_partials > 0) {
        double tot = 0.0;
        for (int i = threadIdx.x; i < sc.n_partials; i += OPT_BLOCK) tot += (double)partial[i];
        tot = opt_block_sum(tot, shd);
        const float norm = (float)__dsqrt_rn(tot);
        if (sc.clip) c = fminf(1.0f, sc.max_norm / (norm + 1e-6f));
        if (grad_norm_out && blockIdx.x == 0 && threadIdx.x == 0) *grad_norm_out = norm;
    }
    const int blk = blockIdx.x, t = opt_tensor_of(tb, blk);
    float* __restrict__ p = tb.p[t];
    const float* __restrict__ g = tb.g[t];
    float* __restrict__ m = tb.m[t];
    float* __restrict__ v = tb.v[t];
    float* __restrict__ slow = tb.slow[t];
    const int64_t n = tb.n[t];
    const bool vec = opt_al16(p) && opt_al16(g) && opt_al16(m) && opt_al16(v) && (sc.sync == 0 || opt_al16(slow));
    const int64_t r0 = (int64_t)(blk - tb.first[t]) * tb.mult * OPT_TILE;
    for (int k = 0; k < tb.mult; ++k) {
        const int64_t i = r0 + (int64_t)k * OPT_TILE + 4 * threadIdx.x;
        if (i >= n) break;
        f32x4 pp = opt_load4(p, i, n, vec), mm = opt_load4(m, i, n, vec), vv = opt_load4(v, i, n, vec), ss;
        const f32x4 gg = opt_load4(g, i, n, vec);
        if (sc.sync == 1) ss = opt_load4(slow, i, n, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = gg[e] * c, w = pp[e];
            if (sc.wd_mode == 1) x = x + sc.wd * w;
            if (sc.wd_mode == 2) w = w + sc.decay * w;
            const float me = sc.beta1 * mm[e] + sc.omb1 * x;
            const float ve = sc.beta2 * vv[e] + (sc.omb2 * x) * x;
            if (sc.form == 0) w = w - sc.a * (me / (__fsqrt_rn(ve) * sc.b + sc.eps));
            else w = w - sc.a * me;
            if (sc.sync == 1) { ss[e] = ss[e] + sc.alpha * (w - ss[e]); w = ss[e]; }
            pp[e] = w; mm[e] = me; vv[e] = ve;
        }
        opt_store4(p, i, n, vec, pp);
        opt_store4(m, i, n, vec, mm);
        opt_store4(v, i, n, vec, vv);
        if (sc.sync == 1) opt_store4(slow, i, n, vec, ss);
        if (sc.sync == 2) opt_store4(slow, i, n, vec, pp);
    }
}

struct OptKindScalars {
    float lr, beta1, beta2, omb2, eps, wd, mu, rho, omrho, alpha, max_norm;
    int nesterov, sync, clip, n_partials;
};

// tb.m / tb.v are the two state tables of a kind: Novograd exp_avg / unused, SGD momentum_buffer (momentum != 0) / unused, Adadelta square_avg / acc_delta
template <int KIND>
__global__ __launch_bounds__(OPT_BLOCK) void k_opt_update_kind(const OptTable tb, const OptKindScalars sc, const float* __restrict__ partial,
                                                               const float* __restrict__ layer_in, float* __restrict__ layer_out,
                                                               float* __restrict__ grad_norm_out)
{
    __shared__ double shd[4];
    const int blk = blockIdx.x, t = opt_tensor_of(tb, blk);
    float c = 1.0f, d = 1.0f;
    if (sc.n_partials > 0) {
        const int s0 = tb.first[t], s1 = tb.first[t + 1];
        double tot = 0.0, seg = 0.0;
        for (int i = threadIdx.x; i < sc.n_partials; i += OPT_BLOCK) {
            const double x = (double)partial[i];
            tot += x;
            if (KIND == NSNP_OPTIM_NOVOGRAD && i >= s0 && i < s1) seg += x;
        }
        tot = opt_block_sum(tot, shd);
        const float norm = (float)__dsqrt_rn(tot);
        if (sc.clip) c = fminf(1.0f, sc.max_norm / (norm + 1e-6f));
        if (grad_norm_out && blk == 0 && threadIdx.x == 0) *grad_norm_out = norm;
        if (KIND == NSNP_OPTIM_NOVOGRAD) {
            seg = opt_block_sum(seg, shd);
            const float nt = (float)(((double)c * (double)c) * seg);
            const float v0 = layer_in[t];
            const float v1 = (v0 == 0.0f) ? nt : sc.beta2 * v0 + sc.omb2 * nt;
            d = __fsqrt_rn(v1) + sc.eps;
            if (blk == s0 && threadIdx.x == 0) layer_out[t] = v1;
        }
    }
    float* __restrict__ p = tb.p[t];
    const float* __restrict__ g = tb.g[t];
    float* __restrict__ sa = tb.m[t];
    float* __restrict__ sb = tb.v[t];
    float* __restrict__ slow = tb.slow[t];
    const int64_t n = tb.n[t];
    const bool use_a = KIND != NSNP_OPTIM_SGD || sc.mu != 0.0f, use_b = KIND == NSNP_OPTIM_ADADELTA;
    const bool vec = opt_al16(p) && opt_al16(g) && (!use_a || opt_al16(sa)) && (!use_b || opt_al16(sb)) && (sc.sync == 0 || opt_al16(slow));
    const int64_t r0 = (int64_t)(blk - tb.first[t]) * tb.mult * OPT_TILE;
    for (int k = 0; k < tb.mult; ++k) {
        const int64_t i = r0 + (int64_t)k * OPT_TILE + 4 * threadIdx.x;
        if (i >= n) break;
        f32x4 pp = opt_load4(p, i, n, vec), aa = {0.0f, 0.0f, 0.0f, 0.0f}, bb = aa, ss;
        const f32x4 gg = opt_load4(g, i, n, vec);
        if (use_a) aa = opt_load4(sa, i, n, vec);
        if (use_b) bb = opt_load4(sb, i, n, vec);
        if (sc.sync == 1) ss = opt_load4(slow, i, n, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = gg[e] * c, w = pp[e];
            if (KIND == NSNP_OPTIM_NOVOGRAD) {
                x = x / d;
                if (sc.wd != 0.0f) x = x + sc.wd * w;
                aa[e] = sc.beta1 * aa[e] + x;
                w = w - sc.lr * aa[e];
            } else if (KIND == NSNP_OPTIM_SGD) {
                if (sc.wd != 0.0f) x = x + sc.wd * w;
                if (use_a) {
                    aa[e] = sc.mu * aa[e] + x;
                    x = sc.nesterov ? x + sc.mu * aa[e] : aa[e];
                }
                w = w - sc.lr * x;
            } else {
                if (sc.wd != 0.0f) x = x + sc.wd * w;
                aa[e] = sc.rho * aa[e] + (sc.omrho * x) * x;
                const float sd = __fsqrt_rn(aa[e] + sc.eps);
                const float delta = (__fsqrt_rn(bb[e] + sc.eps) / sd) * x;
                bb[e] = sc.rho * bb[e] + (sc.omrho * delta) * delta;
                w = w - sc.lr * delta;
            }
            if (sc.sync == 1) { ss[e] = ss[e] + sc.alpha * (w - ss[e]); w = ss[e]; }
            pp[e] = w;
        }
        opt_store4(p, i, n, vec, pp);
        if (use_a) opt_store4(sa, i, n, vec, aa);
        if (use_b) opt_store4(sb, i, n, vec, bb);
        if (sc.sync == 1) opt_store4(slow, i, n, vec, ss);
        if (sc.sync == 2) opt_store4(slow, i, n, vec, pp);
    }
}

// the range map of a set of counts: mult and first[]; false for a count below 1 or a grid beyond 2^31
bool opt_plan(int n_tensors, const int64_t* counts, int* mult, int* first)
{
    for (int i = 0; i < n_tensors; ++i)
        if (counts[i] < 1) return false;
    for (int64_t mu = 1; mu <= (int64_t)1 << 40; mu <<= 1) {
        int64_t blocks = 0;
        for (int i = 0; i < n_tensors; ++i) blocks += NSNP_CDIV(counts[i], mu * OPT_TILE);
        if (blocks > OPT_MAX_GRID) continue;                               // (at most 64 tensors: a large enough mult always fits)
        if (mu > 0x7fffffff / OPT_TILE) return false;
        int64_t b = 0;
        for (int i = 0; i < n_tensors; ++i) { first[i] = (int)b; b += NSNP_CDIV(counts[i], mu * OPT_TILE); }
        first[n_tensors] = (int)b;
        *mult = (int)mu;
        return true;
    }
    return false;
}

}  // namespace

extern "C" int64_t nsnp_optim_scratch_floats(int n_tensors, const int64_t* counts)
{
    int mult, first[OPT_MAX + 1];
    if (n_tensors < 1 || n_tensors > OPT_MAX || !counts || !opt_plan(n_tensors, counts, &mult, first)) return NSNP_EINVAL;
    return first[n_tensors];
}

extern "C" int nsnp_optim_step(nsnp_ctx* ctx, int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                               float* const* exp_avg_sq, float* const* slow, const int64_t* counts, const nsnp_optim_args* args,
                               float* scratch, float* grad_norm_out, void* stream)
{
    if (!ctx || !params || !grads || !exp_avg || !exp_avg_sq || !counts || !args) return NSNP_EINVAL;
    if (n_tensors < 1 || n_tensors > OPT_MAX) return NSNP_EINVAL;
    const nsnp_optim_args& A = *args;
    if (!(A.beta1 >= 0.0 && A.beta1 < 1.0) || !(A.beta2 >= 0.0 && A.beta2 < 1.0) || !(A.alpha >= 0.0 && A.alpha <= 1.0)) return NSNP_EINVAL;
    if (A.form < 0 || A.form > 1 || A.wd_mode < 0 || A.wd_mode > 2 || A.sync < 0 || A.sync > 2) return NSNP_EINVAL;
    if (A.sync != 0 && !slow) return NSNP_EINVAL;
    const bool clip = A.max_norm > 0.0, need_norm = clip || grad_norm_out;
    if (need_norm && !scratch) return NSNP_EINVAL;
    OptTable tb;
    memset(&tb, 0, sizeof tb);
    for (int i = 0; i < n_tensors; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || (A.sync != 0 && !slow[i])) return NSNP_EINVAL;
        if ((reinterpret_cast<uintptr_t>(params[i]) | reinterpret_cast<uintptr_t>(grads[i]) | reinterpret_cast<uintptr_t>(exp_avg[i]) |
             reinterpret_cast<uintptr_t>(exp_avg_sq[i]) | (A.sync != 0 ? reinterpret_cast<uintptr_t>(slow[i]) : 0)) & 3) return NSNP_EINVAL;
        tb.p[i] = params[i]; tb.g[i] = grads[i]; tb.m[i] = exp_avg[i]; tb.v[i] = exp_avg_sq[i];
        tb.slow[i] = A.sync != 0 ? slow[i] : nullptr;
        tb.n[i] = counts[i];
    }
    if (!opt_plan(n_tensors, counts, &tb.mult, tb.first)) return NSNP_EINVAL;
    tb.n_tensors = n_tensors;
    const int grid = tb.first[n_tensors];
    OptScalars sc;
    sc.beta1 = (float)A.beta1; sc.omb1 = (float)(1.0 - A.beta1);
    sc.beta2 = (float)A.beta2; sc.omb2 = (float)(1.0 - A.beta2);
    sc.eps = (float)A.eps; sc.wd = (float)A.weight_decay; sc.decay = (float)A.decay;
    sc.a = (float)A.a; sc.b = (float)A.b; sc.alpha = (float)A.alpha; sc.max_norm = (float)A.max_norm;
    sc.form = A.form; sc.wd_mode = A.wd_mode; sc.sync = A.sync; sc.clip = clip ? 1 : 0;
    sc.n_partials = need_norm ? grid : 0;
    hipStream_t s = (hipStream_t)stream;
    if (need_norm) hipLaunchKernelGGL(k_opt_sqsum, dim3((unsigned)grid), dim3(OPT_BLOCK), 0, s, tb, scratch);
    hipLaunchKernelGGL(k_opt_update, dim3((unsigned)grid), dim3(OPT_BLOCK), 0, s, tb, sc, (const float*)scratch, grad_norm_out);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}

extern "C" int nsnp_optim_step_kind(nsnp_ctx* ctx, int n_tensors, float* const* params, const float* const* grads, float* const* state_a,
                                    float* const* state_b, float* const* slow, const int64_t* counts, const nsnp_optim_kind_args* args,
                                    const float* layer_in, float* layer_out, float* scratch, float* grad_norm_out, void* stream)
{
    if (!ctx || !params || !grads || !counts || !args) return NSNP_EINVAL;
    if (n_tensors < 1 || n_tensors > OPT_MAX) return NSNP_EINVAL;
    const nsnp_optim_kind_args& A = *args;
    if (A.kind != NSNP_OPTIM_NOVOGRAD && A.kind != NSNP_OPTIM_SGD && A.kind != NSNP_OPTIM_ADADELTA) return NSNP_EINVAL;
    const auto unit = [](double x) { return x >= 0.0 && x < 1.0; };          // (false for a NaN)
    if (!unit(A.beta1) || !unit(A.beta2) || !unit(A.rho) || !unit(A.momentum) || !(A.alpha >= 0.0 && A.alpha <= 1.0)) return NSNP_EINVAL;
    if (A.nesterov != 0 && A.nesterov != 1) return NSNP_EINVAL;
    if (A.nesterov && A.momentum == 0.0) return NSNP_EINVAL;                  // torch: "Nesterov momentum requires a momentum"
    if (A.sync < 0 || A.sync > 2 || (A.sync != 0 && !slow)) return NSNP_EINVAL;
    const bool novo = A.kind == NSNP_OPTIM_NOVOGRAD;
    const bool use_a = A.kind != NSNP_OPTIM_SGD || A.momentum != 0.0, use_b = A.kind == NSNP_OPTIM_ADADELTA;
    if ((use_a && !state_a) || (use_b && !state_b)) return NSNP_EINVAL;
    const bool clip = A.max_norm > 0.0, need_norm = novo || clip || grad_norm_out;
    if (need_norm && !scratch) return NSNP_EINVAL;
    if (novo && (!layer_in || !layer_out || layer_in == layer_out)) return NSNP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(layer_in) | reinterpret_cast<uintptr_t>(layer_out) | reinterpret_cast<uintptr_t>(scratch) |
         reinterpret_cast<uintptr_t>(grad_norm_out)) & 3) return NSNP_EINVAL;
    OptTable tb;
    memset(&tb, 0, sizeof tb);
    for (int i = 0; i < n_tensors; ++i) {
        if (!params[i] || !grads[i] || (use_a && !state_a[i]) || (use_b && !state_b[i]) || (A.sync != 0 && !slow[i])) return NSNP_EINVAL;
        if ((reinterpret_cast<uintptr_t>(params[i]) | reinterpret_cast<uintptr_t>(grads[i]) | (use_a ? reinterpret_cast<uintptr_t>(state_a[i]) : 0) |
             (use_b ? reinterpret_cast<uintptr_t>(state_b[i]) : 0) | (A.sync != 0 ? reinterpret_cast<uintptr_t>(slow[i]) : 0)) & 3) return NSNP_EINVAL;
        tb.p[i] = params[i]; tb.g[i] = grads[i];
        tb.m[i] = use_a ? state_a[i] : nullptr;
        tb.v[i] = use_b ? state_b[i] : nullptr;
        tb.slow[i] = A.sync != 0 ? slow[i] : nullptr;
        tb.n[i] = counts[i];
    }
    if (!opt_plan(n_tensors, counts, &tb.mult, tb.first)) return NSNP_EINVAL;
    tb.n_tensors = n_tensors;
    const int grid = tb.first[n_tensors];
    OptKindScalars sc;
    sc.lr = (float)A.lr; sc.beta1 = (float)A.beta1; sc.beta2 = (float)A.beta2; sc.omb2 = (float)(1.0 - A.beta2);
    sc.eps = (float)A.eps; sc.wd = (float)A.weight_decay; sc.mu = (float)A.momentum;
    sc.rho = (float)A.rho; sc.omrho = (float)(1.0 - A.rho); sc.alpha = (float)A.alpha; sc.max_norm = (float)A.max_norm;
    sc.nesterov = A.nesterov; sc.sync = A.sync; sc.clip = clip ? 1 : 0;
    sc.n_partials = need_norm ? grid : 0;
    hipStream_t s = (hipStream_t)stream;
    if (need_norm) hipLaunchKernelGGL(k_opt_sqsum, dim3((unsigned)grid), dim3(OPT_BLOCK), 0, s, tb, scratch);
    const dim3 gd((unsigned)grid), bd(OPT_BLOCK);
    if (novo)
        hipLaunchKernelGGL(k_opt_update_kind<NSNP_OPTIM_NOVOGRAD>, gd, bd, 0, s, tb, sc, (const float*)scratch, layer_in, layer_out, grad_norm_out);
    else if (A.kind == NSNP_OPTIM_SGD)
        hipLaunchKernelGGL(k_opt_update_kind<NSNP_OPTIM_SGD>, gd, bd, 0, s, tb, sc, (const float*)scratch, layer_in, layer_out, grad_norm_out);
    else
        hipLaunchKernelGGL(k_opt_update_kind<NSNP_OPTIM_ADADELTA>, gd, bd, 0, s, tb, sc, (const float*)scratch, layer_in, layer_out, grad_norm_out);
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
