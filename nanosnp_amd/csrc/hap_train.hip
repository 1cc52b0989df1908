// hap_train.hip -- the loss gradients of a batch of labelled haplotype sites: what loss.backward() of HaplotypeModel/train_dev.py:58-59 computes.
//
// Replaces, for features, classes and parameters that are already in HBM,
//   LSTMNetwork.forward in train() mode                        HaplotypeModel/model_dev.py:120-131 (BaseEncoder 76-84, ForwardLayer 96-105)
//   the inter-layer dropout of nn.LSTM(dropout=...)            model_dev.py:63-70, as four explicit keep masks and one scale
//   LabelSmoothingLoss(C, 0.1) and its mean                    HaplotypeModel/optim.py
//   autograd of loss = gt_loss + zy_loss                       model_dev.py:128-130
//
// fp32 only.  The parameters are the caller's 58 device tensors in plain state-dict layout (they change every step, so nothing is packed);
// the inference kernels and the weight images of nsnp_hap_load_weights are not involved.  No site is padded: every kernel checks its bounds.
//
// The schedule is the reduced one of the inference kernels: layers 0 and 1 of an encoder of L positions run L steps per direction (the next
// layer reads every position), layer 2 runs Tc = L / 2 + 1 steps per direction (pileup 17 of 33, haplotype 6 of 11; the forward direction
// walks positions 0 .. L / 2, the reverse L - 1 .. L / 2) and receives a gradient at its last step only.
//
// W_hh is 1024 x 256 per layer and direction: 1 MB, no register file and no LDS holds it.  So the recurrence is one launch pair per step
// over all sites of the chunk: the product through k_tr_gemm, then the cell as a launch of its own.  The two directions and,
// while the short encoder still runs, the two encoders share every launch through blockIdx.z.
//
// Kernels (the product k_tr_gemm, k_tr_loss, k_tr_colsum, k_tr_mask, k_tr_dtanh, k_tr_reduce and their launch helpers: train_common.hpp;
// a weight gradient's slices are HT_KCH rows)
//   k_ht_cell_fwd  gates_t (projection + product) -> sigma(i), sigma(f), tanh(g), sigma(o) in place, c_t and h_t saved; t = 0: no c before it.
//                  Exact activations (expf, tanhf), here and in the dense layer's epilogue (flag 4 of the product).
//   k_ht_cell_bwd  dgates_t from dh_t = dH_external + rec and the carried dc, as k_tr_lstm_bwd forms it; overwrites the activations.
// No floating-point atomic anywhere: the same call gives the same bits twice.
#include "train_common.hpp"

namespace {

constexpr int HH = 256, HG = 1024, H2 = 512;                  // hidden units, gate rows, a bidirectional row
constexpr int HT_KCH = 128;                                   // reduction rows per slice of a weight gradient: short sums in one accumulator, the slices
                                                              // added in order by k_tr_reduce (1,024 rows per accumulator cost accuracy: docs/rounds/r29.md)
constexpr int64_t HT_MAX_SITES = (int64_t)1 << 16;

// floats per site of the workspace, encoder of L positions and Tc layer-2 steps:
//   G   gates of the 2 (2 L + Tc) (layer, direction, step) triples, 1024 each            pileup 169,984   haplotype 57,344
//   H,C h and c, [L][512] for layers 0 and 1 by position, [Tc][512] for layer 2 by step          84,992             28,672
//   X   the masked inputs of layers 1 and 2, [L][512] each                                       33,792             11,264
//   DX  the gradient that reaches a layer's output, [L][512] (reused from layer to layer)        16,896              5,632
//   REC, DC, DHC  [512] each                                                                      1,536              1,536
// and once per site  Y 512, DY 512, MID 256, DMID 256, Z 16, DZ 16 = 1,568:  F_SITE = 413,216 floats = 1,652,864 bytes.
constexpr int64_t enc_floats(int L, int Tc) { return (int64_t)(2 * L + Tc) * (2 * HG + 2 * H2) + 3 * (int64_t)L * H2 + 3 * H2; }
constexpr int64_t F_TAIL = 2 * H2 + 2 * HH + 16 + 16;
constexpr int64_t F_SITE = enc_floats(33, 17) + enc_floats(11, 6) + F_TAIL;
static_assert(F_SITE == 413216, "workspace floats per site");

struct EncWs {
    int L, Tc;
    float *G[3][2], *H[3], *C[3], *X[3], *DX, *REC, *DC, *DHC;       // X[0] unused: layer 0 reads the caller's features
};
struct HtWs { EncWs e[2]; float *Y, *DY, *MID, *DMID, *Z, *DZ, *PART; };
HtWs carve(float* base, int64_t cap)
{
    HtWs w; float* p = base;
    auto take = [&](int64_t per) { float* r = p; p += per * cap; return r; };
    for (int e = 0; e < 2; ++e) {
        EncWs& x = w.e[e];
        x.L = e ? 11 : 33; x.Tc = x.L / 2 + 1;
        for (int l = 0; l < 3; ++l) {
            const int T = l < 2 ? x.L : x.Tc;
            for (int d = 0; d < 2; ++d) x.G[l][d] = take((int64_t)T * HG);
            x.H[l] = take((int64_t)T * H2); x.C[l] = take((int64_t)T * H2);
        }
        x.X[0] = nullptr; x.X[1] = take((int64_t)x.L * H2); x.X[2] = take((int64_t)x.L * H2);
        x.DX = take((int64_t)x.L * H2); x.REC = take(H2); x.DC = take(H2); x.DHC = take(H2);
    }
    w.Y = take(H2); w.DY = take(H2); w.MID = take(HH); w.DMID = take(HH); w.Z = take(16); w.DZ = take(16);
    w.PART = p;
    return w;
}
int64_t part_floats(int64_t cap) { return NSNP_CDIV(cap * 33, (int64_t)HT_KCH) * HG * H2; }

// ---- the cells ------------------------------------------------------------------------------------
// The activations of this file are libm's (expf, tanhf, an IEEE division), not the v_exp_f32 + v_rcp_f32 forms of train_common.hpp, whose
// tanh_f = 1 - 2 / (1 + e^2x) carries an ABSOLUTE error of one rounding of 1: a relative 1e-5 at x = 0.01, where this model's cells live.
// Adam's first steps multiply the absolute error of a near-zero gradient element by up to lr / eps = 1,000 (docs/rounds/r29.md); the cells
// are bound by memory, so the exact forms cost nothing.
__device__ __forceinline__ float sigmoid_x(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_x(float x) { return tanhf(x); }
// One thread per (site, unit) of a (encoder, direction) problem; blockIdx.y selects the problem.  G: the step's gate block of site 0, sg floats
// between sites (gate rows i f g o as nn.LSTM orders them); c, h, cprev: the step's row of site 0 at the direction's columns, sh between sites.
struct HtCellF { float* G; const float* cprev; float* c; float* h; int64_t sg, sh, n; };
struct HtCellFBatch { HtCellF p[4]; };
__global__ __launch_bounds__(256) void k_ht_cell_fwd(const HtCellFBatch batch)
{
    const HtCellF& p = batch.p[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n * HH) return;
    const int64_t site = i >> 8; const int u = (int)(i & 255);
    float* gp = p.G + site * p.sg + u;
    const float ai = sigmoid_x(gp[0]), af = sigmoid_x(gp[HH]), ag = tanh_x(gp[2 * HH]), ao = sigmoid_x(gp[3 * HH]);
    const float cp = p.cprev ? p.cprev[site * p.sh + u] : 0.f;
    const float c = af * cp + ai * ag;
    gp[0] = ai; gp[HH] = af; gp[2 * HH] = ag; gp[3 * HH] = ao;
    p.c[site * p.sh + u] = c;
    p.h[site * p.sh + u] = ao * tanh_x(c);
}

// ext: the gradient that reaches h_t from outside the recurrence (NULL: none), sext floats between sites; rec: W_hh^T dgates_{t+1}, [n][512] at
// the direction's columns (NULL at the last step); dc: the carried cell gradient, same layout, read unless `first`, written always.
struct HtCellB { float* G; const float* c; const float* cprev; const float* ext; const float* rec; float* dc; int64_t sg, sh, sext, n; int first; };
struct HtCellBBatch { HtCellB p[4]; };
__global__ __launch_bounds__(256) void k_ht_cell_bwd(const HtCellBBatch batch)
{
    const HtCellB& p = batch.p[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n * HH) return;
    const int64_t site = i >> 8; const int u = (int)(i & 255);
    float* gp = p.G + site * p.sg + u;
    float dh = p.rec ? p.rec[site * H2 + u] : 0.f;
    if (p.ext) dh += p.ext[site * p.sext + u];
    const float dcin = p.first ? 0.f : p.dc[site * H2 + u];
    const float ai = gp[0], af = gp[HH], ag = gp[2 * HH], ao = gp[3 * HH];
    const float tc = tanh_x(p.c[site * p.sh + u]);
    const float cp = p.cprev ? p.cprev[site * p.sh + u] : 0.f;
    const float d_o = dh * tc * ao * (1.0f - ao);
    const float dct = dcin + dh * ao * (1.0f - tc * tc);
    gp[0] = dct * ag * ai * (1.0f - ai);
    gp[HH] = dct * cp * af * (1.0f - af);
    gp[2 * HH] = dct * ai * (1.0f - ag * ag);
    gp[3 * HH] = d_o;
    p.dc[site * H2 + u] = dct * af;
}

// the walk of direction d of layer l: step t of T is position pos0 + t * dpos of the layer's input, row hrow0 + t * dhrow of H / C
struct Walk { int T, rows, pos0, dpos, hrow0, dhrow; };
Walk walk(const EncWs& e, int l, int d)
{
    Walk k;
    k.T = l < 2 ? e.L : e.Tc; k.rows = k.T;
    k.pos0 = d ? e.L - 1 : 0; k.dpos = d ? -1 : 1;
    if (l < 2) { k.hrow0 = k.pos0; k.dhrow = k.dpos; } else { k.hrow0 = 0; k.dhrow = 1; }
    return k;
}

// one chunk of n <= reservation sites; `add`: the gradients of earlier chunks are in grads already
void run_chunk(nsnp_ctx* ctx, const float* const* P, const float* xp, const float* xh, const uint8_t* cls, int64_t n, float inv_n,
               const uint8_t* const* masks, float scale, float* const* grads, int add, float* site_loss, uint8_t* pred, hipStream_t s)
{
    const HtWs w = carve((float*)ctx->ht_ws, ctx->ht_sites);
    const int F = ctx->ht_F, n_gt = ctx->ht_ngt, n_zy = ctx->ht_nzy;
    const float* xin[2] = {xp, xh};
    // the input rows of layer l: element k of (site, position) -> base + site * so + position * sp + k * sk
    auto in_base = [&](int e, int l) { return l == 0 ? xin[e] : (const float*)w.e[e].X[l]; };
    auto in_so = [&](int e, int l) { return l == 0 ? (int64_t)F * w.e[e].L : (int64_t)w.e[e].L * H2; };
    auto in_sp = [&](int l) { return l == 0 ? (int64_t)1 : (int64_t)H2; };
    auto in_sk = [&](int e, int l) { return l == 0 ? (int64_t)w.e[e].L : (int64_t)1; };
    auto in_k = [&](int l) { return l == 0 ? F : H2; };
    {
        ScopedKernelTimer tm(ctx, NSNP_K_HAPTRAIN_FWD, s);
        for (int l = 0; l < 3; ++l) {
            TrBatch b{}; int nb = 0;
            for (int e = 0; e < 2; ++e)
                for (int d = 0; d < 2; ++d) {      // G[l][d][site][step] = W_ih x(position of the step) + b_ih + b_hh
                    const EncWs& E = w.e[e]; const Walk k = walk(E, l, d);
                    const float* const* Q = P + 26 * e + 8 * l + 4 * d;
                    b.g[nb++] = rows_gemm(Q[0], lin(in_k(l)), lin(1), HG, in_k(l), in_base(e, l) + k.pos0 * in_sp(l), lin(in_sk(e, l)),
                                          two(k.T, in_so(e, l), k.dpos * in_sp(l)), n * k.T, E.G[l][d], lin(HG), Q[2], Q[3], 0);
                }
            launch(s, b, nb);
            const int Tmax = l < 2 ? 33 : 17;
            for (int t = 0; t < Tmax; ++t) {
                TrBatch gb{}; HtCellFBatch cb{}; int np = 0;
                for (int e = 0; e < 2; ++e)
                    for (int d = 0; d < 2; ++d) {
                        const EncWs& E = w.e[e]; const Walk k = walk(E, l, d);
                        if (t >= k.T) continue;
                        const int64_t sh = (int64_t)k.rows * H2, sg = (int64_t)k.T * HG;
                        const int64_t row = k.hrow0 + t * k.dhrow, rowp = row - k.dhrow;
                        float* Gt = E.G[l][d] + (int64_t)t * HG;
                        if (t > 0)                   // G_t += W_hh h_{t-1}
                            gb.g[np] = rows_gemm(P[26 * e + 8 * l + 4 * d + 1], lin(HH), lin(1), HG, HH, E.H[l] + rowp * H2 + d * HH, lin(1),
                                                 lin(sh), n, Gt, lin(sg), nullptr, nullptr, 1);
                        HtCellF& c = cb.p[np++];
                        c.G = Gt; c.cprev = t > 0 ? E.C[l] + rowp * H2 + d * HH : nullptr;
                        c.c = E.C[l] + row * H2 + d * HH; c.h = E.H[l] + row * H2 + d * HH; c.sg = sg; c.sh = sh; c.n = n;
                    }
                if (t > 0) launch(s, gb, np);
                hipLaunchKernelGGL(k_ht_cell_fwd, dim3(blocks(n * HH), (unsigned)np), dim3(256), 0, s, cb);
            }
            if (l < 2)
                for (int e = 0; e < 2; ++e) {
                    const int64_t tot = n * w.e[e].L * H2;
                    hipLaunchKernelGGL(k_tr_mask, dim3(blocks(tot)), dim3(256), 0, s, (const float*)w.e[e].H[l], w.e[e].X[l + 1],
                                       masks ? masks[2 * e + l] : nullptr, scale, tot, tot);
                }
        }
        {   // output_proj of both encoders at the centre = the last step of both directions of layer 2
            TrBatch b{};
            for (int e = 0; e < 2; ++e) {
                const EncWs& E = w.e[e];
                b.g[e] = rows_gemm(P[26 * e + 24], lin(H2), lin(1), HH, H2, E.H[2] + (int64_t)(E.Tc - 1) * H2, lin(1), lin((int64_t)E.Tc * H2), n,
                                   w.Y + e * HH, lin(H2), P[26 * e + 25], nullptr, 0);
            }
            launch(s, b, 2);
        }
        gemm1(s, rows_gemm(P[52], lin(H2), lin(1), HH, H2, w.Y, lin(1), lin(H2), n, w.MID, lin(HH), P[53], nullptr, 4));
        {
            TrBatch b{};
            b.g[0] = rows_gemm(P[54], lin(HH), lin(1), n_gt, HH, w.MID, lin(1), lin(HH), n, w.Z, lin(16), P[55], nullptr, 0);
            b.g[1] = rows_gemm(P[56], lin(HH), lin(1), n_zy, HH, w.MID, lin(1), lin(HH), n, w.Z + n_gt, lin(16), P[57], nullptr, 0);
            launch(s, b, 2);
        }
        hipLaunchKernelGGL(k_tr_loss, dim3(blocks(n)), dim3(256), 0, s, (const float*)w.Z, cls, n, n, n_gt, n_zy, 16, 2, inv_n, w.DZ, site_loss, pred);
    }
    {
        ScopedKernelTimer tm(ctx, NSNP_K_HAPTRAIN_BWD, s);
        // heads^T, tanh', dense^T, output_proj^T
        gemm1(s, rows_gemm(P[54], lin(1), lin(HH), HH, n_gt, w.DZ, lin(1), lin(16), n, w.DMID, lin(HH), nullptr, nullptr, 0));
        gemm1(s, rows_gemm(P[56], lin(1), lin(HH), HH, n_zy, w.DZ + n_gt, lin(1), lin(16), n, w.DMID, lin(HH), nullptr, nullptr, 1));
        hipLaunchKernelGGL(k_tr_dtanh, dim3(blocks(n * HH)), dim3(256), 0, s, w.DMID, (const float*)w.MID, n * HH);
        gemm1(s, rows_gemm(P[52], lin(1), lin(H2), H2, HH, w.DMID, lin(1), lin(HH), n, w.DY, lin(H2), nullptr, nullptr, 0));
        {
            TrBatch b{};
            for (int e = 0; e < 2; ++e)
                b.g[e] = rows_gemm(P[26 * e + 24], lin(1), lin(H2), H2, HH, w.DY + e * HH, lin(1), lin(H2), n, w.e[e].DHC, lin(H2), nullptr, nullptr, 0);
            launch(s, b, 2);
        }
        for (int l = 2; l >= 0; --l) {
            const int Tmax = l < 2 ? 33 : 17;
            for (int j = 0; j < Tmax; ++j) {       // the j-th step from the end of every walk that is that long
                TrBatch gb{}; HtCellBBatch cb{}; int np = 0, ng = 0;
                for (int e = 0; e < 2; ++e)
                    for (int d = 0; d < 2; ++d) {
                        const EncWs& E = w.e[e]; const Walk k = walk(E, l, d);
                        if (j >= k.T) continue;
                        const int t = k.T - 1 - j;
                        const int64_t sh = (int64_t)k.rows * H2, sg = (int64_t)k.T * HG;
                        const int64_t row = k.hrow0 + t * k.dhrow, rowp = row - k.dhrow;
                        float* Gt = E.G[l][d] + (int64_t)t * HG;
                        HtCellB& c = cb.p[np++];
                        c.G = Gt; c.c = E.C[l] + row * H2 + d * HH; c.cprev = t > 0 ? E.C[l] + rowp * H2 + d * HH : nullptr;
                        if (l == 2) { c.ext = j == 0 ? E.DHC + d * HH : nullptr; c.sext = H2; }
                        else { c.ext = E.DX + row * H2 + d * HH; c.sext = (int64_t)E.L * H2; }
                        c.rec = j > 0 ? E.REC + d * HH : nullptr; c.dc = E.DC + d * HH; c.sg = sg; c.sh = sh; c.n = n; c.first = j == 0;
                        if (t > 0)                   // rec = W_hh^T dgates_t for step t - 1
                            gb.g[ng++] = rows_gemm(P[26 * e + 8 * l + 4 * d + 1], lin(1), lin(HH), HH, HG, Gt, lin(1), lin(sg), n, E.REC + d * HH,
                                                   lin(H2), nullptr, nullptr, 0);
                    }
                hipLaunchKernelGGL(k_ht_cell_bwd, dim3(blocks(n * HH), (unsigned)np), dim3(256), 0, s, cb);
                launch(s, gb, ng);
            }
            if (l == 0) break;
            // the gradient of the layer's input: sum over the directions of W_ih^T dgates at the step's position, then the mask's factor
            for (int e = 0; e < 2; ++e) (void)hipMemsetAsync(w.e[e].DX, 0, (size_t)(n * w.e[e].L * H2) * sizeof(float), s);
            for (int d = 0; d < 2; ++d) {          // (the directions meet at positions both walk: one after the other)
                TrBatch b{};
                for (int e = 0; e < 2; ++e) {
                    const EncWs& E = w.e[e]; const Walk k = walk(E, l, d);
                    b.g[e] = rows_gemm(P[26 * e + 8 * l + 4 * d], lin(1), lin(H2), H2, HG, E.G[l][d], lin(1), lin(HG), n * k.T,
                                       E.DX + (int64_t)k.pos0 * H2, two(k.T, (int64_t)E.L * H2, (int64_t)k.dpos * H2), nullptr, nullptr, 1);
                }
                launch(s, b, 2);
            }
            if (masks)
                for (int e = 0; e < 2; ++e) {
                    const int64_t tot = n * w.e[e].L * H2;
                    hipLaunchKernelGGL(k_tr_mask, dim3(blocks(tot)), dim3(256), 0, s, (const float*)w.e[e].DX, w.e[e].DX, masks[2 * e + l - 1], scale,
                                       tot, tot);
                }
        }
    }
    {
        ScopedKernelTimer tm(ctx, NSNP_K_HAPTRAIN_WGRAD, s);
        float* part = w.PART;
        for (int e = 0; e < 2; ++e)
            for (int l = 0; l < 3; ++l)
                for (int d = 0; d < 2; ++d) {
                    const EncWs& E = w.e[e]; const Walk k = walk(E, l, d);
                    float* const* Gr = grads + 26 * e + 8 * l + 4 * d;
                    const float* g = E.G[l][d];
                    const int64_t sh = (int64_t)k.rows * H2;
                    wgrad(s, part, HT_KCH, g, lin(HG), HG, in_base(e, l) + k.pos0 * in_sp(l), two(k.T, in_so(e, l), k.dpos * in_sp(l)), lin(in_sk(e, l)),
                          in_k(l), n * k.T, Gr[0], add);
                    // step t + 1 (t = 0 .. T - 2) meets the h of step t
                    wgrad(s, part, HT_KCH, g + HG, two(k.T - 1, (int64_t)k.T * HG, HG), HG, E.H[l] + (int64_t)k.hrow0 * H2 + d * HH,
                          two(k.T - 1, sh, (int64_t)k.dhrow * H2), lin(1), HH, n * (k.T - 1), Gr[1], add);
                    bgrad(s, part, HT_KCH, g, lin(HG), HG, n * k.T, Gr[2], Gr[3], add);
                }
        for (int e = 0; e < 2; ++e) {
            const EncWs& E = w.e[e];
            wgrad(s, part, HT_KCH, w.DY + e * HH, lin(H2), HH, E.H[2] + (int64_t)(E.Tc - 1) * H2, lin((int64_t)E.Tc * H2), lin(1), H2, n, grads[26 * e + 24], add);
            bgrad(s, part, HT_KCH, w.DY + e * HH, lin(H2), HH, n, grads[26 * e + 25], nullptr, add);
        }
        wgrad(s, part, HT_KCH, w.DMID, lin(HH), HH, w.Y, lin(H2), lin(1), H2, n, grads[52], add);
        bgrad(s, part, HT_KCH, w.DMID, lin(HH), HH, n, grads[53], nullptr, add);
        wgrad(s, part, HT_KCH, w.DZ, lin(16), n_gt, w.MID, lin(HH), lin(1), HH, n, grads[54], add);
        bgrad(s, part, HT_KCH, w.DZ, lin(16), n_gt, n, grads[55], nullptr, add);
        wgrad(s, part, HT_KCH, w.DZ + n_gt, lin(16), n_zy, w.MID, lin(HH), lin(1), HH, n, grads[56], add);
        bgrad(s, part, HT_KCH, w.DZ + n_gt, lin(16), n_zy, n, grads[57], nullptr, add);
    }
}

}  // namespace

void nsnp_hap_train_free(nsnp_ctx* ctx)
{
    if (ctx->ht_ws) (void)hipFree(ctx->ht_ws);
    ctx->ht_ws = nullptr; ctx->ht_sites = 0; ctx->ht_F = ctx->ht_ngt = ctx->ht_nzy = 0;
}

extern "C" int nsnp_hap_train_reserve(nsnp_ctx* ctx, int64_t max_sites, int n_features, int n_gt, int n_zy)
{
    if (!ctx || max_sites <= 0 || max_sites > HT_MAX_SITES) return NSNP_EINVAL;
    if (n_features < 1 || n_features > 128 || n_gt < 1 || n_zy < 1 || n_gt + n_zy > 16) return NSNP_EINVAL;
    if (ctx->ht_ws && ctx->ht_sites == max_sites) {           // the dims shape no buffer: only the size does
        ctx->ht_F = n_features; ctx->ht_ngt = n_gt; ctx->ht_nzy = n_zy;
        return NSNP_OK;
    }
    const int rc = reserve_ws(ctx, &ctx->ht_ws, (size_t)(max_sites * F_SITE + part_floats(max_sites)) * sizeof(float));
    if (rc != NSNP_OK) return rc;
    ctx->ht_sites = max_sites; ctx->ht_F = n_features; ctx->ht_ngt = n_gt; ctx->ht_nzy = n_zy;
    return NSNP_OK;
}

extern "C" int nsnp_hap_loss_grad(nsnp_ctx* ctx, const float* const* params, const float* xp, const float* xh, const uint8_t* cls, int64_t N,
                                  const uint8_t* const* keep_masks, float keep_scale, float* const* grads, float* site_loss, uint8_t* pred,
                                  void* stream)
{
    if (!ctx || N < 0) return NSNP_EINVAL;
    if (ctx->hap_precision != 0) return NSNP_EINVAL;         // fp32 only
    if (N == 0) return NSNP_OK;
    if (!params || !xp || !xh || !cls || !grads) return NSNP_EINVAL;
    for (int i = 0; i < 58; ++i) if (!params[i] || !grads[i]) return NSNP_EINVAL;
    if (keep_masks) for (int i = 0; i < 4; ++i) if (!keep_masks[i]) return NSNP_EINVAL;
    if (!ctx->ht_ws || ctx->ht_sites <= 0) return NSNP_EINVAL;     // nsnp_hap_train_reserve first
    hipStream_t s = (hipStream_t)stream;
    const float inv_n = 1.0f / (float)N;                     // of the whole batch, whatever the chunks
    const int F = ctx->ht_F;
    for (int64_t base = 0; base < N; base += ctx->ht_sites) {
        const int64_t n = N - base < ctx->ht_sites ? N - base : ctx->ht_sites;
        const uint8_t* m[4];
        if (keep_masks)
            for (int i = 0; i < 4; ++i) m[i] = keep_masks[i] + base * (i < 2 ? 33 : 11) * H2;
        run_chunk(ctx, params, xp + base * F * 33, xh + base * F * 11, cls + base * 2, n, inv_n, keep_masks ? m : nullptr, keep_scale, grads,
                  base > 0, site_loss ? site_loss + base * 2 : nullptr, pred ? pred + base * 2 : nullptr, s);
    }
    NSNP_HIP(ctx, hipGetLastError());
    return NSNP_OK;
}
