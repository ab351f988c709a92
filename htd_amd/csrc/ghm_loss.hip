// Gradient harmonising losses (mmdet/models/losses/ghm_loss.py: GHMC :20-94, GHMR :98-172) and the loss of an anchor head that
// trains with the pair over all pyramid levels (dense_heads/anchor_head.py:373-488, one loss call per level).
//
//   GHMC   g = |sigmoid(x) - t| = sigmoid(z),  z = -x for t = 1 and x for t = 0;   BCEWithLogits(x, t) = softplus(z),
//          d BCE / dx = sigmoid(x) - t = +-g
//   GHMR   d = pred - target,  s = sqrt(d^2 + mu^2),  loss = s - mu = d^2 / (s + mu),  d loss / dd = d / s,  g = |d| / s
//
// An element of bin i (edges[i] <= g < edges[i + 1], the module's fp32 edges) weighs tot / acc[i] / n, where acc is the bin's
// count or its moving average, n the number of filled bins and tot the number (GHMC) or the weight sum (GHMR) of the valid
// elements of the call; the weights are constants of the backward.  A call therefore needs the histogram of its g before its
// first weight is known: three launches,
//   1  histogram       integer counts per (level, loss, bin) and tot per (level, loss)
//   2  weights         one small block walks the levels in order, moves acc_sum and leaves mult = loss_weight / (acc n)
//   3  loss + gradient the pass of launch 1 again, each element times mult[level][bin]
// Launches 1 and 3 are one kernel template, so the bin of an element comes from the same instructions in both (the file is
// compiled without floating-point contraction: no fused multiply-add can round g one way here and another way there).
//
// The histogram is built for contention: a freshly initialised head puts most elements into one bin, and one LDS atomic per
// element on one word serialises the wavefront.  A wavefront first agrees on the distinct keys its lanes hold (ballot) and
// issues one LDS add per distinct key with the number of lanes that hold it (popcount); a block adds its LDS table to the
// global one at its end, filled entries only.  Integer adds: any order gives the same table.
#include "common.h"
#include "focal_elem.h"
#include "retina_levels.h"

namespace {

constexpr int GHM_MAX_BINS = 64;
// workspace, in 32-bit words: counts [2][8][64] (0: GHMC, 1: GHMR), tot [2][8], n [2][8] (integers), mult [2][8][64] (floats)
constexpr int GHM_COUNTS = 2 * RETINA_MAX_LEVELS * GHM_MAX_BINS;
constexpr int GHM_TOT = GHM_COUNTS;
constexpr int GHM_N = GHM_TOT + 2 * RETINA_MAX_LEVELS;
constexpr int GHM_MULT = GHM_N + 2 * RETINA_MAX_LEVELS;
constexpr int GHM_WORDS = GHM_MULT + GHM_COUNTS;
constexpr int GHM_INT_WORDS = GHM_MULT;                 // what launch 1 accumulates into: cleared before it

__device__ __forceinline__ int ghm_key(int which, int level, int bin) { return (which * RETINA_MAX_LEVELS + level) * GHM_MAX_BINS + bin; }

// the bin of g, or -1 when no bin holds it (ghm_loss.py:79, :157: edges[i] <= g < edges[i + 1]); edges are increasing.  The
// modules' edges are i / bins up to rounding (and a wider last bin), so the guess (int)(g * bins) is right or off by one: its two
// edges are read at once and the walks that serve any other increasing edges are all but never entered
__device__ __forceinline__ int ghm_bin(float g, const float *edges, int bins)
{
    int i = (int)(g * (float)bins);
    i = i < 0 ? 0 : (i > bins - 1 ? bins - 1 : i);
    const float lo = edges[i], hi = edges[i + 1];
    if (g < lo) {
        if (i == 0) return -1;
        --i;
        while (i > 0 && g < edges[i]) --i;
        return g >= edges[i] ? i : -1;
    }
    if (g >= hi) {
        if (i == bins - 1) return -1;
        ++i;
        while (i < bins - 1 && g >= edges[i + 1]) ++i;
        return g < edges[i + 1] ? i : -1;
    }
    return g >= lo ? i : -1;                // (false only for a NaN)
}

// -> BCEWithLogits(x, t); g = |sigmoid(x) - t|, sgn * g = d BCE / dx.  One exp and one log per element, as in focal_elem.h;
// written out here, because sharing the lines through a function changes the code generated for the focal kernels.
__device__ __forceinline__ float ghmc_elem(float x, bool t, float &g, float &sgn)
{
    const float z = t ? -x : x;
    const float e = __expf(-fabsf(z));
    const float u = 1.f + e;
    const float r = __builtin_amdgcn_rcpf(u);
    const float l = u == 1.f ? e : __logf(u) * (e * __builtin_amdgcn_rcpf(u - 1.f));     // log1p(e)
    g = z >= 0.f ? r : e * r;                                                             // sigmoid(z)
    sgn = t ? -1.f : 1.f;
    return fmaxf(z, 0.f) + l;
}

// -> sqrt(d^2 + mu^2) - mu; gs = d / sqrt(d^2 + mu^2), g = |gs|
__device__ __forceinline__ float ghmr_elem(float d, float mu, float &gs)
{
    const float s = sqrtf(d * d + mu * mu);
    gs = d / s;
    return d * d / (s + mu);
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// table[key] += inc for every lane with key >= 0: one LDS add per distinct key of the wavefront.  Every lane of the
// wavefront calls it.
__device__ __forceinline__ void wave_key_add(int key, unsigned inc, unsigned *table)
{
#ifdef HTD_GHM_HIST_PLAIN
    if (key >= 0) atomicAdd(&table[key], inc);                  // the per-element form, kept for the A/B measurement
#else
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == k);
        if (lane == leader) atomicAdd(&table[k], inc * (unsigned)__popcll(same));
        todo &= ~same;
    }
#endif
}

__device__ __forceinline__ void load_edges(float *s_edges, const float *edges, int bins)
{
    for (int i = threadIdx.x; i <= bins; i += 256) s_edges[i] = edges[i];
}

// a block's table -> the global one (filled entries only)
__device__ __forceinline__ void flush_counts(const unsigned *s_tab, unsigned *ws)
{
    __syncthreads();
    for (int i = threadIdx.x; i < GHM_INT_WORDS; i += 256) {
        const unsigned v = s_tab[i];
        if (v) atomicAdd(&ws[i], v);
    }
}

// ---- matrix form: logits [N][C], labels [N] (C = background), weight [N] (valid where > 0) ---------------------------------
// LOSS = false: launch 1 (counts and tot of level 0 into ws); LOSS = true: launch 3 (partial [FOCAL_BLOCKS][2], column 1 zero,
// and grad).  VEC as in focal_matrix_kernel.
template <int VEC, bool LOSS>
__global__ __launch_bounds__(256) void ghmc_matrix_kernel(const float *__restrict__ x, const int64_t *__restrict__ labels,
                                                          const float *__restrict__ weight, int64_t units, int cols,
                                                          const float *__restrict__ edges, int bins, unsigned *__restrict__ ws,
                                                          float *__restrict__ partial, float *__restrict__ grad)
{
    __shared__ float s_edges[GHM_MAX_BINS + 1];
    __shared__ unsigned s_tab[LOSS ? GHM_MAX_BINS : GHM_INT_WORDS];      // LOSS: mult of level 0 (float bits); else the counts
    load_edges(s_edges, edges, bins);
    if (LOSS) {
        for (int i = threadIdx.x; i < GHM_MAX_BINS; i += 256) s_tab[i] = ws[GHM_MULT + i];
    } else {
        for (int i = threadIdx.x; i < GHM_INT_WORDS; i += 256) s_tab[i] = 0u;
    }
    __syncthreads();
    const float *s_mult = reinterpret_cast<const float *>(s_tab);
    float sum = 0.f;
    unsigned nv = 0;
    for (int64_t u0 = (int64_t)blockIdx.x * 256; u0 < units; u0 += (int64_t)gridDim.x * 256) {      // uniform over the block
        const int64_t u = u0 + threadIdx.x;
        int bin[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) bin[k] = -1;
        if (u < units) {
            int c0;
            const int64_t row = matrix_unit<VEC>(u, units, cols, c0);
            const int64_t lab = labels[row];
            const bool valid = weight[row] > 0.f;
            float go[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) go[k] = 0.f;
            if (valid) {
                float xv[VEC];
                load_unit<VEC>(x, u, xv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    float g, sgn;
                    const float bce = ghmc_elem(xv[k], lab == c0 + k, g, sgn);
                    bin[k] = ghm_bin(g, s_edges, bins);
                    if (LOSS) {
                        const float m = bin[k] >= 0 ? s_mult[bin[k]] : 0.f;
                        sum += bce * m;
                        go[k] = sgn * g * m;
                    }
                }
                nv += VEC;
            }
            if (LOSS) store_unit<VEC>(grad, u, go);
        }
        if (!LOSS) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) wave_key_add(bin[k], 1u, s_tab);
        }
    }
    if (LOSS) {
        block_store_partial2(sum, 0.f, partial);
    } else {
        nv = wave_sum_u32(nv);
        if ((threadIdx.x & 63) == 0 && nv) atomicAdd(&s_tab[GHM_TOT], nv);
        flush_counts(s_tab, ws);
    }
}

// ---- launch 2 --------------------------------------------------------------------------------------------------------------------
// One wavefront, lane i = bin i.  Levels in order, GHMC then GHMR of a level (the order of AnchorHead.loss_single); the two
// losses have separate buffers, so only the level order matters.  acc = mmt * acc + (1 - mmt) * num in double, rounded to
// fp32 once; a bin without elements keeps its acc_sum and does not count in n.
__global__ __launch_bounds__(64) void ghm_weights_kernel(int L, int n_losses, int bins_c, int bins_r, double mmt_c, double mmt_r,
                                                         float *__restrict__ acc_c, float *__restrict__ acc_r, float lw_c, float lw_r,
                                                         unsigned *__restrict__ ws)
{
    const int i = threadIdx.x;
    float *mult = reinterpret_cast<float *>(ws + GHM_MULT);
    for (int l = 0; l < L; ++l) {
        for (int which = 0; which < n_losses; ++which) {
            const int bins = which ? bins_r : bins_c;
            const double mmt = which ? mmt_r : mmt_c;
            float *acc = which ? acc_r : acc_c;
            const unsigned num = i < bins ? ws[ghm_key(which, l, i)] : 0u;
            const int n = __popcll(__ballot(num > 0u));
            const unsigned t = ws[GHM_TOT + which * RETINA_MAX_LEVELS + l];
            const double tot = t > 1u ? (double)t : 1.0;
            float m = 0.f;
            if (num > 0u) {
                double a = (double)num;
                if (mmt > 0.0) {
                    const float moved = (float)(mmt * (double)acc[i] + (1.0 - mmt) * (double)num);
                    acc[i] = moved;
                    a = (double)moved;
                }
                m = (float)((double)(which ? lw_r : lw_c) * (tot / a / (double)n) / tot);
            }
            mult[ghm_key(which, l, i)] = m;
            if (i == 0) ws[GHM_N + which * RETINA_MAX_LEVELS + l] = (unsigned)n;
        }
    }
}

// ---- head form -----------------------------------------------------------------------------------------------------------------
// One wavefront per pixel row of the classification maps, one float4 (the four deltas of an anchor) per thread of the
// regression maps, decoded by retina_levels.h.  Every lane stays in both sweeps: wave_key_add needs the whole wavefront.
// LOSS = false: launch 1; LOSS = true: launch 3, which stores every unit of every gradient map exactly once, zeros and
// padding channels included.  Valid for GHMC: assigned >= 0 (only the sign of a label weight counts, ghm_loss.py:75); for
// GHMR: assigned > 0, weight 1 per delta.
template <int VEC, bool LOSS>
__global__ __launch_bounds__(256) void ghm_head_kernel(RetinaLevels lv, int L, int na, int C, const float *__restrict__ anchors,
                                                       const float *__restrict__ gts, const int64_t *__restrict__ gt_labels,
                                                       const int64_t *__restrict__ assigned, int A, int K, Vec4f means, Vec4f stds,
                                                       const float *__restrict__ edges_c, int bins_c,
                                                       const float *__restrict__ edges_r, int bins_r, float mu,
                                                       unsigned *__restrict__ ws, float *__restrict__ partial)
{
    __shared__ float s_edges[2][GHM_MAX_BINS + 1];
    __shared__ unsigned s_tab[LOSS ? GHM_COUNTS : GHM_INT_WORDS];        // LOSS: mult (float bits); else counts and tot
    load_edges(s_edges[0], edges_c, bins_c);
    load_edges(s_edges[1], edges_r, bins_r);
    if (LOSS) {
        for (int i = threadIdx.x; i < GHM_COUNTS; i += 256) s_tab[i] = ws[GHM_MULT + i];
    } else {
        for (int i = threadIdx.x; i < GHM_INT_WORDS; i += 256) s_tab[i] = 0u;
    }
    __syncthreads();
    const float *s_mult = reinterpret_cast<const float *>(s_tab);
    const unsigned n_cls = lv.coff[L], n_all = lv.roff[L];
    const unsigned nc = (unsigned)(na * C);
    float s_cls = 0.f, s_box = 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned n_rows = lv.rrow[L];
    const float inv_c = 1.f / (float)C;
    for (unsigned rw = wave; rw < n_rows; rw += gridDim.x * 4u) {
        const ClsRow r = cls_row<VEC>(lv, L, rw, na, assigned, A, gt_labels, K);
        const int l = r.l;
        unsigned nv = 0;
        for (unsigned j0 = 0; j0 < r.cu; j0 += 64u) {                               // uniform over the wavefront
            const unsigned j = j0 + lane;
            int bin[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) bin[k] = -1;
            if (j < r.cu) {
                const unsigned ch = j * VEC;
                float go[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) go[k] = 0.f;
                if (ch < nc) {
                    unsigned c0;
                    const int64_t as = r.as_row[anchor_of_channel(ch, (unsigned)C, inv_c, c0)];
                    if (as >= 0) {
                        const int64_t lab = as > 0 ? r.lab_row[as - 1] : (int64_t)C;
                        float xv[VEC];
                        load_unit<VEC>(r.x_row, j, xv);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) {
                            float g, sgn;
                            const float bce = ghmc_elem(xv[k], lab == (int64_t)(c0 + k), g, sgn);
                            bin[k] = ghm_bin(g, s_edges[0], bins_c);
                            if (LOSS) {
                                const float m = bin[k] >= 0 ? s_mult[ghm_key(0, l, bin[k])] : 0.f;
                                s_cls += bce * m;
                                go[k] = sgn * g * m;
                            }
                        }
                        nv += VEC;
                    }
                }
                if (LOSS) store_unit<VEC>(r.g_row, j, go);
            }
            if (!LOSS) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) wave_key_add(bin[k] >= 0 ? ghm_key(0, l, bin[k]) : -1, 1u, s_tab);
            }
        }
        if (!LOSS) {
            nv = wave_sum_u32(nv);
            if (lane == 0 && nv) atomicAdd(&s_tab[GHM_TOT + l], nv);
        }
    }
    // regression maps
    for (unsigned u0 = n_cls + blockIdx.x * 256u; u0 < n_all; u0 += gridDim.x * 256u) {             // uniform over the block
        const unsigned u = u0 + threadIdx.x;
        int key[4] = {-1, -1, -1, -1};
        int tot_key = -1;
        if (u < n_all) {
            const RegUnit r = reg_unit(lv, L, u);
            const int l = r.l;
            float go[4] = {0.f, 0.f, 0.f, 0.f};
            if (r.a < (unsigned)na) {
                unsigned b;
                const unsigned ai = reg_anchor(lv, r, na, b);
                const int64_t as = assigned[(int64_t)b * A + ai];
                if (as > 0) {
                    float tgt[4], rr[4];
                    delta_target(anchors + (int64_t)ai * 4, gts + ((int64_t)b * K + (as - 1)) * 4, means, stds, tgt);
                    load_unit<4>(lv.reg[l], r.v, rr);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float gs;
                        const float loss = ghmr_elem(rr[k] - tgt[k], mu, gs);
                        const int bn = ghm_bin(fabsf(gs), s_edges[1], bins_r);
                        key[k] = bn >= 0 ? ghm_key(1, l, bn) : -1;
                        const float m = (LOSS && bn >= 0) ? s_mult[ghm_key(1, l, bn)] : 0.f;
                        s_box += loss * m;
                        go[k] = gs * m;
                    }
                    tot_key = GHM_TOT + RETINA_MAX_LEVELS + l;
                }
            }
            if (LOSS) store_unit<4>(lv.greg[l], r.v, go);
        }
        if (!LOSS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) wave_key_add(key[k], 1u, s_tab);
            wave_key_add(tot_key, 4u, s_tab);
        }
    }
    if (LOSS)
        block_store_partial2(s_cls, s_box, partial);
    else
        flush_counts(s_tab, ws);
}

int check_ghm(const char *what, const float *edges, int bins, double momentum, const float *acc_sum)
{
    HTD_REQUIRE(edges && bins > 0 && bins <= GHM_MAX_BINS, "%s: edges missing or bins outside 1 .. %d", what, GHM_MAX_BINS);
    HTD_REQUIRE(momentum >= 0.0 && momentum < 1.0 && (momentum == 0.0 || acc_sum), "%s: bad momentum or acc_sum missing", what);
    return HTD_OK;
}

}  // namespace

extern "C" int64_t htd_ghm_workspace_bytes(int L)
{
    return L > 0 && L <= RETINA_MAX_LEVELS ? (int64_t)GHM_WORDS * 4 : -1;
}

extern "C" int htd_ghmc_loss(const float *logits, const int64_t *labels, const float *weight, int64_t N, int C, const float *edges,
                             int bins, double momentum, float *acc_sum, float loss_weight, void *workspace, float *partial,
                             float *grad, void *stream)
{
    HTD_REQUIRE(N >= 0 && C > 0, "ghmc_loss: bad sizes");
    HTD_REQUIRE(workspace && partial && grad && (N == 0 || (logits && labels && weight)), "ghmc_loss: null pointer");
    const int rc = check_ghm("ghmc_loss", edges, bins, momentum, acc_sum);
    if (rc != HTD_OK) return rc;
    const bool vec = (C & 3) == 0 && (((uintptr_t)logits | (uintptr_t)grad) & 15) == 0;
    const int64_t units = vec ? N * (C / 4) : N * C;
    const int cols = vec ? C / 4 : C;
    unsigned *ws = (unsigned *)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, GHM_INT_WORDS * 4, s) != hipSuccess) return htd::check_launch("ghmc_loss");
#define HTD_GHMC_LAUNCH(V, P)                                                                                                       \
    hipLaunchKernelGGL((ghmc_matrix_kernel<V, P>), dim3(FOCAL_BLOCKS), dim3(256), 0, s, logits, labels, weight, units, cols, edges, \
                       bins, ws, partial, grad)
    if (vec) HTD_GHMC_LAUNCH(4, false); else HTD_GHMC_LAUNCH(1, false);
    hipLaunchKernelGGL(ghm_weights_kernel, dim3(1), dim3(64), 0, s, 1, 1, bins, 0, momentum, 0.0, acc_sum, (float *)nullptr,
                       loss_weight, 0.f, ws);
    if (vec) HTD_GHMC_LAUNCH(4, true); else HTD_GHMC_LAUNCH(1, true);
#undef HTD_GHMC_LAUNCH
    return htd::check_launch("ghmc_loss");
}

extern "C" int htd_ghm_head_loss_launches(const float *const *cls, const int64_t *cls_stride, const float *const *reg,
                                 const int64_t *reg_stride, const int64_t *pix, int L, int B, int na, int C, const float *anchors,
                                 const float *gts, const int64_t *gt_labels, const int64_t *assigned, int A, int K,
                                 const float *means4, const float *stds4, const float *edges_c, int bins_c, double momentum_c,
                                 float *acc_sum_c, const float *edges_r, int bins_r, double momentum_r, float *acc_sum_r, float mu,
                                 float cls_weight, float box_weight, void *workspace, float *partial, float *const *grad_cls,
                                 float *const *grad_reg, int launches, void *stream)
{
    HTD_REQUIRE(reg && grad_cls && grad_reg, "ghm_head_loss: null table");
    HTD_REQUIRE(anchors && gts && gt_labels && assigned && means4 && stds4 && workspace && partial, "ghm_head_loss: null pointer");
    HTD_REQUIRE((int64_t)na * C < (1 << 20), "ghm_head_loss: more than 2^20 classification channels");
    HTD_REQUIRE(K > 0 && mu > 0.f, "ghm_head_loss: bad parameters");
    int rc = check_ghm("ghm_head_loss (GHMC)", edges_c, bins_c, momentum_c, acc_sum_c);
    if (rc != HTD_OK) return rc;
    rc = check_ghm("ghm_head_loss (GHMR)", edges_r, bins_r, momentum_r, acc_sum_r);
    if (rc != HTD_OK) return rc;
    RetinaLevels lv = {};
    bool vec;
    Vec4f m, sd;
    rc = head_loss_levels(lv, "ghm_head_loss", cls, cls_stride, reg, reg_stride, grad_cls, grad_reg, pix, L, B, na, C, A, means4,
                          stds4, vec, m, sd);
    if (rc != HTD_OK) return rc;
    unsigned *ws = (unsigned *)workspace;
    hipStream_t s = (hipStream_t)stream;
    if ((launches & 1) && hipMemsetAsync(ws, 0, GHM_INT_WORDS * 4, s) != hipSuccess) return htd::check_launch("ghm_head_loss");
#define HTD_GHM_LAUNCH(V, P)                                                                                                        \
    hipLaunchKernelGGL((ghm_head_kernel<V, P>), dim3(FOCAL_BLOCKS), dim3(256), 0, s, lv, L, na, C, anchors, gts, gt_labels, assigned, \
                       A, K, m, sd, edges_c, bins_c, edges_r, bins_r, mu, ws, partial)
    if (launches & 1) { if (vec) HTD_GHM_LAUNCH(4, false); else HTD_GHM_LAUNCH(1, false); }
    if (launches & 2)
        hipLaunchKernelGGL(ghm_weights_kernel, dim3(1), dim3(64), 0, s, L, 2, bins_c, bins_r, momentum_c, momentum_r, acc_sum_c,
                           acc_sum_r, cls_weight, box_weight, ws);
    if (launches & 4) { if (vec) HTD_GHM_LAUNCH(4, true); else HTD_GHM_LAUNCH(1, true); }
#undef HTD_GHM_LAUNCH
    return htd::check_launch("ghm_head_loss");
}

extern "C" int htd_ghm_head_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg,
                                 const int64_t *reg_stride, const int64_t *pix, int L, int B, int na, int C, const float *anchors,
                                 const float *gts, const int64_t *gt_labels, const int64_t *assigned, int A, int K,
                                 const float *means4, const float *stds4, const float *edges_c, int bins_c, double momentum_c,
                                 float *acc_sum_c, const float *edges_r, int bins_r, double momentum_r, float *acc_sum_r, float mu,
                                 float cls_weight, float box_weight, void *workspace, float *partial, float *const *grad_cls,
                                 float *const *grad_reg, void *stream)
{
    return htd_ghm_head_loss_launches(cls, cls_stride, reg, reg_stride, pix, L, B, na, C, anchors, gts, gt_labels, assigned, A, K,
                                      means4, stds4, edges_c, bins_c, momentum_c, acc_sum_c, edges_r, bins_r, momentum_r, acc_sum_r,
                                      mu, cls_weight, box_weight, workspace, partial, grad_cls, grad_reg, 7, stream);
}
