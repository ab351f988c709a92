// FoveaBox head on the device (dense_heads/fovea_head.py): the fovea-rectangle assignment with its log-distance targets of a whole
// batch over all pyramid levels in one launch (get_targets / _get_target_single :177-258), the focal and smooth-L1 losses with
// their two finished gradient maps in one launch (loss :127-175), and the offsets of FeatureAlign (:13-39) -- a bias-free 1x1
// convolution of exp(bbox_pred) -- with their backward.  Built with -ffp-contract=off: the assignment takes the reference's fp32
// decisions one rounded operation at a time (the square root of the area, the division by the stride, the half extents, the
// shrunk edges, ceil / floor, the clamp), all of them on integers after that, so `assigned` is the reference's bit for bit; the
// divisions and the square root are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).  The classification loss is the
// focal_elem of the anchor heads through the sweep of point_maps.h.
//
// All kernels are small and launch- or memory-bound: plain grids, fixed-order partial sums, no float atomics, every element of
// every output stored exactly once (padding channels and non-positive points as zeros).
#include "common.h"
#include "point_maps.h"
#include "point_scale.h"

namespace {

constexpr int FOVEA_MAX_LEVELS = POINT_MAX_LEVELS;
constexpr int GT_CHUNK = 256;               // gts staged through LDS per pass of the assignment
constexpr int ALIGN_PIX = 64;               // pixels per block of the FeatureAlign kernels
constexpr int ALIGN_MAX_O = 8 * 18;         // deform_groups <= 8

struct FoveaLevels {                         // the pyramid with the head's per-level constants
    int h[FOVEA_MAX_LEVELS], w[FOVEA_MAX_LEVELS];
    int stride[FOVEA_MAX_LEVELS];
    unsigned poff[FOVEA_MAX_LEVELS + 1];    // first point of the level; poff[L] = P
    float base[FOVEA_MAX_LEVELS];           // base_edge_list
    float lo[FOVEA_MAX_LEVELS], hi[FOVEA_MAX_LEVELS];    // scale_ranges
};

enum { CLS = 0, REG = 1 };                  // slots of PointMaps: (B, C, h, w), (B, 4, h, w)

// ---- targets -----------------------------------------------------------------------------------------------------------------
// grid (ceil(P / 256), B); a thread owns one point of one image.  For every level the block's points lie on, the block turns the
// image's gts GT_CHUNK at a time (any K) into their clamped rectangle on that level and their `gt_areas` in LDS -- once per
// block and level --, and the level's threads walk them.  The reference paints the rectangles in descending order of gt_areas
// (a stable sort here), so the last painter of a point is the smallest gt_areas that holds it and, among equal ones, the highest
// index: `<=` over the gts in index order.
__global__ __launch_bounds__(256) void fovea_targets_kernel(FoveaLevels lv, int L, const float *__restrict__ gts,
                                                            const uint8_t *__restrict__ gt_valid, int K, float s_in, float s_out,
                                                            int *__restrict__ assigned, float *__restrict__ bbox_targets,
                                                            int *__restrict__ part_n)
{
    __shared__ int4 s_rect[GT_CHUNK];       // left, right, top, down after the clamp; left > right: not on this level
    __shared__ float s_area[GT_CHUNK];
    __shared__ int red_n[4];
    const unsigned P = lv.poff[L];
    const int b = blockIdx.y;
    const unsigned p_first = blockIdx.x * 256u, p_all = p_first + threadIdx.x;
    const unsigned p_last = p_first + 255u < P ? p_first + 255u : P - 1u;
    const bool live = p_all < P;
    const int l_first = (int)level_of(lv.poff, L, p_first), l_last = (int)level_of(lv.poff, L, p_last);
    int l = -1, row = 0, col = 0;
    if (live) {
        l = (int)level_of(lv.poff, L, p_all);
        const unsigned p = p_all - lv.poff[l];
        row = (int)(p / (unsigned)lv.w[l]);
        col = (int)(p - (unsigned)row * (unsigned)lv.w[l]);
    }
    int best_k = -1;
    float best = INFINITY;
    for (int lb = l_first; lb <= l_last; ++lb) {
        const float stride = (float)lv.stride[lb], lo = lv.lo[lb], hi = lv.hi[lb];
        const float w_max = (float)(lv.w[lb] - 1), h_max = (float)(lv.h[lb] - 1);
        for (int k0 = 0; k0 < K; k0 += GT_CHUNK) {
            const int n = min(GT_CHUNK, K - k0);
            __syncthreads();                // the previous chunk has been read by every thread
            if ((int)threadIdx.x < n) {
                const int64_t gi = (int64_t)b * K + k0 + threadIdx.x;
                int4 r = make_int4(1, 0, 1, 0);
                float a = 0.f;
                if (gt_valid[gi]) {
                    const float4 g = *reinterpret_cast<const float4 *>(gts + gi * 4);
                    a = sqrtf((g.z - g.x) * (g.w - g.y));                       // fovea_head.py:205-206
                    if (a >= lo && a <= hi) {                                   // :218-219
                        const float x1 = g.x / stride, y1 = g.y / stride, x2 = g.z / stride, y2 = g.w / stride;      // :226
                        const float half_w = 0.5f * (x2 - x1), half_h = 0.5f * (y2 - y1);
                        // :231-242: ceil / floor, then clamp(0, size - 1); the emptiness is tested after the clamp
                        const float left = ceilf((x1 + s_in * half_w) - 0.5f), right = floorf((x1 + s_out * half_w) - 0.5f);
                        const float top = ceilf((y1 + s_in * half_h) - 0.5f), down = floorf((y1 + s_out * half_h) - 0.5f);
                        r.x = (int)fminf(fmaxf(left, 0.f), w_max);
                        r.y = (int)fminf(fmaxf(right, 0.f), w_max);
                        r.z = (int)fminf(fmaxf(top, 0.f), h_max);
                        r.w = (int)fminf(fmaxf(down, 0.f), h_max);
                    }
                }
                s_rect[threadIdx.x] = r;
                s_area[threadIdx.x] = a;
            }
            __syncthreads();
            if (l == lb) {
                for (int j = 0; j < n; ++j) {
                    const int4 r = s_rect[j];
                    if (col >= r.x && col <= r.y && row >= r.z && row <= r.w) {
                        const float a = s_area[j];
                        if (a <= best) { best = a; best_k = k0 + j; }
                    }
                }
            }
        }
    }
    int pos = 0;
    if (live) {
        const int64_t o = (int64_t)b * P + p_all;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);     // background: log(1)
        if (best_k >= 0) {
            pos = 1;
            const float4 g = *reinterpret_cast<const float4 *>(gts + ((int64_t)b * K + best_k) * 4);
            const float s = (float)lv.stride[l], base = lv.base[l];
            const float sx = s * ((float)col + 0.5f), sy = s * ((float)row + 0.5f);          // exact
            const float d[4] = {(sx - g.x) / base, (sy - g.y) / base, (g.z - sx) / base, (g.w - sy) / base};     // :247-254
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)     // clamp(1/16, 16) and the log, rounded once from fp64
                v[k] = (float)log((double)fminf(fmaxf(d[k], 0.0625f), 16.f));
            t = make_float4(v[0], v[1], v[2], v[3]);
        }
        assigned[o] = best_k + 1;
        *reinterpret_cast<float4 *>(bbox_targets + o * 4) = t;
    }
    int n = pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) red_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) part_n[(int64_t)b * gridDim.x + blockIdx.x] = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
}

// num_pos [B] and norm = [num_pos_total + B, max(num_pos_total, 1)] from the per-block counts: one wavefront, integers
__global__ __launch_bounds__(64) void fovea_targets_finish_kernel(const int *__restrict__ part_n, int B, int nblk,
                                                                   int *__restrict__ num_pos, float *__restrict__ norm)
{
    int total = 0;
    for (int b = 0; b < B; ++b) {
        int n = 0;
        for (int i = threadIdx.x; i < nblk; i += 64) n += part_n[(int64_t)b * nblk + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (threadIdx.x == 0) num_pos[b] = n;
        total += n;
    }
    if (threadIdx.x == 0) {
        norm[0] = (float)(total + B);
        norm[1] = (float)(total > 1 ? total : 1);
    }
}

// ---- loss --------------------------------------------------------------------------------------------------------------------
// The sweep of point_maps.h with plain focal elements over the classification maps; its tail, on the first lane of the group that
// swept a pixel row, takes the row of the (B, 4, h, w) map: smooth-L1 between the raw prediction and the log target of a
// positive (fp64 on the few positives), zeros elsewhere.  partial [POINT_BLOCKS][2] = {sum focal, sum smooth-L1}, unscaled.
template <int VEC, bool G2>
__global__ __launch_bounds__(256) void fovea_loss_kernel(PointMaps mp, FoveaLevels lv, int L, int C, const int64_t *__restrict__ gt_labels,
                                                         int K, const int *__restrict__ assigned, const float *__restrict__ bbox_targets,
                                                         const float *__restrict__ norm, float beta, float gamma, float alpha,
                                                         float cls_weight, float box_weight, int group_shift, float *__restrict__ partial)
{
    double s_box = 0.;
    const double bs = (double)box_weight / (double)norm[1], bt = (double)beta;
    const float s_cls = cls_sweep<VEC>(
        mp, lv.poff, L, C, assigned, gt_labels, K, nullptr, cls_weight / norm[0], group_shift,
        [=](float x, bool own, float, float &g) { return focal_elem<G2>(x, own, gamma, alpha, g); },
        [&](const PointRow &r, bool pos, unsigned sub, unsigned) {
            if (sub != 0u) return;
            float gr[4] = {0.f, 0.f, 0.f, 0.f};
            if (pos) {
                const float *d = slot_row(mp, REG, r);
                const float4 t = *reinterpret_cast<const float4 *>(bbox_targets + r.o * 4);
                const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {       // losses/smooth_l1_loss.py:9-32
                    const double e = (double)d[k] - (double)tv[k], a = fabs(e);
                    s_box += a < bt ? 0.5 * a * a / bt : a - 0.5 * bt;
                    gr[k] = (float)((a < bt ? e / bt : (e > 0. ? 1. : -1.)) * bs);
                }
            }
            store_padded(slot_grad_row(mp, REG, r), mp.cs[REG][r.l], gr, 4u);
        });
    block_store_partial2(s_cls, (float)s_box, partial);
}

// ---- FeatureAlign offsets ----------------------------------------------------------------------------------------------------
// offset [M][O] = W [O][4] . exp(x [M][4]): a block takes ALIGN_PIX pixels, stages their four exponentials and the weight in
// LDS and writes its [ALIGN_PIX][O] tile of the output contiguously; the four products are added in ascending channel order.
__global__ __launch_bounds__(256) void fovea_align_fwd_kernel(const float *__restrict__ x, int64_t xs, const float *__restrict__ w,
                                                              int O, int64_t M, float *__restrict__ off, int64_t os)
{
    __shared__ float s_e[ALIGN_PIX][4];
    __shared__ float s_w[ALIGN_MAX_O][4];
    const int64_t m0 = (int64_t)blockIdx.x * ALIGN_PIX;
    const int np = (int)(M - m0 < ALIGN_PIX ? M - m0 : ALIGN_PIX);
    {
        const int p = threadIdx.x >> 2, c = threadIdx.x & 3;
        if (p < np) s_e[p][c] = expf(x[(m0 + p) * xs + c]);
    }
    for (int i = threadIdx.x; i < O * 4; i += 256) s_w[i >> 2][i & 3] = w[i];
    __syncthreads();
    const int os_i = (int)os;
    for (int i = threadIdx.x; i < np * os_i; i += 256) {
        const int p = i / os_i, o = i - p * os_i;
        float v = 0.f;
        if (o < O) v = ((s_w[o][0] * s_e[p][0] + s_w[o][1] * s_e[p][1]) + s_w[o][2] * s_e[p][2]) + s_w[o][3] * s_e[p][3];
        off[m0 * os + i] = v;
    }
}

// g_x [M][4] = exp(x) * sum_o W[o][c] * g_off[m][o] (o ascending), written with zeros on its padding channels, and the block's
// share of g_W [O][4] = sum_m g_off[m][o] * exp(x[m][c]) (m ascending) into part [blocks][O * 4]
__global__ __launch_bounds__(256) void fovea_align_bwd_kernel(const float *__restrict__ x, int64_t xs, const float *__restrict__ w,
                                                              const float *__restrict__ g_off, int64_t gs, int O, int64_t M,
                                                              float *__restrict__ g_x, int64_t gxs, float *__restrict__ part)
{
    __shared__ float s_e[ALIGN_PIX][4];
    __shared__ float s_w[ALIGN_MAX_O][4];
    __shared__ float s_g[ALIGN_PIX][ALIGN_MAX_O + 1];
    const int64_t m0 = (int64_t)blockIdx.x * ALIGN_PIX;
    const int np = (int)(M - m0 < ALIGN_PIX ? M - m0 : ALIGN_PIX);
    const int p = threadIdx.x >> 2, c = threadIdx.x & 3;
    s_e[p][c] = p < np ? expf(x[(m0 + p) * xs + c]) : 0.f;
    for (int i = threadIdx.x; i < O * 4; i += 256) s_w[i >> 2][i & 3] = w[i];
    for (int i = threadIdx.x; i < ALIGN_PIX * O; i += 256) {
        const int q = i / O, o = i - q * O;
        s_g[q][o] = q < np ? g_off[(m0 + q) * gs + o] : 0.f;
    }
    __syncthreads();
    if (p < np) {
        float s = 0.f;
        for (int o = 0; o < O; ++o) s += s_w[o][c] * s_g[p][o];
        g_x[(m0 + p) * gxs + c] = s_e[p][c] * s;
        for (int64_t k = 4 + c; k < gxs; k += 4) g_x[(m0 + p) * gxs + k] = 0.f;
    }
    for (int i = threadIdx.x; i < O * 4; i += 256) {
        const int o = i >> 2, ch = i & 3;
        float s = 0.f;
        for (int q = 0; q < ALIGN_PIX; ++q) s += s_g[q][o] * s_e[q][ch];
        part[(int64_t)blockIdx.x * (O * 4) + i] = s;
    }
}

// g_W [O * 4]: one wavefront per element, lane i adds blocks i, i + 64, ... and the lanes are folded in a fixed order
__global__ __launch_bounds__(64) void fovea_align_finish_kernel(const float *__restrict__ part, int nblk, int n, float *__restrict__ g_w)
{
    float s = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 64) s += part[(int64_t)i * n + blockIdx.x];
    s = htd::wave_sum(s);
    if (threadIdx.x == 0) g_w[blockIdx.x] = s;
}

// the level table of the targets (all of it) and of the loss and the scaling (sizes only: hw null)
int fill_levels(FoveaLevels &lv, const char *what, const int64_t *hw, const int64_t *sizes, const int64_t *strides, const float *bases,
                const float *ranges, int L, int64_t *P_out)
{
    HTD_REQUIRE(L > 0 && L <= FOVEA_MAX_LEVELS, "%s: 1 to %d levels, got %d", what, FOVEA_MAX_LEVELS, L);
    HTD_REQUIRE(hw || sizes, "%s: null level table", what);
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
        int64_t n;
        if (hw) {
            HTD_REQUIRE(strides && bases && ranges, "%s: null level table", what);
            HTD_REQUIRE(hw[2 * l] > 0 && hw[2 * l + 1] > 0 && strides[l] > 0 && strides[l] < (1 << 20) && bases[l] > 0.f,
                        "%s: bad level %d", what, l);
            HTD_REQUIRE((hw[2 * l] + 1) * strides[l] < ((int64_t)1 << 23) && (hw[2 * l + 1] + 1) * strides[l] < ((int64_t)1 << 23),
                        "%s: points of level %d are not exact in fp32", what, l);
            lv.h[l] = (int)hw[2 * l];
            lv.w[l] = (int)hw[2 * l + 1];
            lv.stride[l] = (int)strides[l];
            lv.base[l] = bases[l];
            lv.lo[l] = ranges[2 * l];
            lv.hi[l] = ranges[2 * l + 1];
            n = hw[2 * l] * hw[2 * l + 1];
        } else {
            HTD_REQUIRE(sizes[l] > 0, "%s: bad level %d", what, l);
            n = sizes[l];
        }
        lv.poff[l] = (unsigned)off;
        off += n;
        HTD_REQUIRE(off < ((int64_t)1 << 31), "%s: more than 2^31 points", what);
    }
    for (int l = L; l <= FOVEA_MAX_LEVELS; ++l) lv.poff[l] = (unsigned)off;
    *P_out = off;
    return HTD_OK;
}

int check_align(const char *what, int64_t xs, int B, int H, int W, int deform_groups, int64_t os, int64_t *M)
{
    HTD_REQUIRE(B > 0 && H > 0 && W > 0 && deform_groups >= 1 && deform_groups <= 8, "%s: bad sizes", what);
    *M = (int64_t)B * H * W;
    HTD_REQUIRE(xs >= 4 && xs < (1 << 20) && os >= deform_groups * 18 && os < (1 << 12), "%s: bad channel strides", what);
    HTD_REQUIRE(*M * (xs > os ? xs : os) < ((int64_t)1 << 40) && *M < ((int64_t)1 << 31) * ALIGN_PIX, "%s: maps too large", what);
    return HTD_OK;
}

}  // namespace

extern "C" int64_t htd_fovea_targets_workspace_bytes(int B, int64_t P)
{
    const int64_t n = (int64_t)B * blocks_of(P) * 4;      // one int per block
    return n > 8 ? (n + 7) / 8 * 8 : 8;
}

extern "C" int htd_fovea_targets(const int64_t *hw, const int64_t *strides, const float *base_edges, const float *ranges, int L,
                                 double sigma, const float *gts, const uint8_t *gt_valid, int B, int K, int *assigned,
                                 float *bbox_targets, void *workspace, int *num_pos, float *norm, void *stream)
{
    HTD_REQUIRE(B > 0 && B < 65536 && K >= 0, "fovea_targets: bad sizes");
    HTD_REQUIRE(sigma >= 0. && sigma <= 1., "fovea_targets: sigma must lie in [0, 1]");
    HTD_REQUIRE((K == 0 || (gts && gt_valid)) && assigned && bbox_targets && workspace && num_pos && norm, "fovea_targets: null pointer");
    HTD_REQUIRE((((uintptr_t)gts | (uintptr_t)bbox_targets) & 15) == 0 && ((uintptr_t)workspace & 3) == 0,
                "fovea_targets: gts / bbox_targets must be 16-byte aligned, the workspace 4-byte");
    FoveaLevels lv = {};
    int64_t P = 0;
    const int rc = fill_levels(lv, "fovea_targets", hw, nullptr, strides, base_edges, ranges, L, &P);
    if (rc != HTD_OK) return rc;
    HTD_REQUIRE((int64_t)B * P < ((int64_t)1 << 31), "fovea_targets: more than 2^31 points in the batch");
    const int nblk = (int)blocks_of(P);
    int *part_n = (int *)workspace;
    // 1 -+ sigma is formed in double and rounded to fp32 when it meets the fp32 tensor (fovea_head.py:232-241)
    hipLaunchKernelGGL(fovea_targets_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, lv, L, gts, gt_valid, K,
                       (float)(1. - sigma), (float)(1. + sigma), assigned, bbox_targets, part_n);
    hipLaunchKernelGGL(fovea_targets_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int *)part_n, B, nblk, num_pos,
                       norm);
    return htd::check_launch("fovea_targets");
}

extern "C" int htd_fovea_loss_partial_rows(void) { return POINT_BLOCKS; }

extern "C" int htd_fovea_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                              const int64_t *level_sizes, int L, int B, int C, const int64_t *gt_labels, int K, const int *assigned,
                              const float *bbox_targets, const float *norm, float beta, float gamma, float alpha, float cls_weight,
                              float box_weight, float *partial, float *const *grad_cls, float *const *grad_reg, void *stream)
{
    HTD_REQUIRE(assigned && bbox_targets && norm && partial && (gt_labels || K == 0), "fovea_loss: null pointer");
    HTD_REQUIRE(K >= 0 && C > 0 && gamma >= 0.f && beta > 0.f, "fovea_loss: bad parameters");
    HTD_REQUIRE(((uintptr_t)bbox_targets & 15) == 0, "fovea_loss: bbox_targets must be 16-byte aligned");
    FoveaLevels lv = {};
    int64_t P = 0;
    int rc = fill_levels(lv, "fovea_loss", nullptr, level_sizes, nullptr, nullptr, nullptr, L, &P);
    if (rc != HTD_OK) return rc;
    const SweepForm f = sweep_form(C, cls_stride, L);
    const PointSlot slots[POINT_SLOTS] = {{cls, grad_cls, cls_stride, C, true, true}, {reg, grad_reg, reg_stride, 4, true, true}, {}};
    PointMaps mp = {};
    rc = fill_point_maps(mp, "fovea_loss", lv.poff, L, B, slots, f.vec);
    if (rc != HTD_OK) return rc;
    HTD_POINT_LAUNCH(fovea_loss_kernel, f.vec, gamma == 2.f, stream, mp, lv, L, C, gt_labels, K, assigned, bbox_targets, norm, beta,
                     gamma, alpha, cls_weight, box_weight, f.group_shift, partial);
    return htd::check_launch("fovea_loss");
}

extern "C" int htd_fovea_grad_scale(float *const *grad_cls, const int64_t *cls_stride, float *const *grad_reg,
                                    const int64_t *reg_stride, const int64_t *level_sizes, int L, int B, int C, const float *g_cls,
                                    const float *g_box, void *stream)
{
    FoveaLevels lv = {};
    int64_t P = 0;
    const int rc = fill_levels(lv, "fovea_grad_scale", nullptr, level_sizes, nullptr, nullptr, nullptr, L, &P);
    if (rc != HTD_OK) return rc;
    return point_grad_scale<4, 0>("fovea_grad_scale", lv.poff, L, B, grad_cls, cls_stride, C, grad_reg, reg_stride, nullptr, nullptr,
                                  g_cls, g_box, nullptr, stream);
}

extern "C" int htd_fovea_align_fwd(const float *x, int64_t x_stride, const float *weight, int B, int H, int W, int deform_groups,
                                   float *offset, int64_t offset_stride, void *stream)
{
    HTD_REQUIRE(x && weight && offset, "fovea_align_fwd: null pointer");
    int64_t M = 0;
    const int rc = check_align("fovea_align_fwd", x_stride, B, H, W, deform_groups, offset_stride, &M);
    if (rc != HTD_OK) return rc;
    hipLaunchKernelGGL(fovea_align_fwd_kernel, dim3((unsigned)htd::ceil_div(M, ALIGN_PIX)), dim3(256), 0, (hipStream_t)stream, x,
                       x_stride, weight, deform_groups * 18, M, offset, offset_stride);
    return htd::check_launch("fovea_align_fwd");
}

extern "C" int64_t htd_fovea_align_bwd_workspace_bytes(int B, int H, int W, int deform_groups)
{
    return htd::ceil_div((int64_t)B * H * W, ALIGN_PIX) * deform_groups * 18 * 4 * (int64_t)sizeof(float);
}

extern "C" int htd_fovea_align_bwd(const float *x, int64_t x_stride, const float *weight, const float *g_offset,
                                   int64_t g_offset_stride, int B, int H, int W, int deform_groups, float *g_x, int64_t g_x_stride,
                                   float *g_weight, void *workspace, void *stream)
{
    HTD_REQUIRE(x && weight && g_offset && g_x && g_weight && workspace, "fovea_align_bwd: null pointer");
    HTD_REQUIRE(((uintptr_t)workspace & 3) == 0, "fovea_align_bwd: the workspace must be 4-byte aligned");
    int64_t M = 0;
    int rc = check_align("fovea_align_bwd", x_stride, B, H, W, deform_groups, g_offset_stride, &M);
    if (rc != HTD_OK) return rc;
    HTD_REQUIRE(g_x_stride >= 4 && g_x_stride < (1 << 20), "fovea_align_bwd: bad channel stride of g_x");
    const int O = deform_groups * 18, nblk = (int)htd::ceil_div(M, ALIGN_PIX);
    hipLaunchKernelGGL(fovea_align_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, x_stride, weight, g_offset,
                       g_offset_stride, O, M, g_x, g_x_stride, (float *)workspace);
    hipLaunchKernelGGL(fovea_align_finish_kernel, dim3(O * 4), dim3(64), 0, (hipStream_t)stream, (const float *)workspace, nblk, O * 4,
                       g_weight);
    return htd::check_launch("fovea_align_bwd");
}
