// GFL head on the device (dense_heads/gfl_head.py, losses/gfocal_loss.py): the quality pass that the averaging factor of
// GFLHead.loss depends on (loss_single :254-265: the weight max_c sigmoid(cls) and the IoU score of every positive, and their
// sum :364-365), the three losses (QFL, weighted IoU / GIoU on the integral-decoded box, DFL) with both finished gradient maps of
// all pyramid levels in one launch (:209-369), the re-scaling of those maps by incoming gradients, and the ranking keys and
// distances of _get_bboxes_single (:420-428).  The assignment is htd_atss_targets (atss.hip), unchanged.
//
// Built with -ffp-contract=off.  A positive's centre and target box are the reference's fp32 values (anchor centre / stride,
// gt / stride), its DFL target and the two bin weights are fp32 too (bbox2distance, label.long(), dis_right.float() - label);
// the softmax, the integral, the box loss and every derivative of the few positives are fp64, as in atss_loss_kernel.  The
// classification sweep is fp32 on lane groups per pixel row (focal_elem with alpha = 0 is QFL's negative element).
//
// Two pieces of reference behaviour are kept: the averaging factor wsum is not clamped, so a batch without positives gives
// 0 / 0 = NaN box and DFL losses and a NaN regression gradient (`bbox_pred.sum() * 0` over avg_factor 0) beside a finite
// classification loss; and the DFL targets are clamped to [0, reg_max - 0.1] before they are split into bins.
//
// No atomics: every sum has a fixed order and every element of every output is stored exactly once with plain vector stores.
#include "common.h"
#include "anchor_levels.h"
#include "iou_family.h"

namespace {

constexpr int GFL_MAX_REG_MAX = 31;         // at most 32 bins per side

enum { CLS = 0, REG = 1 };                // slots of PointMaps: (B, C, h, w), (B, 4 * bins, h, w); the third is not used

struct GflStrides { float v[ATSS_MAX_LEVELS]; };        // the pyramid's strides, as the reference's fp32 tensors hold them

// softmax-integral sum_j j * softmax(x)_j of one side's `nb` logits, fp64; mx / den: the maximum and the sum of exp(x - mx)
__device__ __forceinline__ double integral_of(const float *__restrict__ x, int nb, double &mx, double &den)
{
    mx = (double)x[0];
    for (int j = 1; j < nb; ++j) mx = fmax(mx, (double)x[j]);
    den = 0.;
    double num = 0.;
    for (int j = 0; j < nb; ++j) {
        const double e = exp((double)x[j] - mx);
        den += e;
        num += (double)j * e;
    }
    return num / den;
}

// gfl_head.py:254,261: the anchor's centre and the gt in stride units, as the reference's fp32 tensors hold them
struct GflGeometry { float cx, cy; float4 t; };

__device__ __forceinline__ GflGeometry geometry_of(float4 a, float4 g, float stride)
{
    GflGeometry q;
    q.cx = ((a.z + a.x) / 2.f) / stride;
    q.cy = ((a.w + a.y) / 2.f) / stride;
    q.t = make_float4(g.x / stride, g.y / stride, g.z / stride, g.w / stride);
    return q;
}

// One positive: box loss of distance2bbox(centre, integral(x)) against gt / stride and the DFL of the four sides (targets by
// bbox2distance(centre, gt / stride, reg_max), clamped to [0, reg_max - 0.1]); out [rs] receives bscale * d box + dscale * d dfl
// for all 4 * nb logits -- the box gradient through the integral (d dist / d x_j = p_j (j - dist)) and the softmax, the DFL's
// cross-entropy gradient (wl + wr) p - wl [j = left] - wr [j = right] added -- and zeros on the padding channels.
__device__ __forceinline__ void positive_row(const float *__restrict__ x, float *__restrict__ out, unsigned rs, int nb, float4 a,
                                             float4 g, float stride, int box_kind, double eps, double bscale, double dscale,
                                             double &l_box, double &l_dfl)
{
    const int R = nb - 1;
    const GflGeometry q = geometry_of(a, g, stride);
    double d[4], mx[4], den[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = integral_of(x + k * nb, nb, mx[k], den[k]);
    const Box pb = {(double)q.cx - d[0], (double)q.cy - d[1], (double)q.cx + d[2], (double)q.cy + d[3]};
    const Box tb = {(double)q.t.x, (double)q.t.y, (double)q.t.z, (double)q.t.w};
    Box G;
    l_box = iou_family_loss(box_kind, pb, tb, eps, G);
    const double dd[4] = {-G.x1, -G.y1, G.x2, G.y2};
    const float tmax = (float)((double)R - 0.1);
    const float td[4] = {q.cx - q.t.x, q.cy - q.t.y, q.t.z - q.cx, q.t.w - q.cy};
    l_dfl = 0.;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float tk = fminf(fmaxf(td[k], 0.f), tmax);
        int il = (int)tk;
        il = il < 0 ? 0 : (il > R - 1 ? R - 1 : il);          // (tk is inside [0, R - 0.1]; a NaN gt must not index)
        const float wl = (float)(il + 1) - tk, wr = tk - (float)il;
        const float *xk = x + k * nb;
        const double lse = mx[k] + log(den[k]);
        l_dfl += (lse - (double)xk[il]) * (double)wl + (lse - (double)xk[il + 1]) * (double)wr;
        const double wsum2 = (double)wl + (double)wr;
        for (int j = 0; j < nb; ++j) {
            const double p = exp((double)xk[j] - mx[k]) / den[k];
            const double ce = wsum2 * p - (j == il ? (double)wl : 0.) - (j == il + 1 ? (double)wr : 0.);
            out[k * nb + j] = (float)(bscale * dd[k] * p * ((double)j - d[k]) + dscale * ce);
        }
    }
    for (unsigned j = 4u * (unsigned)nb; j < rs; ++j) out[j] = 0.f;
}

// ---- quality -----------------------------------------------------------------------------------------------------------------
// grid (ceil(A / 256), B), one thread per anchor: weight = max_c sigmoid(cls) (the fp32 rounding of the fp64 sigmoid of the
// largest logit) and score = aligned fp32 IoU (eps 1e-6) of the integral-decoded box with gt / stride on positives, 0 elsewhere;
// the block's weight sum (fp64) goes to part
__global__ __launch_bounds__(256) void gfl_quality_kernel(PointMaps mp, AtssLevels lv, GflStrides st, int L, int C, int nb,
                                                          const float *__restrict__ anchors, const float *__restrict__ gts, int K,
                                                          const int *__restrict__ assigned, float *__restrict__ weight,
                                                          float *__restrict__ score, double *__restrict__ part)
{
    __shared__ double red[4];
    const unsigned A = lv.aoff[L];
    const int b = blockIdx.y;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    double wv = 0.;
    if (i < A) {
        const int64_t o = (int64_t)b * A + i;
        const int as = assigned[o];
        float w = 0.f, s = 0.f;
        if (as > 0 && as <= K) {
            const unsigned l = level_of(lv.aoff, L, i);
            const int64_t row = (int64_t)b * mp.pix[l] + (i - lv.aoff[l]);
            const float *x = mp.map[CLS][l] + row * mp.cs[CLS][l];
            float m = x[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
            w = (float)(1. / (1. + exp(-(double)m)));
            const float *r = mp.map[REG][l] + row * mp.cs[REG][l];
            float d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double mx, den;
                d[k] = (float)integral_of(r + k * nb, nb, mx, den);
            }
            const GflGeometry q = geometry_of(load4(anchors, i), load4(gts, (int64_t)b * K + (as - 1)), st.v[l]);
            s = iou_ref(make_float4(q.cx - d[0], q.cy - d[1], q.cx + d[2], q.cy + d[3]), q.t);
        }
        weight[o] = w;
        score[o] = s;
        wv = (double)w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wv += __shfl_xor(wv, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wv;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// wsum[0] = the sum of the n block partials in a fixed order: one wavefront, lane i takes partials i, i + 64, ...
__global__ __launch_bounds__(64) void gfl_quality_finish_kernel(const double *__restrict__ part, int n, float *__restrict__ wsum)
{
    double s = 0.;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) wsum[0] = (float)s;
}

// ---- loss --------------------------------------------------------------------------------------------------------------------
// QFL of a positive's own class (gfocal_loss.py:42-46) against its score y, fp64: BCE(x, y) * |y - sigmoid(x)|^beta with the
// derivative through both factors
__device__ __forceinline__ float qfl_positive(float xf, float yf, float beta, float &g)
{
    const double x = (double)xf, y = (double)yf;
    double l1p, s;
    sigmoid_log1p(x, l1p, s);
    const double bce = fmax(x, 0.) + l1p - x * y;
    const double d = y - s, ad = fabs(d);
    const double m = beta == 2.f ? d * d : pow(ad, (double)beta);
    const double dm = ad > 0. ? (double)beta * m / ad * (d > 0. ? 1. : -1.) : 0.;       // d m / d d; d d / d x = -s (1 - s)
    g = (float)(-d * m - bce * dm * s * (1. - s));
    return (float)(bce * m);
}

// Classification maps: the sweep of point_maps.h, one anchor per pixel, label weight 1: QFL against the score on a positive's own
// class, focal_elem with alpha = 0 (softplus(x) * sigmoid(x)^beta) elsewhere; the lane group of a row zero-fills the regression
// gradient row of a non-positive anchor (0 * (1 / wsum): NaN when the batch has no positive, as the reference's
// bbox_pred.sum() * 0 over avg_factor 0).  Then one thread per anchor: a positive's box and DFL terms and its gradient row.
// partial [POINT_BLOCKS][2] = {sum QFL, sum weight * box loss}, partial + 2 * POINT_BLOCKS: [POINT_BLOCKS][2] = {sum weight * DFL
// of the four sides, 0}, unscaled.
template <int VEC, bool B2>
__global__ __launch_bounds__(256) void gfl_loss_kernel(PointMaps mp, AtssLevels lv, GflStrides st, int L, int C, int nb,
                                                       const float *__restrict__ anchors, const float *__restrict__ gts,
                                                       const int64_t *__restrict__ gt_labels, int K,
                                                       const int *__restrict__ assigned, const float *__restrict__ weight,
                                                       const float *__restrict__ score, const float *__restrict__ norm,
                                                       const float *__restrict__ wsum, int box_kind, double eps, float beta,
                                                       float cls_weight, float box_weight, float dfl_weight, int group_shift,
                                                       float *__restrict__ partial)
{
    const float ws = wsum[0];
    const float zfill = 0.f * (1.f / ws);
    const unsigned n_rows = mp.rrow[L];
    const unsigned nreg = 4u * (unsigned)nb;
    const float s_cls = cls_sweep<VEC>(
        mp, lv.aoff, L, C, assigned, gt_labels, K, score, cls_weight / norm[0], group_shift,
        [=](float x, bool own, float sc, float &g) { return own ? qfl_positive(x, sc, beta, g) : focal_elem<B2>(x, false, beta, 0.f, g); },
        [&](const PointRow &r, bool pos, unsigned sub, unsigned gl) {
            if (pos) return;
            const unsigned rs = mp.cs[REG][r.l];
            float *g_reg = slot_grad_row(mp, REG, r);
            for (unsigned j = sub; j < rs; j += gl) g_reg[j] = j < nreg ? zfill : 0.f;
        });
    double s_box = 0., s_dfl = 0.;
    for (unsigned rw = blockIdx.x * 256u + threadIdx.x; rw < n_rows; rw += gridDim.x * 256u) {
        const PointRow r = point_row(mp, lv.aoff, L, rw);
        const int as = assigned[r.o];
        if (as > 0 && as <= K) {
            const double w = (double)weight[r.o];
            double l_box, l_dfl;
            positive_row(slot_row(mp, REG, r), slot_grad_row(mp, REG, r), mp.cs[REG][r.l], nb, load4(anchors, r.i),
                         load4(gts, (int64_t)r.b * K + (as - 1)), st.v[r.l], box_kind, eps, w * (double)box_weight / (double)ws,
                         w * (double)dfl_weight / (4. * (double)ws), l_box, l_dfl);
            s_box += w * l_box;
            s_dfl += w * l_dfl;
        }
    }
    block_store_partial2(s_cls, (float)s_box, partial);
    __syncthreads();                        // the reduction's LDS is read before the second pair overwrites it
    block_store_partial2((float)s_dfl, 0.f, partial + 2 * POINT_BLOCKS);
}

// The gradient maps of gfl_loss_kernel under incoming gradients (device scalars): the classification map *= g_cls; a positive's
// regression row, where the box and the DFL gradient are summed, is written again from the logits with the two scales times
// g_box / g_dfl (the other rows are 0, or NaN, under any factor).  A factor of exactly 1 leaves its maps alone, decided here.
__global__ __launch_bounds__(256) void gfl_scale_kernel(PointMaps mp, AtssLevels lv, GflStrides st, int L, int cls_width, int nb,
                                                        const float *__restrict__ anchors, const float *__restrict__ gts, int K,
                                                        const int *__restrict__ assigned, const float *__restrict__ weight,
                                                        const float *__restrict__ wsum, int box_kind, double eps, float box_weight,
                                                        float dfl_weight, const float *__restrict__ g_cls,
                                                        const float *__restrict__ g_box, const float *__restrict__ g_dfl)
{
    const float gc = *g_cls, gb = *g_box, gd = *g_dfl;
    const unsigned n_rows = mp.rrow[L];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (gc != 1.f) {
        for (unsigned rw = wave; rw < n_rows; rw += gridDim.x * 4u) {
            const int l = level_of(mp.rrow, L, rw);
            float *g_row = mp.grad[CLS][l] + (int64_t)(rw - mp.rrow[l]) * mp.cs[CLS][l];
            for (unsigned j = lane; j < (unsigned)cls_width; j += 64u) g_row[j] *= gc;
        }
    }
    if (gb != 1.f || gd != 1.f) {
        const double ws = (double)wsum[0];
        for (unsigned rw = blockIdx.x * 256u + threadIdx.x; rw < n_rows; rw += gridDim.x * 256u) {
            const PointRow r = point_row(mp, lv.aoff, L, rw);
            const int as = assigned[r.o];
            if (as > 0 && as <= K) {
                const double w = (double)weight[r.o];
                double l_box, l_dfl;
                positive_row(slot_row(mp, REG, r), slot_grad_row(mp, REG, r), mp.cs[REG][r.l], nb, load4(anchors, r.i),
                             load4(gts, (int64_t)r.b * K + (as - 1)), st.v[r.l], box_kind, eps,
                             w * (double)box_weight / ws * (double)gb, w * (double)dfl_weight / (4. * ws) * (double)gd, l_box, l_dfl);
            }
        }
    }
}

// ---- inference ---------------------------------------------------------------------------------------------------------------
// keys [B][A] = max_c sigmoid(cls) = sigmoid(max_c cls) and dist [B][A][4] = integral(reg) * stride, fp32 as the reference's
// tensors: 16 lanes per anchor, 4 per side
__global__ __launch_bounds__(256) void gfl_decode_kernel(PointMaps mp, AtssLevels lv, GflStrides st_, int L, int B, int C, int nb,
                                                         float *__restrict__ keys, float *__restrict__ dist)
{
    const int sub = threadIdx.x & 15, k = sub >> 2, q = sub & 3;
    const unsigned A = lv.aoff[L];
    const int64_t rows = (int64_t)B * A;
    const int64_t step = (int64_t)gridDim.x * 16;
    for (int64_t i0 = (int64_t)blockIdx.x * 16; i0 < rows; i0 += step) {      // every lane of a 16-lane group stays in the loop
        const int64_t i = i0 + (threadIdx.x >> 4);
        const bool live = i < rows;
        float m = -INFINITY, mx = -INFINITY, st = 1.f;
        const float *xs = nullptr;
        if (live) {
            const unsigned b = (unsigned)(i / A), ai = (unsigned)(i - (int64_t)b * A);
            const int l = level_of(lv.aoff, L, ai);
            const int64_t row = (int64_t)b * mp.pix[l] + (ai - lv.aoff[l]);
            const float *x = mp.map[CLS][l] + row * mp.cs[CLS][l];
            if ((C & 3) == 0 && (mp.cs[CLS][l] & 3) == 0 && ((uintptr_t)mp.map[CLS][l] & 15) == 0) {
                for (int c = sub * 4; c < C; c += 64) {
                    const float4 v = *reinterpret_cast<const float4 *>(x + c);
                    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
                }
            } else {
                for (int c = sub; c < C; c += 16) m = fmaxf(m, x[c]);
            }
            xs = mp.map[REG][l] + row * mp.cs[REG][l] + k * nb;
            for (int j = q; j < nb; j += 4) mx = fmaxf(mx, xs[j]);
            st = st_.v[l];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        float den = 0.f, num = 0.f;
        if (live) {
            for (int j = q; j < nb; j += 4) {
                const float e = expf(xs[j] - mx);
                den += e;
                num += (float)j * e;
            }
        }
        den += __shfl_xor(den, 1, 64); num += __shfl_xor(num, 1, 64);
        den += __shfl_xor(den, 2, 64); num += __shfl_xor(num, 2, 64);
        if (live && q == 0) dist[i * 4 + k] = (num / den) * st;
        if (live && sub == 0) keys[i] = 1.f / (1.f + expf(-m));
    }
}

// The prologue of every entry point: the level table, the map table of the two slots (reg_slot.channels is filled in here) and
// the pyramid's strides.  vec: units of the classification map.
struct GflTables { AtssLevels lv; PointMaps mp; GflStrides st; int64_t A; };

int gfl_tables(GflTables &t, const char *what, const PointSlot &cls_slot, PointSlot reg_slot, const int64_t *level_sizes,
               const int64_t *strides, int L, int B, int reg_max, int vec)
{
    HTD_REQUIRE(reg_max >= 1 && reg_max <= GFL_MAX_REG_MAX, "%s: reg_max must be 1 to %d, got %d", what, GFL_MAX_REG_MAX, reg_max);
    int rc = fill_levels(t.lv, what, level_sizes, L, &t.A);
    if (rc != HTD_OK) return rc;
    reg_slot.channels = 4 * (reg_max + 1);
    const PointSlot slots[POINT_SLOTS] = {cls_slot, reg_slot, {}};
    rc = fill_point_maps(t.mp, what, t.lv.aoff, L, B, slots, vec);
    if (rc != HTD_OK) return rc;
    HTD_REQUIRE(strides, "%s: null table", what);
    for (int l = 0; l < L; ++l) {
        HTD_REQUIRE(strides[l] > 0 && strides[l] < (1 << 20), "%s: bad stride of level %d", what, l);
        t.st.v[l] = (float)strides[l];
    }
    return HTD_OK;
}

}  // namespace

extern "C" int64_t htd_gfl_quality_workspace_bytes(int B, int64_t A) { return (int64_t)B * blocks_of(A) * 8; }

extern "C" int htd_gfl_quality(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                               const int64_t *level_sizes, const int64_t *strides, int L, int B, int C, int reg_max,
                               const float *anchors, const float *gts, int K, const int *assigned, float *weight, float *score,
                               float *wsum, void *workspace, void *stream)
{
    HTD_REQUIRE(anchors && gts && assigned && weight && score && wsum && workspace, "gfl_quality: null pointer");
    HTD_REQUIRE(K > 0, "gfl_quality: bad parameters");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                "gfl_quality: anchors / gts must be 16-byte aligned, the workspace 8-byte");
    GflTables t = {};
    const int rc = gfl_tables(t, "gfl_quality", {cls, nullptr, cls_stride, C, true, false}, {reg, nullptr, reg_stride, 0, true, false},
                              level_sizes, strides, L, B, reg_max, 1);
    if (rc != HTD_OK) return rc;
    const int nblk = (int)blocks_of(t.A);
    hipLaunchKernelGGL(gfl_quality_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, t.mp, t.lv, t.st, L, C, reg_max + 1,
                       anchors, gts, K, assigned, weight, score, (double *)workspace);
    hipLaunchKernelGGL(gfl_quality_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, B * nblk,
                       wsum);
    return htd::check_launch("gfl_quality");
}

extern "C" int htd_gfl_loss_partial_rows(void) { return 2 * POINT_BLOCKS; }

extern "C" int htd_gfl_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                            const int64_t *level_sizes, const int64_t *strides, int L, int B, int C, int reg_max,
                            const float *anchors, const float *gts, const int64_t *gt_labels, int K, const int *assigned,
                            const float *weight, const float *score, const float *norm, const float *wsum, int box_kind, double eps,
                            float beta, float cls_weight, float box_weight, float dfl_weight, float *partial,
                            float *const *grad_cls, float *const *grad_reg, void *stream)
{
    HTD_REQUIRE(anchors && gts && gt_labels && assigned && weight && score && norm && wsum && partial, "gfl_loss: null pointer");
    HTD_REQUIRE(K > 0 && beta >= 0.f && (box_kind == BOX_IOU || box_kind == BOX_GIOU), "gfl_loss: bad parameters");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0, "gfl_loss: anchors / gts must be 16-byte aligned");
    const SweepForm f = sweep_form(C, cls_stride, L);
    GflTables t = {};
    const int rc = gfl_tables(t, "gfl_loss", {cls, grad_cls, cls_stride, C, true, true}, {reg, grad_reg, reg_stride, 0, true, true},
                              level_sizes, strides, L, B, reg_max, f.vec);
    if (rc != HTD_OK) return rc;
    HTD_POINT_LAUNCH(gfl_loss_kernel, f.vec, beta == 2.f, stream, t.mp, t.lv, t.st, L, C, reg_max + 1, anchors, gts, gt_labels, K,
                     assigned, weight, score, norm, wsum, box_kind, eps, beta, cls_weight, box_weight, dfl_weight, f.group_shift,
                     partial);
    return htd::check_launch("gfl_loss");
}

extern "C" int htd_gfl_grad_scale(float *const *grad_cls, const int64_t *cls_stride, const float *const *reg, float *const *grad_reg,
                                  const int64_t *reg_stride, const int64_t *level_sizes, const int64_t *strides, int L, int B, int C,
                                  int reg_max, const float *anchors, const float *gts, int K, const int *assigned,
                                  const float *weight, const float *wsum, int box_kind, double eps, float box_weight,
                                  float dfl_weight, const float *g_cls, const float *g_box, const float *g_dfl, void *stream)
{
    HTD_REQUIRE(anchors && gts && assigned && weight && wsum && g_cls && g_box && g_dfl, "gfl_grad_scale: null pointer");
    HTD_REQUIRE(K > 0 && (box_kind == BOX_IOU || box_kind == BOX_GIOU), "gfl_grad_scale: bad parameters");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0, "gfl_grad_scale: anchors / gts must be 16-byte aligned");
    GflTables t = {};
    const int rc = gfl_tables(t, "gfl_grad_scale", {nullptr, grad_cls, cls_stride, C, false, true},
                              {reg, grad_reg, reg_stride, 0, true, true}, level_sizes, strides, L, B, reg_max, 1);
    if (rc != HTD_OK) return rc;
    hipLaunchKernelGGL(gfl_scale_kernel, dim3(POINT_BLOCKS), dim3(256), 0, (hipStream_t)stream, t.mp, t.lv, t.st, L, C, reg_max + 1,
                       anchors, gts, K, assigned, weight, wsum, box_kind, eps, box_weight, dfl_weight, g_cls, g_box, g_dfl);
    return htd::check_launch("gfl_grad_scale");
}

extern "C" int htd_gfl_decode(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                              const int64_t *level_sizes, const int64_t *strides, int L, int B, int C, int reg_max, float *keys,
                              float *dist, void *stream)
{
    HTD_REQUIRE(keys && dist, "gfl_decode: null pointer");
    GflTables t = {};
    const int rc = gfl_tables(t, "gfl_decode", {cls, nullptr, cls_stride, C, true, false}, {reg, nullptr, reg_stride, 0, true, false},
                              level_sizes, strides, L, B, reg_max, 1);
    if (rc != HTD_OK) return rc;
    const int64_t groups = ((int64_t)B * t.A + 15) / 16;
    hipLaunchKernelGGL(gfl_decode_kernel, dim3((unsigned)(groups < POINT_BLOCKS ? groups : POINT_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, t.mp, t.lv, t.st, L, B, C, reg_max + 1, keys, dist);
    return htd::check_launch("gfl_decode");
}
