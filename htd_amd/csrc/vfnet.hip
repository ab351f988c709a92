// VFNet head on the device (dense_heads/vfnet_head.py, losses/varifocal_loss.py): the star-shaped deformable-convolution offsets
// built from the predicted box with their backward (forward_single :246-261, star_dcn_offset :275-314), the quality pass that the
// three averaging factors of VFNetHead.loss depend on (:384-430: the IoU of the initial and of the refined box of every positive
// with its gt, the number of positives and the two IoU sums), the three losses (varifocal loss over every (anchor, class), two
// IoU-weighted IoU / GIoU losses) with the three finished gradient maps of all pyramid levels in one launch (:400-463), and the
// re-scaling of those maps by incoming gradients.  The assignment is htd_atss_targets (atss.hip), unchanged.
//
// Built with -ffp-contract=off.  A positive's point (the anchor's centre), its target distances, both decoded boxes and the two
// IoUs are the reference's fp32 values, one rounded operation at a time; the box losses and every derivative of the few
// positives are fp64, as in atss_loss_kernel, and so is the varifocal element of a positive's own class.  The classification
// sweep is fp32 on lane groups per pixel row (focal_elem with alpha' = 1 - alpha is the varifocal negative element).
//
// The three averaging factors are clamped to at least 1 where they are used, as the reference's max(reduce_mean(.), 1.0): a batch
// without positives gives box losses of exactly 0 with zero gradients and a finite varifocal loss over factor 1.
//
// No atomics: every sum has a fixed order and every element of every output is stored exactly once with plain vector stores.
#include "common.h"
#include "anchor_levels.h"
#include "iou_family.h"
#include "point_scale.h"

namespace {

enum { CLS = 0, REG = 1, REF = 2 };       // slots of PointMaps: (B, C, h, w), the initial and the refined (B, 4, h, w)

// ---- star offsets ------------------------------------------------------------------------------------------------------------
// vfnet_head.py:300-311: offset channel c takes sign * q[side] (q = l, t, r, b in map units) or nothing
__device__ __forceinline__ void star_offsets(const float (&q)[4], float (&o)[18])
{
#pragma unroll
    for (int c = 0; c < 18; ++c) o[c] = 0.f;
    const float nx1 = -1.0f * q[0], ny1 = -1.0f * q[1], x2 = q[2], y2 = q[3];
    o[0] = ny1; o[1] = nx1; o[2] = ny1; o[4] = ny1; o[5] = x2; o[7] = nx1;
    o[11] = x2; o[12] = y2; o[13] = nx1; o[14] = y2; o[16] = y2; o[17] = x2;
#pragma unroll
    for (int c = 0; c < 18; ++c) {
        const int k = c >> 1;
        const float base = (c & 1) ? (float)(k % 3 - 1) : (float)(k / 3 - 1);       // dcn_base_offset: (y, x) of the 3 x 3 taps
        o[c] = o[c] - base;
    }
}

// one thread per pixel: pred = exp(x) * denom (the exponential correctly rounded from fp64), offset as star_dcn_offset in its
// fp32 order ((1 - gm) * p + gm * p) / stride; padding channels of both outputs are zeros
__global__ __launch_bounds__(256) void vfnet_star_fwd_kernel(const float *__restrict__ x, int64_t n, unsigned xs, float denom,
                                                             float stride, float gm, float omg, float *__restrict__ pred,
                                                             unsigned ps, float *__restrict__ off, unsigned os)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float *xr = x + i * xs;
        float *pr = pred + i * ps, *orow = off + i * os;
        float p[4], q[4], o[18];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p[k] = (float)exp((double)xr[k]) * denom;
            q[k] = ((omg * p[k]) + (gm * p[k])) / stride;
        }
        star_offsets(q, o);
        for (unsigned k = 0; k < ps; ++k) pr[k] = k < 4u ? p[k] : 0.f;
        for (unsigned c = 0; c < os; ++c) orow[c] = c < 18u ? o[c] : 0.f;
    }
}

// g_x = (g_pred + (gm / stride) * fold(g_off)) * pred; either incoming gradient may be null
__global__ __launch_bounds__(256) void vfnet_star_bwd_kernel(const float *__restrict__ pred, unsigned ps,
                                                             const float *__restrict__ g_pred, unsigned gps,
                                                             const float *__restrict__ g_off, unsigned gos, int64_t n, float stride,
                                                             float gm, float *__restrict__ g_x, unsigned xs)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (g_off) {
            const float *o = g_off + i * gos;
            g[0] = -((o[1] + o[7]) + o[13]);
            g[1] = -((o[0] + o[2]) + o[4]);
            g[2] = (o[5] + o[11]) + o[17];
            g[3] = (o[12] + o[14]) + o[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = (g[k] / stride) * gm;
        }
        if (g_pred) {
            const float *gp = g_pred + i * gps;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = gp[k] + g[k];
        }
        const float *pr = pred + i * ps;
        float *gx = g_x + i * xs;
        for (unsigned k = 0; k < xs; ++k) gx[k] = k < 4u ? g[k] * pr[k] : 0.f;
    }
}

// ---- geometry of a positive --------------------------------------------------------------------------------------------------
// vfnet_head.py:401-406 with transform_bbox_targets :785: the point is the anchor's centre, the target distances are
// bbox2distance(point, gt), and both sides go through distance2bbox again -- all fp32, as the reference's tensors
struct VfGeometry { float px, py; float4 t; };

__device__ __forceinline__ VfGeometry vf_geometry(float4 a, float4 g)
{
    VfGeometry q;
    q.px = (a.z + a.x) / 2.f;
    q.py = (a.w + a.y) / 2.f;
    const float l = q.px - g.x, t = q.py - g.y, r = g.z - q.px, b = g.w - q.py;
    q.t = make_float4(q.px - l, q.py - t, q.px + r, q.py + b);
    return q;
}

__device__ __forceinline__ float vf_iou(const VfGeometry &q, const float *__restrict__ d)
{
    const float iou = iou_ref(make_float4(q.px - d[0], q.py - d[1], q.px + d[2], q.py + d[3]), q.t);
    return fmaxf(iou, 1e-6f);               // .clamp(min=1e-6)
}

// ---- quality -----------------------------------------------------------------------------------------------------------------
// grid (ceil(A / 256), B), one thread per anchor: iou_ini / iou_rf of a positive, 0 elsewhere; the block's {count, sum iou_ini,
// sum iou_rf} (fp64) go to part [B * blocks][3]
__global__ __launch_bounds__(256) void vfnet_quality_kernel(PointMaps mp, AtssLevels lv, int L, const float *__restrict__ anchors,
                                                            const float *__restrict__ gts, int K, const int *__restrict__ assigned,
                                                            float *__restrict__ iou_ini, float *__restrict__ iou_rf,
                                                            double *__restrict__ part)
{
    __shared__ double red[3][4];
    const unsigned A = lv.aoff[L];
    const int b = blockIdx.y;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    double v[3] = {0., 0., 0.};
    if (i < A) {
        const int64_t o = (int64_t)b * A + i;
        const int as = assigned[o];
        float qi = 0.f, qr = 0.f;
        if (as > 0 && as <= K) {
            const unsigned l = level_of(lv.aoff, L, i);
            const int64_t row = (int64_t)b * mp.pix[l] + (i - lv.aoff[l]);
            const VfGeometry q = vf_geometry(load4(anchors, i), load4(gts, (int64_t)b * K + (as - 1)));
            qi = vf_iou(q, mp.map[REG][l] + row * mp.cs[REG][l]);
            qr = vf_iou(q, mp.map[REF][l] + row * mp.cs[REF][l]);
            v[0] = 1.;
        }
        iou_ini[o] = qi;
        iou_rf[o] = qr;
        v[1] = (double)qi;
        v[2] = (double)qr;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3)
        part[((int64_t)b * gridDim.x + blockIdx.x) * 3 + threadIdx.x] =
            (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// sums[k] = the sum of the n block partials of kind k in a fixed order: one wavefront, lane i takes partials i, i + 64, ...
__global__ __launch_bounds__(64) void vfnet_quality_finish_kernel(const double *__restrict__ part, int n, float *__restrict__ sums)
{
    for (int k = 0; k < 3; ++k) {
        double s = 0.;
        for (int i = threadIdx.x; i < n; i += 64) s += part[(int64_t)i * 3 + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (threadIdx.x == 0) sums[k] = (float)s;
    }
}

// ---- loss --------------------------------------------------------------------------------------------------------------------
// varifocal loss of a positive's own class (varifocal_loss.py:40-51) against its IoU target q > 0, fp64: BCE(x, q) times q
// (iou_weighted) or 1; the target and the weight are detached
__device__ __forceinline__ float vfl_positive(float xf, float qf, bool iou_weighted, float &g)
{
    const double x = (double)xf, q = (double)qf;
    double l1p, s;
    sigmoid_log1p(x, l1p, s);
    const double w = iou_weighted ? q : 1.;
    g = (float)((s - q) * w);
    return (float)((fmax(x, 0.) + l1p - x * q) * w);
}

// one positive's box loss on decoded boxes, fp64; out [stride] = scale * d loss / d (l, t, r, b) and zeros on the padding
__device__ __forceinline__ double vf_box_row(const float *__restrict__ d, float *__restrict__ out, unsigned stride,
                                             const VfGeometry &q, int box_kind, double eps, double scale)
{
    const double px = (double)q.px, py = (double)q.py;
    const Box pb = {px - (double)d[0], py - (double)d[1], px + (double)d[2], py + (double)d[3]};
    const Box tb = {(double)q.t.x, (double)q.t.y, (double)q.t.z, (double)q.t.w};
    Box G;
    const double loss = iou_family_loss(box_kind, pb, tb, eps, G);
    out[0] = (float)(-scale * G.x1);
    out[1] = (float)(-scale * G.y1);
    out[2] = (float)(scale * G.x2);
    out[3] = (float)(scale * G.y2);
    for (unsigned j = 4u; j < stride; ++j) out[j] = 0.f;
    return loss;
}

// Classification maps: the sweep of point_maps.h, one anchor per pixel: the varifocal element against iou_rf on a positive's own
// class, focal_elem with alpha' = 1 - alpha (alpha * sigmoid(x)^gamma * softplus(x)) elsewhere; the lane group of a row zero-fills
// both regression gradient rows of a non-positive anchor.  Then one thread per anchor: a positive's two box losses and gradient
// rows.  partial [POINT_BLOCKS][2] = {sum VFL, sum iou_ini * initial box loss}, partial + 2 * POINT_BLOCKS: [POINT_BLOCKS][2] =
// {sum iou_rf * refined box loss, 0}, unscaled.
template <int VEC, bool G2>
__global__ __launch_bounds__(256) void vfnet_loss_kernel(PointMaps mp, AtssLevels lv, int L, int C, const float *__restrict__ anchors,
                                                         const float *__restrict__ gts, const int64_t *__restrict__ gt_labels, int K,
                                                         const int *__restrict__ assigned, const float *__restrict__ iou_ini,
                                                         const float *__restrict__ iou_rf, const float *__restrict__ sums,
                                                         int box_kind, double eps_ini, int ref_kind, double eps_rf, float alpha,
                                                         float gamma, int iou_weighted, float cls_weight, float box_weight,
                                                         float ref_weight, int group_shift, float *__restrict__ partial)
{
    const float n_pos = fmaxf(sums[0], 1.f), n_ini = fmaxf(sums[1], 1.f), n_rf = fmaxf(sums[2], 1.f);
    const float neg_alpha = 1.f - alpha;        // focal_elem weighs a negative by 1 - its alpha
    const unsigned n_rows = mp.rrow[L];
    const float s_cls = cls_sweep<VEC>(
        mp, lv.aoff, L, C, assigned, gt_labels, K, iou_rf, cls_weight / n_pos, group_shift,
        [=](float x, bool own, float qr, float &g) {
            return own ? vfl_positive(x, qr, iou_weighted != 0, g) : focal_elem<G2>(x, false, gamma, neg_alpha, g);
        },
        [&](const PointRow &r, bool pos, unsigned sub, unsigned gl) {
            if (pos) return;
            const unsigned rs = mp.cs[REG][r.l], fs = mp.cs[REF][r.l];
            float *g_reg = slot_grad_row(mp, REG, r), *g_ref = slot_grad_row(mp, REF, r);
            for (unsigned j = sub; j < rs; j += gl) g_reg[j] = 0.f;
            for (unsigned j = sub; j < fs; j += gl) g_ref[j] = 0.f;
        });
    double s_ini = 0., s_rf = 0.;
    for (unsigned rw = blockIdx.x * 256u + threadIdx.x; rw < n_rows; rw += gridDim.x * 256u) {
        const PointRow r = point_row(mp, lv.aoff, L, rw);
        const int as = assigned[r.o];
        if (as > 0 && as <= K) {
            const VfGeometry q = vf_geometry(load4(anchors, r.i), load4(gts, (int64_t)r.b * K + (as - 1)));
            const double wi = (double)iou_ini[r.o], wr = (double)iou_rf[r.o];
            s_ini += wi * vf_box_row(slot_row(mp, REG, r), slot_grad_row(mp, REG, r), mp.cs[REG][r.l], q, box_kind, eps_ini,
                                     wi * (double)box_weight / (double)n_ini);
            s_rf += wr * vf_box_row(slot_row(mp, REF, r), slot_grad_row(mp, REF, r), mp.cs[REF][r.l], q, ref_kind, eps_rf,
                                    wr * (double)ref_weight / (double)n_rf);
        }
    }
    block_store_partial2(s_cls, (float)s_ini, partial);
    __syncthreads();                        // the reduction's LDS is read before the second pair overwrites it
    block_store_partial2((float)s_rf, 0.f, partial + 2 * POINT_BLOCKS);
}

unsigned star_grid(int64_t n)
{
    const int64_t blocks = blocks_of(n);
    return (unsigned)(blocks < POINT_BLOCKS ? blocks : POINT_BLOCKS);
}

bool box_kind_ok(int k) { return k == BOX_IOU || k == BOX_GIOU; }

}  // namespace

extern "C" int htd_vfnet_star_fwd(const float *x, int64_t x_stride, int B, int H, int W, double denom, double stride,
                                  double gradient_mul, float *bbox_pred, int64_t pred_stride, float *dcn_offset,
                                  int64_t offset_stride, void *stream)
{
    HTD_REQUIRE(x && bbox_pred && dcn_offset, "vfnet_star_fwd: null pointer");
    HTD_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < ((int64_t)1 << 31), "vfnet_star_fwd: bad sizes");
    HTD_REQUIRE(x_stride >= 4 && pred_stride >= 4 && offset_stride >= 18 && x_stride < (1 << 20) && pred_stride < (1 << 20) &&
                offset_stride < (1 << 20), "vfnet_star_fwd: bad channel strides");
    HTD_REQUIRE(denom > 0. && stride > 0., "vfnet_star_fwd: denominator and stride must be positive");
    const int64_t n = (int64_t)B * H * W;
    hipLaunchKernelGGL(vfnet_star_fwd_kernel, dim3(star_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n, (unsigned)x_stride,
                       (float)denom, (float)stride, (float)gradient_mul, (float)(1. - gradient_mul), bbox_pred,
                       (unsigned)pred_stride, dcn_offset, (unsigned)offset_stride);
    return htd::check_launch("vfnet_star_fwd");
}

extern "C" int htd_vfnet_star_bwd(const float *bbox_pred, int64_t pred_stride, const float *g_pred, int64_t g_pred_stride,
                                  const float *g_offset, int64_t g_offset_stride, int B, int H, int W, double stride,
                                  double gradient_mul, float *g_x, int64_t x_stride, void *stream)
{
    HTD_REQUIRE(bbox_pred && g_x, "vfnet_star_bwd: null pointer");
    HTD_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < ((int64_t)1 << 31), "vfnet_star_bwd: bad sizes");
    HTD_REQUIRE(pred_stride >= 4 && x_stride >= 4 && pred_stride < (1 << 20) && x_stride < (1 << 20) &&
                (!g_pred || (g_pred_stride >= 4 && g_pred_stride < (1 << 20))) &&
                (!g_offset || (g_offset_stride >= 18 && g_offset_stride < (1 << 20))), "vfnet_star_bwd: bad channel strides");
    HTD_REQUIRE(stride > 0., "vfnet_star_bwd: the stride must be positive");
    const int64_t n = (int64_t)B * H * W;
    hipLaunchKernelGGL(vfnet_star_bwd_kernel, dim3(star_grid(n)), dim3(256), 0, (hipStream_t)stream, bbox_pred,
                       (unsigned)pred_stride, g_pred, (unsigned)(g_pred ? g_pred_stride : 0), g_offset,
                       (unsigned)(g_offset ? g_offset_stride : 0), n, (float)stride, (float)gradient_mul, g_x, (unsigned)x_stride);
    return htd::check_launch("vfnet_star_bwd");
}

extern "C" int64_t htd_vfnet_quality_workspace_bytes(int B, int64_t A) { return (int64_t)B * blocks_of(A) * 3 * 8; }

extern "C" int htd_vfnet_quality(const float *const *reg, const int64_t *reg_stride, const float *const *ref,
                                 const int64_t *ref_stride, const int64_t *level_sizes, int L, int B, const float *anchors,
                                 const float *gts, int K, const int *assigned, float *iou_ini, float *iou_rf, float *sums,
                                 void *workspace, void *stream)
{
    HTD_REQUIRE(anchors && gts && assigned && iou_ini && iou_rf && sums && workspace, "vfnet_quality: null pointer");
    HTD_REQUIRE(K > 0, "vfnet_quality: bad parameters");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                "vfnet_quality: anchors / gts must be 16-byte aligned, the workspace 8-byte");
    AtssLevels lv = {};
    int64_t A = 0;
    int rc = fill_levels(lv, "vfnet_quality", level_sizes, L, &A);
    if (rc != HTD_OK) return rc;
    const PointSlot slots[POINT_SLOTS] = {{}, {reg, nullptr, reg_stride, 4, true, false}, {ref, nullptr, ref_stride, 4, true, false}};
    PointMaps mp = {};
    rc = fill_point_maps(mp, "vfnet_quality", lv.aoff, L, B, slots, 1);
    if (rc != HTD_OK) return rc;
    const int nblk = (int)blocks_of(A);
    hipLaunchKernelGGL(vfnet_quality_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, mp, lv, L, anchors, gts, K, assigned,
                       iou_ini, iou_rf, (double *)workspace);
    hipLaunchKernelGGL(vfnet_quality_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, B * nblk,
                       sums);
    return htd::check_launch("vfnet_quality");
}

extern "C" int htd_vfnet_loss_partial_rows(void) { return 2 * POINT_BLOCKS; }

extern "C" int htd_vfnet_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                              const float *const *ref, const int64_t *ref_stride, const int64_t *level_sizes, int L, int B, int C,
                              const float *anchors, const float *gts, const int64_t *gt_labels, int K, const int *assigned,
                              const float *iou_ini, const float *iou_rf, const float *sums, int box_kind, double eps_ini,
                              int ref_kind, double eps_rf, float alpha, float gamma, int iou_weighted, float cls_weight,
                              float box_weight, float ref_weight, float *partial, float *const *grad_cls, float *const *grad_reg,
                              float *const *grad_ref, void *stream)
{
    HTD_REQUIRE(anchors && gts && gt_labels && assigned && iou_ini && iou_rf && sums && partial, "vfnet_loss: null pointer");
    HTD_REQUIRE(K > 0 && alpha >= 0.f && gamma >= 0.f && box_kind_ok(box_kind) && box_kind_ok(ref_kind), "vfnet_loss: bad parameters");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0, "vfnet_loss: anchors / gts must be 16-byte aligned");
    AtssLevels lv = {};
    int64_t A = 0;
    int rc = fill_levels(lv, "vfnet_loss", level_sizes, L, &A);
    if (rc != HTD_OK) return rc;
    const SweepForm f = sweep_form(C, cls_stride, L);
    const PointSlot slots[POINT_SLOTS] = {{cls, grad_cls, cls_stride, C, true, true}, {reg, grad_reg, reg_stride, 4, true, true},
                                          {ref, grad_ref, ref_stride, 4, true, true}};
    PointMaps mp = {};
    rc = fill_point_maps(mp, "vfnet_loss", lv.aoff, L, B, slots, f.vec);
    if (rc != HTD_OK) return rc;
    HTD_POINT_LAUNCH(vfnet_loss_kernel, f.vec, gamma == 2.f, stream, mp, lv, L, C, anchors, gts, gt_labels, K, assigned, iou_ini, iou_rf,
                     sums, box_kind, eps_ini, ref_kind, eps_rf, alpha, gamma, iou_weighted, cls_weight, box_weight, ref_weight,
                     f.group_shift, partial);
    return htd::check_launch("vfnet_loss");
}

extern "C" int htd_vfnet_grad_scale(float *const *grad_cls, const int64_t *cls_stride, float *const *grad_reg,
                                    const int64_t *reg_stride, float *const *grad_ref, const int64_t *ref_stride,
                                    const int64_t *level_sizes, int L, int B, int C, const float *g_cls, const float *g_box,
                                    const float *g_ref, void *stream)
{
    AtssLevels lv = {};
    int64_t A = 0;
    const int rc = fill_levels(lv, "vfnet_grad_scale", level_sizes, L, &A);
    if (rc != HTD_OK) return rc;
    return point_grad_scale<4, 4>("vfnet_grad_scale", lv.aoff, L, B, grad_cls, cls_stride, C, grad_reg, reg_stride, grad_ref,
                                  ref_stride, g_cls, g_box, g_ref, stream);
}
