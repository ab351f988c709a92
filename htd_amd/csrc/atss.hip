// ATSS head on the device (core/bbox/assigners/atss_assigner.py, dense_heads/atss_head.py): the adaptive assignment of a whole
// batch with its centerness targets and averaging factors (ATSSAssigner.assign :33-178, ATSSHead.centerness_target :297-313,
// the num_total_samples / bbox_avg_factor of ATSSHead.loss :271-290) and the three losses with their three finished gradient
// maps of all pyramid levels in one launch (loss / loss_single :145-295).  Built with -ffp-contract=off: distances and IoUs
// are the reference's fp32 values one rounded operation at a time (dx * dx + dy * dy is two products and a sum), divisions and
// square roots are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), and the logarithm and exponential of the delta
// coding are the fp32 roundings of the fp64 functions.  The box loss is the fp64 iou_family_loss of the RoI heads, the
// classification loss the sweep of point_maps.h with the focal_elem of the anchor heads: one implementation each.
//
// The ranking keys of get_bboxes are htd_fcos_keys and the scaling of the gradient maps by incoming gradients is
// htd_fcos_grad_scale (fcos.hip): the map table is the same.
//
// No float atomics: the one atomic is a 64-bit integer maximum, which does not depend on the order it is taken in; every sum
// has a fixed order; every element of every output is stored exactly once with plain vector stores.
#include "common.h"
#include "anchor_levels.h"
#include "iou_family.h"

namespace {

constexpr int ATSS_MAX_TOPK = 16;
constexpr double ATSS_EPS = 1e-12;          // atss_head.py:12

struct AtssCoder {                          // DeltaXYWHBBoxCoder: means, stds, |log(wh_ratio_clip)|
    float mean[4], std[4], max_ratio;          // as the reference's fp32 tensors hold them
    double mean_d[4], std_d[4], max_ratio_d;    // as its fp64 run does
};

enum { CLS = 0, REG = 1, CTR = 2 };       // slots of PointMaps: (B, C, h, w), (B, 4, h, w), (B, 1, h, w)

__device__ __forceinline__ float log_rounded(float x) { return (float)log((double)x); }
__device__ __forceinline__ float exp_rounded(float x) { return (float)exp((double)x); }

// delta2bbox(anchor, bbox2delta(anchor, gt)) (delta_xywh_bbox_coder.py:98-118, 171-197) in the reference's fp32 order: the box
// ATSSHead.loss_single regresses to and centerness_target measures
__device__ __forceinline__ float4 target_box_ref(float4 a, float4 g, const AtssCoder &cd)
{
    const float px = (a.x + a.z) * 0.5f, py = (a.y + a.w) * 0.5f, pw = a.z - a.x, ph = a.w - a.y;
    const float gx = (g.x + g.z) * 0.5f, gy = (g.y + g.w) * 0.5f, gw = g.z - g.x, gh = g.w - g.y;
    float d[4] = {(gx - px) / pw, (gy - py) / ph, log_rounded(gw / pw), log_rounded(gh / ph)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d[i] = (d[i] - cd.mean[i]) / cd.std[i];
        d[i] = d[i] * cd.std[i] + cd.mean[i];
    }
    const float dw = fminf(fmaxf(d[2], -cd.max_ratio), cd.max_ratio), dh = fminf(fmaxf(d[3], -cd.max_ratio), cd.max_ratio);
    const float w2 = pw * exp_rounded(dw), h2 = ph * exp_rounded(dh);
    const float x2 = px + pw * d[0], y2 = py + ph * d[1];
    return make_float4(x2 - w2 * 0.5f, y2 - h2 * 0.5f, x2 + w2 * 0.5f, y2 + h2 * 0.5f);
}

// ATSSHead.centerness_target (atss_head.py:297-313) of that box
__device__ __forceinline__ float centerness_ref(float4 a, float4 box)
{
    const float cx = (a.z + a.x) / 2.f, cy = (a.w + a.y) / 2.f;
    const float l_ = cx - box.x, t_ = cy - box.y, r_ = box.z - cx, b_ = box.w - cy;
    return sqrtf((fminf(l_, r_) / fmaxf(l_, r_)) * (fminf(t_, b_) / fmaxf(t_, b_)));
}

// ---- assignment, first launch --------------------------------------------------------------------------------------------
// grid (K, B), 64 * L threads: a workgroup per (image, gt), a wavefront per level.  A lane scans its stride of the level and
// keeps its 16 smallest keys (fp32 distance bits << 32 | index in the level: distances are >= 0, so the bits order like the
// values and the index breaks ties) sorted in registers; min(topk, n_level) rounds of a wave-wide minimum then take the
// candidates in the order of the whole level.  The candidate IoUs meet in LDS; every thread forms the threshold from them in
// the same fixed order (two fp32 passes, n - 1 in the variance: one candidate gives 0 / 0 = NaN and no positive).  A surviving
// candidate is published with a 64-bit maximum of (IoU bits << 32 | K - k) on best [B][A], zeroed before the launch: IoU >= 0
// keeps its bits ordered, the larger K - k is the lower gt index, and the word is never 0.
__global__ __launch_bounds__(64 * ATSS_MAX_LEVELS) void atss_select_kernel(AtssLevels lv, int L, const float *__restrict__ anchors,
                                                                             const float *__restrict__ gts,
                                                                             const uint8_t *__restrict__ gt_valid, int K, int topk,
                                                                             unsigned long long *__restrict__ best)
{
    __shared__ float s_iou[ATSS_MAX_LEVELS * ATSS_MAX_TOPK];
    const int k = blockIdx.x, b = blockIdx.y;
    if (!gt_valid[(int64_t)b * K + k]) return;          // the whole workgroup
    const int l = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float4 g = load4(gts, (int64_t)b * K + k);
    const float gcx = (g.x + g.z) / 2.f, gcy = (g.y + g.w) / 2.f;
    const unsigned a0 = lv.aoff[l], n = lv.aoff[l + 1] - a0;
    const int kl = (unsigned)topk < n ? topk : (int)n;
    const unsigned long long NONE = ~0ull;
    unsigned long long mine[ATSS_MAX_TOPK];
#pragma unroll
    for (int i = 0; i < ATSS_MAX_TOPK; ++i) mine[i] = NONE;
    for (unsigned j = lane; j < n; j += 64u) {
        const float4 a = load4(anchors, (int64_t)a0 + j);
        const float dx = (a.x + a.z) / 2.f - gcx, dy = (a.y + a.w) / 2.f - gcy;
        const float d = sqrtf(dx * dx + dy * dy);
        unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | j;
#pragma unroll
        for (int i = 0; i < ATSS_MAX_TOPK; ++i) {
            if (key < mine[i]) { const unsigned long long t = mine[i]; mine[i] = key; key = t; }
        }
    }
    unsigned long long chosen = NONE;
    for (int r = 0; r < kl; ++r) {                      // kl is the wavefront's: every lane takes every round
        unsigned long long m = mine[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, 64);
            m = other < m ? other : m;
        }
        if (mine[0] == m) {                             // keys are distinct: one lane
#pragma unroll
            for (int i = 0; i + 1 < ATSS_MAX_TOPK; ++i) mine[i] = mine[i + 1];
            mine[ATSS_MAX_TOPK - 1] = NONE;
        }
        if (lane == r) chosen = m;
    }
    const bool cand = lane < kl;
    float iou = 0.f;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned idx = 0;
    if (cand) {
        idx = a0 + (unsigned)(chosen & 0xffffffffull);
        a = load4(anchors, idx);
        iou = iou_ref(a, g);
        s_iou[l * ATSS_MAX_TOPK + lane] = iou;
    }
    __syncthreads();
    float sum = 0.f;
    int cnt = 0;
    for (int l2 = 0; l2 < L; ++l2) {
        const unsigned n2 = lv.aoff[l2 + 1] - lv.aoff[l2];
        const int k2 = (unsigned)topk < n2 ? topk : (int)n2;
        for (int r = 0; r < k2; ++r) sum += s_iou[l2 * ATSS_MAX_TOPK + r];
        cnt += k2;
    }
    const float mean = sum / (float)cnt;
    float s2 = 0.f;
    for (int l2 = 0; l2 < L; ++l2) {
        const unsigned n2 = lv.aoff[l2 + 1] - lv.aoff[l2];
        const int k2 = (unsigned)topk < n2 ? topk : (int)n2;
        for (int r = 0; r < k2; ++r) {
            const float d = s_iou[l2 * ATSS_MAX_TOPK + r] - mean;
            s2 += d * d;
        }
    }
    const float thr = mean + sqrtf(s2 / (float)(cnt - 1));
    if (cand) {
        const float cx = (a.x + a.z) / 2.f, cy = (a.y + a.w) / 2.f;
        const float inside = fminf(fminf(cx - g.x, cy - g.y), fminf(g.z - cx, g.w - cy));
        if (iou >= thr && inside > 0.01f) {
            const unsigned long long word = ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)(K - k);
            __hip_atomic_fetch_max(best + (int64_t)b * lv.aoff[L] + idx, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- assignment, second launch -------------------------------------------------------------------------------------------
// grid (ceil(A / 256), B): the word of an anchor -> assigned and the centerness target; positives and the centerness sum of the
// block (fp64) go to the partials
__global__ __launch_bounds__(256) void atss_decode_kernel(unsigned A, const float *__restrict__ anchors, const float *__restrict__ gts,
                                                          int K, AtssCoder cd, const unsigned long long *__restrict__ best,
                                                          int *__restrict__ assigned, float *__restrict__ ctr_targets,
                                                          int *__restrict__ part_n, double *__restrict__ part_c)
{
    __shared__ int red_n[4];
    __shared__ double red_c[4];
    const int b = blockIdx.y;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    int pos = 0;
    double c_sum = 0.;
    if (i < A) {
        const int64_t o = (int64_t)b * A + i;
        const unsigned long long word = best[o];
        float c = 0.f;
        int as = 0;
        if (word != 0ull) {
            const int k = K - (int)(unsigned)(word & 0xffffffffull);
            as = k + 1;
            pos = 1;
            const float4 a = load4(anchors, i);
            c = centerness_ref(a, target_box_ref(a, load4(gts, (int64_t)b * K + k), cd));
        }
        assigned[o] = as;
        ctr_targets[o] = c;
        c_sum = (double)c;
    }
    int n = pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o, 64); c_sum += __shfl_xor(c_sum, o, 64); }
    if ((threadIdx.x & 63) == 0) { red_n[threadIdx.x >> 6] = n; red_c[threadIdx.x >> 6] = c_sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t o = (int64_t)b * gridDim.x + blockIdx.x;
        part_n[o] = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
        part_c[o] = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
    }
}

// num_pos [B] and norm = [sum_b max(num_pos_b, 1), the same, sum of ctr_targets] from the per-block partials, in a fixed order:
// one wavefront, lane i takes blocks i, i + 64, ... of an image
__global__ __launch_bounds__(64) void atss_targets_finish_kernel(const int *__restrict__ part_n, const double *__restrict__ part_c,
                                                                  int B, int nblk, int *__restrict__ num_pos, float *__restrict__ norm)
{
    int total = 0;
    double csum = 0.;
    for (int b = 0; b < B; ++b) {
        int n = 0;
        double c = 0.;
        for (int i = threadIdx.x; i < nblk; i += 64) { n += part_n[(int64_t)b * nblk + i]; c += part_c[(int64_t)b * nblk + i]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o, 64); c += __shfl_xor(c, o, 64); }
        if (threadIdx.x == 0) num_pos[b] = n;
        total += n > 1 ? n : 1;
        csum += c;
    }
    if (threadIdx.x == 0) {
        norm[0] = (float)total;
        norm[1] = (float)total;
        norm[2] = (float)csum;
    }
}

// ---- loss --------------------------------------------------------------------------------------------------------------------
// Classification maps: the sweep of point_maps.h with plain focal elements, one anchor per pixel, every anchor with label weight
// 1.  Then one thread per anchor for the four deltas and the centerness logit.  partial [POINT_BLOCKS][2] = {sum focal, sum
// ctr_target * box loss}, partial + 2 * POINT_BLOCKS: [POINT_BLOCKS][2] = {sum centerness BCE, 0}, unscaled.
template <int VEC, bool G2>
__global__ __launch_bounds__(256) void atss_loss_kernel(PointMaps mp, AtssLevels lv, int L, int C, const float *__restrict__ anchors,
                                                        const float *__restrict__ gts, const int64_t *__restrict__ gt_labels, int K,
                                                        const int *__restrict__ assigned, const float *__restrict__ ctr_targets,
                                                        const float *__restrict__ norm, AtssCoder cd, int box_kind, double eps,
                                                        float gamma, float alpha, float cls_weight, float box_weight,
                                                        float ctr_weight, int group_shift, float *__restrict__ partial)
{
    const unsigned n_rows = mp.rrow[L];
    const float s_cls = cls_sweep<VEC>(mp, lv.aoff, L, C, assigned, gt_labels, K, nullptr, cls_weight / norm[0], group_shift,
                                       [=](float x, bool own, float, float &g) { return focal_elem<G2>(x, own, gamma, alpha, g); });
    // the anchors: prediction and target decoded against the anchor (delta2bbox of the deltas, and of bbox2delta of the gt), the
    // box loss weighted by the centerness target over norm[2] (1 where that is below EPS), the centerness BCE-with-logits over
    // norm[1]; both in fp64 on the few positives
    const double nb = (double)norm[2] < ATSS_EPS ? 1. : (double)norm[2];
    double s_box = 0., s_ctr = 0.;
    for (unsigned rw = blockIdx.x * 256u + threadIdx.x; rw < n_rows; rw += gridDim.x * 256u) {
        const PointRow r = point_row(mp, lv.aoff, L, rw);
        float gr[4] = {0.f, 0.f, 0.f, 0.f}, gc = 0.f;
        const int as = assigned[r.o];
        if (as > 0) {
            const float4 a = load4(anchors, r.i), g = load4(gts, (int64_t)r.b * K + (as - 1));
            const float *d = slot_row(mp, REG, r);
            const double w = (double)ctr_targets[r.o];
            const double px = ((double)a.x + a.z) * 0.5, py = ((double)a.y + a.w) * 0.5, pw = (double)a.z - a.x, ph = (double)a.w - a.y;
            const double *m = cd.mean_d, *s = cd.std_d;
            // the target in fp32, as the reference's fp64 run has it too (bbox2delta works in fp32); the prediction in fp64
            const float4 tf = target_box_ref(a, g, cd);
            const Box tb = {(double)tf.x, (double)tf.y, (double)tf.z, (double)tf.w};
            double e[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = (double)d[i] * s[i] + m[i];
            const bool in_w = e[2] >= -cd.max_ratio_d && e[2] <= cd.max_ratio_d, in_h = e[3] >= -cd.max_ratio_d && e[3] <= cd.max_ratio_d;
            const double qw = pw * exp(fmin(fmax(e[2], -cd.max_ratio_d), cd.max_ratio_d));
            const double qh = ph * exp(fmin(fmax(e[3], -cd.max_ratio_d), cd.max_ratio_d));
            const double qx = px + pw * e[0], qy = py + ph * e[1];
            const Box pb = {qx - qw * 0.5, qy - qh * 0.5, qx + qw * 0.5, qy + qh * 0.5};
            Box G;
            s_box += w * iou_family_loss(box_kind, pb, tb, eps, G);
            const double bs = w * (double)box_weight / nb;
            gr[0] = (float)((G.x1 + G.x2) * pw * s[0] * bs);
            gr[1] = (float)((G.y1 + G.y2) * ph * s[1] * bs);
            gr[2] = in_w ? (float)((G.x2 - G.x1) * 0.5 * qw * s[2] * bs) : 0.f;
            gr[3] = in_h ? (float)((G.y2 - G.y1) * 0.5 * qh * s[3] * bs) : 0.f;
            const double z = (double)slot_row(mp, CTR, r)[0];
            double l1p, sig;
            sigmoid_log1p(z, l1p, sig);
            s_ctr += fmax(z, 0.) - z * w + l1p;
            gc = (float)((sig - w) * (double)ctr_weight / (double)norm[1]);
        }
        store_padded(slot_grad_row(mp, REG, r), mp.cs[REG][r.l], gr, 4u);
        store_padded(slot_grad_row(mp, CTR, r), mp.cs[CTR][r.l], &gc, 1u);
    }
    block_store_partial2(s_cls, (float)s_box, partial);
    __syncthreads();                        // the reduction's LDS is read before the second pair overwrites it
    block_store_partial2((float)s_ctr, 0.f, partial + 2 * POINT_BLOCKS);
}

int fill_coder(AtssCoder &cd, const char *what, const double *means4, const double *stds4, double wh_ratio_clip)
{
    HTD_REQUIRE(means4 && stds4, "%s: null means / stds", what);
    HTD_REQUIRE(wh_ratio_clip > 0., "%s: wh_ratio_clip must be positive", what);
    for (int i = 0; i < 4; ++i) {
        HTD_REQUIRE(stds4[i] > 0., "%s: stds must be positive", what);
        cd.mean_d[i] = means4[i];
        cd.std_d[i] = stds4[i];
        cd.mean[i] = (float)means4[i];
        cd.std[i] = (float)stds4[i];
    }
    cd.max_ratio_d = fabs(log(wh_ratio_clip));
    cd.max_ratio = (float)cd.max_ratio_d;
    return HTD_OK;
}

}  // namespace

extern "C" int64_t htd_atss_targets_workspace_bytes(int B, int64_t A)
{
    return (int64_t)B * A * 8 + (int64_t)B * blocks_of(A) * 16;      // the words, then one double and one int (padded) per block
}

extern "C" int htd_atss_targets(const float *anchors, const int64_t *level_sizes, int L, const float *gts, const uint8_t *gt_valid,
                                int B, int K, int topk, const double *means4, const double *stds4, double wh_ratio_clip,
                                int *assigned, float *ctr_targets, void *workspace, int *num_pos, float *norm, void *stream)
{
    HTD_REQUIRE(B > 0 && B < 65536 && K > 0 && K < 65536, "atss_targets: bad sizes");
    HTD_REQUIRE(topk > 0 && topk <= ATSS_MAX_TOPK, "atss_targets: topk must be 1 to %d, got %d", ATSS_MAX_TOPK, topk);
    HTD_REQUIRE(anchors && gts && gt_valid && assigned && ctr_targets && workspace && num_pos && norm, "atss_targets: null pointer");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                "atss_targets: anchors / gts must be 16-byte aligned, the workspace 8-byte");
    AtssLevels lv = {};
    int64_t A = 0;
    int rc = fill_levels(lv, "atss_targets", level_sizes, L, &A);
    if (rc != HTD_OK) return rc;
    AtssCoder cd = {};
    rc = fill_coder(cd, "atss_targets", means4, stds4, wh_ratio_clip);
    if (rc != HTD_OK) return rc;
    HTD_REQUIRE((int64_t)B * A < ((int64_t)1 << 31), "atss_targets: more than 2^31 anchors in the batch");
    const int nblk = (int)blocks_of(A);
    unsigned long long *best = (unsigned long long *)workspace;
    double *part_c = (double *)(best + (int64_t)B * A);
    int *part_n = (int *)(part_c + (int64_t)B * nblk);
    if (hipMemsetAsync(best, 0, (size_t)B * A * 8, (hipStream_t)stream) != hipSuccess) {
        htd::set_error("atss_targets: clearing the workspace failed");
        return HTD_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(atss_select_kernel, dim3(K, B), dim3(64 * L), 0, (hipStream_t)stream, lv, L, anchors, gts, gt_valid, K, topk,
                       best);
    hipLaunchKernelGGL(atss_decode_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, (unsigned)A, anchors, gts, K, cd,
                       (const unsigned long long *)best, assigned, ctr_targets, part_n, part_c);
    hipLaunchKernelGGL(atss_targets_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int *)part_n,
                       (const double *)part_c, B, nblk, num_pos, norm);
    return htd::check_launch("atss_targets");
}

extern "C" int htd_atss_loss_partial_rows(void) { return 2 * POINT_BLOCKS; }

extern "C" int htd_atss_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                             const float *const *ctr, const int64_t *ctr_stride, const int64_t *level_sizes, int L, int B, int C,
                             const float *anchors, const float *gts, const int64_t *gt_labels, int K, const int *assigned,
                             const float *ctr_targets, const float *norm, const double *means4, const double *stds4,
                             double wh_ratio_clip, int box_kind, double eps, float gamma, float alpha, float cls_weight,
                             float box_weight, float ctr_weight, float *partial, float *const *grad_cls, float *const *grad_reg,
                             float *const *grad_ctr, void *stream)
{
    HTD_REQUIRE(anchors && gts && gt_labels && assigned && ctr_targets && norm && partial, "atss_loss: null pointer");
    HTD_REQUIRE(K > 0 && gamma >= 0.f && (box_kind == BOX_IOU || box_kind == BOX_GIOU), "atss_loss: bad parameters");
    HTD_REQUIRE((((uintptr_t)anchors | (uintptr_t)gts) & 15) == 0, "atss_loss: anchors / gts must be 16-byte aligned");
    AtssLevels lv = {};
    int64_t A = 0;
    int rc = fill_levels(lv, "atss_loss", level_sizes, L, &A);
    if (rc != HTD_OK) return rc;
    AtssCoder cd = {};
    rc = fill_coder(cd, "atss_loss", means4, stds4, wh_ratio_clip);
    if (rc != HTD_OK) return rc;
    const SweepForm f = sweep_form(C, cls_stride, L);
    const PointSlot slots[POINT_SLOTS] = {{cls, grad_cls, cls_stride, C, true, true}, {reg, grad_reg, reg_stride, 4, true, true},
                                          {ctr, grad_ctr, ctr_stride, 1, true, true}};
    PointMaps mp = {};
    rc = fill_point_maps(mp, "atss_loss", lv.aoff, L, B, slots, f.vec);
    if (rc != HTD_OK) return rc;
    HTD_POINT_LAUNCH(atss_loss_kernel, f.vec, gamma == 2.f, stream, mp, lv, L, C, anchors, gts, gt_labels, K, assigned, ctr_targets,
                     norm, cd, box_kind, eps, gamma, alpha, cls_weight, box_weight, ctr_weight, f.group_shift, partial);
    return htd::check_launch("atss_loss");
}
