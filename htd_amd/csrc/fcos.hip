// FCOS head on the device (dense_heads/fcos_head.py): the point-to-gt assignment with its regression and centerness targets of a
// whole batch over all pyramid levels in one launch (get_targets / _get_target_single :415-558, centerness_target :560-576), the
// three losses with their three finished gradient maps in one launch (loss :159-253), and the ranking keys of get_bboxes
// (_get_bboxes_single :364-372).  Built with -ffp-contract=off: the assignment takes the reference's fp32 decisions one rounded
// operation at a time (x - x1, the clipped centre box, the range test, the area product), so `assigned` and `bbox_targets` are
// the reference's bit for bit; the divisions and the square root of the centerness are correctly rounded
// (-fhip-fp32-correctly-rounded-divide-sqrt).  The box loss is the fp64 iou_family_loss of the RoI heads, the classification
// loss the focal_elem of the anchor heads: one implementation each.
//
// All three kernels are small and launch- or memory-bound: plain grids, fixed-order partial sums, no float atomics, every element
// of every output stored exactly once (padding channels and non-positive points as zeros).
#include "common.h"
#include "iou_family.h"
#include "point_maps.h"
#include "point_scale.h"

namespace {

constexpr int FCOS_MAX_LEVELS = POINT_MAX_LEVELS;
constexpr int GT_CHUNK = 256;               // gts staged through LDS per pass of the assignment
constexpr float FCOS_INF = 1e8f;            // fcos_head.py:11

struct FcosPoints {                          // the pyramid as the point generator sees it (get_points :403-413)
    int w[FCOS_MAX_LEVELS];                 // map width: point p of a level is (row p / w, column p % w)
    int stride[FCOS_MAX_LEVELS];
    unsigned poff[FCOS_MAX_LEVELS + 1];     // first point of the level; poff[L] = P
    float lo[FCOS_MAX_LEVELS], hi[FCOS_MAX_LEVELS];      // regress range
    float sr[FCOS_MAX_LEVELS];              // stride * center_sample_radius, rounded to fp32 as the reference's tensor holds it
};

enum { CLS = 0, REG = 1, CTR = 2 };       // slots of PointMaps: (B, C, h, w), (B, 4, h, w), (B, 1, h, w)

__device__ __forceinline__ void point_xy(const FcosPoints &pt, int l, unsigned p, float &x, float &y)
{
    const unsigned row = p / (unsigned)pt.w[l], col = p - row * (unsigned)pt.w[l];
    // x * stride + stride // 2 on small integers: exact in fp32
    x = (float)(col * (unsigned)pt.stride[l] + (unsigned)(pt.stride[l] / 2));
    y = (float)(row * (unsigned)pt.stride[l] + (unsigned)(pt.stride[l] / 2));
}

// ---- targets -----------------------------------------------------------------------------------------------------------------
// grid (ceil(P / 256), B); a thread owns one point of one image and walks the image's gts, which the block stages through LDS
// GT_CHUNK at a time (any K).  The smallest area among the gts that hold the point (or whose clipped centre box does) and whose
// largest distance lies in the level's range wins; equal areas go to the lower index: the first minimum, as torch.min on the CPU
// returns it.  A point without candidate is background and still carries the distances to the first minimum of the all-INF row
// (gt 0 of the image), as the reference's bbox_targets do; an image without gts gives zeros.
__global__ __launch_bounds__(256) void fcos_targets_kernel(FcosPoints pt, int L, const float *__restrict__ gts,
                                                           const uint8_t *__restrict__ gt_valid, int K, int center_sampling,
                                                           int norm_on_bbox, int *__restrict__ assigned,
                                                           float *__restrict__ bbox_targets, float *__restrict__ ctr_targets,
                                                           int *__restrict__ part_n, double *__restrict__ part_c)
{
    __shared__ float4 s_gt[GT_CHUNK];
    __shared__ float s_area[GT_CHUNK];
    __shared__ uint8_t s_ok[GT_CHUNK];
    __shared__ int red_n[4];
    __shared__ double red_c[4];
    const unsigned P = pt.poff[L];
    const int b = blockIdx.y;
    const unsigned p_all = blockIdx.x * 256u + threadIdx.x;
    const bool live = p_all < P;
    int l = 0;
    float x = 0.f, y = 0.f;
    if (live) {
        l = level_of(pt.poff, L, p_all);
        point_xy(pt, l, p_all - pt.poff[l], x, y);
    }
    const float lo = pt.lo[l], hi = pt.hi[l], sr = pt.sr[l];
    int best_k = -1;
    float best = 0.f;
    float4 best_gt = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < K; k0 += GT_CHUNK) {
        const int n = min(GT_CHUNK, K - k0);
        __syncthreads();                    // the previous chunk has been read by every thread
        if ((int)threadIdx.x < n) {
            const int64_t gi = (int64_t)b * K + k0 + threadIdx.x;
            const float4 g = *reinterpret_cast<const float4 *>(gts + gi * 4);
            s_gt[threadIdx.x] = g;
            s_area[threadIdx.x] = (g.z - g.x) * (g.w - g.y);
            s_ok[threadIdx.x] = gt_valid[gi];
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < n; ++j) {
                if (!s_ok[j]) continue;
                const float4 g = s_gt[j];
                const float dl = x - g.x, dr = g.z - x, dt = y - g.y, db = g.w - y;
                bool inside;
                if (center_sampling) {      // fcos_head.py:503-537
                    const float cx = (g.x + g.z) / 2.f, cy = (g.y + g.w) / 2.f;
                    const float x_min = cx - sr, y_min = cy - sr, x_max = cx + sr, y_max = cy + sr;
                    const float c0 = x_min > g.x ? x_min : g.x, c1 = y_min > g.y ? y_min : g.y;
                    const float c2 = x_max > g.z ? g.z : x_max, c3 = y_max > g.w ? g.w : y_max;
                    inside = fminf(fminf(x - c0, y - c1), fminf(c2 - x, c3 - y)) > 0.f;
                } else {
                    inside = fminf(fminf(dl, dt), fminf(dr, db)) > 0.f;
                }
                const float far = fmaxf(fmaxf(dl, dt), fmaxf(dr, db));
                const bool cand = inside && far >= lo && far <= hi;
                const float a = cand ? s_area[j] : FCOS_INF;
                if (best_k < 0 || a < best) { best = a; best_k = k0 + j; best_gt = g; }
            }
        }
    }
    int pos = 0;
    double c_sum = 0.;
    if (live) {
        const int64_t o = (int64_t)b * P + p_all;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, c = 0.f;
        if (best_k >= 0) {
            t0 = x - best_gt.x; t1 = y - best_gt.y; t2 = best_gt.z - x; t3 = best_gt.w - y;
            if (norm_on_bbox) {
                const float s = (float)pt.stride[l];
                t0 = t0 / s; t1 = t1 / s; t2 = t2 / s; t3 = t3 / s;
            }
            pos = best != FCOS_INF ? 1 : 0;                                 // labels[min_area == INF] = background
            if (pos) c = sqrtf((fminf(t0, t2) / fmaxf(t0, t2)) * (fminf(t1, t3) / fmaxf(t1, t3)));
        }
        assigned[o] = pos ? best_k + 1 : 0;
        *reinterpret_cast<float4 *>(bbox_targets + o * 4) = make_float4(t0, t1, t2, t3);
        ctr_targets[o] = c;
        c_sum = (double)c;
    }
    // positives (integers) and the centerness sum (fp64: the finished sum is the fp32 rounding of a sum good to fp64) of the block
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

// num_pos [B] and norm = [num_pos_total + B, max(num_pos_total, 1), sum of ctr_targets] from the per-block partials, in a fixed
// order: one wavefront, lane i takes blocks i, i + 64, ... of an image
__global__ __launch_bounds__(64) void fcos_targets_finish_kernel(const int *__restrict__ part_n, const double *__restrict__ part_c,
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
        total += n;
        csum += c;
    }
    if (threadIdx.x == 0) {
        norm[0] = (float)(total + B);
        norm[1] = (float)(total > 1 ? total : 1);
        norm[2] = (float)csum;
    }
}

// ---- loss --------------------------------------------------------------------------------------------------------------------
// Classification maps: the sweep of point_maps.h with plain focal elements (one "anchor" per pixel).  Then one thread per point
// for the four distances and the centerness logit: a sixteenth of the data.  partial [POINT_BLOCKS][2] = {sum focal, sum
// ctr_target * box loss}, partial + 2 * POINT_BLOCKS: [POINT_BLOCKS][2] = {sum centerness BCE, 0}, unscaled.
template <int VEC, bool G2>
__global__ __launch_bounds__(256) void fcos_loss_kernel(PointMaps mp, FcosPoints pt, int L, int C, const int64_t *__restrict__ gt_labels,
                                                        int K, const int *__restrict__ assigned,
                                                        const float *__restrict__ bbox_targets, const float *__restrict__ ctr_targets,
                                                        const float *__restrict__ norm, int box_kind, double eps, float gamma,
                                                        float alpha, float cls_weight, float box_weight, float ctr_weight,
                                                        int group_shift, float *__restrict__ partial)
{
    const unsigned n_rows = mp.rrow[L];
    const float s_cls = cls_sweep<VEC>(mp, pt.poff, L, C, assigned, gt_labels, K, nullptr, cls_weight / norm[0], group_shift,
                                       [=](float x, bool own, float, float &g) { return focal_elem<G2>(x, own, gamma, alpha, g); });
    // the points: decode prediction and target against the point (distance2bbox), the box loss weighted by the centerness target
    // over norm[2], the centerness BCE-with-logits over norm[1]; both in fp64 on the few positives
    double s_box = 0., s_ctr = 0.;
    for (unsigned rw = blockIdx.x * 256u + threadIdx.x; rw < n_rows; rw += gridDim.x * 256u) {
        const PointRow r = point_row(mp, pt.poff, L, rw);
        float gr[4] = {0.f, 0.f, 0.f, 0.f}, gc = 0.f;
        if (assigned[r.o] > 0) {
            float x, y;
            point_xy(pt, r.l, r.p, x, y);
            const float *d = slot_row(mp, REG, r);
            const float4 t = *reinterpret_cast<const float4 *>(bbox_targets + r.o * 4);
            const double w = (double)ctr_targets[r.o];
            const Box pb = {(double)x - d[0], (double)y - d[1], (double)x + d[2], (double)y + d[3]};
            const Box tb = {(double)x - t.x, (double)y - t.y, (double)x + t.z, (double)y + t.w};
            Box G;
            s_box += w * iou_family_loss(box_kind, pb, tb, eps, G);
            const double bs = w * (double)box_weight / (double)norm[2];
            gr[0] = (float)(-G.x1 * bs); gr[1] = (float)(-G.y1 * bs); gr[2] = (float)(G.x2 * bs); gr[3] = (float)(G.y2 * bs);
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

// key [B][P] = max_c sigmoid(cls) * sigmoid(centerness) = sigmoid(max_c cls) * sigmoid(centerness) (both factors rounded to fp32
// as the reference's tensors are; the product with a positive factor keeps the order of the maximum): 16 lanes per point
__global__ __launch_bounds__(256) void fcos_keys_kernel(PointMaps mp, FcosPoints pt, int L, int B, int C, float *__restrict__ keys)
{
    const int sub = threadIdx.x & 15;
    const unsigned P = pt.poff[L];
    const int64_t rows = (int64_t)B * P;
    const int64_t stride = (int64_t)gridDim.x * 16;
    for (int64_t i0 = (int64_t)blockIdx.x * 16; i0 < rows; i0 += stride) {      // every lane of a 16-lane group stays in the loop
        const int64_t i = i0 + (threadIdx.x >> 4);
        float m = -INFINITY, ct = 0.f;
        if (i < rows) {
            const unsigned b = (unsigned)(i / P), pi = (unsigned)(i - (int64_t)b * P);
            const int l = level_of(pt.poff, L, pi);
            const int64_t row = (int64_t)b * mp.pix[l] + (pi - pt.poff[l]);
            const float *x = mp.map[CLS][l] + row * mp.cs[CLS][l];
            if ((C & 3) == 0 && (mp.cs[CLS][l] & 3) == 0) {
                for (int c = sub * 4; c < C; c += 64) {
                    const float4 v = *reinterpret_cast<const float4 *>(x + c);
                    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
                }
            } else {
                for (int c = sub; c < C; c += 16) m = fmaxf(m, x[c]);
            }
            ct = mp.map[CTR][l][row * mp.cs[CTR][l]];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (sub == 0 && i < rows) keys[i] = (1.f / (1.f + expf(-m))) * (1.f / (1.f + expf(-ct)));
    }
}

int fill_points(FcosPoints &pt, const char *what, const int64_t *hw, const int64_t *strides, const float *ranges, int L,
                double radius, int64_t *P_out)
{
    HTD_REQUIRE(L > 0 && L <= FCOS_MAX_LEVELS, "%s: 1 to %d levels, got %d", what, FCOS_MAX_LEVELS, L);
    HTD_REQUIRE(hw && strides, "%s: null level table", what);
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
        HTD_REQUIRE(hw[2 * l] > 0 && hw[2 * l + 1] > 0 && strides[l] > 0 && strides[l] < (1 << 20), "%s: bad level %d", what, l);
        HTD_REQUIRE((hw[2 * l] + 1) * strides[l] < ((int64_t)1 << 24) && (hw[2 * l + 1] + 1) * strides[l] < ((int64_t)1 << 24),
                    "%s: points of level %d are not exact in fp32", what, l);
        pt.w[l] = (int)hw[2 * l + 1];
        pt.stride[l] = (int)strides[l];
        pt.poff[l] = (unsigned)off;
        pt.lo[l] = ranges ? ranges[2 * l] : 0.f;
        pt.hi[l] = ranges ? ranges[2 * l + 1] : 0.f;
        pt.sr[l] = (float)((double)strides[l] * radius);
        off += hw[2 * l] * hw[2 * l + 1];
        HTD_REQUIRE(off < ((int64_t)1 << 31), "%s: more than 2^31 points", what);
    }
    for (int l = L; l <= FCOS_MAX_LEVELS; ++l) pt.poff[l] = (unsigned)off;
    *P_out = off;
    return HTD_OK;
}

}  // namespace

extern "C" int64_t htd_fcos_targets_workspace_bytes(int B, int64_t P)
{
    return (int64_t)B * blocks_of(P) * 16;      // one double and one int (padded to 8 bytes) per block
}

extern "C" int htd_fcos_targets(const int64_t *hw, const int64_t *strides, const float *ranges, int L, const float *gts,
                                const uint8_t *gt_valid, int B, int K, int center_sampling, double radius, int norm_on_bbox,
                                int *assigned, float *bbox_targets, float *ctr_targets, void *workspace, int *num_pos, float *norm,
                                void *stream)
{
    HTD_REQUIRE(B > 0 && B < 65536 && K > 0, "fcos_targets: bad sizes");
    HTD_REQUIRE(ranges && gts && gt_valid && assigned && bbox_targets && ctr_targets && workspace && num_pos && norm,
                "fcos_targets: null pointer");
    HTD_REQUIRE((((uintptr_t)gts | (uintptr_t)bbox_targets) & 15) == 0 && ((uintptr_t)workspace & 7) == 0,
                "fcos_targets: gts / bbox_targets must be 16-byte aligned, the workspace 8-byte");
    FcosPoints pt = {};
    int64_t P = 0;
    const int rc = fill_points(pt, "fcos_targets", hw, strides, ranges, L, radius, &P);
    if (rc != HTD_OK) return rc;
    HTD_REQUIRE((int64_t)B * P < ((int64_t)1 << 31), "fcos_targets: more than 2^31 points in the batch");
    const int nblk = (int)blocks_of(P);
    double *part_c = (double *)workspace;
    int *part_n = (int *)(part_c + (int64_t)B * nblk);
    hipLaunchKernelGGL(fcos_targets_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, pt, L, gts, gt_valid, K,
                       center_sampling, norm_on_bbox, assigned, bbox_targets, ctr_targets, part_n, part_c);
    hipLaunchKernelGGL(fcos_targets_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int *)part_n,
                       (const double *)part_c, B, nblk, num_pos, norm);
    return htd::check_launch("fcos_targets");
}

extern "C" int htd_fcos_loss_partial_rows(void) { return 2 * POINT_BLOCKS; }

extern "C" int htd_fcos_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                             const float *const *ctr, const int64_t *ctr_stride, const int64_t *hw, const int64_t *strides, int L,
                             int B, int C, const int64_t *gt_labels, int K, const int *assigned, const float *bbox_targets,
                             const float *ctr_targets, const float *norm, int box_kind, double eps, float gamma, float alpha,
                             float cls_weight, float box_weight, float ctr_weight, float *partial, float *const *grad_cls,
                             float *const *grad_reg, float *const *grad_ctr, void *stream)
{
    HTD_REQUIRE(gt_labels && assigned && bbox_targets && ctr_targets && norm && partial, "fcos_loss: null pointer");
    HTD_REQUIRE(K > 0 && gamma >= 0.f && (box_kind == BOX_IOU || box_kind == BOX_GIOU), "fcos_loss: bad parameters");
    HTD_REQUIRE(((uintptr_t)bbox_targets & 15) == 0, "fcos_loss: bbox_targets must be 16-byte aligned");
    FcosPoints pt = {};
    int64_t P = 0;
    int rc = fill_points(pt, "fcos_loss", hw, strides, nullptr, L, 0., &P);
    if (rc != HTD_OK) return rc;
    const SweepForm f = sweep_form(C, cls_stride, L);
    const PointSlot slots[POINT_SLOTS] = {{cls, grad_cls, cls_stride, C, true, true}, {reg, grad_reg, reg_stride, 4, true, true},
                                          {ctr, grad_ctr, ctr_stride, 1, true, true}};
    PointMaps mp = {};
    rc = fill_point_maps(mp, "fcos_loss", pt.poff, L, B, slots, f.vec);
    if (rc != HTD_OK) return rc;
    HTD_POINT_LAUNCH(fcos_loss_kernel, f.vec, gamma == 2.f, stream, mp, pt, L, C, gt_labels, K, assigned, bbox_targets, ctr_targets,
                     norm, box_kind, eps, gamma, alpha, cls_weight, box_weight, ctr_weight, f.group_shift, partial);
    return htd::check_launch("fcos_loss");
}

extern "C" int htd_fcos_grad_scale(float *const *grad_cls, const int64_t *cls_stride, float *const *grad_reg,
                                   const int64_t *reg_stride, float *const *grad_ctr, const int64_t *ctr_stride, const int64_t *hw,
                                   const int64_t *strides, int L, int B, int C, const float *g_cls, const float *g_box,
                                   const float *g_ctr, void *stream)
{
    FcosPoints pt = {};
    int64_t P = 0;
    const int rc = fill_points(pt, "fcos_grad_scale", hw, strides, nullptr, L, 0., &P);
    if (rc != HTD_OK) return rc;
    return point_grad_scale<4, 1>("fcos_grad_scale", pt.poff, L, B, grad_cls, cls_stride, C, grad_reg, reg_stride, grad_ctr, ctr_stride,
                                  g_cls, g_box, g_ctr, stream);
}

extern "C" int htd_fcos_keys(const float *const *cls, const int64_t *cls_stride, const float *const *ctr, const int64_t *ctr_stride,
                             const int64_t *hw, const int64_t *strides, int L, int B, int C, float *keys, void *stream)
{
    HTD_REQUIRE(keys, "fcos_keys: null pointer");
    FcosPoints pt = {};
    int64_t P = 0;
    int rc = fill_points(pt, "fcos_keys", hw, strides, nullptr, L, 0., &P);
    if (rc != HTD_OK) return rc;
    const PointSlot slots[POINT_SLOTS] = {{cls, nullptr, cls_stride, C, true, false}, {}, {ctr, nullptr, ctr_stride, 1, true, false}};
    PointMaps mp = {};
    rc = fill_point_maps(mp, "fcos_keys", pt.poff, L, B, slots, 1);
    if (rc != HTD_OK) return rc;
    const int64_t groups = htd::ceil_div((int64_t)B * P, 16);
    hipLaunchKernelGGL(fcos_keys_kernel, dim3((unsigned)(groups < POINT_BLOCKS ? groups : POINT_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, mp, pt, L, B, C, keys);
    return htd::check_launch("fcos_keys");
}
