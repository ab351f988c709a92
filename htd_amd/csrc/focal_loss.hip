// Sigmoid focal loss (mmdet/models/losses/focal_loss.py:10-41, py_sigmoid_focal_loss; the role of mmcv.ops.sigmoid_focal_loss)
// and the RetinaNet head loss over all pyramid levels in one launch (dense_heads/anchor_head.py:172-269 targets, :373-488 loss).
//
//   loss = BCEWithLogits(x, t) * (alpha t + (1 - alpha)(1 - t)) * pt^gamma,   pt = (1 - sigmoid(x)) t + sigmoid(x) (1 - t)
//
// With z = -x for t = 1 and z = x for t = 0 this is   loss = a_t * sigmoid(z)^gamma * softplus(z),   and
//   d loss / dz = a_t * sigmoid(z)^gamma * (sigmoid(z) + gamma * softplus(z) * (1 - sigmoid(z))),   dz/dx = -1 or 1.
// softplus(z) = max(z, 0) + log1p(exp(-|z|)) (finite for any finite z), sigmoid(z) and 1 - sigmoid(z) from the same exp(-|z|):
// one exp and one log per element serve the loss and its derivative (the hardware's v_exp_f32 / v_log_f32 / v_rcp_f32: with the
// accurate library forms the kernel is bound by arithmetic at a quarter of the HBM rate).
#include "common.h"
#include "focal_elem.h"
#include "retina_levels.h"

namespace {

constexpr int COUNT_CHUNKS = 64;

// ---- matrix form: logits [N][C], labels [N] (C = background), weight [N] or NULL ------------------------------------------
// VEC = 4: C % 4 == 0, a lane handles four classes of one row (C = 80: 20 lanes per row, a wave reads whole 256-B segments);
// VEC = 1: any C.  partial [FOCAL_BLOCKS] = per-block sums of the weighted loss.
template <int VEC, bool G2>
__global__ __launch_bounds__(256) void focal_matrix_kernel(const float *__restrict__ x, const int64_t *__restrict__ labels,
                                                           const float *__restrict__ weight, int64_t units, int cols,
                                                           float gamma, float alpha, float *__restrict__ loss_out,
                                                           float *__restrict__ partial, float *__restrict__ grad)
{
    float sum = 0.f;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        int c0;
        const int64_t row = matrix_unit<VEC>(u, units, cols, c0);
        const int64_t lab = labels[row];
        const float w = weight ? weight[row] : 1.f;
        float xv[VEC], lo[VEC], go[VEC];
        load_unit<VEC>(x, u, xv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float g;
            const float l = focal_elem<G2>(xv[k], lab == c0 + k, gamma, alpha, g);
            lo[k] = w * l;
            go[k] = w * g;
            sum += lo[k];
        }
        if (loss_out) store_unit<VEC>(loss_out, u, lo);
        store_unit<VEC>(grad, u, go);
    }
    __shared__ float red[4];
    sum = htd::wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- head form ---------------------------------------------------------------------------------------------------------------

template <bool L1>
__device__ __forceinline__ float box_elem(float d, float beta, float &g)
{
    const float ad = fabsf(d);
    if (!L1 && ad < beta) { g = d / beta; return 0.5f * ad * ad / beta; }
    g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    return L1 ? ad : ad - 0.5f * beta;
}

// One unit = VEC classes of one anchor of one pixel of one image (or VEC padding channels), then one unit = the four deltas of
// one anchor (or four padding channels).  Every unit of every gradient map is stored exactly once, zeros included.
template <int VEC, bool G2, bool L1>
__global__ __launch_bounds__(256) void retina_loss_kernel(RetinaLevels lv, int L, int na, int C, const float *__restrict__ anchors,
                                                          const float *__restrict__ gts, const int64_t *__restrict__ gt_labels,
                                                          const int64_t *__restrict__ assigned, int A, int K, Vec4f means,
                                                          Vec4f stds, float gamma, float alpha, float pos_weight, float beta,
                                                          const float *__restrict__ avg_factor, float cls_weight, float box_weight,
                                                          float *__restrict__ partial)
{
    const float inv = 1.f / *avg_factor;
    const float cs = cls_weight * inv, bs = box_weight * inv;
    const unsigned n_cls = lv.coff[L], n_all = lv.roff[L];
    const unsigned nc = (unsigned)(na * C);
    float s_cls = 0.f, s_box = 0.f;
    // classification maps: one wavefront per pixel row [cu units] (C = 80, na = 9: 180 float4s, three sweeps of the wave), so the
    // level, image and pixel of a row are found once per row on the scalar unit and a lane only splits its channel into
    // (anchor, class); consecutive lanes read consecutive float4s
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned n_rows = lv.rrow[L];
    const float inv_c = 1.f / (float)C;
    for (unsigned rw = wave; rw < n_rows; rw += gridDim.x * 4u) {
        const ClsRow r = cls_row<VEC>(lv, L, rw, na, assigned, A, gt_labels, K);
        for (unsigned j = lane; j < r.cu; j += 64u) {
            const unsigned ch = j * VEC;
            float go[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) go[k] = 0.f;
            if (ch < nc) {
                unsigned c0;
                const int64_t as = r.as_row[anchor_of_channel(ch, (unsigned)C, inv_c, c0)];
                if (as >= 0) {
                    const int64_t lab = as > 0 ? r.lab_row[as - 1] : (int64_t)C;
                    const float w = (as > 0 && pos_weight > 0.f) ? pos_weight : 1.f;
                    float xv[VEC];
                    load_unit<VEC>(r.x_row, j, xv);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        float g;
                        s_cls += w * focal_elem<G2>(xv[k], lab == (int64_t)(c0 + k), gamma, alpha, g);
                        go[k] = w * g * cs;
                    }
                }
            }
            store_unit<VEC>(r.g_row, j, go);
        }
    }
    // regression maps: a twentieth of the data, one float4 (the four deltas of an anchor) per thread
    for (unsigned u = n_cls + blockIdx.x * 256u + threadIdx.x; u < n_all; u += gridDim.x * 256u) {
        const RegUnit r = reg_unit(lv, L, u);
        float go[4] = {0.f, 0.f, 0.f, 0.f};
        if (r.a < (unsigned)na) {
            unsigned b;
            const unsigned ai = reg_anchor(lv, r, na, b);
            const int64_t as = assigned[(int64_t)b * A + ai];
            if (as > 0) {
                float tgt[4], rr[4];
                delta_target(anchors + (int64_t)ai * 4, gts + ((int64_t)b * K + (as - 1)) * 4, means, stds, tgt);
                load_unit<4>(lv.reg[r.l], r.v, rr);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s_box += box_elem<L1>(rr[k] - tgt[k], beta, go[k]);
                    go[k] *= bs;
                }
            }
        }
        store_unit<4>(lv.greg[r.l], r.v, go);
    }
    block_store_partial2(s_cls, s_box, partial);
}

// positives per (image, chunk) -> counts [B][COUNT_CHUNKS] (integers: any order gives the same sum)
__global__ __launch_bounds__(256) void retina_count_kernel(const int64_t *__restrict__ assigned, int A, int *__restrict__ counts)
{
    __shared__ int red[4];
    const int b = blockIdx.y;
    int n = 0;
    for (int a = blockIdx.x * 256 + threadIdx.x; a < A; a += COUNT_CHUNKS * 256) n += assigned[(int64_t)b * A + a] > 0 ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[b * COUNT_CHUNKS + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// num_pos [B] and avg = sum_b max(num_pos_b, 1) (anchor_head.py:288-291)
__global__ __launch_bounds__(64) void retina_avg_kernel(const int *__restrict__ counts, int B, int *__restrict__ num_pos,
                                                        float *__restrict__ avg)
{
    int total = 0;
    for (int b = 0; b < B; ++b) {
        int n = counts[b * COUNT_CHUNKS + threadIdx.x];
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (threadIdx.x == 0) num_pos[b] = n;
        total += n > 1 ? n : 1;
    }
    if (threadIdx.x == 0) *avg = (float)total;
}

// gradient maps *= *g, skipped as a whole when *g == 1 (the usual root gradient): no host read decides it
__global__ __launch_bounds__(256) void retina_scale_kernel(RetinaLevels lv, int L, const float *__restrict__ g_cls,
                                                           const float *__restrict__ g_box)
{
    const float gc = *g_cls, gb = *g_box;
    const unsigned n_cls = lv.coff[L], n_all = lv.roff[L];
    const unsigned lo = gc == 1.f ? n_cls : 0u, hi = gb == 1.f ? n_cls : n_all;
    for (unsigned u = lo + blockIdx.x * 256u + threadIdx.x; u < hi; u += gridDim.x * 256u) {
        const bool is_cls = u < n_cls;
        const unsigned *off = is_cls ? lv.coff : lv.roff;
        const int l = level_of(off, L, u);
        float4 *p = reinterpret_cast<float4 *>(is_cls ? lv.gcls[l] : lv.greg[l]) + (u - off[l]);
        float4 q = *p;
        const float s = is_cls ? gc : gb;
        q.x *= s; q.y *= s; q.z *= s; q.w *= s;
        *p = q;
    }
}

// key [B][A] = max_c sigmoid(x[b][anchor][c]): 16 lanes per anchor read its classes as float4s
__global__ __launch_bounds__(256) void retina_keys_kernel(RetinaLevels lv, int L, int B, int na, int C, int A, float *__restrict__ keys)
{
    const int sub = threadIdx.x & 15;
    const int64_t rows = (int64_t)B * A;
    const int64_t stride = (int64_t)gridDim.x * 16;
    for (int64_t i0 = (int64_t)blockIdx.x * 16; i0 < rows; i0 += stride) {      // every lane of a 16-lane group stays in the loop
        const int64_t i = i0 + (threadIdx.x >> 4);
        float m = -INFINITY;
        if (i < rows) {
            const int b = (int)(i / A);
            const unsigned ai = (unsigned)(i - (int64_t)b * A);
            const int l = level_of(lv.aoff, L, ai);
            const unsigned q = ai - lv.aoff[l], p = q / (unsigned)na, a = q - p * (unsigned)na;
            const float *x = lv.cls[l] + ((int64_t)b * lv.pix[l] + p) * lv.cu[l] + (int64_t)a * C;   // cu: channel stride in floats here
            if ((C & 3) == 0 && (lv.cu[l] & 3) == 0) {
                for (int c = sub * 4; c < C; c += 64) {
                    const float4 v = *reinterpret_cast<const float4 *>(x + c);
                    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
                }
            } else {
                for (int c = sub; c < C; c += 16) m = fmaxf(m, x[c]);
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (sub == 0 && i < rows) keys[i] = 1.f / (1.f + expf(-m));
    }
}

}  // namespace

extern "C" int htd_focal_loss_partial_rows(void) { return FOCAL_BLOCKS; }

extern "C" int htd_sigmoid_focal_loss(const float *logits, const int64_t *labels, const float *weight, int64_t N, int C, float gamma,
                                      float alpha, float *loss_out, float *partial, float *grad, void *stream)
{
    HTD_REQUIRE(N >= 0 && C > 0 && gamma >= 0.f, "sigmoid_focal_loss: bad sizes");
    HTD_REQUIRE(partial && grad && (N == 0 || (logits && labels)), "sigmoid_focal_loss: null pointer");
    const bool vec = (C & 3) == 0 && (((uintptr_t)logits | (uintptr_t)grad | (uintptr_t)loss_out) & 15) == 0;
    const int64_t units = vec ? N * (C / 4) : N * C;
    const int cols = vec ? C / 4 : C;
    const bool g2 = gamma == 2.f;
#define HTD_FOCAL_LAUNCH(V, G)                                                                                                      \
    hipLaunchKernelGGL((focal_matrix_kernel<V, G>), dim3(FOCAL_BLOCKS), dim3(256), 0, (hipStream_t)stream, logits, labels, weight, \
                       units, cols, gamma, alpha, loss_out, partial, grad)
    if (vec) { if (g2) HTD_FOCAL_LAUNCH(4, true); else HTD_FOCAL_LAUNCH(4, false); }
    else { if (g2) HTD_FOCAL_LAUNCH(1, true); else HTD_FOCAL_LAUNCH(1, false); }
#undef HTD_FOCAL_LAUNCH
    return htd::check_launch("sigmoid_focal_loss");
}

extern "C" int64_t htd_retina_avg_factor_workspace_bytes(int B) { return (int64_t)B * COUNT_CHUNKS * sizeof(int); }

extern "C" int htd_retina_avg_factor(const int64_t *assigned, int B, int A, void *workspace, int *num_pos, float *avg_factor,
                                     void *stream)
{
    HTD_REQUIRE(B > 0 && A > 0, "retina_avg_factor: bad sizes");
    HTD_REQUIRE(assigned && workspace && num_pos && avg_factor, "retina_avg_factor: null pointer");
    hipLaunchKernelGGL(retina_count_kernel, dim3(COUNT_CHUNKS, B), dim3(256), 0, (hipStream_t)stream, assigned, A, (int *)workspace);
    hipLaunchKernelGGL(retina_avg_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int *)workspace, B, num_pos, avg_factor);
    return htd::check_launch("retina_avg_factor");
}

extern "C" int htd_retina_loss(const float *const *cls, const int64_t *cls_stride, const float *const *reg, const int64_t *reg_stride,
                               const int64_t *pix, int L, int B, int na, int C, const float *anchors, const float *gts,
                               const int64_t *gt_labels, const int64_t *assigned, int A, int K, const float *means4,
                               const float *stds4, float gamma, float alpha, float pos_weight, int box_loss, float beta,
                               const float *avg_factor, float cls_weight, float box_weight, float *partial, float *const *grad_cls,
                               float *const *grad_reg, void *stream)
{
    HTD_REQUIRE(reg && grad_cls && grad_reg, "retina_loss: null table");
    HTD_REQUIRE(anchors && gts && gt_labels && assigned && means4 && stds4 && avg_factor && partial, "retina_loss: null pointer");
    HTD_REQUIRE((int64_t)na * C < (1 << 20), "retina_loss: more than 2^20 classification channels");
    HTD_REQUIRE(K > 0 && gamma >= 0.f && (box_loss == 1 || (box_loss == 0 && beta > 0.f)), "retina_loss: bad parameters");
    RetinaLevels lv = {};
    bool vec;
    Vec4f m, sd;
    const int rc = head_loss_levels(lv, "retina_loss", cls, cls_stride, reg, reg_stride, grad_cls, grad_reg, pix, L, B, na, C, A,
                                    means4, stds4, vec, m, sd);
    if (rc != HTD_OK) return rc;
    const bool g2 = gamma == 2.f, l1 = box_loss == 1;
#define HTD_RETINA_LAUNCH(V, G, B1)                                                                                                    \
    hipLaunchKernelGGL((retina_loss_kernel<V, G, B1>), dim3(FOCAL_BLOCKS), dim3(256), 0, (hipStream_t)stream, lv, L, na, C, anchors, \
                       gts, gt_labels, assigned, A, K, m, sd, gamma, alpha, pos_weight, beta, avg_factor, cls_weight, box_weight,   \
                       partial)
    if (vec) {
        if (g2) { if (l1) HTD_RETINA_LAUNCH(4, true, true); else HTD_RETINA_LAUNCH(4, true, false); }
        else { if (l1) HTD_RETINA_LAUNCH(4, false, true); else HTD_RETINA_LAUNCH(4, false, false); }
    } else {
        if (g2) { if (l1) HTD_RETINA_LAUNCH(1, true, true); else HTD_RETINA_LAUNCH(1, true, false); }
        else { if (l1) HTD_RETINA_LAUNCH(1, false, true); else HTD_RETINA_LAUNCH(1, false, false); }
    }
#undef HTD_RETINA_LAUNCH
    return htd::check_launch("retina_loss");
}

extern "C" int htd_retina_grad_scale(float *const *grad_cls, const int64_t *cls_stride, float *const *grad_reg,
                                     const int64_t *reg_stride, const int64_t *pix, int L, int B, int na, int C, const float *g_cls,
                                     const float *g_box, void *stream)
{
    HTD_REQUIRE(grad_cls && grad_reg && g_cls && g_box, "retina_grad_scale: null pointer");
    RetinaLevels lv = {};
    int64_t A_lv = 0;
    for (int l = 0; l < L && l < RETINA_MAX_LEVELS; ++l)
        HTD_REQUIRE(cls_stride && (cls_stride[l] & 3) == 0, "retina_grad_scale: channel strides must be multiples of 4");
    const int rc = fill_levels(lv, "retina_grad_scale", grad_cls, cls_stride, grad_reg, reg_stride, grad_cls, grad_reg, pix, L, B, na,
                               C, 4, &A_lv);
    if (rc != HTD_OK) return rc;
    hipLaunchKernelGGL(retina_scale_kernel, dim3(FOCAL_BLOCKS), dim3(256), 0, (hipStream_t)stream, lv, L, g_cls, g_box);
    return htd::check_launch("retina_grad_scale");
}

extern "C" int htd_retina_keys(const float *const *cls, const int64_t *cls_stride, const int64_t *pix, int L, int B, int na, int C,
                               float *keys, void *stream)
{
    HTD_REQUIRE(keys, "retina_keys: null pointer");
    RetinaLevels lv = {};
    int64_t A = 0;
    const int rc = fill_levels(lv, "retina_keys", cls, cls_stride, nullptr, nullptr, nullptr, nullptr, pix, L, B, na, C, 1, &A);
    if (rc != HTD_OK) return rc;
    const int64_t groups = htd::ceil_div((int64_t)B * A, 16);
    hipLaunchKernelGGL(retina_keys_kernel, dim3((unsigned)(groups < FOCAL_BLOCKS ? groups : FOCAL_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, lv, L, B, na, C, (int)A, keys);
    return htd::check_launch("retina_keys");
}
