// Pascal VOC mean AP on the device (gfx950): the per-(class, image) TP / FP assignment of tpfp_default and the
// per-class precision / recall accumulation of eval_map and average_precision (core/evaluation/mean_ap.py).
//
// Compiled with -ffp-contract=off: IoUs, areas, recalls, precisions and the 'area' terms are the exact IEEE
// expressions of the host code (float32 bbox_overlaps; float64 recall; float32 precision), so every comparison takes
// the same branch and every value has the same bits.
//
// tpfp_default never un-matches a ground truth: a detection whose IoU maximum reaches iou_thr on a non-ignored,
// in-range ground truth g is a TP exactly when no better-ranked detection of the same image and class has its first
// argmax on g with the maximum reaching iou_thr.  The assignment is therefore data-parallel: no greedy loop, no float
// atomics.
#include "common.h"

namespace {

constexpr int kTpfpThreads = 64;                 // one wavefront per (class, image) pair
constexpr int kAccThreads = 256;                 // one workgroup per (class, scale range)
constexpr int kPoints = 11;                      // the VOC07 11-point recall thresholds

__device__ __forceinline__ float box_area(const float *b)
{
    return (b[2] - b[0]) * (b[3] - b[1]);
}

// core/evaluation/bbox_overlaps.py, mode 'iou', eps = 1e-6 (float32; the expression is symmetric in its operands)
__device__ __forceinline__ float voc_iou(const float *d, float da, const float *g)
{
    const float ga = box_area(g);
    const float w = fmaxf(fminf(d[2], g[2]) - fmaxf(d[0], g[0]), 0.f);
    const float h = fmaxf(fminf(d[3], g[3]) - fmaxf(d[1], g[1]), 0.f);
    const float ov = w * h;
    const float un = fmaxf(da + ga - ov, 1e-6f);
    return ov / un;
}

__device__ __forceinline__ bool in_range(float area, const float *rng, int s)
{
    return !rng || (area >= rng[2 * s] && area < rng[2 * s + 1]);
}

struct TpfpParams {
    const float *dets;                           // [n_det][5] grouped by pair
    const int64_t *det_off;                      // [P+1]
    const float *gts;                            // [n_gt][4] grouped by pair: non-ignored, then ignored
    const int64_t *gt_off;                       // [P+1]
    const int32_t *n_keep;                       // [P] non-ignored ground truths of the pair
    const float *area_rng;                       // [S][2] (lo, hi) or null
    int S;
    float iou_thr;
    uint8_t *flags;                              // [n_det][S] bit 0 = TP, bit 1 = FP
    int32_t *num_gts;                            // [P][S]
    int32_t *cand;                               // [n_det] workspace
};

__global__ __launch_bounds__(kTpfpThreads) void voc_tpfp_kernel(TpfpParams p)
{
    const int pair = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t d0 = p.det_off[pair], g0 = p.gt_off[pair];
    const int D = (int)(p.det_off[pair + 1] - d0), G = (int)(p.gt_off[pair + 1] - g0);
    const int K = p.n_keep[pair];
    const float *db = p.dets + d0 * 5, *gb = p.gts + g0 * 4;

    // eval_map's num_gts: the pair's non-ignored ground truths inside each area range
    for (int s = 0; s < p.S; ++s) {
        float n = 0.f;
        for (int g = lane; g < K; g += kTpfpThreads) n += in_range(box_area(gb + 4 * g), p.area_rng, s) ? 1.f : 0.f;
        n = htd::wave_sum(n);
        if (lane == 0) p.num_gts[(int64_t)pair * p.S + s] = (int32_t)n;
    }
    if (D == 0) return;

    // every detection's IoU maximum and first argmax over all G ground truths; a candidate when the maximum reaches
    // iou_thr (NEP 50: the float32 maximum against the threshold as float32)
    int32_t *cand = p.cand + d0;
    for (int d = lane; d < D; d += kTpfpThreads) {
        const float *b = db + 5 * d;
        const float da = box_area(b);
        float best = 0.f;
        int m = -1;
        for (int g = 0; g < G; ++g) {
            const float v = voc_iou(b, da, gb + 4 * g);
            if (m < 0 || v > best) {
                best = v;
                m = g;
            }
        }
        cand[d] = (m >= 0 && best >= p.iou_thr) ? m : -1;
    }
    __syncthreads();

    for (int d = lane; d < D; d += kTpfpThreads) {
        const float *b = db + 5 * d;
        const int m = cand[d];
        uint8_t *out = p.flags + (d0 + d) * p.S;
        if (m < 0) {                                       // below the threshold (or no ground truth at all)
            const float da = box_area(b);
            for (int s = 0; s < p.S; ++s) out[s] = in_range(da, p.area_rng, s) ? 2 : 0;
            continue;
        }
        if (m >= K) {                                      // an ignored ground truth: neither TP nor FP
            for (int s = 0; s < p.S; ++s) out[s] = 0;
            continue;
        }
        // first in score order (ties: row order) among the detections whose candidate is m
        const float sc = b[4];
        bool first = true;
        for (int e = 0; e < D && first; ++e) {
            if (e == d || cand[e] != m) continue;
            const float se = db[5 * e + 4];
            if (se > sc || (se == sc && e < d)) first = false;
        }
        const float ga = box_area(gb + 4 * m);
        for (int s = 0; s < p.S; ++s) out[s] = in_range(ga, p.area_rng, s) ? (first ? 1 : 2) : 0;
    }
}

// ------------------------------------------------------------------------------------------- accumulate
template <typename V, typename Op>
__device__ __forceinline__ V block_scan(V v, Op op, V *red, bool reverse)
{
    // inclusive scan over the 256 threads of the block (reverse: from the last thread down)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    V x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V y = __shfl(x, reverse ? min(lane + o, 63) : max(lane - o, 0), 64);
        if (reverse ? lane + o < 64 : lane >= o) x = op(x, y);
    }
    __syncthreads();
    if (lane == (reverse ? 0 : 63)) red[w] = x;
    __syncthreads();
    if (!reverse) {
        for (int i = 0; i < w; ++i) x = op(red[i], x);
    } else {
        for (int i = 3; i > w; --i) x = op(x, red[i]);
    }
    return x;
}

struct AccParams {
    const uint8_t *flags;                        // [n_det][S]
    const int64_t *order;                        // [n_det] class-grouped, score descending
    const int64_t *cls_off;                      // [K+1]
    const int32_t *num_gts;                      // [K * I][S]
    const double *thr11;                         // [11]
    int K, I, S;
    int64_t n_det;
    double *recall;                              // [S][n_det]
    float *precision;                            // [S][n_det]
    double *terms;                               // [S][n_det + K]
    int32_t *n_terms;                            // [K][S]
    int32_t *gts_out;                            // [K][S]
    float *ap11;                                 // [K][S]
    double *env;                                 // [S][n_det] workspace
};

__global__ __launch_bounds__(kAccThreads) void voc_accumulate_kernel(AccParams p)
{
    __shared__ int s_red_i[4];
    __shared__ double s_red_d[4];
    __shared__ int s_n;
    __shared__ float s_pt[kPoints];
    const int s = blockIdx.x % p.S, c = blockIdx.x / p.S;
    const int tid = threadIdx.x;
    const int64_t e0 = p.cls_off[c];
    const int64_t N = p.cls_off[c + 1] - e0;

    int n = 0;
    for (int64_t q = (int64_t)c * p.I + tid; q < (int64_t)(c + 1) * p.I; q += kAccThreads) n += p.num_gts[q * p.S + s];
    n = block_scan(n, [](int x, int y) { return x + y; }, s_red_i, false);
    if (tid == kAccThreads - 1) s_n = n;
    __syncthreads();
    const int ngt = s_n;
    const double denom = fmax((double)ngt, (double)__FLT_EPSILON__);       // np.maximum(num_gts, eps) in float64
    double *rec = p.recall + (int64_t)s * p.n_det + e0;
    float *prec = p.precision + (int64_t)s * p.n_det + e0;
    double *env = p.env + (int64_t)s * p.n_det + e0;

    // cumulative TP / FP in score order -> recall (float64) and precision (float32)
    int c_tp = 0, c_fp = 0;
    for (int64_t i0 = 0; i0 < N; i0 += kAccThreads) {
        const int64_t i = i0 + tid;
        int tp = 0, fp = 0;
        if (i < N) {
            const uint8_t f = p.flags[p.order[e0 + i] * p.S + s];
            tp = f & 1;
            fp = (f >> 1) & 1;
        }
        const int tps = c_tp + block_scan(tp, [](int x, int y) { return x + y; }, s_red_i, false);
        const int fps = c_fp + block_scan(fp, [](int x, int y) { return x + y; }, s_red_i, false);
        if (i < N) {
            const float ftp = (float)tps, ffp = (float)fps;
            const float pr = ftp / fmaxf(ftp + ffp, __FLT_EPSILON__);
            rec[i] = (double)ftp / denom;
            prec[i] = pr;
            env[i] = (double)pr;
        }
        __syncthreads();
        if (tid == kAccThreads - 1) { s_red_i[0] = tps; s_red_i[1] = fps; }
        __syncthreads();
        c_tp = s_red_i[0];
        c_fp = s_red_i[1];
        __syncthreads();
    }

    // precision envelope: running maximum from the right, starting from the appended 0
    double carry = 0.0;
    for (int64_t j0 = N - kAccThreads; j0 > -kAccThreads; j0 -= kAccThreads) {
        const int64_t j = j0 + tid;
        double v = j >= 0 ? env[j] : 0.0;
        v = fmax(block_scan(v, [](double x, double y) { return fmax(x, y); }, s_red_d, true), carry);
        if (j >= 0) env[j] = v;
        __syncthreads();
        if (tid == 0) s_red_d[0] = v;
        __syncthreads();
        carry = s_red_d[0];
        __syncthreads();
    }

    // 'area' terms: with mrec = [0, rec, 1] and mpre = [0, env, 0], (mrec[j+1] - mrec[j]) * mpre[j+1] for every
    // j = 0..N where mrec changes, compacted in order
    double *terms = p.terms + (int64_t)s * (p.n_det + p.K) + e0 + c;
    int c_n = 0;
    for (int64_t j0 = 0; j0 <= N; j0 += kAccThreads) {
        const int64_t j = j0 + tid;
        int keep = 0;
        double t = 0.0;
        if (j <= N) {
            const double lo = j == 0 ? 0.0 : rec[j - 1];
            const double hi = j == N ? 1.0 : rec[j];
            const double mp = j == N ? 0.0 : env[j];
            keep = hi != lo;
            t = (hi - lo) * mp;
        }
        const int pos = block_scan(keep, [](int x, int y) { return x + y; }, s_red_i, false);
        if (keep) terms[c_n + pos - 1] = t;
        __syncthreads();
        if (tid == kAccThreads - 1) s_red_i[0] = pos;
        __syncthreads();
        c_n += s_red_i[0];
        __syncthreads();
    }

    // '11points': the largest precision at recall >= thr (the envelope at the first such position), summed in
    // float32 in threshold order
    if (tid < kPoints) {
        const double thr = p.thr11[tid];
        int64_t lo = 0, hi = N;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (rec[mid] >= thr) hi = mid;
            else lo = mid + 1;
        }
        s_pt[tid] = lo < N ? (float)env[lo] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        float ap = 0.f;
        for (int t = 0; t < kPoints; ++t) ap += s_pt[t];
        // mean_ap.py divides the whole `ap` array by 11 inside its loop over scales: scale s is divided S - s times
        for (int k = s; k < p.S; ++k) ap /= 11.f;
        p.ap11[c * p.S + s] = ap;
        p.n_terms[c * p.S + s] = c_n;
        p.gts_out[c * p.S + s] = ngt;
    }
}

}  // namespace

extern "C" int64_t htd_voc_tpfp_workspace_bytes(int64_t n_det)
{
    return n_det * (int64_t)sizeof(int32_t) + 16;
}

extern "C" int htd_voc_tpfp(const float *dets, const int64_t *det_off, const float *gts, const int64_t *gt_off,
                            const int32_t *n_keep, int P, const float *area_rng, int S, float iou_thr, uint8_t *flags,
                            int32_t *num_gts, void *workspace, void *stream)
{
    HTD_REQUIRE(P >= 0 && S > 0, "htd_voc_tpfp: P=%d S=%d", P, S);
    HTD_REQUIRE(det_off && gt_off && n_keep && num_gts && workspace, "htd_voc_tpfp: null pointer");
    if (P == 0) return HTD_OK;
    TpfpParams p{dets, det_off, gts, gt_off, n_keep, area_rng, S, iou_thr, flags, num_gts, (int32_t *)workspace};
    hipLaunchKernelGGL(voc_tpfp_kernel, dim3(P), dim3(kTpfpThreads), 0, (hipStream_t)stream, p);
    return htd::check_launch("htd_voc_tpfp");
}

extern "C" int64_t htd_voc_accumulate_workspace_bytes(int64_t n_det, int S)
{
    return n_det * (int64_t)S * (int64_t)sizeof(double) + 16;
}

extern "C" int htd_voc_accumulate(const uint8_t *flags, const int64_t *order, const int64_t *cls_off,
                                  const int32_t *num_gts, int K, int I, int S, int64_t n_det, const double *thr11,
                                  double *recall, float *precision, double *terms, int32_t *n_terms, int32_t *gts_out,
                                  float *ap11, void *workspace, void *stream)
{
    HTD_REQUIRE(K > 0 && I > 0 && S > 0 && n_det >= 0, "htd_voc_accumulate: K=%d I=%d S=%d", K, I, S);
    HTD_REQUIRE(n_det < (1ll << 24), "htd_voc_accumulate: %lld detections; float32 counts are exact below 2^24",
                (long long)n_det);
    HTD_REQUIRE(cls_off && num_gts && thr11 && n_terms && gts_out && ap11 && workspace,
                "htd_voc_accumulate: null pointer");
    AccParams p{flags, order, cls_off, num_gts, thr11, K, I, S, n_det, recall, precision, terms, n_terms, gts_out,
                ap11, (double *)workspace};
    hipLaunchKernelGGL(voc_accumulate_kernel, dim3(K * S), dim3(kAccThreads), 0, (hipStream_t)stream, p);
    return htd::check_launch("htd_voc_accumulate");
}
