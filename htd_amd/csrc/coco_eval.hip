// COCO detection evaluation on the device (gfx950): the per-(category, image) greedy matching and the per-category
// accumulation of pycocotools' COCOeval (evaluateImg / accumulate, as driven by CocoDataset.evaluate,
// datasets/coco.py:363-545), and the greedy recall assignment of eval_recalls (core/evaluation/recall.py:_recalls).
//
// Compiled with -ffp-contract=off: every IoU, precision and recall is the exact IEEE expression of the host code
// (double for COCOeval, float32 for bbox_overlaps), so each comparison against a threshold takes the same branch.
#include "common.h"

namespace {

constexpr int kMatchThreads = 64;                // one wavefront per (category, image) pair
constexpr int kIouCache = 2048;                  // doubles of the pair's D x G IoU matrix kept in LDS (16 KiB)
constexpr int kGtmLds = 4096;                    // bytes of "ground truth already matched" flags kept in LDS
constexpr int kAccThreads = 256;
constexpr int kRecallThreads = 256;
constexpr int kRecallFlagsLds = 16384;

// maskApi.c bbIou: xywh boxes, crowd ground truths measured against the detection's area only
__device__ __forceinline__ double coco_iou(const double *d, const double *g, bool crowd)
{
    const double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
    if (w <= 0.0) return 0.0;
    const double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double da = d[2] * d[3];
    const double u = crowd ? da : da + g[2] * g[3] - i;
    return i / u;
}

struct MatchParams {
    const double *gt_box, *gt_area;
    const uint8_t *gt_crowd;
    const int64_t *gt_id;
    const double *dt_box;
    const int64_t *pair_gt, *pair_dt;
    const double *area_rng, *iou_thrs;
    int A, T;
    uint8_t *dt_flags;
    int32_t *npig;
    uint8_t *gtm_ws;
};

__global__ __launch_bounds__(kMatchThreads) void coco_match_kernel(MatchParams p)
{
    __shared__ double s_iou[kIouCache];
    __shared__ uint8_t s_gtm[kGtmLds];
    const int pair = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t g0 = p.pair_gt[pair], d0 = p.pair_dt[pair];
    const int G = (int)(p.pair_gt[pair + 1] - g0), D = (int)(p.pair_dt[pair + 1] - d0);
    const int AT = p.A * p.T;
    const double *gb = p.gt_box + g0 * 4, *db = p.dt_box + d0 * 4;
    const double *ga = p.gt_area + g0;
    const uint8_t *gc = p.gt_crowd + g0;

    // non-ignored ground truths per area range (accumulate's npig)
    for (int a = 0; a < p.A; ++a) {
        const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
        float n = 0.f;
        for (int g = lane; g < G; g += kMatchThreads) n += (!gc[g] && !(ga[g] < lo || ga[g] > hi)) ? 1.f : 0.f;
        n = htd::wave_sum(n);
        if (lane == 0) p.npig[(int64_t)pair * p.A + a] = (int32_t)n;
    }

    const bool cached = (int64_t)D * G <= kIouCache;
    if (cached)
        for (int e = lane; e < D * G; e += kMatchThreads) {
            const int d = e / G, g = e - d * G;
            s_iou[e] = coco_iou(db + 4 * d, gb + 4 * g, gc[g] != 0);
        }
    uint8_t *gtm = (int64_t)AT * G <= kGtmLds ? s_gtm : p.gtm_ws + g0 * AT;
    for (int e = lane; e < AT * G; e += kMatchThreads) gtm[e] = 0;
    __syncthreads();

    for (int s = lane; s < AT; s += kMatchThreads) {
        const int a = s / p.T, t = s - a * p.T;
        const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
        const double thr = fmin(p.iou_thrs[t], 1.0 - 1e-10);
        uint8_t *my = gtm + (int64_t)s * G;
        for (int d = 0; d < D; ++d) {
            double best = thr;
            int m = -1;
            // ground truths in COCOeval's order: the area range's non-ignored ones first, then the ignored ones, each
            // in their original order.  A detection holding a non-ignored match never reaches the ignored ones.
            for (int pass = 0; pass < 2 && !(pass == 1 && m >= 0); ++pass)
                for (int g = 0; g < G; ++g) {
                    const bool crowd = gc[g] != 0;
                    const int ig = (crowd || ga[g] < lo || ga[g] > hi) ? 1 : 0;
                    if (ig != pass) continue;
                    if (my[g] && !crowd) continue;
                    const double v = cached ? s_iou[d * G + g] : coco_iou(db + 4 * d, gb + 4 * g, crowd);
                    if (v < best) continue;
                    best = v;
                    m = g;
                }
            int matched = 0, ignored = 0;
            if (m >= 0) {
                const double am = ga[m];
                ignored = (gc[m] || am < lo || am > hi) ? 1 : 0;
                matched = p.gt_id[g0 + m] != 0;            // dtMatches holds the ground truth's id
                my[m] = 1;
            }
            if (!matched) {
                const double area = db[4 * d + 2] * db[4 * d + 3];
                if (area < lo || area > hi) ignored = 1;
            }
            p.dt_flags[(d0 + d) * AT + s] = (uint8_t)(matched | (ignored << 1));
        }
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

struct AccEntry {
    double pr;
    int32_t tp;
    int32_t src;
};

struct AccParams {
    const uint8_t *dt_flags;
    const int64_t *order;
    const int32_t *dt_rank;
    const double *dt_score;
    const int64_t *cat_dt, *cat_pair;
    const int32_t *npig;
    const int32_t *max_dets;
    const double *rec_thrs;
    int K, A, M, T, R;
    double *precision, *recall, *scores;
    AccEntry *ws;
};

__global__ __launch_bounds__(kAccThreads) void coco_accumulate_kernel(AccParams p)
{
    __shared__ int s_red_i[4];
    __shared__ double s_red_d[4];
    __shared__ int s_npig;
    const int m = blockIdx.x % p.M, a = (blockIdx.x / p.M) % p.A, k = blockIdx.x / (p.M * p.A);
    const int tid = threadIdx.x;
    const int64_t e0 = p.cat_dt[k], N = p.cat_dt[k + 1] - e0;
    const int max_det = p.max_dets[m];
    AccEntry *ws = p.ws + e0 * p.A * p.M + (int64_t)(a * p.M + m) * N;

    int n = 0;
    for (int64_t q = p.cat_pair[k] + tid; q < p.cat_pair[k + 1]; q += kAccThreads) n += p.npig[q * p.A + a];
    n = block_scan(n, [](int x, int y) { return x + y; }, s_red_i, false);
    if (tid == kAccThreads - 1) s_npig = n;
    __syncthreads();
    const int npig = s_npig;
    const int AT = p.A * p.T;
    const int64_t KAM = (int64_t)p.K * p.A * p.M;

    for (int t = 0; t < p.T; ++t) {
        const int64_t pr_base = (int64_t)t * p.R * KAM + (int64_t)k * p.A * p.M + a * p.M + m;   // + r * KAM
        if (npig == 0) {                                                   // stays -1, as pycocotools leaves it
            for (int r = tid; r < p.R; r += kAccThreads) {
                p.precision[pr_base + r * KAM] = -1.0;
                p.scores[pr_base + r * KAM] = -1.0;
            }
            if (tid == 0) p.recall[(int64_t)t * KAM + (int64_t)k * p.A * p.M + a * p.M + m] = -1.0;
            continue;
        }
        // cumulative TP / FP over the category's detections in score order (each image cut to maxDet), compacted
        int c_n = 0, c_tp = 0, c_fp = 0;
        for (int64_t i0 = 0; i0 < N; i0 += kAccThreads) {
            const int64_t i = i0 + tid;
            int in = 0, tp = 0, fp = 0;
            int64_t src = 0;
            if (i < N) {
                src = p.order[e0 + i];
                in = p.dt_rank[src] < max_det;
                const uint8_t f = p.dt_flags[src * AT + a * p.T + t];
                const int matched = f & 1, ign = (f >> 1) & 1;
                tp = in && matched && !ign;
                fp = in && !matched && !ign;
            }
            const int pos = block_scan(in, [](int x, int y) { return x + y; }, s_red_i, false);
            const int tps = block_scan(tp, [](int x, int y) { return x + y; }, s_red_i, false);
            const int fps = block_scan(fp, [](int x, int y) { return x + y; }, s_red_i, false);
            if (in) {
                const double dtp = (double)(c_tp + tps), dfp = (double)(c_fp + fps);
                AccEntry ent;
                ent.pr = dtp / (dfp + dtp + 0x1p-52);                 // np.spacing(1)
                ent.tp = c_tp + tps;
                ent.src = (int32_t)src;
                ws[c_n + pos - 1] = ent;
            }
            __syncthreads();
            if (tid == kAccThreads - 1) { s_red_i[0] = pos; s_red_i[1] = tps; s_red_i[2] = fps; }
            __syncthreads();
            c_n += s_red_i[0];
            c_tp += s_red_i[1];
            c_fp += s_red_i[2];
            __syncthreads();
        }
        const int nd = c_n;
        __syncthreads();
        // precision envelope: running maximum from the right
        double carry = -1.0;
        for (int j0 = nd - kAccThreads; j0 > -kAccThreads; j0 -= kAccThreads) {
            const int j = j0 + tid;
            double v = j >= 0 ? ws[j].pr : -1.0;
            v = fmax(block_scan(v, [](double x, double y) { return fmax(x, y); }, s_red_d, true), carry);
            if (j >= 0) ws[j].pr = v;
            __syncthreads();
            if (tid == 0) s_red_d[0] = v;
            __syncthreads();
            carry = s_red_d[0];
            __syncthreads();
        }
        // precision at each recall threshold: first position whose recall reaches it (searchsorted, side='left')
        for (int r = tid; r < p.R; r += kAccThreads) {
            const double thr = p.rec_thrs[r];
            int lo = 0, hi = nd;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((double)ws[mid].tp / (double)npig < thr) lo = mid + 1;
                else hi = mid;
            }
            double q = 0.0, ss = 0.0;
            if (lo < nd) {
                q = ws[lo].pr;
                ss = p.dt_score[ws[lo].src];
            }
            p.precision[pr_base + r * KAM] = q;
            p.scores[pr_base + r * KAM] = ss;
        }
        if (tid == 0)
            p.recall[(int64_t)t * KAM + (int64_t)k * p.A * p.M + a * p.M + m] =
                nd ? (double)ws[nd - 1].tp / (double)npig : 0.0;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------- eval_recalls
__device__ __forceinline__ float overlap_f32(float4 g, float4 b)
{
    // core/evaluation/bbox_overlaps.py, mode 'iou', eps = 1e-6
    const float ga = (g.z - g.x) * (g.w - g.y);
    const float ba = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(g.z, b.z) - fmaxf(g.x, b.x), 0.f);
    const float h = fmaxf(fminf(g.w, b.w) - fmaxf(g.y, b.y), 0.f);
    const float ov = w * h;
    const float un = fmaxf(ga + ba - ov, 1e-6f);
    return ov / un;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(v, o, 64);
        v = y > v ? y : v;
    }
    return v;
}

struct RecallParams {
    const float *gts, *props;
    const int64_t *gt_off, *prop_off;
    const int32_t *prop_nums;
    int64_t n_gt, n_prop;
    float *gt_ious;
    uint8_t *flags_ws;
};

__global__ __launch_bounds__(kRecallThreads) void eval_recalls_kernel(RecallParams p)
{
    __shared__ uint8_t s_flags[kRecallFlagsLds];
    __shared__ unsigned long long s_red[4];
    const int img = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int64_t g0 = p.gt_off[img], p0 = p.prop_off[img];
    const int G = (int)(p.gt_off[img + 1] - g0);
    const int P = min((int)(p.prop_off[img + 1] - p0), p.prop_nums[k]);
    float *out = p.gt_ious + (int64_t)k * p.n_gt + g0;
    if (G == 0) return;
    if (P == 0) {
        for (int j = tid; j < G; j += kRecallThreads) out[j] = 0.f;
        return;
    }
    uint8_t *row_done = G + P <= kRecallFlagsLds ? s_flags : p.flags_ws + (int64_t)k * (p.n_gt + p.n_prop) + g0 + p0;
    uint8_t *col_done = row_done + G;
    for (int e = tid; e < G + P; e += kRecallThreads) row_done[e] = 0;
    __syncthreads();
    const float4 *gb = reinterpret_cast<const float4 *>(p.gts) + g0;
    const float4 *pb = reinterpret_cast<const float4 *>(p.props) + p0;
    const unsigned n = (unsigned)G * (unsigned)P;
    for (int j = 0; j < G; ++j) {
        // the largest IoU left, first row then first column on ties: key = (iou bits, ~(row * P + col))
        unsigned long long key = 0;
        for (unsigned e = tid; e < n; e += kRecallThreads) {
            const unsigned r = e / (unsigned)P, c = e - r * (unsigned)P;
            if (row_done[r] || col_done[c]) continue;
            const float v = overlap_f32(gb[r], pb[c]) + 0.f;   // -0 -> +0: ties with 0 go by index, as in argmax
            const unsigned long long kk = ((unsigned long long)__float_as_uint(v) << 32) | (0xffffffffu - e);
            key = kk > key ? kk : key;
        }
        key = wave_max_u64(key);
        if ((tid & 63) == 0) s_red[tid >> 6] = key;
        __syncthreads();
        unsigned long long best = s_red[0];
        for (int w = 1; w < 4; ++w) best = s_red[w] > best ? s_red[w] : best;
        __syncthreads();
        if (best == 0) {                                   // every row or every column used: the rest stay -1
            for (int i = j + tid; i < G; i += kRecallThreads) out[i] = -1.f;
            return;
        }
        if (tid == 0) {
            const unsigned e = 0xffffffffu - (unsigned)(best & 0xffffffffu);
            const unsigned r = e / (unsigned)P, c = e - r * (unsigned)P;
            out[j] = __uint_as_float((unsigned)(best >> 32));
            row_done[r] = 1;
            col_done[c] = 1;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int64_t htd_coco_match_workspace_bytes(int64_t n_gt, int A, int T)
{
    return n_gt * (int64_t)A * T + 16;
}

extern "C" int htd_coco_match(const double *gt_box, const double *gt_area, const uint8_t *gt_crowd, const int64_t *gt_id,
                              const double *dt_box, const int64_t *pair_gt, const int64_t *pair_dt, int P,
                              const double *area_rng, int A, const double *iou_thrs, int T, uint8_t *dt_flags,
                              int32_t *npig, void *workspace, void *stream)
{
    HTD_REQUIRE(P >= 0 && A > 0 && T > 0, "htd_coco_match: P=%d A=%d T=%d", P, A, T);
    HTD_REQUIRE(pair_gt && pair_dt && area_rng && iou_thrs && npig, "htd_coco_match: null pointer");
    if (P == 0) return HTD_OK;
    MatchParams p{gt_box, gt_area, gt_crowd, gt_id, dt_box, pair_gt, pair_dt, area_rng, iou_thrs,
                  A, T, dt_flags, npig, (uint8_t *)workspace};
    hipLaunchKernelGGL(coco_match_kernel, dim3(P), dim3(kMatchThreads), 0, (hipStream_t)stream, p);
    return htd::check_launch("htd_coco_match");
}

extern "C" int64_t htd_coco_accumulate_workspace_bytes(int64_t n_dt, int A, int M)
{
    return n_dt * (int64_t)A * M * (int64_t)sizeof(AccEntry) + 16;
}

extern "C" int htd_coco_accumulate(const uint8_t *dt_flags, const int64_t *order, const int32_t *dt_rank,
                                   const double *dt_score, const int64_t *cat_dt, const int64_t *cat_pair,
                                   const int32_t *npig, int K, int A, const int32_t *max_dets, int M, int T,
                                   const double *rec_thrs, int R, double *precision, double *recall, double *scores,
                                   void *workspace, void *stream)
{
    HTD_REQUIRE(K > 0 && A > 0 && M > 0 && T > 0 && R > 0, "htd_coco_accumulate: K=%d A=%d M=%d T=%d R=%d", K, A, M, T, R);
    HTD_REQUIRE(cat_dt && cat_pair && max_dets && rec_thrs && precision && recall && scores && workspace,
                "htd_coco_accumulate: null pointer");
    AccParams p{dt_flags, order, dt_rank, dt_score, cat_dt, cat_pair, npig, max_dets, rec_thrs,
                K, A, M, T, R, precision, recall, scores, (AccEntry *)workspace};
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3(K * A * M), dim3(kAccThreads), 0, (hipStream_t)stream, p);
    return htd::check_launch("htd_coco_accumulate");
}

extern "C" int64_t htd_eval_recalls_workspace_bytes(int64_t n_gt, int64_t n_prop, int n_nums)
{
    return (n_gt + n_prop) * (int64_t)n_nums + 16;
}

extern "C" int htd_eval_recalls(const float *gts, const int64_t *gt_off, const float *props, const int64_t *prop_off,
                                int n_img, int64_t n_gt, int64_t n_prop, const int32_t *prop_nums, int n_nums,
                                float *gt_ious, void *workspace, void *stream)
{
    HTD_REQUIRE(n_img >= 0 && n_nums > 0, "htd_eval_recalls: n_img=%d n_nums=%d", n_img, n_nums);
    HTD_REQUIRE(n_gt < (1ll << 31) && n_prop < (1ll << 31), "htd_eval_recalls: too many boxes");
    HTD_REQUIRE(gt_off && prop_off && prop_nums && workspace, "htd_eval_recalls: null pointer");
    if (n_img == 0 || n_gt == 0) return HTD_OK;
    RecallParams p{gts, props, gt_off, prop_off, prop_nums, n_gt, n_prop, gt_ious, (uint8_t *)workspace};
    hipLaunchKernelGGL(eval_recalls_kernel, dim3(n_img, n_nums), dim3(kRecallThreads), 0, (hipStream_t)stream, p);
    return htd::check_launch("htd_eval_recalls");
}
