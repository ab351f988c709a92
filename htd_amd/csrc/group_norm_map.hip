// Whole-map GroupNorm (+ residual, + ReLU) and weight standardisation, fp32, NHWC / KRSC (gfx950).
//
// The RoI-tile kernels of roi_ops.hip give a sample ONE workgroup and a thread all P positions of its channel: right for
// thousands of 7x7 tiles, 4 workgroups on a 4-image backbone map.  Here a sample is cut into position slabs (at most kMaxSlabs
// of them, htd_group_norm_map_slab) and every launch is an ordinary grid over (slab, sample):
//
//   forward   gn_map_stats_kernel   per slab and group (count, mean, M2) -> workspace
//             gn_map_norm_kernel    merges the slabs of its sample in a fixed order, y = [relu](x * ga + be [+ residual])
//   backward  gn_map_bwd_sums_kernel  per slab and channel sum d, sum d * xhat (the rows colsum_rows_kernel adds up for
//                                     ggamma / gbeta) and, per slab and group, the gamma-weighted sums gx needs
//             gn_map_bwd_gx_kernel  adds the group sums of its sample's slabs in a fixed order, writes gx (and the residual's
//                                   gradient, the masked gy)
//             colsum_rows_kernel    ggamma, gbeta
//
// No grid barrier, no flag, no float atomic: two runs give the same bits.  A thread is (four adjacent channels, every R-th
// position): 16-byte loads and stores that run through the slab's contiguous [positions][C] block, kPos positions (32 values)
// in registers at a time.  Traffic: forward 2 reads + 1 write of the map (+ the residual), backward 2 x (x, y, gy) reads + 1
// write (+ the residual's gradient); the workspace is a few hundred KB and stays in the L2.
//
// Statistics: a thread takes the <= 32 values it holds in two passes in registers (pairwise sum -> mean, then squared
// deviations) and the (count, mean, M2) triples are merged by Chan's formula: over a thread's passes, over the group's lanes
// (shuffle tree), over the row groups (LDS), over the slabs (two levels).  A large common offset costs nothing: no E[x^2].
#include "common.h"

namespace htd {
void launch_colsum_rows(const float *ws, float *out0, float *out1, int n, int rows, hipStream_t s);      // roi_ops.hip
}

namespace {

constexpr int kThreads = 256;
constexpr int kPos = 8;            // positions a thread holds per pass
constexpr int kMaxSlabs = 128;     // per sample: what the second launch of a pair merges per group
constexpr int kMaxG = 1024;        // C <= 2048, cpg >= 2

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

struct Stat { float n, m, q; };    // count, mean, sum of squared deviations

// a <- a merged with b (Chan et al.); an empty side (n = 0, m = 0) leaves the other unchanged
__device__ __forceinline__ void chan(Stat &a, const Stat b)
{
    const float n = a.n + b.n;
    const float f = n > 0.f ? b.n / n : 0.f;
    const float d = b.m - a.m;
    a.m = a.m + d * f;
    a.q = a.q + b.q + d * d * a.n * f;
    a.n = n;
}

// (count, mean, M2) of the lo (x, y) and hi (z, w) halves of the kPos float4 a thread holds; in[k]: position k is inside the slab
__device__ __forceinline__ void stat8(const float4 (&v)[kPos], const bool (&in)[kPos], Stat &lo, Stat &hi)
{
    float tl[kPos], th[kPos], cnt = 0.f;
#pragma unroll
    for (int k = 0; k < kPos; ++k) {
        tl[k] = in[k] ? v[k].x + v[k].y : 0.f;
        th[k] = in[k] ? v[k].z + v[k].w : 0.f;
        cnt += in[k] ? 2.f : 0.f;
    }
    const float sl = ((tl[0] + tl[1]) + (tl[2] + tl[3])) + ((tl[4] + tl[5]) + (tl[6] + tl[7]));
    const float sh = ((th[0] + th[1]) + (th[2] + th[3])) + ((th[4] + th[5]) + (th[6] + th[7]));
    const float ml = cnt > 0.f ? sl / cnt : 0.f, mh = cnt > 0.f ? sh / cnt : 0.f;     // equal values: their mean exactly
    float ql = 0.f, qh = 0.f;
#pragma unroll
    for (int k = 0; k < kPos; ++k)
        if (in[k]) {
            const float a = v[k].x - ml, b = v[k].y - ml, c = v[k].z - mh, d = v[k].w - mh;
            ql += a * a + b * b;
            qh += c * c + d * d;
        }
    lo = Stat{cnt, ml, ql};
    hi = Stat{cnt, mh, qh};
}

// Geometry shared by the four kernels: C4 float4 columns, taken CW <= 256 at a time by R = 256 / CW row groups.
struct Geo {
    int C4, CW, R, cpg, lanes;     // lanes: adjacent float4 columns of one group (1 at cpg = 2 and 4)
    int tid, r, cl;
    bool live;                     // this thread has a row group (CW * R may be below 256)
};
__device__ __forceinline__ Geo geometry(int C, int G)
{
    Geo g;
    g.C4 = C >> 2;
    g.CW = g.C4 < kThreads ? g.C4 : kThreads;
    g.R = kThreads / g.CW;
    g.cpg = C / G;
    g.lanes = g.cpg >= 4 ? g.cpg >> 2 : 1;
    g.tid = threadIdx.x;
    g.r = g.tid / g.CW;
    g.cl = g.tid - g.r * g.CW;
    g.live = g.r < g.R;
    return g;
}

__global__ __launch_bounds__(kThreads) void gn_map_stats_kernel(const float *__restrict__ x, float4 *__restrict__ part, int P,
                                                                int C, int G, int S, int nslab)
{
    __shared__ float rn[512], rm[512], rq[512];
    const Geo e = geometry(C, G);
    const int slab = blockIdx.x;
    const int64_t i = blockIdx.y;
    const int p0 = slab * S, p1 = min(P, p0 + S);
    const float *xs = x + i * P * C;
    const int GW = e.cpg >= 4 ? e.CW / e.lanes : 2 * e.CW;         // groups per column pass
    for (int c0 = 0; c0 < e.C4; c0 += e.CW) {
        const int c4 = c0 + e.cl;
        const bool ok = e.live && c4 < e.C4;
        Stat lo{0.f, 0.f, 0.f}, hi{0.f, 0.f, 0.f};
        for (int pb = p0; pb < p1; pb += kPos * e.R) {
            float4 v[kPos];
            bool in[kPos];
#pragma unroll
            for (int k = 0; k < kPos; ++k) {
                const int p = pb + e.r + k * e.R;
                in[k] = ok && p < p1;
                v[k] = in[k] ? ld4(xs + ((int64_t)p * e.C4 + c4) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            Stat a, b;
            stat8(v, in, a, b);
            chan(lo, a);
            chan(hi, b);
        }
        if (e.cpg >= 4) {              // the float4 lies in one group; then the group's adjacent lanes, as a tree
            chan(lo, hi);
            for (int o = 1; o < e.lanes; o <<= 1) {
                Stat b;
                b.n = __shfl_down(lo.n, o, 64);
                b.m = __shfl_down(lo.m, o, 64);
                b.q = __shfl_down(lo.q, o, 64);
                chan(lo, b);
            }
            if (e.live && e.cl % e.lanes == 0) {
                const int k = e.r * GW + e.cl / e.lanes;
                rn[k] = lo.n; rm[k] = lo.m; rq[k] = lo.q;
            }
        } else if (e.live) {           // cpg = 2: the float4 spans two groups
            const int k = e.r * GW + 2 * e.cl;
            rn[k] = lo.n; rm[k] = lo.m; rq[k] = lo.q;
            rn[k + 1] = hi.n; rm[k + 1] = hi.m; rq[k + 1] = hi.q;
        }
        __syncthreads();
        for (int t = e.tid; t < GW; t += kThreads) {               // the row groups, in order
            const int g = (c0 * 4) / e.cpg + t;
            if (g >= G) continue;
            Stat s{rn[t], rm[t], rq[t]};
            for (int rr = 1; rr < e.R; ++rr) chan(s, Stat{rn[rr * GW + t], rm[rr * GW + t], rq[rr * GW + t]});
            part[(i * nslab + slab) * G + g] = make_float4(s.n, s.m, s.q, 0.f);
        }
        __syncthreads();
    }
}

// one unsigned maximum per workgroup -> *amax_out (NaN sorts on top)
__device__ __forceinline__ void block_mag_out(unsigned bits, float *amax_out, unsigned *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) bits = max(bits, sh[w]);
        if (bits > *reinterpret_cast<volatile unsigned *>(amax_out)) atomicMax(reinterpret_cast<unsigned *>(amax_out), bits);
    }
}

__global__ __launch_bounds__(kThreads) void gn_map_norm_kernel(const float *__restrict__ x, const float *__restrict__ res,
                                                               const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               float *__restrict__ y, float *__restrict__ mean,
                                                               float *__restrict__ rstd, const float4 *__restrict__ part, int P,
                                                               int C, int G, int S, int nslab, float eps, int relu,
                                                               float *__restrict__ amax_out)
{
    __shared__ float smu[kMaxG], srs[kMaxG];
    __shared__ float cn[kThreads], cm[kThreads], cq[kThreads];
    __shared__ unsigned mxs[kThreads / 64];
    const Geo e = geometry(C, G);
    const int slab = blockIdx.x;
    const int64_t i = blockIdx.y;
    // the sample's statistics: J threads per group merge a run of slabs each, the first of them merges the J runs
    {
        const int GW = G < kThreads ? G : kThreads, J = kThreads / GW, L = (nslab + J - 1) / J;
        const int j = e.tid / GW, gl = e.tid - j * GW;
        for (int g0 = 0; g0 < G; g0 += GW) {
            const int g = g0 + gl;
            Stat s{0.f, 0.f, 0.f};
            if (j < J && g < G) {
                const int s1 = min(nslab, (j + 1) * L);
                for (int k = j * L; k < s1; ++k) {
                    const float4 t = part[(i * nslab + k) * G + g];
                    chan(s, Stat{t.x, t.y, t.z});
                }
            }
            cn[e.tid] = s.n; cm[e.tid] = s.m; cq[e.tid] = s.q;
            __syncthreads();
            if (j == 0 && g < G) {
                for (int jj = 1; jj < J; ++jj) chan(s, Stat{cn[jj * GW + gl], cm[jj * GW + gl], cq[jj * GW + gl]});
                const float rs = rsqrtf(s.q / s.n + eps);
                smu[g] = s.m;
                srs[g] = rs;
                if (slab == 0) { mean[i * G + g] = s.m; rstd[i * G + g] = rs; }
            }
            __syncthreads();
        }
    }
    const int p0 = slab * S, p1 = min(P, p0 + S);
    const float *xs = x + i * P * C, *rp = res ? res + i * P * C : nullptr;
    float *ys = y + i * P * C;
    unsigned mx = 0u;
    for (int c0 = 0; c0 < e.C4; c0 += e.CW) {
        const int c4 = c0 + e.cl;
        if (!(e.live && c4 < e.C4)) continue;
        const int gl = (4 * c4) / e.cpg, gh = (4 * c4 + 2) / e.cpg;
        const float4 gm = ld4(gamma + 4 * c4), bt = ld4(beta + 4 * c4);
        const float ml = smu[gl], rl = srs[gl], mh = smu[gh], rh = srs[gh];
        const float4 ga = make_float4(gm.x * rl, gm.y * rl, gm.z * rh, gm.w * rh);
        const float4 be = make_float4(bt.x - ml * ga.x, bt.y - ml * ga.y, bt.z - mh * ga.z, bt.w - mh * ga.w);
        for (int pb = p0; pb < p1; pb += kPos * e.R) {
            float4 v[kPos], q[kPos];
#pragma unroll
            for (int k = 0; k < kPos; ++k) {
                const int p = pb + e.r + k * e.R;
                const int64_t off = ((int64_t)p * e.C4 + c4) * 4;
                v[k] = p < p1 ? ld4(xs + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                q[k] = (rp && p < p1) ? ld4(rp + off) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int k = 0; k < kPos; ++k) {
                const int p = pb + e.r + k * e.R;
                if (p >= p1) continue;
                float4 t = make_float4(v[k].x * ga.x + be.x, v[k].y * ga.y + be.y, v[k].z * ga.z + be.z, v[k].w * ga.w + be.w);
                if (rp) { t.x += q[k].x; t.y += q[k].y; t.z += q[k].z; t.w += q[k].w; }
                if (relu) {            // a NaN stays a NaN
                    t.x = t.x < 0.f ? 0.f : t.x; t.y = t.y < 0.f ? 0.f : t.y;
                    t.z = t.z < 0.f ? 0.f : t.z; t.w = t.w < 0.f ? 0.f : t.w;
                }
                st4(ys + ((int64_t)p * e.C4 + c4) * 4, t);
                mx = htd::mag_bits4(mx, t);
            }
        }
    }
    if (amax_out != nullptr) block_mag_out(mx, amax_out, mxs);
}

// d = gy under the ReLU mask (y > 0)
__device__ __forceinline__ float4 masked(float4 d, float4 yv, int relu)
{
    if (relu) {
        if (!(yv.x > 0.f)) d.x = 0.f;
        if (!(yv.y > 0.f)) d.y = 0.f;
        if (!(yv.z > 0.f)) d.z = 0.f;
        if (!(yv.w > 0.f)) d.w = 0.f;
    }
    return d;
}

// wsC: [2][rows][C] (sum d * xhat, then sum d; rows = n * nslab), wsG: [rows][G] of (sum_c gamma * sum d, sum_c gamma * sum d * xhat)
__global__ __launch_bounds__(kThreads) void gn_map_bwd_sums_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                   const float *__restrict__ gy, float *__restrict__ wsC,
                                                                   float2 *__restrict__ wsG, int P, int C, int G, int S, int nslab,
                                                                   int relu, int64_t rows)
{
    __shared__ float4 ra[kThreads], rb[kThreads];
    const Geo e = geometry(C, G);
    const int slab = blockIdx.x;
    const int64_t i = blockIdx.y, row = i * nslab + slab;
    const int p0 = slab * S, p1 = min(P, p0 + S);
    const float *xs = x + i * P * C, *ys = y + i * P * C, *gs = gy + i * P * C;
    for (int c0 = 0; c0 < e.C4; c0 += e.CW) {
        const int c4 = c0 + e.cl;
        const bool ok = e.live && c4 < e.C4;
        float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sx = sg, gm = sg;
        if (ok) {
            const int gl = (4 * c4) / e.cpg, gh = (4 * c4 + 2) / e.cpg;
            const float ml = mean[i * G + gl], rl = rstd[i * G + gl], mh = mean[i * G + gh], rh = rstd[i * G + gh];
            gm = ld4(gamma + 4 * c4);
            for (int pb = p0; pb < p1; pb += kPos * e.R) {
                float4 v[kPos], d[kPos], t[kPos];
#pragma unroll
                for (int k = 0; k < kPos; ++k) {
                    const int p = pb + e.r + k * e.R;
                    const int64_t off = ((int64_t)p * e.C4 + c4) * 4;
                    const bool in = p < p1;
                    v[k] = in ? ld4(xs + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                    d[k] = in ? ld4(gs + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                    t[k] = (in && relu) ? ld4(ys + off) : make_float4(1.f, 1.f, 1.f, 1.f);
                }
#pragma unroll
                for (int k = 0; k < kPos; ++k) {       // outside the slab d = 0: nothing is added
                    const float4 dd = masked(d[k], t[k], relu);
                    sg.x += dd.x; sg.y += dd.y; sg.z += dd.z; sg.w += dd.w;
                    sx.x += dd.x * (v[k].x - ml) * rl; sx.y += dd.y * (v[k].y - ml) * rl;
                    sx.z += dd.z * (v[k].z - mh) * rh; sx.w += dd.w * (v[k].w - mh) * rh;
                }
            }
        }
        ra[e.tid] = sg;
        rb[e.tid] = sx;
        __syncthreads();
        const bool lead = ok && e.r == 0;
        if (lead) {                     // the row groups, in order
            for (int rr = 1; rr < e.R; ++rr) {
                const float4 a = ra[rr * e.CW + e.cl], b = rb[rr * e.CW + e.cl];
                sg.x += a.x; sg.y += a.y; sg.z += a.z; sg.w += a.w;
                sx.x += b.x; sx.y += b.y; sx.z += b.z; sx.w += b.w;
            }
            st4(wsC + row * C + 4 * c4, sx);
            st4(wsC + (rows + row) * C + 4 * c4, sg);
        }
        // gamma-weighted group sums (every thread takes the shuffles; only the leading rows' results are kept)
        const float al = sg.x * gm.x + sg.y * gm.y, ah = sg.z * gm.z + sg.w * gm.w;
        const float bl = sx.x * gm.x + sx.y * gm.y, bh = sx.z * gm.z + sx.w * gm.w;
        if (e.cpg >= 4) {
            float a = al + ah, b = bl + bh;
            for (int o = 1; o < e.lanes; o <<= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
            if (lead && e.cl % e.lanes == 0) wsG[row * G + (4 * c4) / e.cpg] = make_float2(a, b);
        } else if (lead) {
            wsG[row * G + 2 * c4] = make_float2(al, bl);
            wsG[row * G + 2 * c4 + 1] = make_float2(ah, bh);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void gn_map_bwd_gx_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                 const float *__restrict__ gamma, const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd, const float *__restrict__ gy,
                                                                 float *__restrict__ gx, float *__restrict__ gres,
                                                                 const float2 *__restrict__ wsG, int P, int C, int G, int S,
                                                                 int nslab, int relu, float *__restrict__ amax_out)
{
    __shared__ float sa[kMaxG], sb[kMaxG];
    __shared__ float ca[kThreads], cb[kThreads];
    __shared__ unsigned mxs[kThreads / 64];
    const Geo e = geometry(C, G);
    const int slab = blockIdx.x;
    const int64_t i = blockIdx.y;
    {   // the sample's group sums over its slabs: J runs per group, then the runs in order
        const int GW = G < kThreads ? G : kThreads, J = kThreads / GW, L = (nslab + J - 1) / J;
        const int j = e.tid / GW, gl = e.tid - j * GW;
        const float m = 1.f / ((float)P * (float)e.cpg);
        for (int g0 = 0; g0 < G; g0 += GW) {
            const int g = g0 + gl;
            float a = 0.f, b = 0.f;
            if (j < J && g < G) {
                const int s1 = min(nslab, (j + 1) * L);
                for (int k = j * L; k < s1; ++k) {
                    const float2 t = wsG[(i * nslab + k) * G + g];
                    a += t.x; b += t.y;
                }
            }
            ca[e.tid] = a; cb[e.tid] = b;
            __syncthreads();
            if (j == 0 && g < G) {
                for (int jj = 1; jj < J; ++jj) { a += ca[jj * GW + gl]; b += cb[jj * GW + gl]; }
                sa[g] = a * m;
                sb[g] = b * m;
            }
            __syncthreads();
        }
    }
    const int p0 = slab * S, p1 = min(P, p0 + S);
    const float *xs = x + i * P * C, *ys = y + i * P * C, *gs = gy + i * P * C;
    float *os = gx + i * P * C, *rs_ = (gres && relu) ? gres + i * P * C : nullptr;
    unsigned mx = 0u;
    for (int c0 = 0; c0 < e.C4; c0 += e.CW) {
        const int c4 = c0 + e.cl;
        if (!(e.live && c4 < e.C4)) continue;
        const int gl = (4 * c4) / e.cpg, gh = (4 * c4 + 2) / e.cpg;
        const float ml = mean[i * G + gl], rl = rstd[i * G + gl], mh = mean[i * G + gh], rh = rstd[i * G + gh];
        const float al = sa[gl], bl = sb[gl], ah = sa[gh], bh = sb[gh];
        const float4 gm = ld4(gamma + 4 * c4);
        for (int pb = p0; pb < p1; pb += kPos * e.R) {
            float4 v[kPos], d[kPos], t[kPos];
#pragma unroll
            for (int k = 0; k < kPos; ++k) {
                const int p = pb + e.r + k * e.R;
                const int64_t off = ((int64_t)p * e.C4 + c4) * 4;
                const bool in = p < p1;
                v[k] = in ? ld4(xs + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                d[k] = in ? ld4(gs + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                t[k] = (in && relu) ? ld4(ys + off) : make_float4(1.f, 1.f, 1.f, 1.f);
            }
#pragma unroll
            for (int k = 0; k < kPos; ++k) {
                const int p = pb + e.r + k * e.R;
                if (p >= p1) continue;
                const int64_t off = ((int64_t)p * e.C4 + c4) * 4;
                const float4 dd = masked(d[k], t[k], relu);
                float4 o;
                o.x = rl * (dd.x * gm.x - al - (v[k].x - ml) * rl * bl);
                o.y = rl * (dd.y * gm.y - al - (v[k].y - ml) * rl * bl);
                o.z = rh * (dd.z * gm.z - ah - (v[k].z - mh) * rh * bh);
                o.w = rh * (dd.w * gm.w - ah - (v[k].w - mh) * rh * bh);
                st4(os + off, o);
                if (rs_) st4(rs_ + off, dd);
                mx = htd::mag_bits4(mx, o);
            }
        }
    }
    if (amax_out != nullptr) block_mag_out(mx, amax_out, mxs);
}

// ------------------------------------------------------------------ weight standardisation
// sum over the workgroup in a fixed order (wave shuffles, then the four waves in order); every thread gets the result
__device__ __forceinline__ float block_sum(float v, float *sh)
{
    v = htd::wave_sum(v);
    __syncthreads();                   // sh may still be read from the call before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one workgroup per output channel: a KRSC row of K = kh * kw * Ci weights is contiguous (K = 147: no 16-byte alignment, scalar
// loads; the row is at most 18 KB and its second and third reading come from the cache)
__global__ __launch_bounds__(kThreads) void weight_std_fwd_kernel(const float *__restrict__ w, float *__restrict__ out,
                                                                  float *__restrict__ mean, float *__restrict__ inv, int K,
                                                                  float eps)
{
    __shared__ float sh[kThreads / 64];
    const int64_t row = blockIdx.x;
    const float *wr = w + row * K;
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += kThreads) s += wr[k];
    const float mu = block_sum(s, sh) / (float)K;
    float q = 0.f;
    for (int k = threadIdx.x; k < K; k += kThreads) { const float c = wr[k] - mu; q += c * c; }
    const float sd = sqrtf(block_sum(q, sh) / (float)(K - 1));      // torch.std: unbiased
    const float d = 1.f / (sd + eps);                               // eps beside the root, not under it
    for (int k = threadIdx.x; k < K; k += kThreads) out[row * K + k] = (wr[k] - mu) * d;
    if (threadIdx.x == 0) { mean[row] = mu; inv[row] = d; }
}

// h = g * d - c * (sum g * c) * d^2 / ((K - 1) * std),  gw = h - mean(h);  c = w - mean, d = 1 / (std + eps)
__global__ __launch_bounds__(kThreads) void weight_std_bwd_kernel(const float *__restrict__ w, const float *__restrict__ mean,
                                                                  const float *__restrict__ inv, const float *__restrict__ g,
                                                                  float *__restrict__ gw, int K, float eps)
{
    __shared__ float sh[kThreads / 64];
    const int64_t row = blockIdx.x;
    const float *wr = w + row * K, *gr = g + row * K;
    const float mu = mean[row], d = inv[row];
    float sg = 0.f, sgc = 0.f, sc = 0.f;
    for (int k = threadIdx.x; k < K; k += kThreads) {
        const float c = wr[k] - mu, t = gr[k];
        sg += t; sgc += t * c; sc += c;
    }
    sg = block_sum(sg, sh);
    sgc = block_sum(sgc, sh);
    sc = block_sum(sc, sh);
    const float sd = 1.f / d - eps;
    const float coef = sgc * d * d / ((float)(K - 1) * sd);
    const float mh = (sg * d - sc * coef) / (float)K;
    for (int k = threadIdx.x; k < K; k += kThreads) gw[row * K + k] = gr[k] * d - (wr[k] - mu) * coef - mh;
}

inline int sub_slab(int C)
{
    const int C4 = C / 4, CW = C4 < kThreads ? C4 : kThreads;
    return kPos * (kThreads / CW);
}

inline int slab_len(int P, int C)
{
    const int sub = sub_slab(C);
    const int per = (int)htd::ceil_div(P, kMaxSlabs);
    const int S = (int)htd::ceil_div(per, sub) * sub;
    return S < sub ? sub : S;
}

int map_check(const char *what, int64_t n, int P, int C, int G)
{
    HTD_REQUIRE(n >= 0 && n < 65536 && P > 0, "%s: bad sizes n=%lld P=%d", what, (long long)n, P);
    HTD_REQUIRE(C % 4 == 0 && C >= 64 && C <= 2048, "%s: C=%d must be a multiple of 4 in [64, 2048]", what, C);
    HTD_REQUIRE(G > 0 && C % G == 0, "%s: C=%d not divisible by G=%d", what, C, G);
    const int cpg = C / G;
    HTD_REQUIRE(cpg >= 2 && cpg <= 64 && (cpg & (cpg - 1)) == 0, "%s: channels/group=%d must be a power of two in [2, 64]", what,
                cpg);
    HTD_REQUIRE((int64_t)P * cpg < (1ll << 24), "%s: P * channels/group = %lld: group counts are kept in fp32", what,
                (long long)P * cpg);
    return HTD_OK;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int htd_group_norm_map_slab(int P, int C)
{
    HTD_REQUIRE(P > 0 && C % 4 == 0 && C >= 64 && C <= 2048, "group_norm_map_slab: bad sizes P=%d C=%d", P, C);
    return slab_len(P, C);
}

// forward: n * slabs * G float4; backward: 2 * n * slabs * C floats + n * slabs * G float2.  The larger of the two.
extern "C" int64_t htd_group_norm_map_workspace_bytes(int64_t n, int P, int C, int G)
{
    if (n <= 0 || P <= 0 || C < 64 || C > 2048 || C % 4 || G <= 0 || C % G) return 16;
    const int64_t rows = n * htd::ceil_div(P, slab_len(P, C));
    const int64_t fwd = rows * G * 16, bwd = rows * C * 8 + rows * G * 8;
    return fwd > bwd ? fwd : bwd;
}

extern "C" int htd_group_norm_map_fwd(const float *x, const float *residual, const float *gamma, const float *beta, float *y,
                                      float *mean, float *rstd, int64_t n, int P, int C, int G, float eps, int relu,
                                      void *workspace, float *amax_out, void *stream)
{
    if (int rc = map_check("group_norm_map", n, P, C, G)) return rc;
    if (n == 0) return HTD_OK;
    HTD_REQUIRE(x && gamma && beta && y && mean && rstd && workspace, "group_norm_map: null pointer");
    HTD_REQUIRE(aligned16(x) && aligned16(y) && aligned16(residual) && aligned16(gamma) && aligned16(beta) && aligned16(workspace),
                "group_norm_map: operands must be 16-byte aligned");
    const int S = slab_len(P, C), nslab = (int)htd::ceil_div(P, S);
    const dim3 grid((unsigned)nslab, (unsigned)n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_map_stats_kernel, grid, dim3(kThreads), 0, s, x, (float4 *)workspace, P, C, G, S, nslab);
    hipLaunchKernelGGL(gn_map_norm_kernel, grid, dim3(kThreads), 0, s, x, residual, gamma, beta, y, mean, rstd,
                       (const float4 *)workspace, P, C, G, S, nslab, eps, relu, amax_out);
    return htd::check_launch("group_norm_map_fwd");
}

extern "C" int htd_group_norm_map_bwd(const float *x, const float *y, const float *gamma, const float *mean, const float *rstd,
                                      const float *gy, float *gx, float *gres, float *ggamma, float *gbeta, int64_t n, int P,
                                      int C, int G, int relu, void *workspace, float *amax_out, void *stream)
{
    if (int rc = map_check("group_norm_map_bwd", n, P, C, G)) return rc;
    HTD_REQUIRE(ggamma && gbeta, "group_norm_map_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        (void)hipMemsetAsync(ggamma, 0, sizeof(float) * C, s);
        (void)hipMemsetAsync(gbeta, 0, sizeof(float) * C, s);
        return htd::check_launch("group_norm_map_bwd");
    }
    HTD_REQUIRE(x && y && gamma && mean && rstd && gy && gx && workspace, "group_norm_map_bwd: null pointer");
    HTD_REQUIRE(aligned16(x) && aligned16(y) && aligned16(gy) && aligned16(gx) && aligned16(gres) && aligned16(gamma) &&
                    aligned16(workspace),
                "group_norm_map_bwd: operands must be 16-byte aligned");
    const int S = slab_len(P, C), nslab = (int)htd::ceil_div(P, S);
    const int64_t rows = n * nslab;
    HTD_REQUIRE(rows < (1ll << 31), "group_norm_map_bwd: too many slabs");
    float *wsC = (float *)workspace;
    float2 *wsG = (float2 *)(wsC + 2 * rows * C);
    const dim3 grid((unsigned)nslab, (unsigned)n);
    hipLaunchKernelGGL(gn_map_bwd_sums_kernel, grid, dim3(kThreads), 0, s, x, y, gamma, mean, rstd, gy, wsC, wsG, P, C, G, S,
                       nslab, relu, rows);
    hipLaunchKernelGGL(gn_map_bwd_gx_kernel, grid, dim3(kThreads), 0, s, x, y, gamma, mean, rstd, gy, gx, gres,
                       (const float2 *)wsG, P, C, G, S, nslab, relu, amax_out);
    htd::launch_colsum_rows(wsC, ggamma, gbeta, C, (int)rows, s);
    return htd::check_launch("group_norm_map_bwd");
}

/* mmcv-knowledge: ConvWS2d (mmcv 1.2.1, mmcv/cnn/bricks/conv_ws.py) standardises each output channel's weights with torch.std
 * (unbiased) and adds eps to the std. */
extern "C" int htd_weight_standardize_fwd(const float *w, float *w_hat, float *mean, float *inv, int Co, int K, float eps,
                                          void *stream)
{
    HTD_REQUIRE(Co > 0 && K >= 2, "weight_standardize: bad sizes Co=%d K=%d", Co, K);
    HTD_REQUIRE(w && w_hat && mean && inv, "weight_standardize: null pointer");
    hipLaunchKernelGGL(weight_std_fwd_kernel, dim3((unsigned)Co), dim3(kThreads), 0, (hipStream_t)stream, w, w_hat, mean, inv, K,
                       eps);
    return htd::check_launch("weight_standardize_fwd");
}

extern "C" int htd_weight_standardize_bwd(const float *w, const float *mean, const float *inv, const float *g_hat, float *gw,
                                          int Co, int K, float eps, void *stream)
{
    HTD_REQUIRE(Co > 0 && K >= 2, "weight_standardize_bwd: bad sizes Co=%d K=%d", Co, K);
    HTD_REQUIRE(w && mean && inv && g_hat && gw, "weight_standardize_bwd: null pointer");
    hipLaunchKernelGGL(weight_std_bwd_kernel, dim3((unsigned)Co), dim3(kThreads), 0, (hipStream_t)stream, w, mean, inv, g_hat, gw,
                       K, eps);
    return htd::check_launch("weight_standardize_bwd");
}
