// The sigmoid focal loss of one element with its derivative, the fp64 sigmoid / log1p of one logit and the two-sum block
// reduction of the head-loss kernels: shared by focal_loss.hip (htd_sigmoid_focal_loss, htd_retina_loss) and, through
// point_maps.h, the heads with one prediction per location (fcos.hip, atss.hip, gfl.hip, vfnet.hip), so the dense heads take the
// same arithmetic.  See focal_loss.hip for the formulation; how the kernels address their maps is in loss_units.h.
#pragma once
#include "common.h"

namespace {

// -> loss of one element, g = d(loss)/dx.  G2: gamma == 2 (no pow); otherwise sigmoid(z)^gamma = exp2(gamma * log2 sigmoid(z))
// with log sigmoid(z) = -softplus(-z) from the same log1p.
template <bool G2>
__device__ __forceinline__ float focal_elem(float x, bool t, float gamma, float alpha, float &g)
{
    const float z = t ? -x : x;
    // hardware exp / log / reciprocal.  v_exp_f32 / v_log_f32 / v_rcp_f32 are good to about an ulp, but __expf scales its
    // argument by log2(e) first, so e carries a relative error of about |z| * 2^-24 (4e-6 at |z| = 90).  That is harmless in
    // absolute terms, which is what counts here: e <= exp(-|z|), so every error below is of the order |z| exp(-|z|) 2^-24 or an
    // ulp of a sum of order 1
    const float e = __expf(-fabsf(z));
    const float u = 1.f + e;
    const float r = __builtin_amdgcn_rcpf(u);
    // log1p(e) = log(u) * e / (u - 1): the rounding of u = 1 + e cancels (u - 1 is exact); e below 2^-24 gives u == 1
    const float l = u == 1.f ? e : __logf(u) * (e * __builtin_amdgcn_rcpf(u - 1.f));
    const float big = r, small = e * r;                     // sigmoid(|z|), sigmoid(-|z|)
    const float s = z >= 0.f ? big : small, s1 = z >= 0.f ? small : big;
    const float sp = fmaxf(z, 0.f) + l;                     // softplus(z) = BCEWithLogits(x, t)
    float sg;
    if (G2)
        sg = s * s;
    else
        sg = exp2f(gamma * (-1.44269504088896340736f * (fmaxf(-z, 0.f) + l)));
    const float at = t ? alpha : 1.f - alpha;
    const float gz = at * sg * (s + gamma * sp * s1);
    g = t ? -gz : gz;
    return at * sg * sp;
}

// fp64, for the few elements with a soft target: l1p = log1p(exp(-|z|)) and s = sigmoid(z).  softplus(z) = fmax(z, 0.) + l1p;
// the callers add the terms of their BCE-with-logits in their own order, which their results are pinned to bit for bit.
__device__ __forceinline__ void sigmoid_log1p(double z, double &l1p, double &s)
{
    const double e = exp(-fabs(z));
    l1p = log1p(e);
    s = z >= 0. ? 1. / (1. + e) : e / (1. + e);
}

__device__ __forceinline__ void block_store_partial2(float s0, float s1, float *__restrict__ partial)
{
    __shared__ float red[2][4];
    s0 = htd::wave_sum(s0);
    s1 = htd::wave_sum(s1);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = s0; red[1][wave] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

}  // namespace
