// How focal_loss.hip, ghm_loss.hip and the heads of point_maps.h address their maps: the level of an index in a prefix-sum table, the VEC-wide
// unit of logits or gradients, the unit of a logit matrix.  Each kernel keeps its own loops and calls these.
#pragma once
#include "common.h"

namespace {

// the level l with off[l] <= i < off[l + 1] of a prefix-sum table off[0 .. L]; searched as an unsigned index, which the
// table accesses need not sign-extend
__device__ __forceinline__ unsigned level_of(const unsigned *off, int L, unsigned i)
{
    unsigned l = 0;
    while (l + 1 < (unsigned)L && i >= off[l + 1]) ++l;
    return l;
}

// unit u of p: one float4 (VEC = 4, p 16-byte aligned) or one float (VEC = 1).  1 % VEC and its like keep the VEC = 1
// instantiation inside its one-element array.
template <int VEC>
__device__ __forceinline__ void load_unit(const float *p, int64_t u, float (&v)[VEC])
{
    if (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p + u * 4);
        v[0] = q.x; v[1 % VEC] = q.y; v[2 % VEC] = q.z; v[3 % VEC] = q.w;
    } else {
        v[0] = p[u];
    }
}

template <int VEC>
__device__ __forceinline__ void store_unit(float *p, int64_t u, const float (&v)[VEC])
{
    if (VEC == 4)
        *reinterpret_cast<float4 *>(p + u * 4) = make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]);
    else
        p[u] = v[0];
}

// unit u of a logit matrix [N][C] with cols = C / VEC units per row -> its row; c0 = its first class.  The 64-bit division
// only where the index needs it.
template <int VEC>
__device__ __forceinline__ int64_t matrix_unit(int64_t u, int64_t units, int cols, int &c0)
{
    const int64_t row = units <= 0xffffffffLL ? (int64_t)((unsigned)u / (unsigned)cols) : u / cols;
    c0 = (int)(u - row * cols) * VEC;
    return row;
}

}  // namespace
