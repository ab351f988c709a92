// The kernel that scales the finished gradient maps of a head with one prediction per location by incoming gradients, and its
// host side: htd_fcos_grad_scale (FCOS and ATSS: widths C, 4, 1), htd_vfnet_grad_scale (C, 4, 4) and htd_fovea_grad_scale (C, 4
// and no third map: W2 = 0, whose slot and factor are then never touched) are three prologues onto it.
#pragma once
#include "point_maps.h"

namespace {

// g0 / g1 / g2: device scalars, one per slot; the first w0 / W1 / W2 channels of a slot's rows are scaled, padding is left
// alone, and so is a slot whose factor is exactly 1 (decided here: the host never reads the factors).  The widths of the two
// narrow slots are template parameters, so a thread's few multiplications are straight-line code.
template <int W1, int W2>
__global__ __launch_bounds__(256) void point_scale_kernel(PointMaps mp, int L, int w0, const float *__restrict__ g0,
                                                          const float *__restrict__ g1, const float *__restrict__ g2)
{
    const float f0 = *g0, f1 = *g1, f2 = W2 > 0 ? *g2 : 1.f;
    const unsigned n_rows = mp.rrow[L];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (f0 != 1.f) {
        for (unsigned rw = wave; rw < n_rows; rw += gridDim.x * 4u) {
            const int l = level_of(mp.rrow, L, rw);
            float *g_row = mp.grad[0][l] + (int64_t)(rw - mp.rrow[l]) * mp.cs[0][l];
            for (unsigned j = lane; j < (unsigned)w0; j += 64u) g_row[j] *= f0;
        }
    }
    if (f1 != 1.f || f2 != 1.f) {
        for (unsigned rw = blockIdx.x * 256u + threadIdx.x; rw < n_rows; rw += gridDim.x * 256u) {
            const int l = level_of(mp.rrow, L, rw);
            const unsigned row = rw - mp.rrow[l];
            float *a = mp.grad[1][l] + (int64_t)row * mp.cs[1][l];
            if (f1 != 1.f) {
#pragma unroll
                for (int k = 0; k < W1; ++k) a[k] *= f1;
            }
            if (W2 > 0 && f2 != 1.f) {
                float *b = mp.grad[2][l] + (int64_t)row * mp.cs[2][l];
#pragma unroll
                for (int k = 0; k < W2; ++k) b[k] *= f2;
            }
        }
    }
}

// the body of htd_fcos_grad_scale / htd_vfnet_grad_scale after their level tables: three gradient tables of widths C, W1, W2
template <int W1, int W2>
int point_grad_scale(const char *what, const unsigned *off, int L, int B, float *const *grad0, const int64_t *stride0, int C,
                     float *const *grad1, const int64_t *stride1, float *const *grad2, const int64_t *stride2, const float *g0,
                     const float *g1, const float *g2, void *stream)
{
    HTD_REQUIRE(g0 && g1 && (g2 || W2 == 0), "%s: null pointer", what);
    const PointSlot slots[POINT_SLOTS] = {{nullptr, grad0, stride0, C, false, true}, {nullptr, grad1, stride1, W1, false, true},
                                          W2 > 0 ? PointSlot{nullptr, grad2, stride2, W2, false, true} : PointSlot{}};
    PointMaps mp = {};
    const int rc = fill_point_maps(mp, what, off, L, B, slots, 1);
    if (rc != HTD_OK) return rc;
    hipLaunchKernelGGL((point_scale_kernel<W1, W2>), dim3(POINT_BLOCKS), dim3(256), 0, (hipStream_t)stream, mp, L, C, g0, g1, g2);
    return htd::check_launch(what);
}

}  // namespace
