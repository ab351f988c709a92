// What atss.hip, gfl.hip and vfnet.hip share beyond point_maps.h: the level table of a pyramid with one anchor per location, the
// float4 load of a box and the reference's fp32 IoU.  One implementation each; the kernels keep their own loops.
#pragma once
#include "common.h"
#include "point_maps.h"

namespace {

constexpr int ATSS_MAX_LEVELS = POINT_MAX_LEVELS;

struct AtssLevels {
    unsigned aoff[ATSS_MAX_LEVELS + 1];     // first anchor of the level; aoff[L] = A (one anchor per location)
};

__device__ __forceinline__ float4 load4(const float *p, int64_t i) { return *reinterpret_cast<const float4 *>(p + i * 4); }

// bbox_overlaps(anchor, gt) (iou2d_calculator.py:43-124) in its fp32 order, eps = 1e-6
__device__ __forceinline__ float iou_ref(float4 a, float4 g)
{
    const float area1 = (a.z - a.x) * (a.w - a.y), area2 = (g.z - g.x) * (g.w - g.y);
    const float w = fmaxf(fminf(a.z, g.z) - fmaxf(a.x, g.x), 0.f), h = fmaxf(fminf(a.w, g.w) - fmaxf(a.y, g.y), 0.f);
    const float overlap = w * h;
    const float uni = fmaxf(area1 + area2 - overlap, 1e-6f);
    return overlap / uni;
}

int fill_levels(AtssLevels &lv, const char *what, const int64_t *level_sizes, int L, int64_t *A_out)
{
    HTD_REQUIRE(L > 0 && L <= ATSS_MAX_LEVELS, "%s: 1 to %d levels, got %d", what, ATSS_MAX_LEVELS, L);
    HTD_REQUIRE(level_sizes, "%s: null level table", what);
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
        HTD_REQUIRE(level_sizes[l] > 0, "%s: level %d has no anchor", what, l);
        lv.aoff[l] = (unsigned)off;
        off += level_sizes[l];
        HTD_REQUIRE(off < ((int64_t)1 << 31), "%s: more than 2^31 anchors", what);
    }
    for (int l = L; l <= ATSS_MAX_LEVELS; ++l) lv.aoff[l] = (unsigned)off;
    *A_out = off;
    return HTD_OK;
}

}  // namespace
