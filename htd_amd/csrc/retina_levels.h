// The level table of the dense-head kernels that read the convolution outputs where they lie, its host-side filling, and the
// decoding of a pixel row, a channel and a regression unit of an anchor head with the bbox2delta target of a positive: shared
// by focal_loss.hip (htd_retina_loss, htd_retina_grad_scale, htd_retina_keys) and ghm_loss.hip (htd_ghm_head_loss), so the two
// loss families address the maps and form their targets in one way and htd_retina_grad_scale serves the gradient maps of both.
#pragma once
#include "common.h"
#include "loss_units.h"

namespace {

constexpr int FOCAL_BLOCKS = 2048;          // 256 CUs x 8 blocks: the cap of a memory-bound grid; the rest is grid-stride
constexpr int RETINA_MAX_LEVELS = 8;

struct RetinaLevels {
    const float *cls[RETINA_MAX_LEVELS];
    const float *reg[RETINA_MAX_LEVELS];
    float *gcls[RETINA_MAX_LEVELS];
    float *greg[RETINA_MAX_LEVELS];
    unsigned pix[RETINA_MAX_LEVELS];        // pixels of the level
    unsigned cu[RETINA_MAX_LEVELS];         // units per pixel of the classification map (channel stride / VEC)
    unsigned ru[RETINA_MAX_LEVELS];         // float4s per pixel of the regression map (channel stride / 4)
    unsigned aoff[RETINA_MAX_LEVELS];       // first anchor of the level
    unsigned coff[RETINA_MAX_LEVELS + 1];   // prefix sums of B * pix * cu: the classification units of all levels
    unsigned roff[RETINA_MAX_LEVELS + 1];   // prefix sums of B * pix * ru, continuing after coff[L]
    unsigned rrow[RETINA_MAX_LEVELS + 1];   // prefix sums of B * pix: the pixel rows of all levels
};

struct Vec4f { float v[4]; };

int fill_levels(RetinaLevels &lv, const char *what, const float *const *cls, const int64_t *cls_stride, const float *const *reg,
                const int64_t *reg_stride, float *const *gcls, float *const *greg, const int64_t *pix, int L, int B, int na, int C,
                int vec, int64_t *A_out)
{
    HTD_REQUIRE(L > 0 && L <= RETINA_MAX_LEVELS && B > 0 && na > 0 && C > 0, "%s: bad sizes", what);
    HTD_REQUIRE(cls && cls_stride && pix, "%s: null table", what);
    int64_t coff = 0, aoff = 0, rrow = 0;
    for (int l = 0; l < L; ++l) {
        HTD_REQUIRE(pix[l] > 0 && cls_stride[l] >= (int64_t)na * C && cls_stride[l] % vec == 0, "%s: bad level %d", what, l);
        // float4 access (vec == 4, or the float4 branch of the keys kernel) needs 16-byte aligned rows; the scalar forms do not
        const bool f4 = vec == 4 || ((C & 3) == 0 && (cls_stride[l] & 3) == 0);
        HTD_REQUIRE(cls[l] && (!f4 || ((uintptr_t)cls[l] & 15) == 0), "%s: map of level %d is null or not 16-byte aligned", what, l);
        lv.cls[l] = cls[l];
        lv.gcls[l] = gcls ? gcls[l] : nullptr;
        lv.pix[l] = (unsigned)pix[l];
        lv.cu[l] = (unsigned)(cls_stride[l] / vec);
        lv.aoff[l] = (unsigned)aoff;
        lv.coff[l] = (unsigned)coff;
        lv.rrow[l] = (unsigned)rrow;
        rrow += (int64_t)B * pix[l];
        coff += (int64_t)B * pix[l] * (cls_stride[l] / vec);
        aoff += pix[l] * na;
    }
    int64_t roff = coff;
    for (int l = 0; l < L; ++l) {
        lv.roff[l] = (unsigned)roff;
        if (reg) {
            HTD_REQUIRE(reg_stride && reg_stride[l] >= (int64_t)na * 4 && reg_stride[l] % 4 == 0, "%s: bad regression stride", what);
            HTD_REQUIRE(reg[l] && ((uintptr_t)reg[l] & 15) == 0, "%s: regression map %d is null or not 16-byte aligned", what, l);
            lv.reg[l] = reg[l];
            lv.greg[l] = greg ? greg[l] : nullptr;
            lv.ru[l] = (unsigned)(reg_stride[l] / 4);
            roff += (int64_t)B * pix[l] * (reg_stride[l] / 4);
        }
    }
    for (int l = L; l < RETINA_MAX_LEVELS; ++l) lv.aoff[l] = (unsigned)aoff;
    lv.coff[L] = (unsigned)coff;
    lv.roff[L] = (unsigned)roff;
    lv.rrow[L] = (unsigned)rrow;
    HTD_REQUIRE(roff < (int64_t)1 << 31 && aoff * B < (int64_t)1 << 31, "%s: more than 2^31 units", what);
    *A_out = aoff;
    return HTD_OK;
}

// The prologue of the head-loss entry points: float4 units (-> vec) when C and every channel stride allow them, the level
// table, the anchor count, the gradient maps' alignment, means and stds by value.
int head_loss_levels(RetinaLevels &lv, const char *what, const float *const *cls, const int64_t *cls_stride, const float *const *reg,
                     const int64_t *reg_stride, float *const *grad_cls, float *const *grad_reg, const int64_t *pix, int L, int B,
                     int na, int C, int A, const float *means4, const float *stds4, bool &vec, Vec4f &means, Vec4f &stds)
{
    vec = (C & 3) == 0;
    for (int l = 0; l < L && l < RETINA_MAX_LEVELS && vec; ++l) vec = cls_stride && (cls_stride[l] & 3) == 0;
    int64_t A_lv = 0;
    const int rc = fill_levels(lv, what, cls, cls_stride, reg, reg_stride, grad_cls, grad_reg, pix, L, B, na, C, vec ? 4 : 1, &A_lv);
    if (rc != HTD_OK) return rc;
    HTD_REQUIRE(A_lv == A, "%s: A = %d, the levels hold %lld anchors", what, A, (long long)A_lv);
    for (int l = 0; l < L; ++l)
        HTD_REQUIRE(grad_cls[l] && grad_reg[l] && (((vec ? (uintptr_t)grad_cls[l] : 0) | (uintptr_t)grad_reg[l]) & 15) == 0,
                    "%s: gradient map %d is null or not 16-byte aligned", what, l);
    for (int k = 0; k < 4; ++k) { means.v[k] = means4[k]; stds.v[k] = stds4[k]; }
    return HTD_OK;
}

// ---- device side: each head kernel keeps its own loops and decodes with these -------------------------------------------------

// Pixel row rw (of lv.rrow[L]) of the classification maps: one row [cu units] of one pixel of one image.  A kernel gives a
// row to a whole wavefront, so all of this is found once per row on the scalar unit.
struct ClsRow {
    int l;                                  // level
    unsigned cu;                            // units of the row
    const int64_t *as_row;                  // assigned [na] of the pixel's anchors
    const int64_t *lab_row;                 // gt_labels [K] of the image
    const float *x_row;                     // logits
    float *g_row;                           // their gradients
};

template <int VEC>
__device__ __forceinline__ ClsRow cls_row(const RetinaLevels &lv, int L, unsigned rw, int na, const int64_t *assigned, int A,
                                          const int64_t *gt_labels, int K)
{
    ClsRow r;
    r.l = level_of(lv.rrow, L, rw);
    const unsigned row = rw - lv.rrow[r.l];                                         // b * pix + p
    const unsigned b = row / lv.pix[r.l], p = row - b * lv.pix[r.l];
    r.cu = lv.cu[r.l];
    r.as_row = assigned + (int64_t)b * A + lv.aoff[r.l] + p * (unsigned)na;
    r.lab_row = gt_labels + (int64_t)b * K;
    r.x_row = lv.cls[r.l] + (int64_t)row * r.cu * VEC;
    r.g_row = lv.gcls[r.l] + (int64_t)row * r.cu * VEC;
    return r;
}

// channel ch of a classification row -> its anchor ch / C; c0 = its class ch % C.  inv_c = 1.f / (float)C.  Requires
// ch < 2^20 (the entry points check na * C): the float quotient is then off by one at most, and the two corrections make it
// exact whatever the rounding.
__device__ __forceinline__ unsigned anchor_of_channel(unsigned ch, unsigned C, float inv_c, unsigned &c0)
{
    unsigned a = (unsigned)(((float)ch + 0.5f) * inv_c);
    a -= (a * C > ch) ? 1u : 0u;
    a += ((a + 1u) * C <= ch) ? 1u : 0u;
    c0 = ch - a * C;
    return a;
}

// Unit u (of lv.roff[L], from lv.coff[L] on) of the regression maps: the four deltas of one anchor, or four padding channels.
struct RegUnit {
    int l;                                  // level
    unsigned v;                             // float4 of the level's map (and of its gradient map)
    unsigned row;                           // b * pix + p
    unsigned a;                             // anchor slot of the pixel; >= na: padding
};

__device__ __forceinline__ RegUnit reg_unit(const RetinaLevels &lv, int L, unsigned u)
{
    RegUnit r;
    r.l = level_of(lv.roff, L, u);
    r.v = u - lv.roff[r.l];
    r.row = r.v / lv.ru[r.l];
    r.a = r.v - r.row * lv.ru[r.l];
    return r;
}

// the anchor of a unit with a < na -> its index in anchors [A] and assigned [b][A]
__device__ __forceinline__ unsigned reg_anchor(const RetinaLevels &lv, const RegUnit &r, int na, unsigned &b)
{
    b = r.row / lv.pix[r.l];
    const unsigned p = r.row - b * lv.pix[r.l];
    return lv.aoff[r.l] + p * (unsigned)na + r.a;
}

// bbox2delta of one positive in the reference's fp32 arithmetic (it casts its inputs to float): anchor and gt as x1 y1 x2 y2
__device__ __forceinline__ void delta_target(const float *anchor, const float *gt, const Vec4f &means, const Vec4f &stds,
                                             float (&tgt)[4])
{
    const float4 an = *reinterpret_cast<const float4 *>(anchor);
    const float4 g = *reinterpret_cast<const float4 *>(gt);
    const float px = (an.x + an.z) * 0.5f, py = (an.y + an.w) * 0.5f, pw = an.z - an.x, ph = an.w - an.y;
    const float cx = (g.x + g.z) * 0.5f, cy = (g.y + g.w) * 0.5f, gw = g.z - g.x, gh = g.w - g.y;
    tgt[0] = ((cx - px) / pw - means.v[0]) / stds.v[0];
    tgt[1] = ((cy - py) / ph - means.v[1]) / stds.v[1];
    tgt[2] = (logf(gw / pw) - means.v[2]) / stds.v[2];
    tgt[3] = (logf(gh / ph) - means.v[3]) / stds.v[3];
}

}  // namespace
