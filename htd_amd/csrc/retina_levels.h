// The level table of the dense-head kernels that read the convolution outputs where they lie, and its host-side filling: shared
// by focal_loss.hip (htd_retina_loss, htd_retina_grad_scale, htd_retina_keys) and ghm_loss.hip (htd_ghm_head_loss), so the two
// loss families address the maps in one way and htd_retina_grad_scale serves the gradient maps of both.
#pragma once
#include "common.h"

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

}  // namespace
