// What the heads with one prediction per location share (fcos.hip, atss.hip, gfl.hip, vfnet.hip): the table of their maps with
// its host-side checker, the grid and the unit width of their loss kernels, the decoding of a pixel row, the classification
// sweep of those kernels.  One implementation each (point_scale.h adds the kernel that scales finished gradient maps); what differs
// between the heads -- the element of a positive's own class, the per-location box, centerness and distribution terms -- stays in
// their files.
#pragma once
#include "common.h"
#include "focal_elem.h"
#include "loss_units.h"

namespace {

constexpr int POINT_BLOCKS = 2048;          // 256 CUs x 8 blocks: the cap of a memory-bound grid; the rest is grid-stride
constexpr int POINT_MAX_LEVELS = 8;
constexpr int POINT_SLOTS = 3;              // kinds of map per head: 0 classification, 1 and 2 the head's own

int64_t blocks_of(int64_t n) { return (n + 255) / 256; }      // blocks of 256 threads, one per location

struct PointMaps {
    const float *map[POINT_SLOTS][POINT_MAX_LEVELS];
    float *grad[POINT_SLOTS][POINT_MAX_LEVELS];
    unsigned cs[POINT_SLOTS][POINT_MAX_LEVELS];     // channel stride in floats
    unsigned cu[POINT_MAX_LEVELS];          // units per pixel of the classification map (cs[0] / VEC)
    unsigned pix[POINT_MAX_LEVELS];
    unsigned rrow[POINT_MAX_LEVELS + 1];    // prefix sums of B * pix: the pixel rows of all levels
};

// One kind of map as an entry point received it.  A null stride table leaves the slot out; a null pointer table is accepted
// only where the entry point's kernels do not touch it (need_map / need_grad false).
struct PointSlot {
    const float *const *map;
    float *const *grad;
    const int64_t *stride;
    int channels;                           // the least channel stride
    bool need_map, need_grad;
};

// off: the prefix table of the locations (FcosPoints::poff, AtssLevels::aoff), checked by its own filler, L with it.
// vec: units of the classification map (4: float4 units, 1: floats).  float4 access -- vec == 4, or the float4 branch of a keys
// kernel -- needs 16-byte aligned classification rows.  Strides stay below 2^20 and B below 2^16, so no product of two of the
// table's entries leaves 64 bits and rrow[L] = B * off[L] < 2^31 bounds every index into a [B][locations] tensor.
int fill_point_maps(PointMaps &mp, const char *what, const unsigned *off, int L, int B, const PointSlot (&slots)[POINT_SLOTS], int vec)
{
    HTD_REQUIRE(B > 0 && B < 65536, "%s: bad batch size %d", what, B);
    int64_t rrow = 0, elems = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t pix = (int64_t)off[l + 1] - off[l];
        mp.pix[l] = (unsigned)pix;
        mp.rrow[l] = (unsigned)rrow;
        rrow += (int64_t)B * pix;
    }
    for (int l = L; l <= POINT_MAX_LEVELS; ++l) mp.rrow[l] = (unsigned)rrow;
    for (int s = 0; s < POINT_SLOTS; ++s) {
        const PointSlot &sl = slots[s];
        HTD_REQUIRE((sl.map || !sl.need_map) && (sl.grad || !sl.need_grad) && (sl.stride || !(sl.map || sl.grad)),
                    "%s: null table of map kind %d", what, s);
        if (!sl.stride) continue;
        HTD_REQUIRE(sl.channels > 0, "%s: map kind %d has no channel", what, s);
        for (int l = 0; l < L; ++l) {
            const int64_t cs = sl.stride[l];
            const int unit = s == 0 ? vec : 1;
            HTD_REQUIRE(cs >= sl.channels && cs < (1 << 20) && cs % unit == 0, "%s: bad channel stride %lld of map kind %d, level %d",
                        what, (long long)cs, s, l);
            const float *m = sl.map ? sl.map[l] : nullptr;
            float *g = sl.grad ? sl.grad[l] : nullptr;
            HTD_REQUIRE((m || !sl.map) && (g || !sl.grad), "%s: null map of kind %d, level %d", what, s, l);
            const bool f4 = s == 0 && (vec == 4 || ((sl.channels & 3) == 0 && (cs & 3) == 0));
            HTD_REQUIRE(!f4 || (((uintptr_t)m | (uintptr_t)g) & 15) == 0, "%s: classification map of level %d is not 16-byte aligned",
                        what, l);
            mp.map[s][l] = m;
            mp.grad[s][l] = g;
            mp.cs[s][l] = (unsigned)cs;
            if (s == 0) mp.cu[l] = (unsigned)(cs / vec);
            elems += (int64_t)B * mp.pix[l] * cs;
        }
    }
    HTD_REQUIRE(rrow < ((int64_t)1 << 31) && elems < ((int64_t)1 << 40), "%s: more than 2^31 pixel rows or 2^40 map elements", what);
    return HTD_OK;
}

// How a loss kernel sweeps the classification maps: float4 units when C and every channel stride allow them, and 2^group_shift
// lanes per pixel row -- the smallest power of two that holds the widest row, from 4 to 64
struct SweepForm { int vec, group_shift; };

SweepForm sweep_form(int C, const int64_t *cls_stride, int L)
{
    L = L < POINT_MAX_LEVELS ? L : POINT_MAX_LEVELS;     // (the level table's filler refuses more)
    bool v4 = (C & 3) == 0;
    for (int l = 0; l < L && v4; ++l) v4 = cls_stride && (cls_stride[l] & 3) == 0;
    SweepForm f = {v4 ? 4 : 1, 2};
    int64_t widest = 1;
    for (int l = 0; l < L && cls_stride; ++l) widest = cls_stride[l] / f.vec > widest ? cls_stride[l] / f.vec : widest;
    while (f.group_shift < 6 && ((int64_t)1 << f.group_shift) < widest) ++f.group_shift;
    return f;
}

// kernel<VEC, G> (G: the exponent is 2) on the loss grid
#define HTD_POINT_LAUNCH(kernel, vec, g, stream, ...)                                                                              \
    do {                                                                                                                            \
        const dim3 grid_(POINT_BLOCKS), block_(256);                                                                                \
        if ((vec) == 4) {                                                                                                           \
            if (g) hipLaunchKernelGGL((kernel<4, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);                     \
            else hipLaunchKernelGGL((kernel<4, false>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);                      \
        } else {                                                                                                                    \
            if (g) hipLaunchKernelGGL((kernel<1, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);                     \
            else hipLaunchKernelGGL((kernel<1, false>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);                      \
        }                                                                                                                           \
    } while (0)

// ---- device side ---------------------------------------------------------------------------------------------------------------

// Pixel row rw (of mp.rrow[L]): one pixel of one image on one level
struct PointRow {
    int l;                                  // level
    unsigned row;                           // b * pix + p: the row of the level's maps
    unsigned b, p;
    unsigned i;                             // the location among those of an image (off[l] + p): index into anchors [A]
    int64_t o;                              // b * off[L] + i: index into assigned [B][off[L]] and its like
    unsigned cu;                            // units of the classification row
    const float *x_row;                     // its logits
    float *g_row;                           // their gradients
};

__device__ __forceinline__ PointRow point_row(const PointMaps &mp, const unsigned *off, int L, unsigned rw)
{
    PointRow r;
    r.l = level_of(mp.rrow, L, rw);
    r.row = rw - mp.rrow[r.l];
    r.b = r.row / mp.pix[r.l];
    r.p = r.row - r.b * mp.pix[r.l];
    r.i = off[r.l] + r.p;
    r.o = (int64_t)r.b * off[L] + r.i;
    r.cu = mp.cu[r.l];
    r.x_row = mp.map[0][r.l] + (int64_t)r.row * mp.cs[0][r.l];
    r.g_row = mp.grad[0][r.l] + (int64_t)r.row * mp.cs[0][r.l];
    return r;
}

// row of slot s of a decoded pixel row: the map's and the gradient map's
__device__ __forceinline__ const float *slot_row(const PointMaps &mp, int s, const PointRow &r)
{
    return mp.map[s][r.l] + (int64_t)r.row * mp.cs[s][r.l];
}

__device__ __forceinline__ float *slot_grad_row(const PointMaps &mp, int s, const PointRow &r)
{
    return mp.grad[s][r.l] + (int64_t)r.row * mp.cs[s][r.l];
}

// out [stride] = v[0 .. n) and zeros on the padding channels
__device__ __forceinline__ void store_padded(float *out, unsigned stride, const float *v, unsigned n)
{
    for (unsigned k = 0; k < stride; ++k) out[k] = k < n ? v[k] : 0.f;
}

struct NoTail {
    __device__ __forceinline__ void operator()(const PointRow &, bool, unsigned, unsigned) const {}
};

// The classification sweep of a loss kernel (256 threads): 2^group_shift lanes sweep one pixel row [cu units], so a wavefront
// takes 64 >> group_shift rows at a time (80 classes are 20 float4s; a whole wavefront per row would leave two thirds of its
// lanes idle).  A location is positive when assigned holds k + 1 of a gt k < K; its class is gt_labels [b][k], every other
// location's is C: none.  elem(x, own class, q, g) -> the loss of one logit and g = its derivative, q = quality [o] (0 without
// the table); the gradient row receives g * scale and zeros on the padding.  tail(row, positive, sub, gl) then runs on the
// lane group (lane sub of gl) that swept the row.  -> the thread's sum of elem.
template <int VEC, class Elem, class Tail = NoTail>
__device__ __forceinline__ float cls_sweep(const PointMaps &mp, const unsigned *off, int L, int C, const int *__restrict__ assigned,
                                           const int64_t *__restrict__ gt_labels, int K, const float *__restrict__ quality,
                                           float scale, int group_shift, Elem elem, Tail tail = Tail())
{
    const unsigned n_rows = mp.rrow[L];
    float s_cls = 0.f;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned gl = 1u << group_shift, sub = lane & (gl - 1u), rpw = 64u >> group_shift;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    for (unsigned rw0 = wave * rpw; rw0 < n_rows; rw0 += gridDim.x * 4u * rpw) {
        const unsigned rw = rw0 + (lane >> group_shift);
        if (rw >= n_rows) continue;
        const PointRow r = point_row(mp, off, L, rw);
        const int as = assigned[r.o];
        const bool pos = as > 0 && as <= K;
        const int64_t lab = pos ? gt_labels[(int64_t)r.b * K + (as - 1)] : (int64_t)C;
        const float q = quality ? quality[r.o] : 0.f;
        for (unsigned j = sub; j < r.cu; j += gl) {
            const unsigned c0 = j * VEC;
            float go[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) go[k] = 0.f;
            if (c0 < (unsigned)C) {                                                 // (VEC = 4: C % 4 == 0, whole units)
                float xv[VEC];
                load_unit<VEC>(r.x_row, j, xv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    float g;
                    s_cls += elem(xv[k], lab == (int64_t)(c0 + k), q, g);
                    go[k] = g * scale;
                }
            }
            store_unit<VEC>(r.g_row, j, go);
        }
        tail(r, pos, sub, gl);
    }
    return s_cls;
}

}  // namespace
