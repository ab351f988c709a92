"""fp64 statement of mmcv's RoIAlign (avg pooling) and the case table of the RoIAlign kernel tests -- TEST INFRASTRUCTURE.

Layouts are the kernels': feature maps (B, H, W, C), pooled tiles (n, ph, pw, C), rois (n, 5) = [batch, x1, y1, x2, y2] in image
coordinates.  Everything is computed in float64 from the float32 values the kernels get.

  roi_align_ref_slow   the operator's per-sample definition, one bilinear read per sample (small cases only)
  roi_align_ref        the same operator with per-axis hat-function weights and einsum; returns (out, A), A = the operator
                       applied to |feat|: the weights are non-negative, so A is the sum of the absolute terms of every output
  roi_align_ref_bwd    its exact transpose, (grad_feat, A)
  *_levels / *_all     the map picked by roi_level (a level outside [0, L) gives zeros) / every RoI on every level
  near_drop_boundary   RoIs with a sample within 1e-3 px of the drop rule's discontinuity (-1 or extent) that is not exactly on it
  SINGLE_CASES, LEVEL_CASES, make_single, make_levels, *_form   the shared case table, its inputs, and the launchers' dispatch
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

D64 = torch.float64
EPS32 = 2.0 ** -24
# c_oracle: the largest |C oracle - reference| / (2^-24 * A) over the whole case table, forward and backward, as
# test_roi_align_ref.py measures it on the CPU (it fails when the measured figure passes this one).  The oracle is an fp32
# per-sample implementation of the operator; the kernels factor the weights per axis and pre-multiply 1 / count, a few more
# roundings per term, so the GPU tests allow them C_BOUND = 4 * c_oracle.
# Measured 7982.3 (case L3, forward; the next are 1906 and 718, the median case is near 50).  It is not summation order that sets
# it but the float32 sample coordinates: a coordinate carries up to 1e-5 px of rounding, which moves weight onto a neighbouring
# pixel that A does not count when the sample sits on a pixel centre -- and of 250 000 unit-normal values under such a sample a
# few are a thousand times smaller than their neighbours.  The exact cases, not this bound, are what a one-ulp weight error fails.
C_ORACLE = 8000.0
C_BOUND = 4 * C_ORACLE


# ------------------------------------------------------------------------------------------------ the operator
def _geom(roi, scale, ph, pw, sr, aligned):
    """start_h, start_w, bin_h, bin_w, grid_h, grid_w, count of one RoI, in Python floats (= float64)"""
    off = 0.5 if aligned else 0.0
    x1, y1, x2, y2 = (float(v) * scale - off for v in roi[1:5])
    rw, rh = x2 - x1, y2 - y1
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    gh = sr if sr > 0 else int(math.ceil(rh / ph))
    gw = sr if sr > 0 else int(math.ceil(rw / pw))
    return y1, x1, rh / ph, rw / pw, gh, gw, max(gh * gw, 1)


def roi_align_ref_slow(feat, rois, ph, pw, scale, sampling_ratio, aligned):
    """mmcv's roi_align_forward (avg) sample by sample: (n, ph, pw, C) float64."""
    feat = feat.to(D64)
    B, H, W, C = feat.shape
    n = rois.shape[0]
    out = torch.zeros(n, ph, pw, C, dtype=D64)
    for k in range(n):
        b = int(rois[k, 0])
        if b < 0 or b >= B:
            continue
        sh, sw, bh, bw, gh, gw, count = _geom(rois[k].tolist(), scale, ph, pw, sampling_ratio, aligned)
        for i in range(ph):
            for j in range(pw):
                acc = torch.zeros(C, dtype=D64)
                for iy in range(gh):
                    y = sh + i * bh + (iy + 0.5) * bh / gh
                    for ix in range(gw):
                        x = sw + j * bw + (ix + 0.5) * bw / gw
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yy, xx = max(y, 0.0), max(x, 0.0)
                        yl, xl = int(yy), int(xx)
                        if yl >= H - 1:
                            yl = yh = H - 1
                            yy = float(yl)
                        else:
                            yh = yl + 1
                        if xl >= W - 1:
                            xl = xh = W - 1
                            xx = float(xl)
                        else:
                            xh = xl + 1
                        ly, lx = yy - yl, xx - xl
                        hy, hx = 1.0 - ly, 1.0 - lx
                        acc += hy * hx * feat[b, yl, xl] + hy * lx * feat[b, yl, xh] + ly * hx * feat[b, yh, xl] + ly * lx * feat[b, yh, xh]
                out[k, i, j] = acc / count
    return out


def _samples(rois, scale, bins, sr, aligned, axis):
    """Sample coordinates along one axis: v (n, bins, G) float64, live (n, 1, G) bool (sample index < the RoI's grid), grid (n)."""
    r = rois.to(D64)
    off = 0.5 if aligned else 0.0
    lo = r[:, 1 + axis] * scale - off
    hi = r[:, 3 + axis] * scale - off
    size = hi - lo
    if not aligned:
        size = size.clamp(min=1.0)
    bin_ = size / bins
    grid = torch.full_like(size, float(sr)) if sr > 0 else torch.ceil(size / bins)
    G = max(int(grid.max().item()) if grid.numel() else 0, 1)
    s = torch.arange(G, dtype=D64)
    live = (s[None, :] < grid[:, None])[:, None, :]
    g = grid.clamp(min=1.0)
    idx = torch.arange(bins, dtype=D64)
    v = lo[:, None, None] + idx[None, :, None] * bin_[:, None, None] + (s[None, None, :] + 0.5) * (bin_ / g)[:, None, None]
    return v, live, grid


def _axis_weights(rois, scale, bins, sr, aligned, axis, extent):
    """Hat-function weights (n, bins, extent) of the kept samples of every bin along one axis, and the grid (n)."""
    v, live, grid = _samples(rois, scale, bins, sr, aligned, axis)
    keep = live & ~((v < -1.0) | (v > extent))
    vc = v.clamp(0.0, float(extent - 1))
    p = torch.arange(extent, dtype=D64)
    hat = (1.0 - (vc[..., None] - p).abs()).clamp(min=0.0) * keep[..., None]
    return hat.sum(2), grid


def _operator(rois, B, H, W, ph, pw, scale, sr, aligned):
    wy, gh = _axis_weights(rois, scale, ph, sr, aligned, 1, H)
    wx, gw = _axis_weights(rois, scale, pw, sr, aligned, 0, W)
    inv = 1.0 / (gh * gw).clamp(min=1.0)
    b = rois[:, 0].to(D64).trunc().long()
    return wy * inv[:, None, None], wx, b


def roi_align_ref(feat, rois, ph, pw, scale, sampling_ratio, aligned):
    """-> (out, A), both (n, ph, pw, C) float64."""
    feat = feat.to(D64)
    B, H, W, C = feat.shape
    wy, wx, b = _operator(rois, B, H, W, ph, pw, scale, sampling_ratio, aligned)
    outs = []
    for f in (feat, feat.abs()):
        out = torch.zeros(rois.shape[0], ph, pw, C, dtype=D64)
        for img in range(B):
            sel = (b == img).nonzero().flatten()
            if sel.numel():
                t = torch.einsum('njc,rck->njrk', wx[sel], f[img])
                out[sel] = torch.einsum('nir,njrk->nijk', wy[sel], t)
        outs.append(out)
    return outs[0], outs[1]


def roi_align_ref_bwd(grad_out, rois, feat_shape, ph, pw, scale, sampling_ratio, aligned):
    """The transpose of roi_align_ref: -> (grad_feat, A), both (B, H, W, C) float64."""
    grad_out = grad_out.to(D64)
    B, H, W, C = feat_shape
    wy, wx, b = _operator(rois, B, H, W, ph, pw, scale, sampling_ratio, aligned)
    outs = []
    for g in (grad_out, grad_out.abs()):
        gf = torch.zeros(B, H, W, C, dtype=D64)
        for img in range(B):
            sel = (b == img).nonzero().flatten()
            if sel.numel():
                t = torch.einsum('nir,nijk->njrk', wy[sel], g[sel])
                gf[img] = torch.einsum('njc,njrk->rck', wx[sel], t)
        outs.append(gf)
    return outs[0], outs[1]


def roi_align_ref_levels(feats, rois, roi_level, ph, pw, scales, sampling_ratio, aligned):
    """SingleRoIExtractor: RoI i pooled from map roi_level[i]; a level outside [0, L) gives zeros.  -> (out, A)"""
    n, C = rois.shape[0], feats[0].shape[3]
    out, A = torch.zeros(n, ph, pw, C, dtype=D64), torch.zeros(n, ph, pw, C, dtype=D64)
    for l, f in enumerate(feats):
        sel = (roi_level == l).nonzero().flatten()
        if sel.numel():
            out[sel], A[sel] = roi_align_ref(f, rois[sel], ph, pw, scales[l], sampling_ratio, aligned)
    return out, A


def roi_align_ref_levels_bwd(grad_out, rois, roi_level, shapes, ph, pw, scales, sampling_ratio, aligned):
    """-> [(grad_feat_l, A_l)] per level"""
    res = []
    for l, shp in enumerate(shapes):
        sel = (roi_level == l).nonzero().flatten()
        res.append(roi_align_ref_bwd(grad_out[sel], rois[sel], shp, ph, pw, scales[l], sampling_ratio, aligned))
    return res


def roi_align_ref_all(feats, rois, ph, pw, scales, sampling_ratio, aligned):
    """AdptRoIExtractor: every RoI pooled on every level.  -> [(out_l, A_l)]"""
    return [roi_align_ref(f, rois, ph, pw, s, sampling_ratio, aligned) for f, s in zip(feats, scales)]


def roi_align_ref_all_bwd(grad_outs, rois, shapes, ph, pw, scales, sampling_ratio, aligned):
    return [roi_align_ref_bwd(g, rois, shp, ph, pw, s, sampling_ratio, aligned) for g, shp, s in zip(grad_outs, shapes, scales)]


def _samples32(rois, scale, bins, sr, aligned, axis):
    """The sample coordinates as the kernels compute them, in float32 steps (numpy float32 arithmetic rounds every operation)."""
    r = rois.numpy().astype(np.float32)
    f = np.float32
    off = f(0.5 if aligned else 0.0)
    lo = r[:, 1 + axis] * f(scale) - off
    hi = r[:, 3 + axis] * f(scale) - off
    size = hi - lo
    if not aligned:
        size = np.maximum(size, f(1.0))
    bin_ = size / f(bins)
    grid = np.full_like(size, f(sr)) if sr > 0 else np.ceil(size / f(bins))
    G = max(int(grid.max()) if grid.size else 0, 1)
    step = bin_ / np.maximum(grid, f(1.0))
    base = lo[:, None] + np.arange(bins, dtype=np.float32)[None, :] * bin_[:, None]
    v = base[:, :, None] + (np.arange(G, dtype=np.float32) + f(0.5))[None, None, :] * step[:, None, None]
    assert v.dtype == np.float32
    return torch.from_numpy(v)


def near_drop_boundary(rois, H, W, ph, pw, scale, sampling_ratio, aligned, tol=1e-3):
    """bool[n]: a sample of the RoI lies within `tol` px of -1 or of the extent on either axis without sitting exactly on it (in
    float64 and in the kernels' float32 arithmetic alike).  `v < -1 || v > extent` is a discontinuity: there a float32 kernel and
    a float64 reference may legitimately keep different samples."""
    flag = torch.zeros(rois.shape[0], dtype=torch.bool)
    for axis, bins, extent in ((0, pw, W), (1, ph, H)):
        v, live, _ = _samples(rois, scale, bins, sampling_ratio, aligned, axis)
        v32 = _samples32(rois, scale, bins, sampling_ratio, aligned, axis).to(D64)
        for edge in (-1.0, float(extent)):
            near = ((v - edge).abs() < tol) | ((v32 - edge).abs() < tol)
            on = (v == edge) & (v32 == edge)
            flag |= (near & ~on & live).flatten(1).any(1)
    return flag


# ------------------------------------------------------------------------------------------------ the launchers' dispatch
# The thresholds of htd_amd/csrc/roi_align.hip, restated: test_roi_align_ref.py::test_cases_select_every_kernel_form holds the case
# table below against them.
MAXP, GL_MAX = 8, 6


def chunks_of(C):
    return (C + 255) // 256


def fwd_form(n, ph, pw, C):
    return 'fwd_split8' if n * ph * pw * chunks_of(C) < 8192 else 'fwd_wave'


def all_fwd_form(L, n, ph, pw, C):
    return 'all_fwd_w8' if L * n * ph * pw * chunks_of(C) < 4 * 8192 else 'all_fwd_w1'


def bwd_form(n, ph, pw, C, H):
    nc = n * chunks_of(C)
    if ph <= MAXP and pw <= MAXP and nc >= 256:
        row_slots = min(H, max(8, -(-16384 // nc)))
        return 'bwd_rows_full' if row_slots >= H else 'bwd_rows_strided'
    return 'bwd_bins'


def gather_ok(ph, pw, L=1):
    return ph <= MAXP and pw <= MAXP and L <= GL_MAX


# ------------------------------------------------------------------------------------------------ the case table
# kind: 'random' (unit-normal values, RoI corners on the 1/8-pixel grid, compared within c * 2^-24 * A), 'exact' (every quantity
# dyadic: compared with torch.equal), 'edge' (exact, and samples sit exactly on -1 and on the extent).
# flags: F = the fixed rows (zero-size, whole image, reversed, over each border, outside on each side, batch -1 and B),
#        D = twenty identical RoIs over one strip, T = every RoI taller than 8 rows, X = a RoI more than 64 columns wide
Single = namedtuple('Single', 'name kind B C H W scale ph pw sr aligned n flags fwd bwd')
SINGLE_CASES = [
    #      name        kind      B  C    H   W    scale  ph pw sr al n     flags  fwd           bwd
    Single('n5',       'random', 2, 256, 9,  13,  1 / 4, 7, 7, 0, 1, 5,    '',    'fwd_split8', 'bwd_bins'),
    Single('n1',       'random', 2, 8,   6,  8,   1 / 4, 7, 7, 2, 1, 1,    '',    'fwd_split8', 'bwd_bins'),
    Single('fixed',    'random', 2, 4,   12, 13,  1 / 8, 7, 7, 2, 0, 65,   'FD',  'fwd_split8', 'bwd_bins'),
    Single('fixed_a',  'random', 2, 8,   10, 13,  1 / 4, 7, 7, 4, 1, 20,   'F',   'fwd_split8', 'bwd_bins'),
    Single('wide',     'random', 2, 4,   5,  150, 1.0,   3, 2, 0, 1, 63,   'FX',  'fwd_split8', 'bwd_bins'),
    Single('tall',     'random', 2, 4,   70, 5,   1.0,   1, 4, 0, 1, 65,   'F',   'fwd_split8', 'bwd_bins'),
    Single('p1',       'random', 2, 260, 8,  8,   1 / 4, 1, 1, 4, 0, 130,  'F',   'fwd_split8', 'bwd_rows_full'),
    Single('p8',       'random', 2, 256, 16, 24,  1 / 4, 8, 8, 1, 1, 63,   'F',   'fwd_split8', 'bwd_bins'),
    Single('p83',      'random', 2, 4,   13, 8,   1 / 8, 8, 3, 2, 1, 20,   'F',   'fwd_split8', 'bwd_bins'),
    Single('p25',      'random', 2, 260, 7,  5,   1 / 4, 2, 5, 0, 0, 33,   'F',   'fwd_split8', 'bwd_bins'),
    Single('p9',       'random', 2, 4,   14, 14,  1 / 4, 9, 9, 0, 1, 300,  'F',   'fwd_wave',   'bwd_bins'),
    Single('wave4',    'random', 2, 4,   9,  13,  1 / 4, 7, 7, 0, 1, 168,  'F',   'fwd_wave',   'bwd_bins'),
    Single('wave260',  'random', 2, 260, 9,  13,  1 / 4, 7, 7, 0, 0, 84,   'F',   'fwd_wave',   'bwd_bins'),
    # one bin over the whole map, four samples a side: a footprint from pixel 18 to 132 walked by the wavefront-per-bin forward
    Single('wide_wave', 'random', 2, 4,  5,  150, 1.0,   8, 1, 4, 1, 1024, 'F',   'fwd_wave',   'bwd_rows_full'),
    Single('tall_wave', 'random', 2, 4,  150, 5,  1.0,   1, 8, 4, 1, 1024, 'F',   'fwd_wave',   'bwd_rows_strided'),
    Single('rows',     'random', 2, 4,   9,  70, 1 / 4, 7, 7, 0, 1, 256,  'FX',  'fwd_wave',   'bwd_rows_full'),
    Single('rows_sr',  'random', 2, 260, 9,  13,  1 / 4, 8, 3, 2, 1, 130, 'F',   'fwd_split8', 'bwd_rows_full'),
    Single('strided',  'random', 2, 4,   20, 8,   1 / 4, 7, 7, 0, 1, 2048, 'FT',  'fwd_wave',   'bwd_rows_strided'),
    Single('w1',       'random', 2, 4,   6,  1,   1 / 4, 7, 7, 0, 1, 20,   'F',   'fwd_split8', 'bwd_bins'),
    Single('h1',       'random', 2, 4,   1,  13,  1 / 4, 7, 7, 4, 0, 20,  'F',   'fwd_split8', 'bwd_bins'),
    Single('m1',       'random', 2, 4,   1,  1,   1 / 4, 2, 5, 0, 1, 20,   'F',   'fwd_split8', 'bwd_bins'),
    Single('odd',      'random', 1, 4,   3,  5,   1 / 4, 2, 5, 1, 1, 20,   'F',   'fwd_split8', 'bwd_bins'),
    Single('x_small',  'exact',  2, 260, 12, 16,  1 / 8, 4, 2, 2, 1, 24,   '',    'fwd_split8', 'bwd_bins'),
    Single('x_wave',   'exact',  2, 4,   10, 12,  1 / 4, 8, 8, 1, 1, 130,  '',    'fwd_wave',   'bwd_bins'),
    Single('x_rows',   'exact',  2, 4,   9,  70,  1 / 4, 1, 2, 4, 1, 256,  'X',   'fwd_split8', 'bwd_rows_full'),
    Single('x_strided', 'exact', 2, 4,   20, 8,   1 / 16, 2, 2, 2, 1, 2048, 'T',  'fwd_wave',   'bwd_rows_strided'),
    Single('x_odd',    'exact',  1, 4,   3,  5,   1 / 4, 2, 1, 4, 1, 9,    '',    'fwd_split8', 'bwd_bins'),
    Single('x_edge',   'edge',   2, 4,   6,  5,   1 / 4, 1, 1, 1, 0, 8,    '',    'fwd_split8', 'bwd_bins'),
    Single('x_edge_r', 'edge',   2, 4,   6,  5,   1 / 4, 1, 1, 1, 0, 256,  '',    'fwd_split8', 'bwd_rows_full'),
    Single('x_edge_w', 'edge',   2, 4,   6,  5,   1 / 4, 1, 1, 1, 0, 8192, '',    'fwd_wave',   'bwd_rows_full'),
]

# maps: ((H, W, scale), ...) finest first; levels are dealt to the RoIs at random from `use` (a level left out stays empty), and with
# the flag F two rows get level -1 and L (zeros).  all_fwd: the form of htd_roi_align_all_levels_fwd at this size.
Levels = namedtuple('Levels', 'name kind B C maps ph pw sr aligned n flags use all_fwd')
_PYR3 = ((16, 24, 1 / 4), (8, 12, 1 / 8), (4, 6, 1 / 16))
_PYR8 = ((9, 13, 1 / 4), (8, 8, 1 / 8), (5, 7, 1 / 16), (4, 4, 1 / 32), (3, 5, 1 / 64), (2, 2, 1 / 128), (1, 3, 1 / 256), (1, 1, 1 / 512))
LEVEL_CASES = [
    Levels('L3',      'random', 2, 256, _PYR3, 7, 7, 0, 1, 20,  'F',  (0, 2), 'all_fwd_w8'),
    Levels('L3_sr',   'random', 2, 260, _PYR3, 8, 3, 2, 0, 65,  'FD', (0, 2), 'all_fwd_w8'),
    Levels('L3_w1',   'random', 2, 4,   _PYR3, 7, 7, 0, 1, 224, 'F',  (0, 1, 2), 'all_fwd_w1'),
    # bins 70 rows tall and 75 columns wide on the finest map; one bin with four samples a side reaching from pixel 11 to 78
    Levels('L3_wide', 'random', 2, 8,   ((70, 150, 1.0), (35, 75, 1 / 2), (18, 38, 1 / 4)), 1, 2, 0, 1, 40, 'FX', (0, 2), 'all_fwd_w8'),
    Levels('L3_big',  'random', 2, 4,   ((88, 88, 1.0), (44, 44, 1 / 2), (22, 22, 1 / 4)), 1, 1, 4, 1, 10923, 'F', (0, 1, 2), 'all_fwd_w1'),
    Levels('L8',      'random', 2, 4,   _PYR8, 2, 5, 2, 0, 65,  'F',  tuple(range(8)), 'all_fwd_w8'),
    Levels('xL3',     'exact',  2, 260, ((12, 16, 1 / 4), (6, 8, 1 / 8), (3, 4, 1 / 16)), 4, 4, 2, 1, 20, '', (0, 2), 'all_fwd_w8'),
    Levels('xL3_w1',  'exact',  2, 4,   ((12, 16, 1 / 4), (6, 8, 1 / 8), (3, 4, 1 / 16)), 8, 8, 1, 1, 171, '', (0, 1, 2), 'all_fwd_w1'),
    Levels('xL8',     'exact',  2, 4,   _PYR8[:2] + ((4, 4, 1 / 16), (2, 2, 1 / 32), (1, 1, 1 / 64), (1, 1, 1 / 64), (1, 1, 1 / 64), (1, 1, 1 / 64)),
           2, 1, 2, 1, 30, '', tuple(range(8)), 'all_fwd_w8'),
]
SINGLE = {c.name: c for c in SINGLE_CASES}
LEVELS = {c.name: c for c in LEVEL_CASES}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _fixed_rows(B, Hi, Wi):
    """the fixed geometry in image coordinates (Hi, Wi = the image the finest map covers)"""
    rows = [[0, 3.0, 5.0, 3.0, 5.0],                                   # zero size
            [B - 1, 0.0, 0.0, Wi, Hi],                                 # the whole image
            [0, 0.75 * Wi, 0.75 * Hi, 0.25 * Wi, 0.25 * Hi],           # reversed
            [0, -0.25 * Wi, 0.25 * Hi, 0.5 * Wi, 0.5 * Hi],            # over the left / top / right / bottom border
            [B - 1, 0.25 * Wi, -0.25 * Hi, 0.5 * Wi, 0.5 * Hi],
            [0, 0.5 * Wi, 0.25 * Hi, 1.25 * Wi, 0.5 * Hi],
            [B - 1, 0.25 * Wi, 0.5 * Hi, 0.5 * Wi, 1.25 * Hi],
            [0, -2.0 * Wi - 16, 0.0, -1.0 * Wi - 16, Hi],              # outside on the left / top / right / bottom
            [0, 0.0, -2.0 * Hi - 16, Wi, -1.0 * Hi - 16],
            [B - 1, 2.0 * Wi + 16, 0.0, 3.0 * Wi + 16, Hi],
            [B - 1, 0.0, 2.0 * Hi + 16, Wi, 3.0 * Hi + 16],
            [-1, 0.0, 0.0, Wi, Hi],                                    # batch index out of range: zeros, no gradient
            [B, 0.0, 0.0, Wi, Hi]]
    return (torch.tensor(rows, dtype=D64) * 8).round() / 8


N_FIXED = 13


def _random_rois(gen, n, B, Hi, Wi, tall=0.0):
    """corners on the 1/8-pixel grid, from a fraction of a map pixel to the whole image, a little over the borders"""
    size = torch.exp(torch.rand(n, 2, generator=gen, dtype=D64) * math.log(40.0)) / 40.0            # 1/40 .. 1 of the image
    w, h = size[:, 0] * Wi, size[:, 1] * Hi
    if tall:
        h = h.clamp(min=tall)
    cx = (torch.rand(n, generator=gen, dtype=D64) * 1.1 - 0.05) * Wi
    cy = (torch.rand(n, generator=gen, dtype=D64) * 1.1 - 0.05) * Hi
    b = torch.randint(0, B, (n, ), generator=gen).to(D64)
    r = torch.stack([b, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    r[:, 1:] = (r[:, 1:] * 8).round() / 8
    return r


def _exact_rois(gen, n, B, H, W, scale, ph, pw, sr, tall=0, wide=False):
    """bin / sr a multiple of 1/8 pixel of the map (H, W, scale), corners on its 1/8-pixel grid, up to two pixels over the borders"""
    def axis(extent, bins, least):
        unit = bins * sr                                                  # size in 1/8 pixels = unit * k
        kmax = max(1, (extent * 8) // unit)
        kmin = min(kmax, max(1, -(-least * 8 // unit)))
        k = torch.randint(kmin, kmax + 1, (n, ), generator=gen)
        size = unit * k
        lo = torch.randint(-16, extent * 8 + 16, (n, ), generator=gen)
        lo = torch.minimum(lo, extent * 8 + 16 - size)
        return lo.to(D64) / 8, (lo + size).to(D64) / 8
    x1, x2 = axis(W, pw, 0)
    y1, y2 = axis(H, ph, tall)
    b = torch.randint(0, B, (n, ), generator=gen).to(D64)
    r = torch.stack([b, x1, y1, x2, y2], 1)
    if wide:
        k = (W * 8) // (pw * sr)
        r[0, 1], r[0, 3] = 0.0, pw * sr * k / 8.0
    r[:, 1:] = (r[:, 1:] + 0.5) / scale                                   # aligned = 1: map pixel -> image coordinate
    return r


def _edge_rois(n, B, H, W, scale):
    """aligned = 0, sampling_ratio = 1, one bin: the one sample of a RoI is its centre.  Centres exactly on -1 and on the extent, per
    axis and at the corners; repeated up to n rows, the batch index alternating."""
    xs, ys = (-1.0, float(W), 1.5), (-1.0, float(H), 2.25)
    rows = [[0, x - 1, y - 1, x + 1, y + 1] for x in xs for y in ys if not (x == 1.5 and y == 2.25)]
    r = torch.tensor(rows, dtype=D64)
    r = r.repeat(-(-n // len(rows)), 1)[:n]
    r[:, 0] = torch.arange(n) % B
    r[:, 1:] = r[:, 1:] / scale
    return r


def _values(gen, shape, kind):
    if kind == 'random':
        return torch.randn(shape, generator=gen, dtype=torch.float32)
    return torch.randint(-8, 9, shape, generator=gen).to(torch.float32)


def _rois_for(c, gen, H, W, scale, B):
    """the RoI list of a case on the map (H, W, scale) (level cases: the coarsest map for exact geometry, else the finest)"""
    Hi, Wi = H / scale, W / scale
    if c.kind == 'edge':
        return _edge_rois(c.n, B, H, W, scale)
    if c.kind == 'exact':
        return _exact_rois(gen, c.n, B, H, W, scale, c.ph, c.pw, c.sr, tall=9 if 'T' in c.flags else 0, wide='X' in c.flags)
    parts = []
    if 'F' in c.flags:
        parts.append(_fixed_rows(B, Hi, Wi))
    if 'D' in c.flags:
        parts.append(torch.tensor([[B - 1, 0.125 * Wi, 0.25 * Hi, 0.75 * Wi, 0.5 * Hi]], dtype=D64).repeat(20, 1))
    if 'X' in c.flags:
        parts.append(torch.tensor([[0, 0.0, 0.125 * Hi, (min(W, 70) - 0.5) / scale, 0.75 * Hi]], dtype=D64))
    fixed = sum(p.shape[0] for p in parts)
    assert fixed <= c.n or not c.flags, c.name
    parts.append(_random_rois(gen, max(c.n - fixed, 0), B, Hi, Wi, tall=9.5 / scale if 'T' in c.flags else 0.0))
    r = torch.cat(parts)[:c.n]
    r[:, 1:] = (r[:, 1:] * 8).round() / 8
    return r


SingleData = namedtuple('SingleData', 'case feat rois grad')
LevelData = namedtuple('LevelData', 'case feats rois levels grad grads shapes scales')


@functools.lru_cache(maxsize=None)
def make_single(name):
    """-> feat (B, H, W, C) f32, rois (n, 5) f32, grad (n, ph, pw, C) f32 of a single-map case"""
    c = SINGLE[name]
    gen = torch.Generator().manual_seed(_seed(name))
    rois = _rois_for(c, gen, c.H, c.W, c.scale, c.B).to(torch.float32)
    assert rois.shape[0] == c.n
    feat = _values(gen, (c.B, c.H, c.W, c.C), c.kind)
    grad = _values(gen, (c.n, c.ph, c.pw, c.C), c.kind)
    return SingleData(c, feat, rois, grad)


@functools.lru_cache(maxsize=None)
def make_levels(name):
    """-> feats [(B, H_l, W_l, C)], rois, levels (n) int64, grad (one for the level list), grads (one per level, all-levels forms)"""
    c = LEVELS[name]
    gen = torch.Generator().manual_seed(_seed(name))
    L = len(c.maps)
    H, W, s = c.maps[2 if c.kind == 'exact' else 0]      # exact: dyadic on the third map, hence on the finer ones; coarser maps of
    rois = _rois_for(c, gen, H, W, s, c.B).to(torch.float32)  # xL8 are 1 x 1 .. 2 x 2 pixels with scales that keep the bins dyadic
    assert rois.shape[0] == c.n
    levels = torch.tensor(c.use)[torch.randint(0, len(c.use), (c.n, ), generator=gen)].to(torch.int64)
    if 'F' in c.flags:
        levels[1] = 0                                    # the whole image on the finest map: the largest footprints
        levels[3], levels[4] = -1, L
    if 'X' in c.flags:
        levels[N_FIXED + (20 if 'D' in c.flags else 0)] = 0          # the wide RoI too
    feats = [_values(gen, (c.B, h, w, c.C), c.kind) for h, w, _ in c.maps]
    grads = [_values(gen, (c.n, c.ph, c.pw, c.C), c.kind) for _ in c.maps]
    return LevelData(c, feats, rois, levels, grads[0], grads, [(c.B, h, w, c.C) for h, w, _ in c.maps], [m[2] for m in c.maps])


# ------------------------------------------------------------------------------------------------ cached references
@functools.lru_cache(maxsize=None)
def ref_single(name):
    """(out, A_out, grad_feat, A_grad, near) of a single-map case; nobody writes into these"""
    d = make_single(name)
    c = d.case
    out, A = roi_align_ref(d.feat, d.rois, c.ph, c.pw, c.scale, c.sr, c.aligned)
    near = near_drop_boundary(d.rois, c.H, c.W, c.ph, c.pw, c.scale, c.sr, c.aligned)
    gf, gA = roi_align_ref_bwd(d.grad[~near], d.rois[~near], d.feat.shape, c.ph, c.pw, c.scale, c.sr, c.aligned)
    return out, A, gf, gA, near


@functools.lru_cache(maxsize=None)
def ref_single_odd(name):
    """(grad_feat, A) of the odd rows of a single-map case (the other rows sit on another level) that are not near the boundary"""
    d = make_single(name)
    c = d.case
    keep = (torch.arange(c.n) % 2 == 1) & ~ref_single(name)[4]
    return roi_align_ref_bwd(d.grad[keep], d.rois[keep], d.feat.shape, c.ph, c.pw, c.scale, c.sr, c.aligned)


@functools.lru_cache(maxsize=None)
def near_levels(name):
    """bool[L][n]: near_drop_boundary of every RoI on every level"""
    d = make_levels(name)
    c = d.case
    return torch.stack([near_drop_boundary(d.rois, h, w, c.ph, c.pw, s, c.sr, c.aligned) for h, w, s in c.maps])


@functools.lru_cache(maxsize=None)
def ref_levels(name):
    """level-list forms: (out, A, [(grad_feat_l, A_l)], near[n]); rows near the boundary on their own level carry no gradient"""
    d = make_levels(name)
    c = d.case
    out, A = roi_align_ref_levels(d.feats, d.rois, d.levels, c.ph, c.pw, d.scales, c.sr, c.aligned)
    nl = near_levels(name)
    lv = d.levels.clamp(0, len(c.maps) - 1)
    near = nl[lv, torch.arange(c.n)] & (d.levels >= 0) & (d.levels < len(c.maps))
    bw = roi_align_ref_levels_bwd(d.grad[~near], d.rois[~near], d.levels[~near], d.shapes, c.ph, c.pw, d.scales, c.sr, c.aligned)
    return out, A, bw, near


@functools.lru_cache(maxsize=None)
def ref_all(name):
    """all-levels forms: ([(out_l, A_l)], [(grad_feat_l, A_l)], near[L][n])"""
    d = make_levels(name)
    c = d.case
    nl = near_levels(name)
    fw = roi_align_ref_all(d.feats, d.rois, c.ph, c.pw, d.scales, c.sr, c.aligned)
    bw = [roi_align_ref_bwd(g[~m], d.rois[~m], shp, c.ph, c.pw, s, c.sr, c.aligned)
          for g, m, shp, s in zip(d.grads, nl, d.shapes, d.scales)]
    return fw, bw, nl
