"""Operator surface of the HTD hot path on MI355X.

Mirrors the names, argument meaning and error behaviour of the `mmcv.ops` entry points
the reference's modules call (mmdet/ops/__init__.py:5-16): `RoIAlign`, `roi_align`,
`nms`, `batched_nms` (+ `soft_nms`, `DeformConv2dPack` in their own modules), and adds
the HTD-specific fused operators (`fuse_global`, `ba_fuse`, `global_avg_pool`,
`group_norm_relu`).  Every op calls libhtd_amd.so through the C ABI (htd_amd/capi.py);
tensors must live on the GPU -- a CPU tensor raises NotImplementedError exactly like the
reference wrappers (build/lib/mmdet/ops/roi_align/roi_align.py:39-40).  No fallbacks.

Memory layout contract: 4-D activations are logical NCHW tensors in
torch.channels_last memory format (= physical NHWC, what the kernels index).
"""
import ctypes
import os

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import capi

CL = torch.channels_last


def _drop_amax(t):
    """t is about to be modified in place by a kernel torch does not see: a maximum carried on it is void (dense.drop_amax)."""
    from . import dense
    dense.drop_amax(t)


def _need_gpu(t, name):
    if not t.is_cuda:
        raise NotImplementedError(f'{name}: only GPU tensors are supported (libhtd_amd.so has no CPU path)')


def nhwc(x):
    """Logical NCHW -> channels_last memory (no copy if already so)."""
    return x.contiguous(memory_format=CL)


def _f32(x, name):
    if x.dtype != torch.float32:
        raise ValueError(f'{name}: expected float32, got {x.dtype}')
    return x


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


_S = capi.current_stream_ptr
_P = capi.ptr


# ====================================================================== RoIAlign
class PyramidTaps:
    """The FPN levels as seen by a SEQUENCE of RoIAlign consumers (stage-1 extractor, stage-2 extractor, BA).  Each
    consumer reads `levels`, and replaces them by identity aliases that its autograd node outputs; the next consumer
    therefore hangs off the previous one instead of off the pyramid itself.  In backward the gradient map of a level
    is then handed from node to node and every node scatter-adds into it IN PLACE: one zero fill and no
    `grad += other` per level instead of one of each per consumer."""

    def __init__(self, feats):
        self.levels = list(feats)

    def __len__(self):
        return len(self.levels)

    def __getitem__(self, i):
        return self.levels[i]

    def tap(self, consumer, first=0, count=1):
        """consumer(*levels[first:first + count]) -> (*outs, one alias per level): the aliases become the levels the next
        consumer reads; -> outs (a tuple)"""
        res = consumer(*self.levels[first:first + count])
        self.levels[first:first + count] = res[-count:]
        return res[:-count]


def chain_outputs(ctx, outs, srcs, chain):
    """What the forward of a node of the gradient hand-off returns: `outs` (a tensor or a tuple), and with `chain`
    an identity alias of every tensor of `srcs` behind them.  Outputs and aliases nobody used arrive in backward as None, not
    as full-size maps of zeros: every such backward passes a handed map on, or returns nothing, when its own output is None."""
    ctx.set_materialize_grads(False)
    if not chain:
        return outs
    return (*(outs if isinstance(outs, tuple) else (outs, )), *[t.view_as(t) for t in srcs])


def _grad_map(handed, shape, dtype, device, zero=False):
    """The map a node's backward writes its share of a gradient into -> (map, acc).  A gradient handed to the node's alias is
    that map itself when a kernel can write it in place (right dtype and shape, channels-last): acc = 1, and the maximum it may
    carry is void (dense.drop_amax: modified behind torch's back).  Otherwise a fresh map: a copy of the handed gradient
    (acc = 1), or with nothing handed uninitialised (acc = 0: the kernel writes every element), zero-filled on request (the
    scatter kernels, which only add)."""
    if handed is not None and handed.dtype == dtype and tuple(handed.shape) == tuple(shape) and \
            handed.is_contiguous(memory_format=CL):
        _drop_amax(handed)
        return handed, 1
    gf = torch.empty(shape, device=device, dtype=dtype, memory_format=CL)
    if handed is not None:
        gf.copy_(handed)
        return gf, 1
    return (gf.zero_() if zero else gf), 0


def _level_maps(handed, write, shapes, dtype, device):
    """_grad_map of every level a multi-level gather launch writes (write[i]) -> (maps, accs); (None, 0) for the others"""
    pairs = [_grad_map(handed[i], shape, dtype, device) if write[i] else (None, 0) for i, shape in enumerate(shapes)]
    return [m for m, _ in pairs], [a for _, a in pairs]


def _roi_level_tables(shapes, scales, *tensor_lists, accs=None):
    """The per-level arguments of a multi-level launch as ctypes arrays -> [one pointer table per tensor list (None: NULL)..., Hs,
    Ws, scales(, accs)]"""
    L = len(shapes)
    tabs = [(ctypes.c_void_p * L)(*[t.data_ptr() if t is not None else None for t in ts]) for ts in tensor_lists]
    tabs += [(ctypes.c_int * L)(*[s_[2] for s_ in shapes]), (ctypes.c_int * L)(*[s_[3] for s_ in shapes]),
             (ctypes.c_float * L)(*[float(v) for v in scales])]
    if accs is not None:
        tabs.append((ctypes.c_int * L)(*accs))
    return tabs


# RoIAlign backward: 'gather' (default) -- a wavefront owns a strip of feature-map pixels and sums the RoIs covering it in
# RoI order: no float atomics, bit-stable, every pixel written once (no memset); 'scatter' -- the atomic kernels.
ROI_BWD = os.environ.get('HTD_ROI_BWD', 'gather')
ROI_BWD_ONE_LAUNCH = True        # gather form: all levels of a SingleRoIExtractor in one launch (False: one launch per level)


def _roi_align_bwd(g, rois, lvls, level, galias, shape, ph, pw, scale, sr, aligned):
    """-> gradient map of one level: galias (+)= RoIAlign^T(g), or a fresh map when nothing was handed down."""
    B, C, H, W = shape
    n = rois.size(0)
    if ROI_BWD != 'gather' or ph > 8 or pw > 8:
        gf, _ = _grad_map(galias, shape, g.dtype, g.device, zero=True)
        capi.call('htd_roi_align_bwd', _P(g), _P(rois), _P(lvls), level, _P(gf), n, B, C, H, W, ph, pw, scale, sr, aligned, _S())
        return gf
    gf, acc = _grad_map(galias, shape, g.dtype, g.device)
    ws = torch.empty(capi.lib().htd_roi_align_bwd_gather_workspace_bytes(n), dtype=torch.uint8, device=g.device)
    # algorithmic bytes: the map written once (+ read when accumulating) + every RoI's 7x7xC gradient read once
    work = ('byte', 4.0 * (B * H * W * C * (1 + acc) + n * ph * pw * C)) if level in (0, None) or lvls is None else ('byte', 0.0)
    capi.call('htd_roi_align_bwd_gather', _P(g), _P(rois), _P(lvls), level if level is not None else 0, _P(gf), n, B, C, H, W,
              ph, pw, scale, sr, aligned, acc, _P(ws), _S(), work=work)
    return gf


ROI_FOLD = os.environ.get('HTD_ROI_FOLD', '1') != '0'                  # 0: every strip folds its RoIs' bins itself (A/B runs)
ROI_FOLD_MAX_BYTES = int(float(os.environ.get('HTD_ROI_FOLD_MAX_GB', '8')) * 2**30)
ROI_FOLD_MIN_ROIS = int(os.environ.get('HTD_ROI_FOLD_MIN_ROIS', '64'))
# One level per RoI (SingleRoIExtractor): a RoI is 7-14 pixels wide on ITS level, one or two strips per row, and the extra pass
# costs more than it saves (2048 RoIs: 470 -> 546 us).  BA pools every RoI from every level: ~20 strips per row on the fine ones.
ROI_FOLD_SINGLE = os.environ.get('HTD_ROI_FOLD_SINGLE', '0') != '0'


def _fold_workspace(n, Hs, L, pw, C, dev):
    """Folded-bin buffer of the two-pass gather backward (htd_roi_align_*_bwd_gather_folded), or None when folding is off, the
    buffer would not fit the cap, or there are too few RoIs for the extra launch to pay."""
    if not ROI_FOLD or n < ROI_FOLD_MIN_ROIS:
        return None
    nbytes = capi.lib().htd_roi_align_fold_workspace_bytes(n, Hs, L, pw, C)
    if nbytes > ROI_FOLD_MAX_BYTES:
        return None
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _roi_align_levels_bwd(g, rois, lvls, handed, need, shapes, ph, pw, scales, sr, aligned):
    """Gradient maps of every level that needs one, ONE launch (htd_roi_align_levels_bwd_gather): handed[i] (+)= RoIAlign_i^T(g),
    or a fresh map where nothing was handed down."""
    L, n = len(shapes), rois.size(0)
    maps, accs = _level_maps(handed, need, shapes, g.dtype, g.device)
    ws = torch.empty(L * capi.lib().htd_roi_align_bwd_gather_workspace_bytes(n), dtype=torch.uint8, device=g.device)
    ptrs, Hs, Ws, sc, ac = _roi_level_tables(shapes, scales, maps, accs=accs)
    B, C = shapes[0][0], shapes[0][1]
    # algorithmic bytes: every map written once (+ read when accumulating) + every RoI's 7x7xC gradient read once
    work = ('byte', 4.0 * (sum(s_[0] * s_[2] * s_[3] * C * (1 + a) for s_, a, m in zip(shapes, accs, maps) if m is not None) +
                           n * ph * pw * C))
    fold = _fold_workspace(n, Hs, L, pw, C, g.device) if (C % 4 == 0 and ROI_FOLD_SINGLE) else None
    if fold is not None:
        capi.call('htd_roi_align_levels_bwd_gather_folded', _P(g), _P(rois), _P(lvls), ptrs, Hs, Ws, sc, ac, L, n, B, C, ph, pw,
                  int(sr), int(bool(aligned)), _P(ws), _P(fold), _S(), work=work, key='htd_roi_align_levels_bwd_gather')
    else:
        capi.call('htd_roi_align_levels_bwd_gather', _P(g), _P(rois), _P(lvls), ptrs, Hs, Ws, sc, ac, L, n, B, C, ph, pw, int(sr),
                  int(bool(aligned)), _P(ws), _S(), work=work)
    return maps


class RoIAlignFunction(Function):
    """mmcv.ops.roi_align semantics (avg pooling, aligned flag, sampling_ratio=0 => adaptive).  chain=True also
    returns an identity alias of `feat` (see PyramidTaps)."""

    @staticmethod
    def forward(ctx, feat, rois, output_size, spatial_scale, sampling_ratio, aligned, chain=False):
        _need_gpu(feat, 'roi_align')
        if rois.dim() != 2 or rois.size(1) != 5:
            raise AssertionError('RoI must be (idx, x1, y1, x2, y2)!')  # roi_align.py:136
        src, feat = feat, nhwc(_f32(feat, 'roi_align'))
        rois = _f32(rois, 'roi_align').contiguous()
        ph, pw = _pair(output_size)
        B, C, H, W = feat.shape
        n = rois.size(0)
        out = torch.empty((n, C, ph, pw), device=feat.device, dtype=feat.dtype, memory_format=CL)
        capi.call('htd_roi_align_fwd', _P(feat), _P(rois), None, 0, _P(out), n, B, C, H, W, ph, pw,
                  float(spatial_scale), int(sampling_ratio), int(bool(aligned)), _S())
        ctx.save_for_backward(rois)
        ctx.args = ((B, C, H, W), ph, pw, float(spatial_scale), int(sampling_ratio), int(bool(aligned)))
        return chain_outputs(ctx, out, (src, ), chain)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, galias=None):
        rois, = ctx.saved_tensors
        (B, C, H, W), ph, pw, scale, sr, aligned = ctx.args
        if not ctx.needs_input_grad[0] or (grad_out is None and galias is None):
            return (None, ) * 7
        if grad_out is None:
            return (galias, ) + (None, ) * 6
        grad_out = nhwc(grad_out)
        gfeat = _roi_align_bwd(grad_out, rois, None, 0, galias, (B, C, H, W), ph, pw, scale, sr, aligned)
        return gfeat, None, None, None, None, None, None


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True,
              chain=False):
    if pool_mode != 'avg':
        raise NotImplementedError("roi_align: only pool_mode='avg' (what the HTD configs use)")
    return RoIAlignFunction.apply(input, rois, output_size, spatial_scale, sampling_ratio, aligned, chain)


class RoIAlign(nn.Module):
    """Drop-in for mmcv.ops.RoIAlign as constructed by BaseRoIExtractor.build_roi_layers
    (roi_extractors/base_roi_extractor.py:49-56): RoIAlign(spatial_scale=1/s, output_size=7,
    sampling_ratio=0) -> aligned=True, avg pooling."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True,
                 use_torchvision=False):
        super().__init__()
        self.output_size = _pair(output_size)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)
        self.pool_mode = pool_mode
        self.aligned = aligned

    def forward(self, input, rois, chain=False):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.pool_mode,
                         self.aligned, chain)

    def __repr__(self):
        return (f'{self.__class__.__name__}(output_size={self.output_size}, spatial_scale={self.spatial_scale}, '
                f'sampling_ratio={self.sampling_ratio}, pool_mode={self.pool_mode}, aligned={self.aligned})')


def roi_align_levels(feats, rois, target_lvls, output_size, scales, sampling_ratio=0, aligned=True):
    """All pyramid levels of SingleRoIExtractor.forward (single_level_roi_extractor.py:81-99) into one
    (N,C,ph,pw) tensor: level i's kernel only touches RoIs with target_lvls == i.  No nonzero(), no
    scatter, no host sync.  Differentiable w.r.t. every feats[i].  feats may be a PyramidTaps (chained gradients)."""
    if isinstance(feats, PyramidTaps):
        return feats.tap(lambda *fs: _RoIAlignLevels.apply(rois, target_lvls, output_size, tuple(scales), sampling_ratio, aligned,
                                                           True, *fs), 0, len(scales))[0]
    return _RoIAlignLevels.apply(rois, target_lvls, output_size, tuple(scales), sampling_ratio, aligned, False, *feats)


class _RoIAlignLevels(Function):
    @staticmethod
    def forward(ctx, rois, lvls, output_size, scales, sampling_ratio, aligned, chain, *feats):
        _need_gpu(feats[0], 'roi_align')
        ph, pw = _pair(output_size)
        rois = _f32(rois, 'roi_align').contiguous()
        lvls = lvls.to(torch.int64).contiguous()
        n, C = rois.size(0), feats[0].size(1)
        # every RoI is written by exactly one level's launch (map_roi_levels clamps to [0, L)): no zero fill
        out = torch.empty((n, C, ph, pw), device=rois.device, dtype=torch.float32, memory_format=CL)
        fs = [nhwc(_f32(f, 'roi_align')) for f in feats]
        shapes = [(f.size(0), C, f.size(2), f.size(3)) for f in fs]
        L = len(fs)
        if n:
            # one launch for all levels; algorithmic bytes: each RoI is pooled on ONE level: write ph*pw*C*4 B,
            # read its footprint, mid-range 21x21 px of the 14..28 px the level mapping yields
            ptrs, Hs, Ws, sc = _roi_level_tables(shapes, scales, fs)
            work = ('byte', n * C * 4.0 * (ph * pw + 21 * 21))
            from . import dense
            if dense.emits('roi'):
                # the tiles go into the head's first FC layer: their maximum rides along for its H2 launches (dense.carried_amax)
                slot = dense._amax_slot(out.device)
                capi.call('htd_roi_align_levels_fwd_amax', ptrs, Hs, Ws, sc, L, _P(rois), _P(lvls), _P(out), n, shapes[0][0], C, ph,
                          pw, int(sampling_ratio), int(bool(aligned)), _P(slot), _S(), key='htd_roi_align_levels_fwd', work=work)
                dense.tag_amax(out, slot)
            else:
                capi.call('htd_roi_align_levels_fwd', ptrs, Hs, Ws, sc, L, _P(rois), _P(lvls), _P(out), n, shapes[0][0], C, ph, pw,
                          int(sampling_ratio), int(bool(aligned)), _S(), work=work)
        ctx.save_for_backward(rois, lvls)
        ctx.args = (shapes, ph, pw, scales, int(sampling_ratio), int(bool(aligned)))
        return chain_outputs(ctx, out, feats, chain)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *galias):
        rois, lvls = ctx.saved_tensors
        shapes, ph, pw, scales, sr, aligned = ctx.args
        handed = list(galias) or [None] * len(shapes)          # (no aliases without chain)
        if g is None:                            # pooled features unused: hand the chained maps on unchanged
            return (None, ) * 7 + tuple(handed)
        g = nhwc(g)
        need = [bool(ctx.needs_input_grad[7 + i]) for i in range(len(shapes))]
        if ROI_BWD == 'gather' and ROI_BWD_ONE_LAUNCH and ph <= 8 and pw <= 8 and rois.size(0) > 0 and len(shapes) <= 6 and any(need):
            grads = _roi_align_levels_bwd(g, rois, lvls, handed, need, shapes, ph, pw, scales, sr, aligned)
            return (None, None, None, None, None, None, None, *grads)
        grads = []
        for i, (B, C, H, W) in enumerate(shapes):
            if not need[i]:
                grads.append(None)
                continue
            grads.append(_roi_align_bwd(g, rois, lvls, i, handed[i], (B, C, H, W), ph, pw, float(scales[i]), sr, aligned))
        return (None, None, None, None, None, None, None, *grads)


class _RoIAlignAllLevels(Function):
    """EVERY RoI pooled from EVERY level (AdptRoIExtractor / BA, adaptative_roi_extractor.py:66-76: one RoIAlign per level over
    the same RoI list) as ONE launch forward (htd_roi_align_all_levels_fwd) and ONE gather launch backward
    (htd_roi_align_all_levels_bwd_gather): launched level by level, the coarse maps' strips each walk all RoIs of their image
    while the rest of the chip idles.  -> (out_0 .. out_{L-1}[, alias_0 .. alias_{L-1}]); same values as L roi_align calls."""

    @staticmethod
    def forward(ctx, rois, output_size, scales, sampling_ratio, aligned, chain, *feats):
        _need_gpu(feats[0], 'roi_align')
        if rois.dim() != 2 or rois.size(1) != 5:
            raise AssertionError('RoI must be (idx, x1, y1, x2, y2)!')  # roi_align.py:136
        ph, pw = _pair(output_size)
        rois = _f32(rois, 'roi_align').contiguous()
        n, C, L = rois.size(0), feats[0].size(1), len(feats)
        fs = [nhwc(_f32(f, 'roi_align')) for f in feats]
        shapes = [(f.size(0), C, f.size(2), f.size(3)) for f in fs]
        outs = [torch.empty((n, C, ph, pw), device=rois.device, dtype=torch.float32, memory_format=CL) for _ in range(L)]
        if n:
            ptrs, optr, Hs, Ws, sc = _roi_level_tables(shapes, scales, fs, outs)
            capi.call('htd_roi_align_all_levels_fwd', ptrs, Hs, Ws, sc, L, _P(rois), optr, n, shapes[0][0], C, ph, pw,
                      int(sampling_ratio), int(bool(aligned)), _S(), work=('byte', L * n * C * 4.0 * ph * pw))
        ctx.save_for_backward(rois)
        ctx.args = (shapes, ph, pw, tuple(float(v) for v in scales), int(sampling_ratio), int(bool(aligned)))
        return chain_outputs(ctx, tuple(outs), feats, chain)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        rois, = ctx.saved_tensors
        shapes, ph, pw, scales, sr, aligned = ctx.args
        L, n = len(shapes), rois.size(0)
        gouts = [nhwc(g) if g is not None else None for g in grads[:L]]
        handed = list(grads[L:]) or [None] * L                 # (no aliases without chain)
        need = [bool(ctx.needs_input_grad[6 + i]) for i in range(L)]
        dev = rois.device
        if n == 0 or ROI_BWD != 'gather' or ph > 8 or pw > 8 or L > 6:
            res = []
            for i, shape in enumerate(shapes):
                if not need[i] or gouts[i] is None:
                    res.append(handed[i] if need[i] else None)
                    continue
                res.append(_roi_align_bwd(gouts[i], rois, None, 0, handed[i], shape, ph, pw, scales[i], sr, aligned))
            return (None, ) * 6 + tuple(res)
        # (a level whose output nobody used gets no launch share: its handed map, if any, goes on unchanged)
        maps, accs = _level_maps(handed, [need[i] and gouts[i] is not None for i in range(L)], shapes, torch.float32, dev)
        if any(m is not None for m in maps):
            ws = torch.empty(L * capi.lib().htd_roi_align_bwd_gather_workspace_bytes(n), dtype=torch.uint8, device=dev)
            gused = [g if m is not None else None for g, m in zip(gouts, maps)]
            gptr, mptr, Hs, Ws, sc, ac = _roi_level_tables(shapes, scales, gused, maps, accs=accs)
            B, C = shapes[0][0], shapes[0][1]
            work = ('byte', 4.0 * sum(s_[0] * s_[2] * s_[3] * C * (1 + a) + n * ph * pw * C
                                      for s_, a, m in zip(shapes, accs, maps) if m is not None))
            fold = _fold_workspace(n, Hs, L, pw, C, dev) if C % 4 == 0 else None
            if fold is not None:
                capi.call('htd_roi_align_all_levels_bwd_gather_folded', gptr, _P(rois), mptr, Hs, Ws, sc, ac, L, n, B, C, ph, pw, sr,
                          aligned, _P(ws), _P(fold), _S(), work=work, key='htd_roi_align_all_levels_bwd_gather')
            else:
                capi.call('htd_roi_align_all_levels_bwd_gather', gptr, _P(rois), mptr, Hs, Ws, sc, ac, L, n, B, C, ph, pw, sr, aligned,
                          _P(ws), _S(), work=work)
        res = [m if m is not None else (handed[i] if need[i] else None) for i, m in enumerate(maps)]
        return (None, ) * 6 + tuple(res)


def roi_align_all_levels(feats, rois, output_size, scales, sampling_ratio=0, aligned=True):
    """[RoIAlign(feats[i], rois) for i] in one launch each way.  feats: list of maps or a PyramidTaps (chained gradients)."""
    L = len(scales)
    if isinstance(feats, PyramidTaps):
        return list(feats.tap(lambda *fs: _RoIAlignAllLevels.apply(rois, output_size, tuple(scales), sampling_ratio, aligned, True,
                                                                   *fs), 0, L))
    return list(_RoIAlignAllLevels.apply(rois, output_size, tuple(scales), sampling_ratio, aligned, False, *list(feats)[:L]))


# ====================================================================== max pooling (ResNet stem)
class MaxPool2dFunction(Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        _need_gpu(x, 'max_pool2d')
        x = nhwc(_f32(x, 'max_pool2d'))
        B, C, H, W = x.shape
        Ho, Wo = (H + 2 * padding - kernel) // stride + 1, (W + 2 * padding - kernel) // stride + 1
        y = torch.empty((B, C, Ho, Wo), device=x.device, dtype=x.dtype, memory_format=CL)
        need = ctx.needs_input_grad[0]
        idx = torch.empty((B, Ho, Wo, C), device=x.device, dtype=torch.int32) if need else None
        from . import dense
        if dense.emits('pool'):                              # the 1x1 layers behind the pool read y on H2: its maximum rides along
            slot = dense._amax_slot(y.device)
            capi.call('htd_max_pool2d_fwd_amax', _P(x), _P(y), _P(idx), B, H, W, C, kernel, stride, padding, _P(slot), _S(),
                      key='htd_max_pool2d_fwd')
            dense.tag_amax(y, slot)
        else:
            capi.call('htd_max_pool2d_fwd', _P(x), _P(y), _P(idx), B, H, W, C, kernel, stride, padding, _S())
        ctx.save_for_backward(idx)
        ctx.args = ((B, C, H, W), kernel, stride, padding)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        (B, C, H, W), kernel, stride, padding = ctx.args
        g = nhwc(g)
        gx = torch.empty((B, C, H, W), device=g.device, dtype=g.dtype, memory_format=CL)
        capi.call('htd_max_pool2d_bwd', _P(g), _P(idx), _P(gx), B, H, W, C, kernel, stride, padding, _S())
        return gx, None, None, None


def max_pool2d(x, kernel_size, stride, padding=0):
    """nn.MaxPool2d(kernel_size, stride, padding) on NHWC maps (the ResNet stem pool)."""
    return MaxPool2dFunction.apply(x, int(kernel_size), int(stride), int(padding))


# ====================================================================== NMS
def nms_sorted_mask(sorted_boxes, iou_threshold, offset=0, seg_offsets=None, max_seg=None):
    """keep mask (uint8) for boxes already sorted by descending score.  With `seg_offsets`
    (int64 device tensor [S+1]) the rows form S independent problems handled in one launch."""
    _need_gpu(sorted_boxes, 'nms')
    b = _f32(sorted_boxes, 'nms').contiguous()
    n = b.size(0)
    keep = torch.zeros(n, dtype=torch.uint8, device=b.device)
    if n == 0:
        return keep
    if seg_offsets is None:
        ws = torch.empty(capi.lib().htd_nms_workspace_bytes(n), dtype=torch.uint8, device=b.device)
        capi.call('htd_nms_sorted', _P(b), _P(keep), n, float(iou_threshold), int(offset), _P(ws), _S())
    else:
        S = seg_offsets.numel() - 1
        max_seg = n if max_seg is None else int(max_seg)
        ncb = (max_seg + 63) // 64
        ws = torch.empty(n * ncb * 8 + 64, dtype=torch.uint8, device=b.device)
        seg64 = seg_offsets.to(torch.int64).contiguous()      # referenced until the launch is queued
        capi.call('htd_nms_sorted_batched', _P(b), _P(seg64), S, n, max_seg,
                  _P(keep), float(iou_threshold), int(offset), _P(ws), _S())
    return keep


def nms(boxes, scores, iou_threshold, offset=0):
    """mmcv.ops.nms: -> (dets (k,5), inds (k,) int64 in descending-score order).
    IoU > iou_threshold suppresses; ties in score keep the lower index first."""
    assert boxes.size(1) == 4 and boxes.size(0) == scores.size(0) and offset in (0, 1)
    _need_gpu(boxes, 'nms')
    order = torch.sort(scores, descending=True, stable=True)[1]
    keep = nms_sorted_mask(boxes[order], iou_threshold, offset)
    inds = order[keep.bool()]
    dets = torch.cat((boxes[inds], scores[inds].reshape(-1, 1)), dim=1)
    return dets, inds


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv.ops.batched_nms (used at dense_heads/rpn_head.py:166-167 and
    core/post_processing/bbox_nms.py:65).  Boxes of different `idxs` never suppress each other.
    Like mmcv, IoUs are taken on boxes shifted by idx*(max_coordinate+1) -- the shift changes fp32
    rounding, so it is reproduced, not optimised away -- but each class is its own segment of one
    batched launch instead of relying on zero overlap (and there is no split_thr loop)."""
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    nms_type = cfg.pop('type', 'nms')
    cfg.pop('split_thr', None)
    if nms_type == 'soft_nms':
        from .soft_nms import soft_nms_batched
        return soft_nms_batched(boxes, scores, idxs, class_agnostic=class_agnostic, **cfg)
    if nms_type != 'nms':
        raise KeyError(f'unsupported nms type {nms_type}')
    thr = cfg.pop('iou_threshold', cfg.pop('iou_thr', None))
    offset = cfg.pop('offset', 0)
    _need_gpu(boxes, 'batched_nms')
    n = boxes.size(0)
    if n == 0:
        return boxes.new_zeros((0, 5)), boxes.new_zeros((0, ), dtype=torch.long)
    if class_agnostic:
        boxes_for_nms = boxes
        idxs = torch.zeros_like(idxs)
    else:
        max_coordinate = boxes.max()
        boxes_for_nms = boxes + (idxs.to(boxes) * (max_coordinate + 1))[:, None]
    order = torch.sort(scores, descending=True, stable=True)[1]          # global score order
    by_cls = torch.sort(idxs[order], stable=True)[1]                     # group by class, order kept inside
    perm = order[by_cls]
    cls_sorted = idxs[perm]
    counts = torch.bincount(cls_sorted)
    seg = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=boxes.device)
    seg[1:] = torch.cumsum(counts, 0)
    max_seg = int(counts.max().item())
    keep_sorted = nms_sorted_mask(boxes_for_nms[perm], thr, offset, seg, max_seg)
    keep_global = torch.zeros(n, dtype=torch.bool, device=boxes.device)
    keep_global[perm] = keep_sorted.bool()
    keep = order[keep_global[order]]
    return torch.cat([boxes[keep], scores[keep, None]], -1), keep


# ====================================================================== fuse_global
class FuseGlobalFunction(Function):
    """out = roi_feats + global_feat[img(roi)] (+ alpha * extra): HTDRoIHead._fuse_global
    htd_roi_head.py:133-141, and with `extra` the x_reg + g + alpha*enhanced of htd_bbox_head.py:163,184."""

    @staticmethod
    def forward(ctx, roi_feats, rois, global_feat, extra, alpha):
        _need_gpu(roi_feats, 'fuse_global')
        assert roi_feats.size(0) == rois.size(0)
        x = nhwc(_f32(roi_feats, 'fuse_global'))
        n, C, ph, pw = x.shape
        B = global_feat.size(0)
        g = global_feat.reshape(B, C).contiguous()
        e = nhwc(extra) if extra is not None else None
        rois = rois.contiguous()
        out = torch.empty_like(x, memory_format=CL)
        from . import dense
        if n and dense.emits('roi'):                         # the FC layer behind this reads `out` on H2: its maximum rides along
            slot = dense._amax_slot(out.device)
            capi.call('htd_fuse_global_fwd_amax', _P(x), _P(rois), _P(g), _P(e), float(alpha), _P(out), n, ph * pw, C, B, _P(slot), _S(),
                      key='htd_fuse_global_fwd')
            dense.tag_amax(out, slot)
        else:
            capi.call('htd_fuse_global_fwd', _P(x), _P(rois), _P(g), _P(e), float(alpha), _P(out), n, ph * pw, C, B, _S())
        ctx.save_for_backward(rois)
        ctx.meta = (tuple(global_feat.shape), float(alpha), extra is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        rois, = ctx.saved_tensors
        gshape, alpha, has_extra = ctx.meta
        go = nhwc(go)
        n, C, ph, pw = go.shape
        gg = None
        if ctx.needs_input_grad[2]:
            gg = _fuse_global_grad(go, rois, n, ph * pw, C, gshape[0]).view(gshape)
        ge = go * alpha if (has_extra and ctx.needs_input_grad[3]) else None
        return go, None, gg, ge, None


def _fuse_global_grad(go, rois, n, P, C, B):
    """grad_global [B, C] = per-image sums of the RoI tile gradients: the bit-reproducible two-pass kernel (no float atomics)."""
    gg = torch.empty(B, C, device=go.device, dtype=go.dtype)
    if C % 4 == 0:
        ws = torch.empty((max(n, 1) + (max(n, 1) + 63) // 64 * B) * C, device=go.device, dtype=go.dtype)
        capi.call('htd_fuse_global_bwd_global_ws', _P(go), _P(rois), _P(gg), n, P, C, B, _P(ws), _S())
    else:
        gg.zero_()
        if n:
            capi.call('htd_fuse_global_bwd_global', _P(go), _P(rois), _P(gg), n, P, C, B, _S())
    return gg


class RowStash:
    """Side channel between PlainAndFusedFunction and select_rows_via: the gradient of the selected rows travels here instead
    of through a full-size dense tensor (see PlainAndFusedFunction)."""

    def __init__(self):
        self.alias = None        # identity alias of roi_feats, output of the PlainAndFused node
        self.rows = self.grad = None
        self.pending = False     # a select hangs off the alias and has not delivered its gradient yet


class PlainAndFusedFunction(Function):
    """(2n, C, ph, pw) = [roi_feats ; roi_feats + global_feat[img(roi)]]: the two inputs the HTD classification FCs run on
    (htd_bbox_head.py:198,201) as one batch, written by ONE kernel that reads roi_feats once (no fuse output, no torch.cat, no
    copy of the plain half); the gradient of roi_feats is ONE sum of the two halves.
    With a RowStash the node also outputs an identity alias of roi_feats for select_rows_via (the stage-2 positives of the
    regression branch, htd_roi_head.py:163-166, whose row indices are known only after this node has been queued): the
    gradient of those few rows is handed over through the stash and added into the sum IN PLACE.  As a second autograd
    consumer of roi_feats, index_select's backward (zero fill + index_add into default-strided storage) and the engine's
    accumulation cost a strided full-size add and a layout copy in the RoIAlign backward: 0.26 ms per step."""

    @staticmethod
    def forward(ctx, roi_feats, rois, global_feat, stash=None):
        _need_gpu(roi_feats, 'fuse_global')
        assert roi_feats.size(0) == rois.size(0)
        x = nhwc(_f32(roi_feats, 'fuse_global'))
        n, C, ph, pw = x.shape
        B = global_feat.size(0)
        g = global_feat.reshape(B, C).contiguous()
        rois = rois.contiguous()
        both = torch.empty((2 * n, C, ph, pw), device=x.device, dtype=x.dtype, memory_format=CL)
        from . import dense
        if n and dense.emits('roi'):
            slot = dense._amax_slot(both.device)
            capi.call('htd_plain_and_fused_fwd_amax', _P(x), _P(rois), _P(g), _P(both), n, ph * pw, C, B, _P(slot), _S(),
                      key='htd_plain_and_fused_fwd')
            dense.tag_amax(both, slot)
        else:
            capi.call('htd_plain_and_fused_fwd', _P(x), _P(rois), _P(g), _P(both), n, ph * pw, C, B, _S())
        ctx.save_for_backward(rois)
        ctx.meta = (tuple(global_feat.shape), n, tuple(x.shape))
        ctx.stash = stash
        ctx.set_materialize_grads(False)
        if stash is None:
            return both
        return both, x.view_as(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, go, galias=None):
        rois, = ctx.saved_tensors
        gshape, n, xshape = ctx.meta
        stash = ctx.stash
        gg = gx = None
        if go is not None:
            go = nhwc(go)
            C, ph, pw = go.shape[1:]
            if ctx.needs_input_grad[2]:
                gg = _fuse_global_grad(go[n:], rois, n, ph * pw, C, gshape[0]).view(gshape)
            if ctx.needs_input_grad[0]:
                gx = torch.add(go[:n], go[n:])
        if galias is not None and ctx.needs_input_grad[0]:       # someone else used the alias densely
            gx = nhwc(galias) if gx is None else gx.add_(galias)
        if stash is not None:
            if stash.pending:
                raise RuntimeError('PlainAndFused: the row selection hanging off its alias has not run its backward yet')
            if stash.grad is not None and ctx.needs_input_grad[0]:
                if gx is None:
                    gx = torch.zeros(xshape, device=stash.grad.device, dtype=stash.grad.dtype).contiguous(memory_format=CL)
                sg = stash.grad
                if gx.is_cuda and gx.dtype == torch.float32 and gx.is_contiguous(memory_format=CL) and sg.dtype == torch.float32 and \
                        (gx[0].numel() % 4) == 0:
                    sg = nhwc(sg)
                    _drop_amax(gx)                                # written behind torch's back
                    capi.call('htd_rows_add', _P(sg), _P(stash.rows.to(torch.int64).contiguous()), _P(gx), sg.size(0), gx.size(0),
                              gx[0].numel(), _S(), work=('byte', 12.0 * sg.numel()))
                else:
                    gx.index_add_(0, stash.rows, stash.grad)      # distinct rows: plain sums, deterministic
            stash.rows = stash.grad = None
        return gx, None, gg, None


class _SelectRowsVia(Function):
    @staticmethod
    def forward(ctx, alias, rows, stash):
        ctx.stash, ctx.rows = stash, rows
        stash.pending = True
        if alias.is_cuda and alias.dtype == torch.float32 and alias.dim() == 4 and alias.is_contiguous(memory_format=CL) and \
                (alias[0].numel() % 4) == 0:
            rows = rows.to(torch.int64).contiguous()
            out = torch.empty((rows.numel(), ) + tuple(alias.shape[1:]), device=alias.device, dtype=alias.dtype, memory_format=CL)
            capi.call('htd_rows_gather', _P(alias), _P(rows), _P(out), rows.numel(), alias.size(0), alias[0].numel(), _S(),
                      work=('byte', 8.0 * out.numel()))
            return out
        return torch.index_select(alias, 0, rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ctx.stash.rows, ctx.stash.grad, ctx.stash.pending = ctx.rows, g, False
        return None, None, None               # delivered through the stash (PlainAndFusedFunction.backward)


def plain_and_fused(roi_feats, rois, global_feat, stash=None):
    """-> both; with a RowStash also stash.alias (see select_rows_via)"""
    if stash is None:
        return PlainAndFusedFunction.apply(roi_feats, rois, global_feat, None)
    both, stash.alias = PlainAndFusedFunction.apply(roi_feats, rois, global_feat, stash)
    return both


def select_rows_via(stash, rows):
    """roi_feats[rows] (rows: int64, no duplicates) read through the alias a plain_and_fused(..., stash) call left in the stash;
    differentiable, the gradient joins the PlainAndFused node's sum in place."""
    return _SelectRowsVia.apply(stash.alias, rows, stash)


def fuse_global(roi_feats, rois, global_feat, extra=None, alpha=1.0):
    return FuseGlobalFunction.apply(roi_feats, rois, global_feat, extra, alpha)


# ====================================================================== BA fusion
class BAFuseFunction(Function):
    """softmax-over-levels weighted sum of the per-level RoI features + P2 border ring
    (AdptRoIExtractor.forward adaptative_roi_extractor.py:76-91).  lvl_feats[0] is also the
    border source (roi_layers[0] on feats[0] is evaluated once, not twice)."""

    @staticmethod
    def forward(ctx, att, edge, *lvl_feats):
        _need_gpu(att, 'ba_fuse')
        L = len(lvl_feats)
        lv = [nhwc(_f32(f, 'ba_fuse')) for f in lvl_feats]
        n, C, ph, pw = lv[0].shape
        att = att.contiguous()
        assert att.shape == (L, n)
        out = torch.empty_like(lv[0], memory_format=CL)
        arr = (ctypes.c_void_p * L)(*[f.data_ptr() for f in lv])
        capi.call('htd_ba_fuse_fwd', arr, L, _P(lv[0]), _P(att), _P(out), n, ph, pw, C, int(edge), _S())
        ctx.save_for_backward(att, *lv)
        ctx.edge = int(edge)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        att, *lv = ctx.saved_tensors
        L = len(lv)
        n, C, ph, pw = lv[0].shape
        go = nhwc(go)
        glv = [torch.empty_like(f, memory_format=CL) for f in lv]
        gatt = torch.empty_like(att)
        arr = (ctypes.c_void_p * L)(*[f.data_ptr() for f in lv])
        garr = (ctypes.c_void_p * L)(*[f.data_ptr() for f in glv])
        # (no border map: the border source is level 0, the kernel adds the ring's gradient into glv[0])
        capi.call('htd_ba_fuse_bwd', arr, L, _P(att), _P(go), garr, None, _P(gatt), n, ph, pw, C, ctx.edge, _S())
        return (gatt, None, *glv)


def ba_fuse(att, lvl_feats, edge):
    return BAFuseFunction.apply(att, edge, *lvl_feats)


# ====================================================================== pooling / GN
class GlobalAvgPoolFunction(Function):
    """(n,C,h,w) -> (n,C,1,1) mean over h*w: nn.AdaptiveAvgPool2d(1) of SFA
    (global_context_head.py:372,386), BA attention (adaptative_roi_extractor.py:38) and the 7x7
    AvgPool of the reg branch (htd_bbox_head.py:122,188)."""

    @staticmethod
    def forward(ctx, x, chain=False):
        """chain=True: -> (pooled, identity alias of x).  A second consumer of x that reads the alias hands its gradient to
        THIS node's backward, which adds the pooling's share into it in place (htd_global_avg_pool_bwd_acc) -- x's producer
        gets one gradient map and autograd has nothing to add (BA: four (n,256,7,7) adds per step)."""
        _need_gpu(x, 'global_avg_pool')
        src, x = x, nhwc(_f32(x, 'global_avg_pool'))
        n, C, h, w = x.shape
        out = torch.empty(n, C, device=x.device, dtype=x.dtype)
        capi.call('htd_global_avg_pool_fwd', _P(x), _P(out), n, h * w, C, _S())
        ctx.shape = (n, C, h, w)
        return chain_outputs(ctx, out.view(n, C, 1, 1), (src, ), chain)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, galias=None):
        n, C, h, w = ctx.shape
        if g is None:
            return galias, None
        g = g.reshape(n, C).contiguous()
        if C % 4:         # the forward kernel takes any C, the backward kernels move float4 of channels: plain tensor arithmetic
            gx = (g / float(h * w)).view(n, C, 1, 1).expand(n, C, h, w)
            return (gx.contiguous(memory_format=CL) if galias is None else gx + galias), None
        gx, acc = _grad_map(galias, (n, C, h, w), g.dtype, g.device)
        capi.call('htd_global_avg_pool_bwd_acc' if acc else 'htd_global_avg_pool_bwd', _P(g), _P(gx), n, h * w, C, _S())
        return gx, None


def global_avg_pool(x, chain=False):
    return GlobalAvgPoolFunction.apply(x, chain)


class GroupNormReLUFunction(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, relu):
        _need_gpu(x, 'group_norm')
        x = nhwc(_f32(x, 'group_norm'))
        n, C, h, w = x.shape
        y = torch.empty_like(x, memory_format=CL)
        mean = torch.empty(n, num_groups, device=x.device, dtype=x.dtype)
        rstd = torch.empty_like(mean)
        from . import dense
        slot = dense._amax_slot(x.device) if (n > 0 and capi.lib().htd_conv2d_set_h2(-1) == 1) else None
        if slot is not None:              # max |y| for the convolution behind this layer (H2 arithmetic, dense.carried_amax)
            capi.call('htd_group_norm_relu_fwd_amax', _P(x), _P(weight), _P(bias), _P(y), _P(mean), _P(rstd), n, h * w, C,
                      int(num_groups), float(eps), int(bool(relu)), _P(slot), _S())
            dense.tag_amax(y, slot)
        else:
            capi.call('htd_group_norm_relu_fwd', _P(x), _P(weight), _P(bias), _P(y), _P(mean), _P(rstd), n, h * w, C,
                      int(num_groups), float(eps), int(bool(relu)), _S())
        ctx.save_for_backward(x, y, weight, mean, rstd)
        ctx.meta = (int(num_groups), int(bool(relu)))
        ctx.bias_ref = bias                   # only its address is used (gradient sink lookup)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y, weight, mean, rstd = ctx.saved_tensors
        G, relu = ctx.meta
        n, C, h, w = x.shape
        gy = nhwc(gy)
        gx = torch.empty_like(x, memory_format=CL)
        from . import dense
        gw = dense.grad_out(weight)           # straight into the flat gradient buffer when the parameters are registered there
        gb = dense.grad_out(ctx.bias_ref) if ctx.bias_ref is not None and ctx.bias_ref.shape == weight.shape else torch.empty_like(weight)
        ws = torch.empty(2 * max(n, 1) * C, device=x.device, dtype=torch.float32)      # per-tile sums, added in a fixed order
        L = capi.lib()
        if n > 0 and L.htd_conv2d_set_h2(-1) == 1 and L.htd_group_norm_bwd_amax_supported(h * w, C, G):
            slot = dense._amax_slot(x.device)
            capi.call('htd_group_norm_relu_bwd_amax', _P(x), _P(y), _P(weight), _P(mean), _P(rstd), _P(gy), _P(gx), _P(gw),
                      _P(gb), n, h * w, C, G, relu, _P(ws), _P(slot), _S(), key='htd_group_norm_relu_bwd_ws')
            dense.tag_amax(gx, slot)
        else:
            capi.call('htd_group_norm_relu_bwd_ws', _P(x), _P(y), _P(weight), _P(mean), _P(rstd), _P(gy), _P(gx), _P(gw),
                      _P(gb), n, h * w, C, G, relu, _P(ws), _S())
        return gx, gw, gb, None, None, None


def group_norm_relu(x, weight, bias, num_groups, eps=1e-5, relu=True):
    return GroupNormReLUFunction.apply(x, weight, bias, num_groups, eps, relu)


class GroupNormMapFunction(Function):
    """y = [relu](GN(x) [+ residual]) on a whole feature map (csrc/group_norm_map.hip): a sample is spread over many workgroups
    by position slabs, where GroupNormReLUFunction's kernels give it one -- the GroupNorm behind every convolution of a
    norm_cfg=dict(type='GN') backbone / neck.  Two launches forward, three backward, no float atomics."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, relu, residual):
        _need_gpu(x, 'group_norm_map')
        x = nhwc(_f32(x, 'group_norm_map'))
        n, C, h, w = x.shape
        if residual is not None:
            if residual.shape != x.shape:
                raise ValueError(f'group_norm_map: residual {tuple(residual.shape)} against x {tuple(x.shape)}')
            residual = nhwc(_f32(residual, 'group_norm_map'))
        y = torch.empty_like(x, memory_format=CL)
        mean = torch.empty(n, num_groups, device=x.device, dtype=x.dtype)
        rstd = torch.empty_like(mean)
        L = capi.lib()
        ws = torch.empty(L.htd_group_norm_map_workspace_bytes(n, h * w, C, int(num_groups)), dtype=torch.uint8, device=x.device)
        from . import dense
        slot = dense._amax_slot(x.device) if (n > 0 and L.htd_conv2d_set_h2(-1) == 1) else None
        capi.call('htd_group_norm_map_fwd', _P(x), _P(residual), _P(weight), _P(bias), _P(y), _P(mean), _P(rstd), n, h * w, C,
                  int(num_groups), float(eps), int(bool(relu)), _P(ws), _P(slot), _S(),
                  work=('byte', 4.0 * x.numel() * (3 + (residual is not None))))
        if slot is not None:              # max |y| for the convolution behind this layer (H2 arithmetic, dense.carried_amax)
            dense.tag_amax(y, slot)
        ctx.save_for_backward(x, y, weight, mean, rstd)
        ctx.meta = (int(num_groups), int(bool(relu)), residual is not None)
        ctx.bias_ref = bias                   # only its address is used (gradient sink lookup)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y, weight, mean, rstd = ctx.saved_tensors
        G, relu, has_res = ctx.meta
        n, C, h, w = x.shape
        gy = nhwc(gy)
        gx = torch.empty_like(x, memory_format=CL)
        # the residual's gradient is the masked gy; without a ReLU that is gy itself and the kernel writes nothing
        gres = torch.empty_like(x, memory_format=CL) if (has_res and relu and ctx.needs_input_grad[6]) else None
        from . import dense
        gw = dense.grad_out(weight)           # straight into the flat gradient buffer when the parameters are registered there
        gb = dense.grad_out(ctx.bias_ref) if ctx.bias_ref is not None and ctx.bias_ref.shape == weight.shape else torch.empty_like(weight)
        L = capi.lib()
        ws = torch.empty(L.htd_group_norm_map_workspace_bytes(n, h * w, C, G), dtype=torch.uint8, device=x.device)
        slot = dense._amax_slot(x.device) if (n > 0 and L.htd_conv2d_set_h2(-1) == 1) else None
        capi.call('htd_group_norm_map_bwd', _P(x), _P(y), _P(weight), _P(mean), _P(rstd), _P(gy), _P(gx), _P(gres), _P(gw),
                  _P(gb), n, h * w, C, G, relu, _P(ws), _P(slot), _S(),
                  work=('byte', 4.0 * x.numel() * (7 + (gres is not None))))
        if slot is not None:
            dense.tag_amax(gx, slot)
        if has_res and not relu and ctx.needs_input_grad[6]:
            gres = gy
        return gx, gw, gb, None, None, None, gres


def group_norm_map(x, weight, bias, num_groups, eps=1e-5, relu=True, residual=None):
    """[relu](GroupNorm(x) [+ residual]) with the whole-map kernels; GPU fp32, C % 4 == 0, 64 <= C <= 2048, C / num_groups a
    power of two in [2, 64] (anything else raises)."""
    return GroupNormMapFunction.apply(x, weight, bias, num_groups, eps, relu, residual)


def use_group_norm_map(x, num_groups=None):
    """Which GroupNorm kernels take the (n, C, h, w) tensor x.  The RoI-tile kernels of group_norm_relu give a sample one workgroup:
    right for thousands of tiles.  The map kernels take what those cannot cover: fewer samples than the part has compute units
    (n < 256) and more positions than any RoI tile of any config has (h * w > 14 * 14) -- where they support the shape (C % 4 == 0,
    64 <= C <= 2048, C / num_groups a power of two in [2, 64]); any other layer stays where it ran before."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) < 256 and x.size(2) * x.size(3) > 196):
        return False
    C = x.size(1)
    if C % 4 or C < 64 or C > 2048:
        return False
    if num_groups is None:
        return True
    cpg = C // num_groups if num_groups > 0 and C % num_groups == 0 else 0
    return 2 <= cpg <= 64 and cpg & (cpg - 1) == 0


def _weight_standardize_ref(w, eps):
    """mmcv-knowledge (mmcv 1.2.1 ConvWS2d / conv_ws_2d): per output channel, unbiased std, eps added to the std."""
    flat = w.reshape(w.size(0), -1)
    mean = flat.mean(dim=1, keepdim=True)
    std = flat.std(dim=1, keepdim=True)
    return ((flat - mean) / (std + eps)).view_as(w)


class WeightStandardizeFunction(Function):
    """One launch forward (htd_weight_standardize_fwd, keeps each row's mean and 1 / (std + eps)), one backward."""

    @staticmethod
    def forward(ctx, w, eps):
        w = w.contiguous(memory_format=CL) if w.dim() == 4 else w.contiguous()        # KRSC: a row is contiguous
        Co = w.size(0)
        K = w.numel() // max(Co, 1)
        out = torch.empty_like(w, memory_format=CL) if w.dim() == 4 else torch.empty_like(w)
        mean = torch.empty(Co, device=w.device, dtype=w.dtype)
        inv = torch.empty_like(mean)
        capi.call('htd_weight_standardize_fwd', _P(w), _P(out), _P(mean), _P(inv), Co, K, float(eps), _S())
        ctx.save_for_backward(w, mean, inv)
        ctx.eps = float(eps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        w, mean, inv = ctx.saved_tensors
        Co = w.size(0)
        K = w.numel() // Co
        g = g.contiguous(memory_format=CL) if w.dim() == 4 else g.contiguous()
        from . import dense
        gw = dense.grad_out(w)
        capi.call('htd_weight_standardize_bwd', _P(w), _P(mean), _P(inv), _P(g), _P(gw), Co, K, ctx.eps, _S())
        return gw, None


def weight_standardize(w, eps=1e-5):
    """(w - mean) / (std + eps) per output channel over Ci * kh * kw (mmcv-knowledge: ConvWS2d of mmcv 1.2.1: torch.std, i.e.
    the unbiased estimator, eps beside the root).  GPU fp32: the HIP kernels; otherwise the tensor formula."""
    if w.is_cuda and w.dtype == torch.float32:
        return WeightStandardizeFunction.apply(w, eps)
    return _weight_standardize_ref(w, eps)


# ====================================================================== optimizer step
PARAM_EPOCH = 0


def sgd_momentum_step_(flat_param, flat_grad, flat_momentum, lr_dev, momentum, weight_decay, grad_scale=1.0):
    """In-place SGD(momentum, weight_decay) on flat fp32 buffers; lr_dev is a 1-element device tensor."""
    _need_gpu(flat_param, 'sgd')
    global PARAM_EPOCH
    PARAM_EPOCH += 1        # parameters change behind autograd's version counters: invalidates folded-weight caches
    capi.call('htd_sgd_momentum_step', _P(flat_param), _P(flat_grad), _P(flat_momentum), flat_param.numel(),
              _P(lr_dev), float(momentum), float(weight_decay), float(grad_scale), _S())


# ====================================================================== log buffer (epoch runner)
def log_accumulator(n, device):
    """The fp64 running state of log_accumulate_ for n packed scalars: n sums, the summed weight, the first bad iteration."""
    acc = torch.zeros(n + 2, dtype=torch.float64, device=device)
    acc[n + 1] = -1.0
    return acc


def log_accumulate_(acc, packed, weight, it, loss_index=-1):
    """mmcv LogBuffer.update(log_vars, num_samples) on the device: acc[:n] += weight * packed (fp64), acc[n] += weight,
    acc[n + 1] = it if packed[loss_index] is the first non-finite total loss since acc was reset (log_accumulator).
    One htd_log_accumulate launch on the GPU; CPU tensors (the gloo rehearsal of the runner) take the same arithmetic in
    torch."""
    n = packed.numel()
    loss_index = loss_index % n
    if acc.dtype != torch.float64 or acc.numel() != n + 2 or packed.dtype != torch.float32 or not packed.is_contiguous():
        raise ValueError(f'log_accumulate: acc must be fp64 [{n + 2}] and packed contiguous fp32, got {acc.dtype} '
                         f'[{acc.numel()}] / {packed.dtype}')
    if packed.is_cuda:
        capi.call('htd_log_accumulate', _P(packed), n, loss_index, float(weight), int(it), _P(acc), _S())
        return acc
    acc[:n] += packed.double() * float(weight)
    acc[n] += float(weight)
    if float(acc[n + 1]) < 0 and not bool(torch.isfinite(packed[loss_index])):
        acc[n + 1] = float(it)
    return acc


# ====================================================================== segmented top-k (RPN level ranking, samplers)
TOPK_CHUNK, TOPK_KMAX = 4096, 2048
_TOPK_PLANS = {}       # (segments, numel, device) -> device tables: built once per shape, never per call


def segmented_topk(keys, segments):
    """keys: contiguous float32 tensor; segments: sequence of (start, length, k) over keys.view(-1), 0 <= k <= min(length, 2048).
    -> (idx, val): for every segment, back to back, the positions (inside the segment) and values of its k largest keys in
    descending order, equal keys by ascending position (= `keys[start:start+length].sort(descending=True, stable=True)[:k]`)."""
    _need_gpu(keys, 'segmented_topk')
    keys = _f32(keys, 'segmented_topk')
    assert keys.is_contiguous()
    key = (tuple(segments), keys.numel(), str(keys.device))
    plan = _TOPK_PLANS.get(key)
    if plan is None:
        rows, chunks, out = [], [], 0
        for s, (start, length, k) in enumerate(segments):
            if not (0 <= k <= min(length, TOPK_KMAX)) or start < 0 or start + length > keys.numel():
                raise ValueError('segmented_topk: segment %d = (%d, %d, %d) out of range' % (s, start, length, k))
            rows.append((start, length, k, out))
            out += k
            chunks.extend((s, c) for c in range((length + TOPK_CHUNK - 1) // TOPK_CHUNK))
        if len(_TOPK_PLANS) > 256:
            _TOPK_PLANS.clear()
        plan = _TOPK_PLANS[key] = (len(rows), len(chunks), out,
                                   torch.tensor(rows, dtype=torch.int64, device=keys.device).view(-1, 4) if rows else None,
                                   torch.tensor(chunks, dtype=torch.int32, device=keys.device) if chunks else None)
    S, nchunks, out, segs, tab = plan
    idx = torch.empty(out, device=keys.device, dtype=torch.int64)
    val = torch.empty(out, device=keys.device, dtype=torch.float32)
    if S == 0 or out == 0:
        return idx, val
    ws = torch.empty(capi.lib().htd_segmented_topk_workspace_bytes(S, nchunks), dtype=torch.uint8, device=keys.device)
    capi.call('htd_segmented_topk', _P(keys), _P(segs), _P(tab) if tab is not None else None, S, nchunks, _P(idx), _P(val),
              _P(ws), _S())
    return idx, val


# ====================================================================== sigmoid focal loss (mmcv.ops.sigmoid_focal_loss)
def sigmoid_focal_loss_tensor(input, target, gamma=2.0, alpha=0.25):
    """The element losses (N, C) of py_sigmoid_focal_loss (mmdet/models/losses/focal_loss.py:10-41) in tensor operations, with
    softplus in place of sigmoid + log so that any finite logit gives a finite loss.  target (N,) int64, C = background."""
    C = input.size(1)
    t = target.view(-1, 1) == torch.arange(C, device=input.device).view(1, -1)
    z = torch.where(t, -input, input)
    sp = torch.nn.functional.softplus(z, beta=1, threshold=1e4)          # = BCEWithLogits(input, t)
    at = torch.where(t, input.new_full((), alpha), input.new_full((), 1 - alpha))
    return at * torch.exp(-gamma * torch.nn.functional.softplus(-z, beta=1, threshold=1e4)) * sp


def _table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _i64s(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


class SigmoidFocalLossFunction(Function):
    """htd_sigmoid_focal_loss: one launch leaves the element losses (reduction 'none' only), their fixed-grid partial sums and the
    derivative; backward scales the derivative.  weight: (N,) per row or None."""

    @staticmethod
    def forward(ctx, input, target, gamma=2.0, alpha=0.25, weight=None, reduction='mean'):
        assert reduction in ('none', 'mean', 'sum')
        if input.dim() != 2 or target.dim() != 1 or target.size(0) != input.size(0) or target.dtype != torch.int64:
            raise ValueError('sigmoid_focal_loss: input (N, C) float32 and target (N,) int64 expected')
        if weight is not None and (weight.dim() != 1 or weight.size(0) != input.size(0)):
            raise ValueError('sigmoid_focal_loss: weight must have one entry per row')
        if not input.is_cuda:
            with torch.enable_grad():
                x = input.detach().requires_grad_()
                loss = sigmoid_focal_loss_tensor(x, target, gamma, alpha)
                if weight is not None:
                    loss = loss * weight.view(-1, 1)
                grad, = torch.autograd.grad(loss.sum(), x)
            loss = loss.detach()
            out = loss if reduction == 'none' else (loss.sum() if reduction == 'sum' else loss.sum() / max(loss.numel(), 1))
        else:
            x = _f32(input, 'sigmoid_focal_loss').contiguous()
            N, C = x.shape
            w = None if weight is None else _f32(weight, 'sigmoid_focal_loss').contiguous()
            grad = torch.empty_like(x)
            loss = torch.empty_like(x) if reduction == 'none' else None
            partial = torch.empty(capi.lib().htd_focal_loss_partial_rows(), device=x.device, dtype=torch.float32)
            capi.call('htd_sigmoid_focal_loss', _P(x), _P(target.contiguous()), _P(w), N, C, float(gamma), float(alpha), _P(loss),
                      _P(partial), _P(grad), _S())
            out = loss if reduction == 'none' else (partial.sum() if reduction == 'sum' else partial.sum() / max(N * C, 1))
        ctx.save_for_backward(grad)
        ctx.scale = 1.0 / max(input.numel(), 1) if reduction == 'mean' else 1.0
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad * (g * ctx.scale), None, None, None, None, None


def sigmoid_focal_loss(input, target, gamma=2.0, alpha=0.25, weight=None, reduction='mean'):
    """mmcv.ops.sigmoid_focal_loss: input (N, C) logits, target (N,) int64 class indices with C = background."""
    return SigmoidFocalLossFunction.apply(input, target, gamma, alpha, weight, reduction)


class SigmoidFocalLoss(nn.Module):
    def __init__(self, gamma, alpha, weight=None, reduction='mean'):
        super().__init__()
        self.gamma, self.alpha, self.reduction = gamma, alpha, reduction
        self.register_buffer('weight', weight)

    def forward(self, input, target):
        return sigmoid_focal_loss(input, target, self.gamma, self.alpha, self.weight, self.reduction)

    def __repr__(self):
        return f'{self.__class__.__name__}(gamma={self.gamma}, alpha={self.alpha}, reduction={self.reduction})'


def nhwc_channel_stride(m):
    """Per-pixel channel stride of a (B, C, h, w) tensor whose memory is [B][h][w][stride] -- a channels_last map or a channel
    slice of one -- or None for any other layout.  The stride of a size-1 dimension (one channel included) is not looked at."""
    B, C, h, w = m.shape
    sb, sc, sh, sw = m.stride()
    sw = (sb if B > 1 else C) if h * w == 1 else (sh if w == 1 else sw)
    if (C > 1 and sc != 1) or sw < C or (h > 1 and w > 1 and sh != w * sw) or (B > 1 and sb != h * w * sw):
        return None
    return sw


def _level_tables(maps, what='level tables'):
    """channels_last (B, C, h, w) maps (possibly channel slices of wider maps) -> pointer table, channel strides, pixel counts."""
    ptrs, strides, pix = [], [], []
    for m in maps:
        sw = nhwc_channel_stride(m)
        if sw is None:
            raise ValueError(f'{what}: maps must be channels_last (or channel slices of channels_last maps)')
        ptrs.append(m.data_ptr())
        strides.append(sw)
        pix.append(m.size(2) * m.size(3))
    return _table(ptrs), _i64s(strides), _i64s(pix)


def _like_padded(m, stride):
    """An uninitialised gradient map in the memory layout of m: channels_last, a slice of a `stride`-channel map when m is one."""
    full = torch.empty(m.size(0), stride, m.size(2), m.size(3), device=m.device, dtype=torch.float32, memory_format=CL)
    return full if stride == m.size(1) else full[:, :m.size(1)]


def _grad_maps(maps, strides, what):
    """-> gradient maps in the layout of `maps` (a kernel writes their padding as zeros) and their pointer table."""
    grads = [_like_padded(m, s) for m, s in zip(maps, strides)]
    table, gstrides, _ = _level_tables(grads, what)
    assert list(gstrides) == list(strides)
    return grads, table


def _hand_over_once(ctx, what, entry, tables, grads):
    """The backward of a fused head loss whose forward left finished gradient maps: `entry` (..., incoming gradients as device
    scalars, stream) scales the saved maps where they lie (no second pass over a few hundred MB; a factor of exactly 1 is
    skipped on the device) and autograd gets the maps themselves.  So one backward per forward: a second one raises."""
    if getattr(ctx, 'scaled', False):
        raise RuntimeError(f'{what}: a second backward through the same forward (retain_graph=True) is not supported: '
                           'the gradient maps were handed over and scaled in place by the first')
    ctx.scaled = True
    capi.call(entry, *tables, *[_P(g.float().contiguous()) for g in grads], _S())


def _point_tables(what, groups, channels):
    """The per-level maps of a head with one prediction per location, one list per kind of map (None: a kind this call does not
    read), checked: float32 (B, channels[k], h, w) GPU maps (channels[k] None: any count), every kind with the levels, the batch
    and the map sizes of the first.  -> ([(pointer table, channel strides) per kind, (None, None) for a missing one], level sizes,
    their sum), all HOST tables."""
    first = next(g for g in groups if g is not None)
    _need_gpu(first[0], what)
    tabs = []
    for maps, ch in zip(groups, channels):
        if maps is None:
            tabs.append((None, None))
            continue
        if len(maps) != len(first):
            raise ValueError(f'{what}: every kind of map must have one entry per level, got {len(maps)} beside {len(first)}')
        for m, f in zip(maps, first):
            _f32(m, what)
            if m.dim() != 4 or (ch is not None and m.size(1) != ch) or m.shape[-2:] != f.shape[-2:] or m.size(0) != f.size(0):
                raise ValueError(f'{what}: a map of shape {tuple(m.shape)} beside one of shape {tuple(f.shape)}, expected '
                                 f'{"any number of" if ch is None else ch} channels')
        tabs.append(_level_tables(maps, what)[:2])
    sizes = [int(m.shape[-2] * m.shape[-1]) for m in first]
    return tabs, _i64s(sizes), sum(sizes)


def _point_loss_forward(ctx, what, entry, kinds, maps, args, saved=()):
    """The forward of the fused loss of a head with one prediction per location: `entry` (a (table, strides) pair per kind of
    map, *args, partial sums, a gradient table per kind, stream) over `maps` (kind-major, `kinds` lists of L levels) in one
    launch, which leaves the finished gradient maps; they are saved after `saved`.  -> the sums [[a, b], [c, 0]] of the three
    losses, unscaled."""
    L = len(maps) // kinds
    groups = [maps[k * L:(k + 1) * L] for k in range(kinds)]
    tabs = [_level_tables(g, what)[:2] for g in groups]
    grads = [_grad_maps(g, strides, what) for g, (_, strides) in zip(groups, tabs)]
    rows = getattr(capi.lib(), entry + '_partial_rows')()
    partial = torch.empty(rows, 2, device=maps[0].device, dtype=torch.float32)
    capi.call(entry, *[v for t in tabs for v in t], *args, _P(partial), *[table for _, table in grads], _S())
    ctx.point_meta = (kinds, L, len(saved))
    ctx.save_for_backward(*saved, *[g for gs, _ in grads for g in gs])
    return partial.view(2, rows // 2, 2).sum(1)


def _point_loss_backward(ctx, what, entry, args, incoming, arrange=None):
    """The backward of _point_loss_forward: `entry` (the (table, strides) pairs of the saved gradient maps -- or what `arrange`
    makes of the list of pairs --, *args, incoming gradients, stream) through _hand_over_once.  -> the gradient maps."""
    kinds, L, first = ctx.point_meta
    grads = ctx.saved_tensors[first:]
    tabs = [_level_tables(grads[k * L:(k + 1) * L], what)[:2] for k in range(kinds)]
    tables = arrange(tabs) if arrange else [v for t in tabs for v in t]
    _hand_over_once(ctx, what, entry, (*tables, *args), incoming)
    return tuple(grads)


def _anchor_head_backward(ctx, what, g_cls, g_box):
    """-> the gradient maps of retina_loss / ghm_head_loss times the incoming gradients (htd_retina_grad_scale serves both)."""
    na, C, B, L = ctx.meta
    grads = ctx.saved_tensors
    gcls, greg = grads[:L], grads[L:]
    gct, gcs, pix = _level_tables(gcls, what)
    grt, grs, _ = _level_tables(greg, what)
    if all(s % 4 == 0 for s in gcs):
        _hand_over_once(ctx, what, 'htd_retina_grad_scale', (gct, gcs, grt, grs, pix, L, B, na, C), (g_cls, g_box))
        return tuple(grads)
    return tuple(g * g_cls for g in gcls) + tuple(g * g_box for g in greg)


def retina_avg_factor(assigned):
    """(num_pos (B,) int32, avg (1,) float32 = sum_b max(num_pos_b, 1)) on the device (anchor_head.py:288-291)."""
    _need_gpu(assigned, 'retina_avg_factor')
    B, A = assigned.shape
    ws = torch.empty(capi.lib().htd_retina_avg_factor_workspace_bytes(B) // 4, dtype=torch.int32, device=assigned.device)
    num_pos = torch.empty(B, dtype=torch.int32, device=assigned.device)
    avg = torch.empty(1, dtype=torch.float32, device=assigned.device)
    capi.call('htd_retina_avg_factor', _P(assigned.contiguous()), B, A, _P(ws), _P(num_pos), _P(avg), _S())
    return num_pos, avg


class RetinaLossFunction(Function):
    """htd_retina_loss: (sum focal, sum box loss) / avg * loss weights over every level and image in one launch, which also
    writes the finished gradient maps (scaled by loss weight / avg); backward hands them over, after htd_retina_grad_scale
    applies incoming gradients other than 1 on the device, in place.  Single use: a second backward through the same forward
    raises."""

    @staticmethod
    def forward(ctx, na, C, anchors, gts, gt_labels, assigned, avg, means, stds, gamma, alpha, pos_weight, box_loss, beta,
                cls_weight, box_weight, *maps):
        from .core.bbox import _f4
        L = len(maps) // 2
        cls, reg = maps[:L], maps[L:]
        B, A = assigned.shape
        K = gts.size(1)
        ct, cs, pix = _level_tables(cls, 'retina_loss')
        rt, rs, _ = _level_tables(reg, 'retina_loss')
        gcls, gct = _grad_maps(cls, cs, 'retina_loss')
        greg, grt = _grad_maps(reg, rs, 'retina_loss')
        partial = torch.empty(capi.lib().htd_focal_loss_partial_rows(), 2, device=assigned.device, dtype=torch.float32)
        capi.call('htd_retina_loss', ct, cs, rt, rs, pix, L, B, int(na), int(C), _P(anchors), _P(gts), _P(gt_labels), _P(assigned),
                  A, K, _f4(means), _f4(stds), float(gamma), float(alpha), float(pos_weight), int(box_loss), float(beta),
                  _P(avg), float(cls_weight), float(box_weight), _P(partial), gct, grt, _S())
        ctx.meta = (int(na), int(C), B, L)
        ctx.save_for_backward(*gcls, *greg)
        sums = partial.sum(0) / avg
        return sums[0] * cls_weight, sums[1] * box_weight

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box):
        return (None, ) * 16 + _anchor_head_backward(ctx, 'retina_loss', g_cls, g_box)


def retina_loss(cls_maps, reg_maps, na, C, anchors, gts, gt_labels, assigned, avg, means, stds, gamma, alpha, pos_weight,
                box_loss, beta, cls_weight=1.0, box_weight=1.0):
    """-> (loss_cls, loss_bbox) of a RetinaNet-style head from its per-level (B, na * C, h, w) / (B, na * 4, h, w) maps."""
    _need_gpu(assigned, 'retina_loss')
    for m in list(cls_maps) + list(reg_maps):
        _f32(m, 'retina_loss')
    return RetinaLossFunction.apply(na, C, anchors.float().contiguous(), gts.float().contiguous(), gt_labels.contiguous(),
                                    assigned.contiguous(), avg, means, stds, gamma, alpha, pos_weight, box_loss, beta, cls_weight,
                                    box_weight, *cls_maps, *reg_maps)


def retina_keys(cls_maps, na, C):
    """(B, A) max_c sigmoid(score) of every anchor of every level (level-major), one launch (htd_retina_keys)."""
    _need_gpu(cls_maps[0], 'retina_keys')
    for m in cls_maps:
        _f32(m, 'retina_keys')
    ct, cs, pix = _level_tables(cls_maps, 'retina_keys')
    B = cls_maps[0].size(0)
    A = na * sum(pix)
    keys = torch.empty(B, A, device=cls_maps[0].device, dtype=torch.float32)
    capi.call('htd_retina_keys', ct, cs, pix, len(cls_maps), B, int(na), int(C), _P(keys), _S())
    return keys


# ====================================================================== GHM losses (mmdet/models/losses/ghm_loss.py)
GHM_WS_COUNTS, GHM_WS_TOT, GHM_WS_N, GHM_WS_MULT = 0, 1024, 1040, 1056      # word offsets of the workspace (include/htd_amd.h)


def ghm_workspace(L, dev):
    """int32 workspace of the GHM entry points; views of it: ghm_workspace_views."""
    nbytes = capi.lib().htd_ghm_workspace_bytes(int(L))
    if nbytes < 0:
        raise ValueError(f'GHM kernels take 1 .. 8 levels, not {L}')
    return torch.empty(nbytes // 4, dtype=torch.int32, device=dev)


def ghm_workspace_views(ws):
    """-> counts (2, 8, 64) int32 [loss][level][bin], tot (2, 8) int32, n (2, 8) int32, mult (2, 8, 64) float32."""
    return (ws[GHM_WS_COUNTS:GHM_WS_TOT].view(2, 8, 64), ws[GHM_WS_TOT:GHM_WS_N].view(2, 8), ws[GHM_WS_N:GHM_WS_MULT].view(2, 8),
            ws[GHM_WS_MULT:GHM_WS_MULT + 1024].view(torch.float32).view(2, 8, 64))


class GHMCLossFunction(Function):
    """htd_ghmc_loss: histogram, weights and loss + gradient of GHMC.forward in three launches; acc_sum moves in place."""

    @staticmethod
    def forward(ctx, input, target, weight, edges, bins, momentum, acc_sum, loss_weight):
        if input.dim() != 2 or target.dim() != 1 or target.size(0) != input.size(0) or target.dtype != torch.int64:
            raise ValueError('ghmc_loss: input (N, C) float32 and target (N,) int64 expected')
        if weight.dim() != 1 or weight.size(0) != input.size(0):
            raise ValueError('ghmc_loss: weight must have one entry per row')
        _need_gpu(input, 'ghmc_loss')
        x = _f32(input, 'ghmc_loss').contiguous()
        N, C = x.shape
        grad = torch.empty_like(x)
        ws = ghm_workspace(1, x.device)
        partial = torch.empty(capi.lib().htd_focal_loss_partial_rows(), 2, device=x.device, dtype=torch.float32)
        capi.call('htd_ghmc_loss', _P(x), _P(target.contiguous()), _P(weight.float().contiguous()), N, C,
                  _P(_f32(edges, 'ghmc_loss').contiguous()), int(bins), float(momentum), _P(acc_sum) if momentum > 0 else None,
                  float(loss_weight), _P(ws), _P(partial), _P(grad), _S())
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(ws)
        return partial[:, 0].sum(), ws

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        grad, = ctx.saved_tensors
        return grad * g, None, None, None, None, None, None, None


def ghmc_loss(input, target, weight, edges, bins, momentum=0, acc_sum=None, loss_weight=1.0, return_workspace=False):
    """GHMC.forward on an fp32 GPU matrix: input (N, C) logits, target (N,) int64 with C = background, weight (N,).  acc_sum
    (bins,) float32 is updated in place when momentum > 0."""
    if momentum > 0 and (acc_sum is None or not acc_sum.is_contiguous() or acc_sum.dtype != torch.float32):
        raise ValueError('ghmc_loss: momentum > 0 needs a contiguous float32 acc_sum')
    loss, ws = GHMCLossFunction.apply(input, target, weight, edges, bins, momentum, acc_sum, loss_weight)
    return (loss, ws) if return_workspace else loss


class GhmHeadLossFunction(Function):
    """htd_ghm_head_loss: GHMC + GHMR of an anchor head over every level and image, per-level histograms and weights in the
    reference's level order, with the finished gradient maps; backward hands them over after htd_retina_grad_scale applies
    incoming gradients other than 1 in place.  Single use: a second backward through the same forward raises."""

    @staticmethod
    def forward(ctx, na, C, anchors, gts, gt_labels, assigned, means, stds, ghmc, ghmr, ws, *maps):
        from .core.bbox import _f4
        L = len(maps) // 2
        cls, reg = maps[:L], maps[L:]
        B, A = assigned.shape
        K = gts.size(1)
        ct, cs, pix = _level_tables(cls, 'ghm_head_loss')
        rt, rs, _ = _level_tables(reg, 'ghm_head_loss')
        gcls, gct = _grad_maps(cls, cs, 'ghm_head_loss')
        greg, grt = _grad_maps(reg, rs, 'ghm_head_loss')
        edges_c, bins_c, mmt_c, acc_c, w_c = ghmc
        edges_r, bins_r, mmt_r, acc_r, w_r, mu = ghmr
        partial = torch.empty(capi.lib().htd_focal_loss_partial_rows(), 2, device=assigned.device, dtype=torch.float32)
        capi.call('htd_ghm_head_loss', ct, cs, rt, rs, pix, L, B, int(na), int(C), _P(anchors), _P(gts), _P(gt_labels), _P(assigned),
                  A, K, _f4(means), _f4(stds), _P(edges_c), int(bins_c), float(mmt_c), _P(acc_c) if mmt_c > 0 else None,
                  _P(edges_r), int(bins_r), float(mmt_r), _P(acc_r) if mmt_r > 0 else None, float(mu), float(w_c), float(w_r),
                  _P(ws), _P(partial), gct, grt, _S())
        ctx.meta = (int(na), int(C), B, L)
        ctx.save_for_backward(*gcls, *greg)
        sums = partial.sum(0)
        return sums[0], sums[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box):
        return (None, ) * 11 + _anchor_head_backward(ctx, 'ghm_head_loss', g_cls, g_box)


def ghm_head_loss(cls_maps, reg_maps, na, C, anchors, gts, gt_labels, assigned, means, stds, loss_cls, loss_bbox,
                  return_workspace=False):
    """-> (loss_cls, loss_bbox) of an anchor head with the GHMC module loss_cls and the GHMR module loss_bbox from its per-level
    (B, na * C, h, w) / (B, na * 4, h, w) maps; the modules' acc_sum buffers move in place, L times each in level order."""
    _need_gpu(assigned, 'ghm_head_loss')
    for m in list(cls_maps) + list(reg_maps):
        _f32(m, 'ghm_head_loss')
    for mod in (loss_cls, loss_bbox):
        if mod.bins > 64 or not mod.edges.is_cuda or mod.edges.dtype != torch.float32 or not mod.edges.is_contiguous() or \
                (mod.momentum > 0 and not (mod.acc_sum.is_contiguous() and mod.acc_sum.dtype == torch.float32)):
            raise ValueError('ghm_head_loss: at most 64 bins, contiguous float32 edges / acc_sum buffers on the GPU')
    ws = ghm_workspace(len(cls_maps), assigned.device)
    ghmc = (loss_cls.edges, loss_cls.bins, loss_cls.momentum, loss_cls.acc_sum if loss_cls.momentum > 0 else None,
            loss_cls.loss_weight)
    ghmr = (loss_bbox.edges, loss_bbox.bins, loss_bbox.momentum, loss_bbox.acc_sum if loss_bbox.momentum > 0 else None,
            loss_bbox.loss_weight, loss_bbox.mu)
    out = GhmHeadLossFunction.apply(na, C, anchors.float().contiguous(), gts.float().contiguous(), gt_labels.contiguous(),
                                    assigned.contiguous(), means, stds, ghmc, ghmr, ws, *cls_maps, *reg_maps)
    return (out[0], out[1], ws) if return_workspace else out


# ====================================================================== FCOS head (dense_heads/fcos_head.py)
FCOS_BOX_KINDS = dict(IoULoss=0, GIoULoss=2)          # the `kind` of iou_family_loss (csrc/iou_family.h)


def _fcos_levels(featmap_sizes, strides):
    """-> HOST tables hw [L][2] and strides [L] of the pyramid, and P = sum of h * w."""
    sizes = [(int(h), int(w)) for h, w in featmap_sizes]
    strides = [int(s[0] if isinstance(s, (tuple, list)) else s) for s in strides]
    if len(sizes) != len(strides):
        raise ValueError(f'fcos ops: {len(sizes)} map sizes for {len(strides)} strides')
    return _i64s([v for hw in sizes for v in hw]), _i64s(strides), sum(h * w for h, w in sizes)


def fcos_targets(featmap_sizes, strides, regress_ranges, gts, gt_valid, center_sampling=False, radius=1.5, norm_on_bbox=False):
    """htd_fcos_targets: FCOSHead.get_targets and centerness_target of the whole batch in one launch (+ a finishing one).
    gts (B, K, 4) float32 / gt_valid (B, K) bool as pad_gt_batch leaves them.  -> assigned (B, P) int32 (0 background, k + 1 =
    gt k), bbox_targets (B, P, 4), ctr_targets (B, P), num_pos (B,) int32, norm (3,) = [sum num_pos + B, max(sum num_pos, 1),
    sum ctr_targets]; points level-major, nothing read back to the host."""
    _need_gpu(gts, 'fcos_targets')
    gts = _f32(gts, 'fcos_targets').contiguous()
    gt_valid = gt_valid.to(torch.bool).contiguous()
    B, K = gt_valid.shape
    hw, st, P = _fcos_levels(featmap_sizes, strides)
    ranges = (ctypes.c_float * (2 * len(regress_ranges)))(*[float(v) for r in regress_ranges for v in r])
    if len(regress_ranges) != len(st):
        raise ValueError(f'fcos_targets: {len(regress_ranges)} regress ranges for {len(st)} levels')
    dev = gts.device
    assigned = torch.empty(B, P, dtype=torch.int32, device=dev)
    bbox_targets = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
    ctr_targets = torch.empty(B, P, dtype=torch.float32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    norm = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(capi.lib().htd_fcos_targets_workspace_bytes(B, P) // 8, dtype=torch.float64, device=dev)
    capi.call('htd_fcos_targets', hw, st, ranges, len(st), _P(gts), _P(gt_valid), B, K, int(bool(center_sampling)), float(radius),
              int(bool(norm_on_bbox)), _P(assigned), _P(bbox_targets), _P(ctr_targets), _P(ws), _P(num_pos), _P(norm), _S())
    return assigned, bbox_targets, ctr_targets, num_pos, norm


class FcosLossFunction(Function):
    """htd_fcos_loss: the three losses of FCOSHead.loss over every level and image in one launch, which also writes the three
    finished gradient maps (loss weight and normaliser applied); backward hands them over, after htd_fcos_grad_scale applies
    incoming gradients other than 1 on the device, in place.  Single use: a second backward through the same forward raises."""

    @staticmethod
    def forward(ctx, hw, st, C, gt_labels, assigned, bbox_targets, ctr_targets, norm, box_kind, eps, gamma, alpha, cls_weight,
                box_weight, ctr_weight, *maps):
        B, K = gt_labels.shape
        ctx.meta = (hw, st, len(maps) // 3, B, int(C))
        sums = _point_loss_forward(ctx, 'fcos_loss', 'htd_fcos_loss', 3, maps,
                                   (*ctx.meta, _P(gt_labels), K, _P(assigned), _P(bbox_targets), _P(ctr_targets), _P(norm),
                                    int(box_kind), float(eps), float(gamma), float(alpha), float(cls_weight), float(box_weight),
                                    float(ctr_weight)))                 # [[focal, box], [centerness, 0]]
        return sums[0, 0] / norm[0] * cls_weight, sums[0, 1] / norm[2].clamp(min=1e-30) * box_weight, \
            sums[1, 0] / norm[1] * ctr_weight

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box, g_ctr):
        return (None, ) * 15 + _point_loss_backward(ctx, 'fcos_loss', 'htd_fcos_grad_scale', ctx.meta, (g_cls, g_box, g_ctr))


def fcos_loss(cls_maps, reg_maps, ctr_maps, strides, gt_labels, assigned, bbox_targets, ctr_targets, norm, box_kind, eps=1e-6,
              gamma=2.0, alpha=0.25, cls_weight=1.0, box_weight=1.0, ctr_weight=1.0):
    """-> (loss_cls, loss_bbox, loss_centerness) of an FCOS head from its per-level (B, C, h, w) / (B, 4, h, w) / (B, 1, h, w)
    maps and the outputs of fcos_targets.  box_kind: FCOS_BOX_KINDS[type of the box loss]."""
    _point_tables('fcos_loss', (cls_maps, reg_maps, ctr_maps), (None, 4, 1))
    hw, st, P = _fcos_levels([m.shape[-2:] for m in cls_maps], strides)
    if assigned.shape != (cls_maps[0].size(0), P) or assigned.dtype != torch.int32:
        raise ValueError(f'fcos_loss: assigned must be int32 of shape {(cls_maps[0].size(0), P)}')
    return FcosLossFunction.apply(hw, st, cls_maps[0].size(1), gt_labels.contiguous(), assigned.contiguous(),
                                  bbox_targets.contiguous(), ctr_targets.contiguous(), norm, box_kind, eps, gamma, alpha,
                                  cls_weight, box_weight, ctr_weight, *cls_maps, *reg_maps, *ctr_maps)


def fcos_keys(cls_maps, ctr_maps, strides):
    """(B, P) max_c sigmoid(cls) * sigmoid(centerness) of every point of every level (level-major), one launch (htd_fcos_keys)."""
    ((ct, cs), (tt, ts)), _, _ = _point_tables('fcos_keys', (cls_maps, ctr_maps), (None, 1))
    hw, st, P = _fcos_levels([m.shape[-2:] for m in cls_maps], strides)
    B = cls_maps[0].size(0)
    keys = torch.empty(B, P, device=cls_maps[0].device, dtype=torch.float32)
    capi.call('htd_fcos_keys', ct, cs, tt, ts, hw, st, len(cls_maps), B, cls_maps[0].size(1), _P(keys), _S())
    return keys


# ====================================================================== ATSS head (dense_heads/atss_head.py)
def atss_targets(anchors, level_sizes, gts, gt_valid, topk, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.),
                 wh_ratio_clip=16 / 1000):
    """htd_atss_targets: ATSSAssigner.assign, ATSSHead.centerness_target and the averaging factors of ATSSHead.loss for the whole
    batch, nothing read back.  anchors (A, 4) float32 level-major, one per location; level_sizes: anchors per level (host);
    gts (B, K, 4) float32 / gt_valid (B, K) bool as pad_gt_batch leaves them.  -> assigned (B, A) int32 (0 background, k + 1 =
    gt k), ctr_targets (B, A), num_pos (B,) int32, norm (3,) = [sum_b max(num_pos_b, 1), the same, sum ctr_targets]."""
    from .core.bbox import _d4
    _need_gpu(anchors, 'atss_targets')
    anchors = _f32(anchors, 'atss_targets').contiguous()
    gts = _f32(gts, 'atss_targets').contiguous()
    gt_valid = gt_valid.to(torch.bool).contiguous()
    B, K = gt_valid.shape
    A = anchors.size(0)
    if sum(int(n) for n in level_sizes) != A:
        raise ValueError(f'atss_targets: the levels hold {sum(level_sizes)} anchors, the tensor {A}')
    dev = anchors.device
    assigned = torch.empty(B, A, dtype=torch.int32, device=dev)
    ctr_targets = torch.empty(B, A, dtype=torch.float32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    norm = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(capi.lib().htd_atss_targets_workspace_bytes(B, A) // 8, dtype=torch.float64, device=dev)
    capi.call('htd_atss_targets', _P(anchors), _i64s(level_sizes), len(level_sizes), _P(gts), _P(gt_valid), B, K, int(topk),
              _d4(means), _d4(stds), float(wh_ratio_clip), _P(assigned), _P(ctr_targets), _P(ws), _P(num_pos), _P(norm), _S())
    return assigned, ctr_targets, num_pos, norm


class AtssLossFunction(Function):
    """htd_atss_loss: the three losses of ATSSHead.loss over every level and image in one launch, which also writes the three
    finished gradient maps (loss weight and normaliser applied); backward hands them over, after htd_fcos_grad_scale (the
    layouts are FCOS's) applies incoming gradients other than 1 on the device, in place.  Single use: a second backward through
    the same forward raises."""

    @staticmethod
    def forward(ctx, hw, st, sizes, C, anchors, gts, gt_labels, assigned, ctr_targets, norm, means, stds, wh_ratio_clip, box_kind,
                eps, gamma, alpha, cls_weight, box_weight, ctr_weight, *maps):
        from .core.bbox import _d4
        B, K = gt_labels.shape
        L = len(maps) // 3
        ctx.meta = (hw, st, L, B, int(C))
        sums = _point_loss_forward(ctx, 'atss_loss', 'htd_atss_loss', 3, maps,
                                   (sizes, L, B, int(C), _P(anchors), _P(gts), _P(gt_labels), K, _P(assigned), _P(ctr_targets),
                                    _P(norm), _d4(means), _d4(stds), float(wh_ratio_clip), int(box_kind), float(eps), float(gamma),
                                    float(alpha), float(cls_weight), float(box_weight), float(ctr_weight)))
        box_norm = torch.where(norm[2] < 1e-12, torch.ones_like(norm[2]), norm[2])      # atss_head.py:289-290
        return sums[0, 0] / norm[0] * cls_weight, sums[0, 1] / box_norm * box_weight, sums[1, 0] / norm[1] * ctr_weight

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box, g_ctr):
        return (None, ) * 20 + _point_loss_backward(ctx, 'atss_loss', 'htd_fcos_grad_scale', ctx.meta, (g_cls, g_box, g_ctr))


def atss_loss(cls_maps, reg_maps, ctr_maps, strides, anchors, gts, gt_labels, assigned, ctr_targets, norm, means, stds, box_kind,
              eps=1e-6, gamma=2.0, alpha=0.25, cls_weight=1.0, box_weight=1.0, ctr_weight=1.0, wh_ratio_clip=16 / 1000):
    """-> (loss_cls, loss_bbox, loss_centerness) of an ATSS head with one anchor per location from its per-level (B, C, h, w) /
    (B, 4, h, w) / (B, 1, h, w) maps, the (A, 4) anchors, the padded gts and the outputs of atss_targets.  box_kind:
    FCOS_BOX_KINDS[type of the box loss]."""
    _, sizes, _ = _point_tables('atss_loss', (cls_maps, reg_maps, ctr_maps), (None, 4, 1))
    hw, st, A = _fcos_levels([m.shape[-2:] for m in cls_maps], strides)
    if assigned.shape != (cls_maps[0].size(0), A) or assigned.dtype != torch.int32 or anchors.shape != (A, 4):
        raise ValueError(f'atss_loss: assigned must be int32 of shape {(cls_maps[0].size(0), A)}, anchors float32 {(A, 4)}')
    return AtssLossFunction.apply(hw, st, sizes, cls_maps[0].size(1), _f32(anchors, 'atss_loss').contiguous(),
                                  _f32(gts, 'atss_loss').contiguous(), gt_labels.contiguous(), assigned.contiguous(),
                                  ctr_targets.contiguous(), norm, means, stds, wh_ratio_clip, box_kind, eps, gamma, alpha,
                                  cls_weight, box_weight, ctr_weight, *cls_maps, *reg_maps, *ctr_maps)


# ====================================================================== GFL head (dense_heads/gfl_head.py)
def gfl_quality(cls_maps, reg_maps, strides, reg_max, anchors, gts, assigned):
    """htd_gfl_quality: per positive of `assigned` (B, A) (atss_targets) the weight max_c sigmoid(cls) and the IoU score of its
    integral-decoded box with its gt, 0 elsewhere, and the sum of all weights: what the averaging factor of GFLHead.loss and the
    QFL targets are.  -> weight (B, A), score (B, A), wsum (1,); nothing read back."""
    ((ct, cs), (rt, rs)), sizes, A = _point_tables('gfl_quality', (cls_maps, reg_maps), (None, 4 * (int(reg_max) + 1)))
    st = _fcos_levels([m.shape[-2:] for m in cls_maps], strides)[1]
    B, L = cls_maps[0].size(0), len(cls_maps)
    if assigned.shape != (B, A) or assigned.dtype != torch.int32 or anchors.shape != (A, 4) or gts.dim() != 3 or gts.size(0) != B:
        raise ValueError(f'gfl_quality: assigned must be int32 of shape {(B, A)}, anchors float32 {(A, 4)}, gts (B, K, 4)')
    anchors, gts = _f32(anchors, 'gfl_quality').contiguous(), _f32(gts, 'gfl_quality').contiguous()
    dev = assigned.device
    weight = torch.empty(B, A, dtype=torch.float32, device=dev)
    score = torch.empty(B, A, dtype=torch.float32, device=dev)
    wsum = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(max(capi.lib().htd_gfl_quality_workspace_bytes(B, A) // 8, 1), dtype=torch.float64, device=dev)
    capi.call('htd_gfl_quality', ct, cs, rt, rs, sizes, st, L, B, cls_maps[0].size(1), int(reg_max), _P(anchors), _P(gts), gts.size(1),
              _P(assigned.contiguous()), _P(weight), _P(score), _P(wsum), _P(ws), _S())
    return weight, score, wsum


class GflLossFunction(Function):
    """htd_gfl_loss: the three losses of GFLHead.loss over every level and image in one launch, which also writes both finished
    gradient maps (loss weights and normalisers applied); backward hands them over, after htd_gfl_grad_scale applies incoming
    gradients other than 1 on the device, in place.  Single use: a second backward through the same forward raises."""

    @staticmethod
    def forward(ctx, st, sizes, C, reg_max, anchors, gts, gt_labels, assigned, weight, score, norm, wsum, box_kind, eps, beta,
                cls_weight, box_weight, dfl_weight, *maps):
        B, K = gt_labels.shape
        L = len(maps) // 2
        head = (sizes, st, L, B, int(C), int(reg_max))
        ctx.meta = (head, K, int(box_kind), float(eps), float(box_weight), float(dfl_weight))
        sums = _point_loss_forward(ctx, 'gfl_loss', 'htd_gfl_loss', 2, maps,
                                   (*head, _P(anchors), _P(gts), _P(gt_labels), K, _P(assigned), _P(weight), _P(score), _P(norm), _P(wsum), int(box_kind),
                                    float(eps), float(beta), float(cls_weight), float(box_weight), float(dfl_weight)),
                                   saved=(anchors, gts, assigned, weight, wsum, *maps[L:]))        # [[qfl, box], [dfl, 0]]
        # gfl_head.py:364-367: the averaging factor is not clamped (no positive: 0 / 0)
        return sums[0, 0] / norm[0] * cls_weight, sums[0, 1] / wsum[0] * box_weight, sums[1, 0] / (4 * wsum[0]) * dfl_weight

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box, g_dfl):
        head, K, box_kind, eps, box_weight, dfl_weight = ctx.meta
        anchors, gts, assigned, weight, wsum = ctx.saved_tensors[:5]
        rt, rs, _ = _level_tables(ctx.saved_tensors[5:5 + head[2]], 'gfl_loss')

        def arrange(tabs):                                      # the logits' table between the two gradient tables
            (gct, gcs), (grt, grs) = tabs
            assert list(grs) == list(rs)
            return gct, gcs, rt, grt, rs
        return (None, ) * 18 + _point_loss_backward(
            ctx, 'gfl_loss', 'htd_gfl_grad_scale',
            (*head, _P(anchors), _P(gts), K, _P(assigned), _P(weight), _P(wsum), box_kind, eps, box_weight, dfl_weight),
            (g_cls, g_box, g_dfl), arrange)


def gfl_loss(cls_maps, reg_maps, strides, reg_max, anchors, gts, gt_labels, assigned, weight, score, norm, wsum, box_kind,
             eps=1e-6, beta=2.0, cls_weight=1.0, box_weight=1.0, dfl_weight=1.0):
    """-> (loss_cls, loss_bbox, loss_dfl) of a GFL head from its per-level (B, C, h, w) / (B, 4 * (reg_max + 1), h, w) maps, the
    (A, 4) anchors, the padded gts, `assigned` and `norm` of atss_targets and the outputs of gfl_quality.  box_kind:
    FCOS_BOX_KINDS[type of the box loss]."""
    _, sizes, A = _point_tables('gfl_loss', (cls_maps, reg_maps), (None, 4 * (int(reg_max) + 1)))
    st = _fcos_levels([m.shape[-2:] for m in cls_maps], strides)[1]
    B = cls_maps[0].size(0)
    if assigned.shape != (B, A) or assigned.dtype != torch.int32 or anchors.shape != (A, 4) or weight.shape != (B, A) or \
            score.shape != (B, A) or gt_labels.dtype != torch.int64:
        raise ValueError(f'gfl_loss: assigned must be int32 of shape {(B, A)}, anchors float32 {(A, 4)}, weight / score float32 '
                         f'{(B, A)}, gt_labels int64')
    return GflLossFunction.apply(st, sizes, cls_maps[0].size(1), reg_max, _f32(anchors, 'gfl_loss').contiguous(),
                                 _f32(gts, 'gfl_loss').contiguous(), gt_labels.contiguous(), assigned.contiguous(),
                                 _f32(weight, 'gfl_loss').contiguous(), _f32(score, 'gfl_loss').contiguous(),
                                 _f32(norm, 'gfl_loss'), _f32(wsum, 'gfl_loss'), box_kind, eps, beta, cls_weight, box_weight,
                                 dfl_weight, *cls_maps, *reg_maps)


def gfl_decode(cls_maps, reg_maps, strides, reg_max):
    """htd_gfl_decode, one launch: keys (B, A) = max_c sigmoid(cls) and dist (B, A, 4) = integral(reg) * stride of every anchor of
    every level (level-major)."""
    ((ct, cs), (rt, rs)), sizes, A = _point_tables('gfl_decode', (cls_maps, reg_maps), (None, 4 * (int(reg_max) + 1)))
    st = _fcos_levels([m.shape[-2:] for m in cls_maps], strides)[1]
    B = cls_maps[0].size(0)
    keys = torch.empty(B, A, device=cls_maps[0].device, dtype=torch.float32)
    dist = torch.empty(B, A, 4, device=cls_maps[0].device, dtype=torch.float32)
    capi.call('htd_gfl_decode', ct, cs, rt, rs, sizes, st, len(cls_maps), B, cls_maps[0].size(1), int(reg_max), _P(keys), _P(dist),
              _S())
    return keys, dist


# ====================================================================== VFNet head (dense_heads/vfnet_head.py)
class VfnetStarFunction(Function):
    """htd_vfnet_star_fwd / _bwd: the scaled regression logits x (B, 4, H, W) of one level -> bbox_pred = exp(x) * denom and the
    18-channel star offsets of it (vfnet_head.py:246-261,275-314) in one launch; backward folds the offsets' gradient into the
    four sides in one more.  Either incoming gradient may be absent."""

    @staticmethod
    def forward(ctx, x, denom, stride, gradient_mul):
        B, _, H, W = x.shape
        xs = nhwc_channel_stride(x)
        if xs is None:
            x = x.contiguous(memory_format=CL)
            xs = nhwc_channel_stride(x)
        pred = _like_padded(x, xs)
        off = torch.empty(B, 18, H, W, device=x.device, dtype=torch.float32, memory_format=CL)
        capi.call('htd_vfnet_star_fwd', _P(x), xs, B, H, W, float(denom), float(stride), float(gradient_mul), _P(pred), xs, _P(off),
                  18, _S())
        ctx.meta = (B, H, W, xs, float(stride), float(gradient_mul))
        ctx.save_for_backward(pred)
        ctx.set_materialize_grads(False)
        return pred, off

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pred, g_off):
        B, H, W, xs, stride, gm = ctx.meta
        pred, = ctx.saved_tensors
        if g_pred is None and g_off is None:
            return None, None, None, None

        def layout(g):
            if g is None:
                return None, 0
            g = g.float()
            if nhwc_channel_stride(g) is None:
                g = g.contiguous(memory_format=CL)
            return g, nhwc_channel_stride(g)
        g_pred, gps = layout(g_pred)
        g_off, gos = layout(g_off)
        gx = _like_padded(pred, xs)
        capi.call('htd_vfnet_star_bwd', _P(pred), xs, _P(g_pred), gps, _P(g_off), gos, B, H, W, stride, gm, _P(gx), xs, _S())
        return gx, None, None, None


def vfnet_star(x, denom, stride, gradient_mul):
    """-> (bbox_pred (B, 4, H, W), dcn_offset (B, 18, H, W)) of the scaled regression logits x of one level (fp32, GPU)."""
    _need_gpu(x, 'vfnet_star')
    _f32(x, 'vfnet_star')
    if x.dim() != 4 or x.size(1) != 4:
        raise ValueError(f'vfnet_star: x must be (B, 4, H, W), got {tuple(x.shape)}')
    return VfnetStarFunction.apply(x, denom, stride, gradient_mul)


def vfnet_quality(reg_maps, ref_maps, anchors, gts, assigned):
    """htd_vfnet_quality: per positive of `assigned` (B, A) (atss_targets) the IoU of its initial and of its refined box with its
    gt, clamped to at least 1e-6, 0 elsewhere: the box weights, the varifocal targets and, with the number of positives, the three
    averaging factors of VFNetHead.loss.  -> iou_ini (B, A), iou_rf (B, A), sums (3,) = [positives, sum iou_ini, sum iou_rf];
    nothing read back."""
    (_, (rt, rs), (ft, fs)), sizes, A = _point_tables('vfnet_quality', (None, reg_maps, ref_maps), (None, 4, 4))
    B, L = reg_maps[0].size(0), len(reg_maps)
    if assigned.shape != (B, A) or assigned.dtype != torch.int32 or anchors.shape != (A, 4) or gts.dim() != 3 or gts.size(0) != B:
        raise ValueError(f'vfnet_quality: assigned must be int32 of shape {(B, A)}, anchors float32 {(A, 4)}, gts (B, K, 4)')
    anchors, gts = _f32(anchors, 'vfnet_quality').contiguous(), _f32(gts, 'vfnet_quality').contiguous()
    dev = assigned.device
    iou_ini = torch.empty(B, A, dtype=torch.float32, device=dev)
    iou_rf = torch.empty(B, A, dtype=torch.float32, device=dev)
    sums = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(max(capi.lib().htd_vfnet_quality_workspace_bytes(B, A) // 8, 1), dtype=torch.float64, device=dev)
    capi.call('htd_vfnet_quality', rt, rs, ft, fs, sizes, L, B, _P(anchors), _P(gts), gts.size(1), _P(assigned.contiguous()),
              _P(iou_ini), _P(iou_rf), _P(sums), _P(ws), _S())
    return iou_ini, iou_rf, sums


class VfnetLossFunction(Function):
    """htd_vfnet_loss: the three losses of VFNetHead.loss over every level and image in one launch, which also writes the three
    finished gradient maps (loss weights and normalisers applied); backward hands them over, after htd_vfnet_grad_scale applies
    incoming gradients other than 1 on the device, in place.  Single use: a second backward through the same forward raises."""

    @staticmethod
    def forward(ctx, sizes, C, anchors, gts, gt_labels, assigned, iou_ini, iou_rf, sums, box_kind, eps_ini, ref_kind, eps_rf,
                alpha, gamma, iou_weighted, cls_weight, box_weight, ref_weight, *maps):
        B, K = gt_labels.shape
        ctx.meta = (sizes, len(maps) // 3, B, int(C))
        tot = _point_loss_forward(ctx, 'vfnet_loss', 'htd_vfnet_loss', 3, maps,
                                  (*ctx.meta, _P(anchors), _P(gts), _P(gt_labels), K, _P(assigned), _P(iou_ini), _P(iou_rf), _P(sums),
                                   int(box_kind), float(eps_ini), int(ref_kind), float(eps_rf), float(alpha), float(gamma),
                                   int(bool(iou_weighted)), float(cls_weight), float(box_weight), float(ref_weight)))
        norm = sums.clamp(min=1.0)                              # vfnet_head.py:396,414,430: each factor at least 1
        return tot[0, 0] / norm[0] * cls_weight, tot[0, 1] / norm[1] * box_weight, tot[1, 0] / norm[2] * ref_weight

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box, g_ref):
        return (None, ) * 19 + _point_loss_backward(ctx, 'vfnet_loss', 'htd_vfnet_grad_scale', ctx.meta, (g_cls, g_box, g_ref))


def vfnet_loss(cls_maps, reg_maps, ref_maps, anchors, gts, gt_labels, assigned, iou_ini, iou_rf, sums, box_kind, ref_kind,
               eps_ini=1e-6, eps_rf=1e-6, alpha=0.75, gamma=2.0, iou_weighted=True, cls_weight=1.0, box_weight=1.0, ref_weight=1.0):
    """-> (loss_cls, loss_bbox, loss_bbox_rf) of a VFNet head from its per-level (B, C, h, w) / (B, 4, h, w) / (B, 4, h, w) maps,
    the (A, 4) anchors, the padded gts, `assigned` of atss_targets and the outputs of vfnet_quality.  box_kind / ref_kind:
    FCOS_BOX_KINDS[type of the box loss]."""
    _, sizes, A = _point_tables('vfnet_loss', (cls_maps, reg_maps, ref_maps), (None, 4, 4))
    B = cls_maps[0].size(0)
    if assigned.shape != (B, A) or assigned.dtype != torch.int32 or anchors.shape != (A, 4) or iou_ini.shape != (B, A) or \
            iou_rf.shape != (B, A) or gt_labels.dtype != torch.int64 or sums.shape != (3, ):
        raise ValueError(f'vfnet_loss: assigned must be int32 of shape {(B, A)}, anchors float32 {(A, 4)}, iou_ini / iou_rf float32 '
                         f'{(B, A)}, gt_labels int64, sums float32 (3,)')
    return VfnetLossFunction.apply(sizes, cls_maps[0].size(1), _f32(anchors, 'vfnet_loss').contiguous(),
                                   _f32(gts, 'vfnet_loss').contiguous(), gt_labels.contiguous(), assigned.contiguous(),
                                   _f32(iou_ini, 'vfnet_loss').contiguous(), _f32(iou_rf, 'vfnet_loss').contiguous(),
                                   _f32(sums, 'vfnet_loss').contiguous(), box_kind, eps_ini, ref_kind, eps_rf, alpha, gamma,
                                   iou_weighted, cls_weight, box_weight, ref_weight, *cls_maps, *reg_maps, *ref_maps)


# ====================================================================== FoveaBox head (dense_heads/fovea_head.py)
def fovea_targets(featmap_sizes, strides, base_edge_list, scale_ranges, sigma, gts, gt_valid):
    """htd_fovea_targets: FoveaHead.get_targets of the whole batch in one launch (+ a finishing one).  gts (B, K, 4) float32 /
    gt_valid (B, K) bool as pad_gt_batch leaves them (K = 0 allowed).  -> assigned (B, P) int32 (0 background, k + 1 = gt k),
    bbox_targets (B, P, 4) (log distances, 0 on background), num_pos (B,) int32, norm (2,) = [sum num_pos + B, max(sum num_pos,
    1)]; points level-major, nothing read back to the host."""
    _need_gpu(gts, 'fovea_targets')
    gts = _f32(gts, 'fovea_targets').contiguous()
    gt_valid = gt_valid.to(torch.bool).contiguous()
    B, K = gt_valid.shape
    if gts.shape != (B, K, 4):
        raise ValueError(f'fovea_targets: gts must be {(B, K, 4)}, got {tuple(gts.shape)}')
    hw, st, P = _fcos_levels(featmap_sizes, strides)
    if len(base_edge_list) != len(st) or len(scale_ranges) != len(st):
        raise ValueError(f'fovea_targets: {len(base_edge_list)} base edges and {len(scale_ranges)} scale ranges for {len(st)} levels')
    bases = (ctypes.c_float * len(st))(*[float(v) for v in base_edge_list])
    ranges = (ctypes.c_float * (2 * len(st)))(*[float(v) for r in scale_ranges for v in r])
    dev = gts.device
    assigned = torch.empty(B, P, dtype=torch.int32, device=dev)
    bbox_targets = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    norm = torch.empty(2, dtype=torch.float32, device=dev)
    ws = torch.empty(capi.lib().htd_fovea_targets_workspace_bytes(B, P) // 4, dtype=torch.int32, device=dev)
    capi.call('htd_fovea_targets', hw, st, bases, ranges, len(st), float(sigma), _P(gts) if K else None, _P(gt_valid) if K else None,
              B, K, _P(assigned), _P(bbox_targets), _P(ws), _P(num_pos), _P(norm), _S())
    return assigned, bbox_targets, num_pos, norm


class FoveaLossFunction(Function):
    """htd_fovea_loss: the two losses of FoveaHead.loss over every level and image in one launch, which also writes the two
    finished gradient maps (loss weight and normaliser applied); backward hands them over, after htd_fovea_grad_scale applies
    incoming gradients other than 1 on the device, in place.  Single use: a second backward through the same forward raises."""

    @staticmethod
    def forward(ctx, sizes, C, gt_labels, assigned, bbox_targets, norm, beta, gamma, alpha, cls_weight, box_weight, *maps):
        B, K = gt_labels.shape
        ctx.meta = (sizes, len(maps) // 2, B, int(C))
        sums = _point_loss_forward(ctx, 'fovea_loss', 'htd_fovea_loss', 2, maps,
                                   (*ctx.meta, _P(gt_labels) if K else None, K, _P(assigned), _P(bbox_targets), _P(norm), float(beta),
                                    float(gamma), float(alpha), float(cls_weight), float(box_weight))).sum(0)    # [focal, smooth-L1]
        return sums[0] / norm[0] * cls_weight, sums[1] / norm[1] * box_weight

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_box):
        return (None, ) * 11 + _point_loss_backward(ctx, 'fovea_loss', 'htd_fovea_grad_scale', ctx.meta, (g_cls, g_box))


def fovea_loss(cls_maps, reg_maps, gt_labels, assigned, bbox_targets, norm, beta=1.0, gamma=2.0, alpha=0.25, cls_weight=1.0,
               box_weight=1.0):
    """-> (loss_cls, loss_bbox) of a FoveaBox head from its per-level (B, C, h, w) / (B, 4, h, w) maps and the outputs of
    fovea_targets; beta is the SmoothL1Loss's."""
    _, sizes, P = _point_tables('fovea_loss', (cls_maps, reg_maps), (None, 4))
    B = cls_maps[0].size(0)
    if assigned.shape != (B, P) or assigned.dtype != torch.int32 or bbox_targets.shape != (B, P, 4) or \
            gt_labels.dtype != torch.int64 or gt_labels.dim() != 2 or gt_labels.size(0) != B or norm.shape != (2, ):
        raise ValueError(f'fovea_loss: assigned must be int32 of shape {(B, P)}, bbox_targets float32 {(B, P, 4)}, gt_labels int64 '
                         f'(B, K), norm float32 (2,)')
    return FoveaLossFunction.apply(sizes, cls_maps[0].size(1), gt_labels.contiguous(), assigned.contiguous(),
                                   _f32(bbox_targets, 'fovea_loss').contiguous(), _f32(norm, 'fovea_loss').contiguous(), beta, gamma,
                                   alpha, cls_weight, box_weight, *cls_maps, *reg_maps)


class FoveaAlignFunction(Function):
    """htd_fovea_align_fwd / _bwd: the four regression logits x (B, 4, H, W) of one level and conv_offset's weight (O, 4, 1, 1) ->
    the offsets conv_offset(exp(x)) (B, O, H, W) of FeatureAlign in one launch; backward gives the logits' and the weight's
    gradients in one more (+ a finishing one), bitwise reproducible."""

    @staticmethod
    def forward(ctx, x, weight):
        B, _, H, W = x.shape
        xs = nhwc_channel_stride(x)
        if xs is None:
            x = x.contiguous(memory_format=CL)
            xs = nhwc_channel_stride(x)
        O = weight.size(0)
        w = weight.detach().reshape(O, 4).contiguous()
        off = torch.empty(B, O, H, W, device=x.device, dtype=torch.float32, memory_format=CL)
        capi.call('htd_fovea_align_fwd', _P(x), xs, _P(w), B, H, W, O // 18, _P(off), O, _S())
        ctx.meta = (B, H, W, xs, O)
        ctx.save_for_backward(x, w)
        return off

    @staticmethod
    @once_differentiable
    def backward(ctx, g_off):
        B, H, W, xs, O = ctx.meta
        x, w = ctx.saved_tensors
        g_off = g_off.float()
        gs = nhwc_channel_stride(g_off)
        if gs is None:
            g_off = g_off.contiguous(memory_format=CL)
            gs = nhwc_channel_stride(g_off)
        gx = _like_padded(x, xs)
        gw = torch.empty(O, 4, 1, 1, device=x.device, dtype=torch.float32)
        ws = torch.empty(capi.lib().htd_fovea_align_bwd_workspace_bytes(B, H, W, O // 18) // 4, device=x.device, dtype=torch.float32)
        capi.call('htd_fovea_align_bwd', _P(x), xs, _P(w), _P(g_off), gs, B, H, W, O // 18, _P(gx), xs, _P(gw), _P(ws), _S())
        return gx, gw


def fovea_align(x, weight):
    """-> conv_offset(exp(x)) (B, O, H, W), channels_last, of the regression logits x (B, 4, H, W) of one level (fp32, GPU) under
    the bias-free 1 x 1 weight (O, 4, 1, 1), O = deform_groups * 18 with 1 to 8 deformable groups."""
    _need_gpu(x, 'fovea_align')
    _f32(x, 'fovea_align')
    _f32(weight, 'fovea_align')
    if x.dim() != 4 or x.size(1) != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (4, 1, 1) or weight.size(0) % 18 or \
            not 1 <= weight.size(0) // 18 <= 8:
        raise ValueError(f'fovea_align: x must be (B, 4, H, W) and weight (deform_groups * 18, 4, 1, 1) with 1 to 8 groups, got '
                         f'{tuple(x.shape)} and {tuple(weight.shape)}')
    return FoveaAlignFunction.apply(x, weight)
