#!/usr/bin/env python3
"""Cost of the GFL baseline, three tables:

  kernel   htd_gfl_quality, htd_gfl_loss and htd_gfl_decode alone on the five levels of a B = 4 1333 x 800 batch, padded to
           1344 x 800 (4 x 22 400 anchors x 80 classes, 68 distribution logits), each against the time of the bytes it must move at
           the 6.29 TB/s a float4 copy reaches (quality: assigned read, weight and score written, a positive's 148 logits read;
           loss: class logits read + their gradient written, the distribution gradient written, assigned and score read, a
           positive's 68 logits read; decode: both maps read, keys and distances written)
  head     GFLHead.loss forward + backward on the same maps: the fused path against the tensor path (fused_loss=False), legs
           alternated
  step     the GFL-R50 fp32 B = 4 1333 x 800 synthetic train step with the fused loss and with the tensor-path loss, next to the
           ATSS and RetinaNet steps, in one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table; the exit status is non-zero if the fused
head loss or the fused step came out slower than the tensor path measured beside it.
usage: bench_gfl.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, capi  # noqa: E402

KEYS = ('loss_cls', 'loss_bbox', 'loss_dfl')


def head_and_inputs(dev, batch):
    from htd_amd.configs import gfl_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(gfl_config, dev), synthetic_batch(batch, device=dev, seed=0)
    return (head, data, *D.seeded_maps(((80, lambda t, l: t - 4.0), (4 * (head.reg_max + 1), lambda t, l: t)), batch, dev))


def bench_kernel(dev, reps, warmup, batch):
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import pad_gt_batch
    head, data, cls, reg = head_and_inputs(dev, batch)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    anchors = torch.cat(head.anchor_generator.grid_anchors(SIZES, device=dev)).float().contiguous()
    sizes = [h * w for h, w in SIZES]
    strides, R = head.anchor_generator.strides, head.reg_max
    assigned, _, num_pos, norm = M.atss_targets(anchors, sizes, gts, gt_valid, head.assigner.topk)
    weight, score, wsum = M.gfl_quality(cls, reg, strides, R, anchors, gts, assigned)
    B, A = assigned.shape
    K = gts.size(1)
    ((ct, cs), (rt, rs)), lv, _ = M._point_tables('bench_gfl', (cls, reg), (None, 4 * (R + 1)))
    st = M._fcos_levels(SIZES, strides)[1]
    ws = torch.empty(capi.lib().htd_gfl_quality_workspace_bytes(B, A) // 8, dtype=torch.float64, device=dev)
    stream = capi.current_stream_ptr()
    gts = gts.float().contiguous()
    P = capi.ptr

    def quality():
        capi.call('htd_gfl_quality', ct, cs, rt, rs, lv, st, 5, B, 80, R, P(anchors), P(gts), K, P(assigned), P(weight), P(score),
                  P(wsum), P(ws), stream)
    grads = [[torch.empty_like(m) for m in ms] for ms in (cls, reg)]
    gtabs = [M._level_tables(m, 'bench_gfl')[0] for m in grads]
    partial = torch.empty(capi.lib().htd_gfl_loss_partial_rows(), 2, device=dev)

    def loss():
        capi.call('htd_gfl_loss', ct, cs, rt, rs, lv, st, 5, B, 80, R, P(anchors), P(gts), P(labels), K, P(assigned), P(weight),
                  P(score), P(norm), P(wsum), 2, 1e-6, 2.0, 1.0, 2.0, 0.25, P(partial), gtabs[0], gtabs[1], stream)
    keys, dist = torch.empty(B, A, device=dev), torch.empty(B, A, 4, device=dev)

    def decode():
        capi.call('htd_gfl_decode', ct, cs, rt, rs, lv, st, 5, B, 80, R, P(keys), P(dist), stream)
    n, pos, nreg = B * A, int(num_pos.sum()), 4 * (R + 1)
    bytes_ = dict(htd_gfl_quality=n * 12 + pos * (80 + nreg) * 4, htd_gfl_loss=n * (2 * 80 * 4 + nreg * 4 + 8) + pos * nreg * 4,
                  htd_gfl_decode=n * ((80 + nreg) * 4 + 20))
    out = dict(table='kernel', batch=B, anchors=A, classes=80, reg_max=R, gts=K, positives=pos)
    for name, fn in (('htd_gfl_quality', quality), ('htd_gfl_loss', loss), ('htd_gfl_decode', decode)):
        out[name] = D.floor_row(D.timed(fn, reps, warmup), bytes_[name])
    return out


def _total(ls):
    return sum(sum(ls[k]) if isinstance(ls[k], list) else ls[k] for k in KEYS)


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg = head_and_inputs(dev, batch)

    def run_loss():
        maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg)]
        _total(head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])).backward()
    assert head._fused_loss_ok(cls, reg, data['gt_labels'], None, data['img_metas']), 'the fused path must take these maps'
    return D.head_table(head, run_loss, reps, warmup, batch=batch, anchors=sum(h * w for h, w in SIZES))


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'gfl_r50_fpn', (('gfl_fused', 'gfl', True), ('gfl_tensor_path', 'gfl', False), ('atss_fused', 'atss', True),
                                             ('retinanet_fused', 'retinanet', True)),
                        (('gfl_fused', 'gfl_tensor_path'), ), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_gfl.py', dict(kernel=(bench_kernel, D.KERNEL), head=(bench_head, D.HEAD), step=(bench_step, D.STEP)), strict=True)
