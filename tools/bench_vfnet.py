#!/usr/bin/env python3
"""Cost of the VFNet baseline, three tables:

  kernel   htd_vfnet_star_fwd / _bwd on the finest level, htd_vfnet_quality and htd_vfnet_loss on the five levels of a B = 4
           1333 x 800 batch, padded to 1344 x 800 (4 x 22 400 anchors x 80 classes, two maps of 4 distances), each against the time
           of the bytes it must move at the 6.29 TB/s a float4 copy reaches (star forward: 4 logits read, 4 + 18 floats written;
           backward: 4 + 4 + 18 read, 4 written; quality: assigned read, both IoUs written, a positive's 8 distances read; loss:
           class logits read + their gradient written, both distance gradients written, assigned and iou_rf read, a positive's
           8 distances read)
  head     VFNetHead.loss forward + backward on the same maps: the fused path against the tensor path (fused_loss=False), legs
           alternated
  step     the VFNet-R50 fp32 B = 4 1333 x 800 synthetic train step with the kernels and with the tensor-path star offsets and
           loss, next to the GFL and ATSS steps, in one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table; the exit status is non-zero if the fused
head loss or the fused step came out slower than the tensor path measured beside it.
usage: bench_vfnet.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, capi  # noqa: E402

KEYS = ('loss_cls', 'loss_bbox', 'loss_bbox_rf')


def head_and_inputs(dev, batch):
    from htd_amd.configs import vfnet_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(vfnet_config, dev), synthetic_batch(batch, device=dev, seed=0)
    g = torch.Generator().manual_seed(0)
    cls, reg = D.seeded_maps(((80, lambda t, l: t - 4.0), (4, lambda t, l: (t * 0.5 - 1.5).exp() * head.reg_denoms[l])), batch, dev, g)
    ref, = D.seeded_maps(((4, lambda t, l: reg[l].cpu() * (t * 0.3).exp()), ), batch, dev, g)
    return head, data, cls, reg, ref


def bench_kernel(dev, reps, warmup, batch):
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import pad_gt_batch
    head, data, cls, reg, ref = head_and_inputs(dev, batch)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    anchors = torch.cat(head.anchor_generator.grid_anchors(SIZES, device=dev)).float().contiguous()
    sizes = [h * w for h, w in SIZES]
    assigned, _, num_pos, _ = M.atss_targets(anchors, sizes, gts, gt_valid, head.assigner.topk)
    iou_ini, iou_rf, sums = M.vfnet_quality(reg, ref, anchors, gts, assigned)
    B, A = assigned.shape
    K = gts.size(1)
    ((ct, cs), (rt, rs), (ft, fs)), lv, _ = M._point_tables('bench_vfnet', (cls, reg, ref), (None, 4, 4))
    ws = torch.empty(capi.lib().htd_vfnet_quality_workspace_bytes(B, A) // 8, dtype=torch.float64, device=dev)
    stream = capi.current_stream_ptr()
    gts = gts.float().contiguous()
    P = capi.ptr
    h0, w0 = SIZES[0]
    x = torch.randn(B, 4, h0, w0, device=dev).contiguous(memory_format=torch.channels_last)
    pred, off = torch.empty_like(x), torch.empty(B, 18, h0, w0, device=dev).contiguous(memory_format=torch.channels_last)
    gp, go, gx = torch.randn_like(pred), torch.randn_like(off), torch.empty_like(x)

    def star_fwd():
        capi.call('htd_vfnet_star_fwd', P(x), 4, B, h0, w0, 64.0, 8.0, 0.1, P(pred), 4, P(off), 18, stream)

    def star_bwd():
        capi.call('htd_vfnet_star_bwd', P(pred), 4, P(gp), 4, P(go), 18, B, h0, w0, 8.0, 0.1, P(gx), 4, stream)

    def quality():
        capi.call('htd_vfnet_quality', rt, rs, ft, fs, lv, 5, B, P(anchors), P(gts), K, P(assigned), P(iou_ini), P(iou_rf), P(sums),
                  P(ws), stream)
    grads = [[torch.empty_like(m) for m in ms] for ms in (cls, reg, ref)]
    gtabs = [M._level_tables(m, 'bench_vfnet')[0] for m in grads]
    partial = torch.empty(capi.lib().htd_vfnet_loss_partial_rows(), 2, device=dev)

    def loss():
        capi.call('htd_vfnet_loss', ct, cs, rt, rs, ft, fs, lv, 5, B, 80, P(anchors), P(gts), P(labels), K, P(assigned), P(iou_ini),
                  P(iou_rf), P(sums), 2, 1e-6, 2, 1e-6, 0.75, 2.0, 1, 1.0, 1.5, 2.0, P(partial), gtabs[0], gtabs[1], gtabs[2], stream)
    n, n0, pos = B * A, B * h0 * w0, int(num_pos.sum())
    bytes_ = dict(htd_vfnet_star_fwd=n0 * 26 * 4, htd_vfnet_star_bwd=n0 * 30 * 4, htd_vfnet_quality=n * 12 + pos * 32,
                  htd_vfnet_loss=n * (2 * 80 * 4 + 32 + 8) + pos * 32)
    out = dict(table='kernel', batch=B, anchors=A, classes=80, gts=K, positives=pos)
    for name, fn in (('htd_vfnet_star_fwd', star_fwd), ('htd_vfnet_star_bwd', star_bwd), ('htd_vfnet_quality', quality),
                     ('htd_vfnet_loss', loss)):
        out[name] = D.floor_row(D.timed(fn, reps, warmup), bytes_[name])
    return out


def _total(ls):
    return sum(ls[k] for k in KEYS)


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg, ref = head_and_inputs(dev, batch)

    def run_loss():
        maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg, ref)]
        _total(head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])).backward()
    assert head._fused_loss_ok(cls, reg, ref, data['gt_labels'], None, data['img_metas']), 'the fused path must take these maps'
    return D.head_table(head, run_loss, reps, warmup, batch=batch, anchors=sum(h * w for h, w in SIZES))


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'vfnet_r50_fpn', (('vfnet_fused', 'vfnet', True), ('vfnet_tensor_path', 'vfnet', False),
                                               ('gfl_fused', 'gfl', True), ('atss_fused', 'atss', True)),
                        (('vfnet_fused', 'vfnet_tensor_path'), ), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_vfnet.py', dict(kernel=(bench_kernel, D.KERNEL), head=(bench_head, D.HEAD), step=(bench_step, D.STEP)), strict=True)
