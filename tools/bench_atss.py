#!/usr/bin/env python3
"""Cost of the ATSS baseline, three tables:

  kernel   htd_atss_targets and htd_atss_loss alone on the five levels of a B = 4 1333 x 800 batch, padded to 1344 x 800 (4 x 22 400
           anchors x 80 classes), each against the time of its traffic at the 6.29 TB/s a float4 copy reaches (loss: logits read +
           their gradient written, the delta and centerness maps both ways, assigned and the centerness targets read: an HBM
           floor; targets: per valid gt the anchors read once, per image the 8-byte words cleared, written and read and its two
           outputs written: the traffic of this algorithm, which re-reads the anchors for every gt, so more than must move)
  head     ATSSHead.loss forward + backward on the same maps: the fused path against the tensor path (fused_loss=False), legs
           alternated
  step     the ATSS-R50 fp32 B = 4 1333 x 800 synthetic train step with the fused loss and with the tensor-path loss, next to the
           FCOS and RetinaNet steps, in one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_atss.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, capi  # noqa: E402


def head_and_inputs(dev, batch):
    from htd_amd.configs import atss_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(atss_config, dev), synthetic_batch(batch, device=dev, seed=0)
    return (head, data, *D.seeded_maps(((80, lambda t, l: t - 4.0), (4, lambda t, l: t), (1, lambda t, l: t)), batch, dev))


def bench_kernel(dev, reps, warmup, batch):
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import _d4, pad_gt_batch
    head, data, cls, reg, ctr = head_and_inputs(dev, batch)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    anchors = torch.cat(head.anchor_generator.grid_anchors(SIZES, device=dev)).float().contiguous()
    sizes = [h * w for h, w in SIZES]
    means, stds = _d4(head.bbox_coder.means), _d4(head.bbox_coder.stds)
    assigned, ct, num_pos, norm = M.atss_targets(anchors, sizes, gts, gt_valid, head.assigner.topk, head.bbox_coder.means,
                                                 head.bbox_coder.stds)
    B, A = assigned.shape
    K = gts.size(1)
    lv = M._i64s(sizes)
    ws = torch.empty(capi.lib().htd_atss_targets_workspace_bytes(B, A) // 8, dtype=torch.float64, device=dev)
    stream = capi.current_stream_ptr()
    gts, gt_valid = gts.float().contiguous(), gt_valid.contiguous()

    def targets():
        capi.call('htd_atss_targets', capi.ptr(anchors), lv, 5, capi.ptr(gts), capi.ptr(gt_valid), B, K, head.assigner.topk, means,
                  stds, 16 / 1000, capi.ptr(assigned), capi.ptr(ct), capi.ptr(ws), capi.ptr(num_pos), capi.ptr(norm), stream)
    tabs = [M._level_tables(m, 'bench_atss') for m in (cls, reg, ctr)]
    grads = [[torch.empty_like(m) for m in ms] for ms in (cls, reg, ctr)]
    gtabs = [M._level_tables(m, 'bench_atss')[0] for m in grads]
    partial = torch.empty(capi.lib().htd_atss_loss_partial_rows(), 2, device=dev)

    def loss():
        capi.call('htd_atss_loss', tabs[0][0], tabs[0][1], tabs[1][0], tabs[1][1], tabs[2][0], tabs[2][1], lv, 5, B, 80,
                  capi.ptr(anchors), capi.ptr(gts), capi.ptr(labels), K, capi.ptr(assigned), capi.ptr(ct), capi.ptr(norm), means, stds,
                  16 / 1000, 2, 1e-6, 2.0, 0.25, 1.0, 2.0, 1.0, capi.ptr(partial), gtabs[0], gtabs[1], gtabs[2], stream)
    n = B * A
    valid_gts = int(gt_valid.sum())
    bytes_ = dict(htd_atss_targets=valid_gts * A * 16 + n * (3 * 8 + 4 + 4), htd_atss_loss=n * (2 * 80 * 4 + 2 * 4 * 4 + 2 * 4 + 4 + 4))
    out = dict(table='kernel', batch=B, anchors=A, classes=80, gts=K, valid_gts=valid_gts, positives=int(num_pos.sum()))
    for name, fn in (('htd_atss_targets', targets), ('htd_atss_loss', loss)):
        out[name] = D.floor_row(D.timed(fn, reps, warmup), bytes_[name])
    return out


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg, ctr = head_and_inputs(dev, batch)

    def run_loss():
        maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg, ctr)]
        ls = head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
        (sum(ls['loss_cls']) + sum(ls['loss_bbox']) + sum(ls['loss_centerness']) if isinstance(ls['loss_cls'], list)
         else ls['loss_cls'] + ls['loss_bbox'] + ls['loss_centerness']).backward()
    assert head._fused_loss_ok(cls, reg, ctr, data['gt_labels'], None, data['img_metas']), 'the fused path must take these maps'
    return D.head_table(head, run_loss, reps, warmup, batch=batch, anchors=sum(h * w for h, w in SIZES))


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'atss_r50_fpn', (('atss_fused', 'atss', True), ('atss_tensor_path', 'atss', False),
                                              ('fcos_fused', 'fcos', True), ('retinanet_fused', 'retinanet', True)),
                        (('atss_fused', 'atss_tensor_path'), ), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_atss.py', dict(kernel=(bench_kernel, D.KERNEL), head=(bench_head, D.HEAD), step=(bench_step, D.STEP)))
