#!/usr/bin/env python3
"""Cost of the FCOS baseline, three tables:

  kernel   htd_fcos_targets, htd_fcos_loss and htd_fcos_keys alone on the five levels of a B = 4 1344 x 800 batch (4 x 22 400 points
           x 80 classes), each against the HBM floor of its mandatory traffic at the 6.29 TB/s a float4 copy reaches (loss: logits
           read + their gradient written, the distance and centerness maps both ways, the targets read; targets: its outputs
           written; keys: logits and centerness read, keys written)
  head     FCOSHead.loss forward + backward on the same maps: the fused path against the tensor path (fused_loss=False), legs
           alternated
  step     the FCOS-R50 fp32 B = 4 1333 x 800 synthetic train step with the fused loss and with the tensor-path loss, next to the
           RetinaNet step, in one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_fcos.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, STRIDES, capi  # noqa: E402


def head_and_inputs(dev, batch):
    from htd_amd.configs import fcos_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(fcos_config, dev), synthetic_batch(batch, device=dev, seed=0)
    return (head, data, *D.seeded_maps(((80, lambda t, l: t - 4.0), (4, lambda t, l: (0.5 * t).exp().mul(2.0 * STRIDES[l])),
                                        (1, lambda t, l: t)), batch, dev))


def bench_kernel(dev, reps, warmup, batch):
    import ctypes
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import pad_gt_batch
    head, data, cls, reg, ctr = head_and_inputs(dev, batch)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    assigned, bt, ct, num_pos, norm = M.fcos_targets(SIZES, STRIDES, head.regress_ranges, gts, gt_valid)
    B, P = assigned.shape
    K = gts.size(1)
    hw, st, _ = M._fcos_levels(SIZES, STRIDES)
    ranges = (ctypes.c_float * 10)(*[float(v) for r in head.regress_ranges for v in r])
    ws = torch.empty(capi.lib().htd_fcos_targets_workspace_bytes(B, P) // 8, dtype=torch.float64, device=dev)
    stream = capi.current_stream_ptr()
    gts, gt_valid = gts.float().contiguous(), gt_valid.contiguous()

    def targets():
        capi.call('htd_fcos_targets', hw, st, ranges, 5, capi.ptr(gts), capi.ptr(gt_valid), B, K, 0, 1.5, 0, capi.ptr(assigned),
                  capi.ptr(bt), capi.ptr(ct), capi.ptr(ws), capi.ptr(num_pos), capi.ptr(norm), stream)
    tabs = [M._level_tables(m, 'bench_fcos') for m in (cls, reg, ctr)]
    grads = [[torch.empty_like(m) for m in ms] for ms in (cls, reg, ctr)]
    gtabs = [M._level_tables(m, 'bench_fcos')[0] for m in grads]
    partial = torch.empty(capi.lib().htd_fcos_loss_partial_rows(), 2, device=dev)

    def loss():
        capi.call('htd_fcos_loss', tabs[0][0], tabs[0][1], tabs[1][0], tabs[1][1], tabs[2][0], tabs[2][1], hw, st, 5, B, 80,
                  capi.ptr(labels), K, capi.ptr(assigned), capi.ptr(bt), capi.ptr(ct), capi.ptr(norm), 0, 1e-6, 2.0, 0.25, 1.0, 1.0,
                  1.0, capi.ptr(partial), gtabs[0], gtabs[1], gtabs[2], stream)
    keys = torch.empty(B, P, device=dev)

    def keys_():
        capi.call('htd_fcos_keys', tabs[0][0], tabs[0][1], tabs[2][0], tabs[2][1], hw, st, 5, B, 80, capi.ptr(keys), stream)
    n = B * P
    bytes_ = dict(htd_fcos_targets=n * (4 + 16 + 4), htd_fcos_loss=n * (2 * 80 * 4 + 2 * 4 * 4 + 2 * 4 + 4 + 16 + 4),
                  htd_fcos_keys=n * (80 * 4 + 4 + 4))
    out = dict(table='kernel', batch=B, points=P, classes=80, gts=K, positives=int(num_pos.sum()))
    for name, fn in (('htd_fcos_targets', targets), ('htd_fcos_loss', loss), ('htd_fcos_keys', keys_)):
        out[name] = D.floor_row(D.timed(fn, reps, warmup), bytes_[name])
    return out


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg, ctr = head_and_inputs(dev, batch)

    def run_loss():
        maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg, ctr)]
        ls = head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
        (ls['loss_cls'] + ls['loss_bbox'] + ls['loss_centerness']).backward()
    return D.head_table(head, run_loss, reps, warmup, batch=batch, points=sum(h * w for h, w in SIZES))


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'fcos_r50_caffe_fpn_gn-head', (('fcos_fused', 'fcos', True), ('fcos_tensor_path', 'fcos', False),
                                                            ('retinanet_fused', 'retinanet', True)),
                        (('fcos_fused', 'fcos_tensor_path'), ), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_fcos.py', dict(kernel=(bench_kernel, D.KERNEL), head=(bench_head, D.HEAD), step=(bench_step, D.STEP)))
