#!/usr/bin/env python3
"""Cost of the RetinaNet baseline, three tables:

  kernel   htd_retina_loss alone on the five levels of a B = 4 1344 x 800 batch (4 x 201 600 anchors x 80 classes), against the
           HBM floor of its mandatory traffic (logits read + their gradient written, the regression maps both ways, `assigned`)
           at the 6.29 TB/s a float4 copy reaches; htd_sigmoid_focal_loss on the same 806 400 x 80 matrix; htd_retina_keys
  head     RetinaHead.loss forward + backward on the same maps: the fused path against the tensor path (fused_loss=False), legs
           alternated; and the C-ABI calls of head forward + loss + backward on a B = 4 pyramid
  step     the R50 fp32 B = 4 1333 x 800 synthetic train step with the fused loss and with the tensor-path loss in one process,
           legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_retinanet.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, capi  # noqa: E402


def head_and_inputs(dev, batch):
    from htd_amd.configs import retinanet_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(retinanet_config, dev), synthetic_batch(batch, device=dev, seed=0)
    return (head, data, *D.seeded_maps(((720, lambda t, l: t - 4.0), (36, lambda t, l: 0.3 * t)), batch, dev))


def bench_kernel(dev, reps, warmup, batch):
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import batched_max_iou_assign, pad_gt_batch
    head, data, cls, reg = head_and_inputs(dev, batch)
    flat_anchors, inside = head._anchors_inside([c.shape[-2:] for c in cls], data['img_metas'], dev)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    assigned, _ = batched_max_iou_assign(head.assigner, flat_anchors, inside, gts, gt_valid)
    num_pos, avg = M.retina_avg_factor(assigned)
    B, A = assigned.shape
    ct, cs, pix = M._level_tables(cls, 'bench_retinanet')
    rt, rs, _ = M._level_tables(reg, 'bench_retinanet')
    gcls, greg = [torch.empty_like(c) for c in cls], [torch.empty_like(r) for r in reg]
    gct, _, _ = M._level_tables(gcls, 'bench_retinanet')
    grt, _, _ = M._level_tables(greg, 'bench_retinanet')
    partial = torch.empty(capi.lib().htd_focal_loss_partial_rows(), 2, device=dev)
    import ctypes
    means, stds = (ctypes.c_float * 4)(0, 0, 0, 0), (ctypes.c_float * 4)(1, 1, 1, 1)
    stream = capi.current_stream_ptr()

    def loss():
        capi.call('htd_retina_loss', ct, cs, rt, rs, pix, len(cls), B, 9, 80, capi.ptr(flat_anchors), capi.ptr(gts), capi.ptr(labels),
                  capi.ptr(assigned), A, gts.size(1), means, stds, 2.0, 0.25, -1.0, 1, 0.0, capi.ptr(avg), 1.0, 1.0,
                  capi.ptr(partial), gct, grt, stream)
    ws = torch.empty(capi.lib().htd_retina_avg_factor_workspace_bytes(B) // 4, dtype=torch.int32, device=dev)

    def count():
        capi.call('htd_retina_avg_factor', capi.ptr(assigned), B, A, capi.ptr(ws), capi.ptr(num_pos), capi.ptr(avg), stream)
    x = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, 80) for c in cls]).contiguous()
    lab = torch.full((x.size(0), ), 80, dtype=torch.int64, device=dev)
    gx = torch.empty_like(x)
    p1 = torch.empty(capi.lib().htd_focal_loss_partial_rows(), device=dev)

    def matrix():
        capi.call('htd_sigmoid_focal_loss', capi.ptr(x), capi.ptr(lab), None, x.size(0), 80, 2.0, 0.25, None, capi.ptr(p1),
                  capi.ptr(gx), stream)
    keys = torch.empty(B, A, device=dev)

    def keys_():
        capi.call('htd_retina_keys', ct, cs, pix, len(cls), B, 9, 80, capi.ptr(keys), stream)
    cls_bytes, reg_bytes = 2 * B * A * 80 * 4, 2 * B * A * 4 * 4
    floor_us = (cls_bytes + reg_bytes + B * A * 8) / (D.HBM_COPY_TBS * 1e12) * 1e6
    out = dict(table='kernel', batch=B, anchors=A, classes=80, positives=int(num_pos.sum()),
               mandatory_MB=round((cls_bytes + reg_bytes + B * A * 8) / 1e6, 1), hbm_floor_us=round(floor_us, 1),
               htd_retina_loss=D.timed(loss, reps, warmup), htd_retina_avg_factor=D.timed(count, reps, warmup),
               htd_sigmoid_focal_loss=D.timed(matrix, reps, warmup), htd_retina_keys=D.timed(keys_, reps, warmup))
    out['fraction_of_floor'] = round(floor_us / out['htd_retina_loss']['median_us'], 3)
    out['matrix_fraction_of_floor'] = round(cls_bytes / (D.HBM_COPY_TBS * 1e6) / out['htd_sigmoid_focal_loss']['median_us'], 3)
    return out


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg = head_and_inputs(dev, batch)

    def run_loss():
        c, r = [t.detach().requires_grad_() for t in cls], [t.detach().requires_grad_() for t in reg]
        losses = head.loss(c, r, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
        (sum(losses['loss_cls']) + sum(losses['loss_bbox'])).backward()
    out = D.head_table(head, run_loss, reps, warmup, batch=batch, anchors=9 * sum(h * w for h, w in SIZES))
    # the C-ABI calls of the head on a pyramid: forward, loss, backward
    feats = [torch.randn(batch, 256, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_() for h, w in SIZES]
    from htd_amd import dense
    calls, real = collections.Counter(), capi.call

    def spy(name, *a, **k):
        calls[name] += 1
        return real(name, *a, **k)
    for _ in range(2):
        dense.new_step()
        calls.clear()
        capi.call = spy
        try:
            losses = head.forward_train(feats, data['img_metas'], data['gt_bboxes'], data['gt_labels'])
            (sum(losses['loss_cls']) + sum(losses['loss_bbox'])).backward()
        finally:
            capi.call = real
    out['head_abi_calls'] = sum(calls.values())
    out['head_abi_calls_by_entry'] = dict(calls)
    return out


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'retinanet_r50_fpn', (('fused', 'retinanet', True), ('tensor_path', 'retinanet', False)),
                        (('fused', 'tensor_path'), ), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_retinanet.py', dict(kernel=(bench_kernel, D.KERNEL), head=(bench_head, D.HEAD), step=(bench_step, D.STEP)))
