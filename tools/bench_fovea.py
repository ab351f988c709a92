#!/usr/bin/env python3
"""Cost of the FoveaBox baseline, four tables:

  kernel   htd_fovea_targets and htd_fovea_loss alone on the five levels of a B = 4 1344 x 800 batch (4 x 22 400 points x 80
           classes) and htd_fovea_align_fwd / _bwd on its largest level (4 x 100 x 168 pixels, 4 deformable groups), each against the
           HBM floor of its mandatory traffic at the 6.29 TB/s a float4 copy reaches (targets: its outputs written; loss: logits
           read + their gradient written, the distance map both ways, assignment and targets read; align forward: four logits
           read, 72 offsets written; backward: logits and 72 offset gradients read, four gradients written)
  head     FoveaHead.loss forward + backward on the same maps: the fused path against the tensor path (fused_loss=False), legs
           alternated
  align    FeatureAlign's offsets forward + backward on every level of the pyramid: the kernels against the tensor form
           (conv_offset(exp(x))), legs alternated
  step     the FOVEA-R50 fp32 B = 4 1333 x 800 synthetic train step, plain and align config, each with the fused loss (and offset
           kernels) and with the tensor path, next to the FCOS and RetinaNet steps, in one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_fovea.py [kernel] [head] [align] [step] [--steps K] [--warmup W] [--batch B]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_dense as D  # noqa: E402
from bench_dense import SIZES, STRIDES, alternated, capi  # noqa: E402

CL = torch.channels_last


def head_and_inputs(dev, batch):
    from htd_amd.configs import fovea_config
    from htd_amd.runner import synthetic_batch
    head, data = D.head_from_config(fovea_config, dev), synthetic_batch(batch, device=dev, seed=0)
    return (head, data, *D.seeded_maps(((80, lambda t, l: t - 4.0), (4, lambda t, l: 0.5 * t)), batch, dev))


def bench_kernel(dev, reps, warmup, batch):
    import ctypes
    from htd_amd import mmcv_ops as M
    from htd_amd.core.bbox import pad_gt_batch
    head, data, cls, reg = head_and_inputs(dev, batch)
    gts, gt_valid, labels = pad_gt_batch(data['gt_bboxes'], data['gt_labels'])
    assigned, bt, num_pos, norm = M.fovea_targets(SIZES, STRIDES, head.base_edge_list, head.scale_ranges, head.sigma, gts, gt_valid)
    B, P = assigned.shape
    K = gts.size(1)
    hw, st, _ = M._fcos_levels(SIZES, STRIDES)
    bases = (ctypes.c_float * 5)(*[float(v) for v in head.base_edge_list])
    ranges = (ctypes.c_float * 10)(*[float(v) for r in head.scale_ranges for v in r])
    ws = torch.empty(capi.lib().htd_fovea_targets_workspace_bytes(B, P) // 4, dtype=torch.int32, device=dev)
    stream = capi.current_stream_ptr()
    gts, gt_valid = gts.float().contiguous(), gt_valid.contiguous()

    def targets():
        capi.call('htd_fovea_targets', hw, st, bases, ranges, 5, float(head.sigma), capi.ptr(gts), capi.ptr(gt_valid), B, K,
                  capi.ptr(assigned), capi.ptr(bt), capi.ptr(ws), capi.ptr(num_pos), capi.ptr(norm), stream)
    tabs = [M._level_tables(m, 'bench_fovea') for m in (cls, reg)]
    grads = [[torch.empty_like(m) for m in ms] for ms in (cls, reg)]
    gtabs = [M._level_tables(m, 'bench_fovea')[0] for m in grads]
    sizes = M._i64s([h * w for h, w in SIZES])
    partial = torch.empty(capi.lib().htd_fovea_loss_partial_rows(), 2, device=dev)

    def loss():
        capi.call('htd_fovea_loss', tabs[0][0], tabs[0][1], tabs[1][0], tabs[1][1], sizes, 5, B, 80, capi.ptr(labels), K,
                  capi.ptr(assigned), capi.ptr(bt), capi.ptr(norm), 0.11, 1.5, 0.4, 1.0, 1.0, capi.ptr(partial), gtabs[0], gtabs[1],
                  stream)
    H, W = SIZES[0]
    x = reg[0]
    w = (0.1 * torch.randn(72, 4, device=dev)).contiguous()
    off = torch.empty(B, 72, H, W, device=dev).contiguous(memory_format=CL)
    goff = torch.randn(B, 72, H, W, device=dev).contiguous(memory_format=CL)
    gx, gw = torch.empty_like(x), torch.empty(72, 4, device=dev)
    aws = torch.empty(capi.lib().htd_fovea_align_bwd_workspace_bytes(B, H, W, 4) // 4, device=dev)

    def align_fwd():
        capi.call('htd_fovea_align_fwd', capi.ptr(x), 4, capi.ptr(w), B, H, W, 4, capi.ptr(off), 72, stream)

    def align_bwd():
        capi.call('htd_fovea_align_bwd', capi.ptr(x), 4, capi.ptr(w), capi.ptr(goff), 72, B, H, W, 4, capi.ptr(gx), 4, capi.ptr(gw),
                  capi.ptr(aws), stream)
    n, m = B * P, B * H * W
    bytes_ = dict(htd_fovea_targets=n * (4 + 16), htd_fovea_loss=n * (2 * 80 * 4 + 2 * 4 * 4 + 4 + 16),
                  htd_fovea_align_fwd=m * (16 + 72 * 4), htd_fovea_align_bwd=m * (16 + 72 * 4 + 16))
    out = dict(table='kernel', batch=B, points=P, classes=80, gts=K, positives=int(num_pos.sum()), align_pixels=m)
    for name, fn in (('htd_fovea_targets', targets), ('htd_fovea_loss', loss), ('htd_fovea_align_fwd', align_fwd),
                     ('htd_fovea_align_bwd', align_bwd)):
        out[name] = D.floor_row(D.timed(fn, reps, warmup), bytes_[name])
    return out


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg = head_and_inputs(dev, batch)

    def run_loss():
        maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg)]
        ls = head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
        (ls['loss_cls'] + ls['loss_bbox']).backward()
    return D.head_table(head, run_loss, reps, warmup, batch=batch, points=sum(h * w for h, w in SIZES))


def bench_align(dev, reps, warmup, batch):
    from htd_amd.detector import FeatureAlign
    torch.manual_seed(0)
    fa = FeatureAlign(256, 256, kernel_size=3, deform_groups=4).to(dev)
    fa.init_weights()
    g = torch.Generator().manual_seed(0)
    logits = [(0.5 * torch.randn(batch, 4, h, w, generator=g)).to(dev).contiguous(memory_format=CL) for h, w in SIZES]
    gout = [torch.randn(batch, 72, h, w, generator=g).to(dev).contiguous(memory_format=CL) for h, w in SIZES]

    def step(fused):
        def run():
            fa.fused = fused
            fa.conv_offset.weight.grad = None
            xs = [t.detach().requires_grad_() for t in logits]
            offs = [fa.offsets(logits=x) if fused else fa.offsets(shape=x.exp()) for x in xs]
            torch.autograd.backward(offs, gout)
        return run
    out = dict(table='align', batch=batch, pixels=batch * sum(h * w for h, w in SIZES), deform_groups=4)
    out.update(alternated(dict(kernels=step(True), tensor_form=step(False)), reps, warmup))
    out['kernels_no_slower'] = out['kernels']['median_us'] <= out['tensor_form']['median_us']
    return out


def bench_step(dev, steps, warmup, batch):
    return D.step_table(dev, 'fovea_r50_fpn / fovea_align_r50_fpn_gn-head',
                        (('fovea_fused', 'fovea', True), ('fovea_tensor_path', 'fovea', False), ('fovea_align_fused', 'fovea_align', True),
                         ('fovea_align_tensor_path', 'fovea_align', False), ('fcos_fused', 'fcos', True), ('retinanet_fused', 'retinanet', True)),
                        (('fovea_fused', 'fovea_tensor_path'), ('fovea_align_fused', 'fovea_align_tensor_path')), steps, warmup, batch)


if __name__ == '__main__':
    D.main('bench_fovea.py', dict(kernel=(bench_kernel, D.KERNEL), head=(bench_head, D.HEAD),
                                  align=(bench_align, lambda args: (max(10, args.reps // 2), 5)), step=(bench_step, D.STEP)))
