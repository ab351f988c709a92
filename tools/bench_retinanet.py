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
import argparse
import collections
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htd_amd import capi  # noqa: E402

HBM_COPY_TBS = 6.29           # float4 copy on the MI355X (8.0 TB/s on paper)
SIZES = ((100, 168), (50, 84), (25, 42), (13, 21), (7, 11))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(median_us=round(statistics.median(us), 2), min_us=round(us[0], 2), max_us=round(us[-1], 2))


def alternated(legs, reps, warmup):
    """{name: fn} -> {name: median / min / max us}, one call of every leg per round."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
            for k, v in times.items()}


def head_and_inputs(dev, batch):
    from htd_amd import detector  # noqa: F401
    from htd_amd.configs import retinanet_config
    from htd_amd.registry import build_head
    from htd_amd.runner import synthetic_batch
    cfg = retinanet_config()
    spec = cfg.model.bbox_head.to_dict()
    spec.update(train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    head = build_head(spec).to(dev)
    data = synthetic_batch(batch, device=dev, seed=0)
    g = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    cls = [(torch.randn(batch, 720, h, w, generator=g) - 4.0).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    reg = [(0.3 * torch.randn(batch, 36, h, w, generator=g)).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    return head, data, cls, reg


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
    floor_us = (cls_bytes + reg_bytes + B * A * 8) / (HBM_COPY_TBS * 1e12) * 1e6
    out = dict(table='kernel', batch=B, anchors=A, classes=80, positives=int(num_pos.sum()),
               mandatory_MB=round((cls_bytes + reg_bytes + B * A * 8) / 1e6, 1), hbm_floor_us=round(floor_us, 1),
               htd_retina_loss=timed(loss, reps, warmup), htd_retina_avg_factor=timed(count, reps, warmup),
               htd_sigmoid_focal_loss=timed(matrix, reps, warmup), htd_retina_keys=timed(keys_, reps, warmup))
    out['fraction_of_floor'] = round(floor_us / out['htd_retina_loss']['median_us'], 3)
    out['matrix_fraction_of_floor'] = round(cls_bytes / (HBM_COPY_TBS * 1e6) / out['htd_sigmoid_focal_loss']['median_us'], 3)
    return out


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg = head_and_inputs(dev, batch)

    def step(fused):
        def run():
            head.fused_loss = fused
            c, r = [t.detach().requires_grad_() for t in cls], [t.detach().requires_grad_() for t in reg]
            losses = head.loss(c, r, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
            (sum(losses['loss_cls']) + sum(losses['loss_bbox'])).backward()
        return run
    out = dict(table='head', batch=batch, anchors=9 * sum(h * w for h, w in SIZES))
    out.update(alternated(dict(fused=step(True), tensor_path=step(False)), reps, warmup))
    out['fused_no_slower'] = out['fused']['median_us'] <= out['tensor_path']['median_us']
    # the C-ABI calls of the head on a pyramid: forward, loss, backward
    head.fused_loss = True
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
    from htd_amd.configs import build_retinanet_detector
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(fused):
        torch.manual_seed(0)
        model = build_retinanet_detector()
        model.bbox_head.fused_loss = fused
        return Trainer(model.to(dev).train(), lr=0.0)                # lr 0: every leg times the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = dict(fused=trainer(True), tensor_path=trainer(False))
    times = {k: [] for k in legs}
    for tr in legs.values():
        for _ in range(warmup):
            tr.train_step(data)
    torch.cuda.synchronize()
    for _ in range(steps):
        for k, tr in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.train_step(data)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = dict(table='step', model='retinanet_r50_fpn', precision='fp32', batch=batch, image='1333x800', steps=steps, warmup=warmup)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = dict(median_ms=round(med, 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), img_per_s=round(batch * 1e3 / med, 2))
    out['fused_no_slower'] = out['fused']['median_ms'] <= out['tensor_path']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=['kernel', 'head', 'step'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_retinanet.py measures on the GPU only'
    dev = torch.device('cuda:0')
    capi.lib()
    for t in args.tables or ['kernel', 'head', 'step']:
        if t == 'kernel':
            print(json.dumps(bench_kernel(dev, args.reps, 10, args.batch)), flush=True)
        elif t == 'head':
            print(json.dumps(bench_head(dev, max(10, args.reps // 5), 3, args.batch)), flush=True)
        elif t == 'step':
            print(json.dumps(bench_step(dev, args.steps, args.warmup, args.batch)), flush=True)
        else:
            raise SystemExit(f'unknown table {t}')


if __name__ == '__main__':
    main()
