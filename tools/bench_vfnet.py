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
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from htd_amd import capi  # noqa: E402
from bench_retinanet import HBM_COPY_TBS, SIZES, alternated, timed  # noqa: E402

KEYS = ('loss_cls', 'loss_bbox', 'loss_bbox_rf')


def head_and_inputs(dev, batch):
    from htd_amd import detector  # noqa: F401
    from htd_amd.configs import vfnet_config
    from htd_amd.registry import build_head
    from htd_amd.runner import synthetic_batch
    cfg = vfnet_config()
    spec = cfg.model.bbox_head.to_dict()
    spec.update(train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    head = build_head(spec).to(dev)
    data = synthetic_batch(batch, device=dev, seed=0)
    g = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    cls = [(torch.randn(batch, 80, h, w, generator=g) - 4.0).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    reg = [((torch.randn(batch, 4, h, w, generator=g) * 0.5 - 1.5).exp() * d).to(dev).contiguous(memory_format=cl)
           for (h, w), d in zip(SIZES, head.reg_denoms)]
    ref = [(r.cpu() * (torch.randn(r.shape, generator=g) * 0.3).exp()).to(dev).contiguous(memory_format=cl) for r in reg]
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
        r = timed(fn, reps, warmup)
        floor = bytes_[name] / (HBM_COPY_TBS * 1e12) * 1e6
        r.update(mandatory_MB=round(bytes_[name] / 1e6, 2), hbm_floor_us=round(floor, 2), fraction_of_floor=round(floor / r['median_us'], 3))
        out[name] = r
    return out


def _total(ls):
    return sum(ls[k] for k in KEYS)


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg, ref = head_and_inputs(dev, batch)

    def step(fused):
        def run():
            head.fused_loss = fused
            maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg, ref)]
            _total(head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])).backward()
        return run
    assert head._fused_loss_ok(cls, reg, ref, data['gt_labels'], None, data['img_metas']), 'the fused path must take these maps'
    out = dict(table='head', batch=batch, anchors=sum(h * w for h, w in SIZES))
    out.update(alternated(dict(fused=step(True), tensor_path=step(False)), reps, warmup))
    out['fused_no_slower'] = out['fused']['median_us'] <= out['tensor_path']['median_us']
    head.fused_loss = True
    return out


def bench_step(dev, steps, warmup, batch):
    from htd_amd.configs import build_baseline_detector
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(kind, fused):
        torch.manual_seed(0)
        model = build_baseline_detector(kind)
        model.bbox_head.fused_loss = fused
        return Trainer(model.to(dev).train(), lr=0.0)                # lr 0: every leg times the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = dict(vfnet_fused=trainer('vfnet', True), vfnet_tensor_path=trainer('vfnet', False), gfl_fused=trainer('gfl', True),
                atss_fused=trainer('atss', True))
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
    out = dict(table='step', model='vfnet_r50_fpn', precision='fp32', batch=batch, image='1333x800', steps=steps, warmup=warmup)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = dict(median_ms=round(med, 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), img_per_s=round(batch * 1e3 / med, 2))
    out['fused_no_slower'] = out['vfnet_fused']['median_ms'] <= out['vfnet_tensor_path']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=['kernel', 'head', 'step'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_vfnet.py measures on the GPU only'
    dev = torch.device('cuda:0')
    capi.lib()
    slower = []
    for t in args.tables or ['kernel', 'head', 'step']:
        if t == 'kernel':
            out = bench_kernel(dev, args.reps, 10, args.batch)
        elif t == 'head':
            out = bench_head(dev, max(10, args.reps // 5), 3, args.batch)
        elif t == 'step':
            out = bench_step(dev, args.steps, args.warmup, args.batch)
        else:
            raise SystemExit(f'unknown table {t}')
        print(json.dumps(out), flush=True)
        if not out.get('fused_no_slower', True):
            slower.append(t)
    if slower:                                  # the fused path must be faster than the tensor path measured beside it
        raise SystemExit(f'the fused path is slower than the tensor path in: {", ".join(slower)}')


if __name__ == '__main__':
    main()
