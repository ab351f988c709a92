#!/usr/bin/env python3
"""Cost of the IoU-family regression losses on decoded boxes (htd_roi_head_loss_decoded), three tables:

  kernel   the new entry point against htd_roi_head_loss on the same 2048 x 81 inputs, per kind
  head     BBoxHead.loss with reg_decoded_bbox + GIoULoss, forward + backward: fused kernel against the tensor formulation
  step     the R50 B = 4 1333 x 800 synthetic train step with GIoU on both stages against the default smooth-L1 step, in one
           process, legs alternated; the smooth-L1 leg runs twice (two detectors) to give the run-to-run spread

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_iou_loss.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htd_amd import capi  # noqa: E402
from htd_amd.core.bbox import _d4  # noqa: E402

KINDS = ('IoULoss', 'BoundedIoULoss', 'GIoULoss', 'DIoULoss', 'CIoULoss')
STDS = (0.1, 0.1, 0.2, 0.2)


def timed(fn, reps, warmup):
    """Median and spread (min, max) of fn()'s device time in microseconds."""
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


def rows(n, dev, seed=0):
    """RoIs, deltas, gt boxes, weights and labels in the recipe of tests/golden/make_golden_iou_loss.py."""
    g = torch.Generator().manual_seed(seed)
    c = 20 + 280 * torch.rand(n, 2, generator=g)
    s = torch.exp(torch.rand(n, 2, generator=g) * (5.298 - 1.386) + 1.386)
    rois = torch.cat([c - s / 2, c + s / 2], 1)
    gc = c + (torch.rand(n, 2, generator=g) * 0.7 - 0.35) * s
    gs = s * torch.exp(torch.rand(n, 2, generator=g) - 0.5)
    gts = torch.cat([gc - gs / 2, gc + gs / 2], 1)
    deltas = 0.5 * torch.randn(n, 4, generator=g)
    labels = torch.randint(0, 80, (n, ), generator=g)
    labels[torch.rand(n, generator=g) < 0.75] = 80                  # a quarter of the sampled rows are positives
    bw = (labels < 80).float()[:, None].expand(n, 4).contiguous()
    cls = torch.randn(n, 81, generator=g) * 3
    return [t.to(dev) for t in (cls, rois, deltas, gts, bw, labels)]


def bench_kernel(dev, reps, warmup, n=2048):
    cls, rois, deltas, gts, bw, labels = rows(n, dev)
    lw = torch.ones(n, device=dev)
    partial = torch.empty(capi.lib().htd_roi_head_loss_partial_rows(), 4, device=dev)
    box_lo = torch.empty(partial.size(0), device=dev)
    gcls, gbox = torch.empty_like(cls), torch.empty(n, 4, device=dev)
    stream = capi.current_stream_ptr()

    def smooth_l1():
        capi.call('htd_roi_head_loss', capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(deltas), capi.ptr(gts), capi.ptr(bw), n,
                  81, 80, 1.0, capi.ptr(partial), capi.ptr(gcls), capi.ptr(gbox), stream)
    out = dict(table='kernel', n=n, NC=81, htd_roi_head_loss=timed(smooth_l1, reps, warmup))
    for kind, name in enumerate(KINDS):
        def decoded():
            capi.call('htd_roi_head_loss_decoded', capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(rois), capi.ptr(deltas),
                      capi.ptr(gts), capi.ptr(bw), n, 81, 80, _d4((0., 0., 0., 0.)), _d4(STDS), 16 / 1000, kind,
                      1e-3 if kind == 1 else 1e-6, 0.2, capi.ptr(partial), capi.ptr(box_lo), capi.ptr(gcls), capi.ptr(gbox), stream)
        out[name] = timed(decoded, reps, warmup)
    out['htd_roi_head_loss_again'] = timed(smooth_l1, reps, warmup)
    return out


def bench_head(dev, reps, warmup, n=2048):
    from htd_amd.detector.bbox_heads import BBoxHead
    cls, rois, deltas, gts, bw, labels = rows(n, dev)
    lw = torch.ones(n, device=dev)
    rois5 = torch.cat([torch.zeros(n, 1, device=dev), rois], 1)
    ns = torch.tensor(n, device=dev)
    head = BBoxHead(with_avg_pool=False, roi_feat_size=1, in_channels=8, num_classes=80, reg_class_agnostic=True,
                    reg_decoded_bbox=True, loss_bbox=dict(type='GIoULoss', loss_weight=10.0)).to(dev)
    out = dict(table='head', n=n, NC=81, loss='GIoULoss')

    def step():
        c, d = cls.clone().requires_grad_(), deltas.clone().requires_grad_()
        losses = head.loss(c, d, rois5, labels, lw, gts, bw, num_samples=ns)
        (losses['loss_cls'] + losses['loss_bbox']).backward()
    for fused in (True, False, True):
        head.fused_loss = fused
        key = ('fused' if fused else 'tensor_formulation') + ('_again' if fused and 'fused' in out else '')
        out[key] = timed(step, reps, warmup)
    return out


def bench_step(dev, steps, warmup, batch):
    from htd_amd.configs import build_htd_detector, htd_config
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(giou):
        cfg = htd_config(50)
        if giou:
            for h in cfg.model.roi_head.bbox_head:
                h.update(reg_decoded_bbox=True, loss_bbox=dict(type='GIoULoss', loss_weight=10.0))
        torch.manual_seed(0)
        model = build_htd_detector(cfg=cfg).to(dev).train()
        return Trainer(model, lr=0.0), model                       # lr 0: every leg times the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = dict(smooth_l1_a=trainer(False), giou=trainer(True), smooth_l1_b=trainer(False))
    times = {k: [] for k in legs}
    for k, (tr, _) in legs.items():
        for _ in range(warmup):
            tr.train_step(data)
    torch.cuda.synchronize()
    for _ in range(steps):                                          # alternate the legs step by step
        for k, (tr, _) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.train_step(data)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = dict(table='step', model='HTD-R50', batch=batch, image='1333x800', steps=steps, warmup=warmup)
    for k, v in times.items():
        v = sorted(v)
        med = statistics.median(v)
        out[k] = dict(median_ms=round(med, 2), min_ms=round(v[0], 2), max_ms=round(v[-1], 2), img_per_s=round(batch * 1e3 / med, 2))
    out['static_path'] = {k: hasattr(m.roi_head, '_last_static') for k, (_, m) in legs.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=['kernel', 'head', 'step'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_iou_loss.py measures on the GPU only'
    dev = torch.device('cuda:0')
    capi.lib()
    for t in args.tables or ['kernel', 'head', 'step']:
        if t == 'kernel':
            print(json.dumps(bench_kernel(dev, args.reps, 20)), flush=True)
        elif t == 'head':
            print(json.dumps(bench_head(dev, args.reps, 20)), flush=True)
        elif t == 'step':
            print(json.dumps(bench_step(dev, args.steps, args.warmup, args.batch)), flush=True)
        else:
            raise SystemExit(f'unknown table {t}')


if __name__ == '__main__':
    main()
