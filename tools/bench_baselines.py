#!/usr/bin/env python3
"""Cost of the Faster R-CNN / Cascade R-CNN baselines next to HTD, three tables:

  kernel   htd_roi_head_loss_classes on 2048 x 81 inputs: class-specific L1 and smooth-L1 (320 box columns per row) and the
           class-agnostic forms, against htd_roi_head_loss on the same rows
  head     BBoxHead.loss with reg_class_agnostic=False + L1Loss (the Faster R-CNN head), forward + backward at 2048 x 81: fused
           kernel against the tensor formulation (fused_loss=False)
  step     the R50 B = 4 1333 x 800 synthetic train step of Faster R-CNN, Cascade R-CNN and HTD in one process, legs alternated
           step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_baselines.py [kernel] [head] [step] [--steps K] [--warmup W] [--batch B]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htd_amd import capi  # noqa: E402


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
    """Logits, class-specific deltas, encoded targets, weights and labels of n sample slots, a quarter of them positives."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(n, 81, generator=g) * 3
    full = 0.5 * torch.randn(n, 320, generator=g)
    tgt = 0.5 * torch.randn(n, 4, generator=g)
    labels = torch.randint(0, 80, (n, ), generator=g)
    labels[torch.rand(n, generator=g) < 0.75] = 80
    bw = (labels < 80).float()[:, None].expand(n, 4).contiguous()
    own = full.view(n, 80, 4)[torch.arange(n), labels.clamp(max=79)].contiguous()
    return [t.to(dev) for t in (cls, full, own, tgt * bw, bw, labels)]


def bench_kernel(dev, reps, warmup, n=2048):
    cls, full, own, tgt, bw, labels = rows(n, dev)
    lw = torch.ones(n, device=dev)
    partial = torch.empty(capi.lib().htd_roi_head_loss_partial_rows(), 4, device=dev)
    gcls, gfull, gown = torch.empty_like(cls), torch.empty_like(full), torch.empty_like(own)
    stream = capi.current_stream_ptr()

    def agnostic():
        capi.call('htd_roi_head_loss', capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(own), capi.ptr(tgt), capi.ptr(bw), n,
                  81, 80, 1.0, capi.ptr(partial), capi.ptr(gcls), capi.ptr(gown), stream)

    def classes(reg, box_loss):
        pred, gbox = (full, gfull) if reg > 1 else (own, gown)

        def run():
            capi.call('htd_roi_head_loss_classes', capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(pred), capi.ptr(tgt),
                      capi.ptr(bw), n, 81, 80, reg, box_loss, 1.0, capi.ptr(partial), capi.ptr(gcls), capi.ptr(gbox), stream)
        return run
    out = dict(table='kernel', n=n, NC=81, htd_roi_head_loss=timed(agnostic, reps, warmup))
    for key, reg, box_loss in (('classes_80_l1', 80, 1), ('classes_80_smooth_l1', 80, 0), ('classes_1_l1', 1, 1),
                               ('classes_1_smooth_l1', 1, 0)):
        out[key] = timed(classes(reg, box_loss), reps, warmup)
    out['htd_roi_head_loss_again'] = timed(agnostic, reps, warmup)
    return out


def bench_head(dev, reps, warmup, n=2048):
    from htd_amd.detector.bbox_heads import BBoxHead
    cls, full, own, tgt, bw, labels = rows(n, dev)
    lw = torch.ones(n, device=dev)
    ns = torch.tensor(n, device=dev)
    head = BBoxHead(with_avg_pool=False, roi_feat_size=1, in_channels=8, num_classes=80, reg_class_agnostic=False,
                    loss_bbox=dict(type='L1Loss', loss_weight=1.0)).to(dev)
    out = dict(table='head', n=n, NC=81, loss='L1Loss', reg_class_agnostic=False)

    def step():
        c, d = cls.clone().requires_grad_(), full.clone().requires_grad_()
        losses = head.loss(c, d, None, labels, lw, tgt, bw, num_samples=ns)
        (losses['loss_cls'] + losses['loss_bbox']).backward()
    for fused in (True, False, True):
        head.fused_loss = fused
        key = ('fused' if fused else 'tensor_formulation') + ('_again' if fused and 'fused' in out else '')
        out[key] = timed(step, reps, warmup)
    out['fused_no_slower'] = out['fused']['median_us'] <= out['tensor_formulation']['median_us']
    return out


def bench_step(dev, steps, warmup, batch):
    from htd_amd.configs import build_baseline_detector, build_htd_detector
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(kind):
        torch.manual_seed(0)
        model = build_htd_detector(50) if kind == 'htd' else build_baseline_detector(kind)
        return Trainer(model.to(dev).train(), lr=0.0), model         # lr 0: every leg times the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = {k: trainer(k) for k in ('faster_rcnn', 'cascade_rcnn', 'htd')}
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
    out = dict(table='step', backbone='R50', batch=batch, image='1333x800', steps=steps, warmup=warmup)
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
    assert torch.cuda.is_available(), 'bench_baselines.py measures on the GPU only'
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
