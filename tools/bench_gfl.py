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

KEYS = ('loss_cls', 'loss_bbox', 'loss_dfl')


def head_and_inputs(dev, batch):
    from htd_amd import detector  # noqa: F401
    from htd_amd.configs import gfl_config
    from htd_amd.registry import build_head
    from htd_amd.runner import synthetic_batch
    cfg = gfl_config()
    spec = cfg.model.bbox_head.to_dict()
    spec.update(train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    head = build_head(spec).to(dev)
    data = synthetic_batch(batch, device=dev, seed=0)
    g = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    cls = [(torch.randn(batch, 80, h, w, generator=g) - 4.0).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    reg = [torch.randn(batch, 4 * (head.reg_max + 1), h, w, generator=g).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    return head, data, cls, reg


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
        r = timed(fn, reps, warmup)
        floor = bytes_[name] / (HBM_COPY_TBS * 1e12) * 1e6
        r.update(mandatory_MB=round(bytes_[name] / 1e6, 2), hbm_floor_us=round(floor, 2), fraction_of_floor=round(floor / r['median_us'], 3))
        out[name] = r
    return out


def _total(ls):
    return sum(sum(ls[k]) if isinstance(ls[k], list) else ls[k] for k in KEYS)


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg = head_and_inputs(dev, batch)

    def step(fused):
        def run():
            head.fused_loss = fused
            maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg)]
            _total(head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])).backward()
        return run
    assert head._fused_loss_ok(cls, reg, data['gt_labels'], None, data['img_metas']), 'the fused path must take these maps'
    out = dict(table='head', batch=batch, anchors=sum(h * w for h, w in SIZES))
    out.update(alternated(dict(fused=step(True), tensor_path=step(False)), reps, warmup))
    out['fused_no_slower'] = out['fused']['median_us'] <= out['tensor_path']['median_us']
    head.fused_loss = True
    return out


def bench_step(dev, steps, warmup, batch):
    from htd_amd.configs import build_baseline_detector, build_retinanet_detector
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(kind, fused):
        torch.manual_seed(0)
        model = build_retinanet_detector() if kind == 'retinanet' else build_baseline_detector(kind)
        model.bbox_head.fused_loss = fused
        return Trainer(model.to(dev).train(), lr=0.0)                # lr 0: every leg times the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = dict(gfl_fused=trainer('gfl', True), gfl_tensor_path=trainer('gfl', False), atss_fused=trainer('atss', True),
                retinanet_fused=trainer('retinanet', True))
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
    out = dict(table='step', model='gfl_r50_fpn', precision='fp32', batch=batch, image='1333x800', steps=steps, warmup=warmup)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = dict(median_ms=round(med, 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), img_per_s=round(batch * 1e3 / med, 2))
    out['fused_no_slower'] = out['gfl_fused']['median_ms'] <= out['gfl_tensor_path']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=['kernel', 'head', 'step'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_gfl.py measures on the GPU only'
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
