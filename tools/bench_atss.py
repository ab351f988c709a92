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


def head_and_inputs(dev, batch):
    from htd_amd import detector  # noqa: F401
    from htd_amd.configs import atss_config
    from htd_amd.registry import build_head
    from htd_amd.runner import synthetic_batch
    cfg = atss_config()
    spec = cfg.model.bbox_head.to_dict()
    spec.update(train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    head = build_head(spec).to(dev)
    data = synthetic_batch(batch, device=dev, seed=0)
    g = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    cls = [(torch.randn(batch, 80, h, w, generator=g) - 4.0).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    reg = [torch.randn(batch, 4, h, w, generator=g).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    ctr = [torch.randn(batch, 1, h, w, generator=g).to(dev).contiguous(memory_format=cl) for h, w in SIZES]
    return head, data, cls, reg, ctr


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
        r = timed(fn, reps, warmup)
        floor = bytes_[name] / (HBM_COPY_TBS * 1e12) * 1e6
        r.update(mandatory_MB=round(bytes_[name] / 1e6, 2), hbm_floor_us=round(floor, 2), fraction_of_floor=round(floor / r['median_us'], 3))
        out[name] = r
    return out


def bench_head(dev, reps, warmup, batch):
    head, data, cls, reg, ctr = head_and_inputs(dev, batch)

    def step(fused):
        def run():
            head.fused_loss = fused
            maps = [[t.detach().requires_grad_() for t in ms] for ms in (cls, reg, ctr)]
            ls = head.loss(*maps, data['gt_bboxes'], data['gt_labels'], data['img_metas'])
            (sum(ls['loss_cls']) + sum(ls['loss_bbox']) + sum(ls['loss_centerness']) if isinstance(ls['loss_cls'], list)
             else ls['loss_cls'] + ls['loss_bbox'] + ls['loss_centerness']).backward()
        return run
    assert head._fused_loss_ok(cls, reg, ctr, data['gt_labels'], None, data['img_metas']), 'the fused path must take these maps'
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
    legs = dict(atss_fused=trainer('atss', True), atss_tensor_path=trainer('atss', False), fcos_fused=trainer('fcos', True),
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
    out = dict(table='step', model='atss_r50_fpn', precision='fp32', batch=batch, image='1333x800', steps=steps, warmup=warmup)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = dict(median_ms=round(med, 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), img_per_s=round(batch * 1e3 / med, 2))
    out['fused_no_slower'] = out['atss_fused']['median_ms'] <= out['atss_tensor_path']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=['kernel', 'head', 'step'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_atss.py measures on the GPU only'
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
