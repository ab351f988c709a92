#!/usr/bin/env python3
"""Cost of the whole-map GroupNorm and weight-standardisation kernels (csrc/group_norm_map.hip), three tables:

  maps     the GroupNorm maps of an R50-FPN on a 4 x 800 x 1344 batch (stem, the four stages' widths and outputs, the two fine
           pyramid levels): htd_group_norm_map_fwd / _bwd with ReLU, against (a) the float4-copy rate of 6.29 TB/s on their
           algorithmic bytes -- forward 2 reads + 1 write of the map, backward 2 x (x, y, gy) reads + 1 write -- and (b) the RoI-tile
           kernels of group_norm_relu (htd_group_norm_relu_fwd / _bwd_ws) on the same tensor where they accept it (C <= 1024)
  ws       htd_weight_standardize_fwd / _bwd on the distinct weight shapes of the GN+WS R50-FPN Faster R-CNN
  step     the R50 B = 4 1333 x 800 synthetic train step of the GN+WS Faster R-CNN next to the BatchNorm-folded Faster R-CNN, in
           one process, legs alternated step by step

Warm-up first, device events around every timed call, medians.  One JSON line per table.
usage: bench_group_norm.py [maps] [ws] [step] [--steps K] [--warmup W] [--reps R] [--batch B]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htd_amd import capi  # noqa: E402

COPY_TBS = 6.29
P_, S_ = capi.ptr, capi.current_stream_ptr
# (name, C, h, w) at batch 4, 800 x 1344 input; G = 32 throughout
MAPS = [('stem', 64, 400, 672), ('layer1 width', 64, 200, 336), ('layer1 out', 256, 200, 336), ('layer2 width', 128, 100, 168),
        ('layer2 out', 512, 100, 168), ('layer3 width', 256, 50, 84), ('layer3 out', 1024, 50, 84), ('layer4 width', 512, 25, 42),
        ('layer4 out', 2048, 25, 42), ('fpn P2', 256, 200, 336), ('fpn P3', 256, 100, 168)]


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
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def bench_maps(dev, reps, warmup, batch):
    L = capi.lib()
    out = dict(table='maps', batch=batch, copy_tbs=COPY_TBS, rows=[])
    for name, C, h, w in MAPS:
        n, P, G = batch, h * w, 32
        x = torch.randn(n, h, w, C, device=dev)
        gy = torch.randn(n, h, w, C, device=dev)
        y, gx = torch.empty_like(x), torch.empty_like(x)
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
        mean, rstd = torch.empty(n, G, device=dev), torch.empty(n, G, device=dev)
        gg, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(L.htd_group_norm_map_workspace_bytes(n, P, C, G), dtype=torch.uint8, device=dev)
        ws_old = torch.empty(2 * n * C, device=dev)

        def fwd():
            capi.call('htd_group_norm_map_fwd', P_(x), None, P_(gamma), P_(beta), P_(y), P_(mean), P_(rstd), n, P, C, G, 1e-5, 1,
                      P_(ws), None, S_())

        def bwd():
            capi.call('htd_group_norm_map_bwd', P_(x), P_(y), P_(gamma), P_(mean), P_(rstd), P_(gy), P_(gx), None, P_(gg), P_(gb), n,
                      P, C, G, 1, P_(ws), None, S_())

        def fwd_old():
            capi.call('htd_group_norm_relu_fwd', P_(x), P_(gamma), P_(beta), P_(y), P_(mean), P_(rstd), n, P, C, G, 1e-5, 1, S_())

        def bwd_old():
            capi.call('htd_group_norm_relu_bwd_ws', P_(x), P_(y), P_(gamma), P_(mean), P_(rstd), P_(gy), P_(gx), P_(gg), P_(gb), n, P,
                      C, G, 1, P_(ws_old), S_())
        nbytes = 4.0 * x.numel()
        f, b = timed(fwd, reps, warmup), timed(bwd, reps, warmup)
        row = dict(map=name, C=C, hw=[h, w], MB=round(nbytes / 2 ** 20, 1), slab=L.htd_group_norm_map_slab(P, C),
                   fwd_us=round(f, 1), fwd_of_floor=round(3 * nbytes / (COPY_TBS * 1e6) / f, 3),
                   bwd_us=round(b, 1), bwd_of_floor=round(7 * nbytes / (COPY_TBS * 1e6) / b, 3))
        if C <= 1024:                    # the tile kernels: one workgroup per sample; few repetitions, they take milliseconds
            fo, bo = timed(fwd_old, max(3, reps // 20), 1), timed(bwd_old, max(3, reps // 20), 1)
            row.update(tile_fwd_us=round(fo, 1), tile_bwd_us=round(bo, 1), fwd_ratio=round(fo / f, 1), bwd_ratio=round(bo / b, 1))
        out['rows'].append(row)
        del x, gy, y, gx, ws
    out['faster_on_every_map'] = all(r.get('fwd_ratio', 2) > 1 and r.get('bwd_ratio', 2) > 1 for r in out['rows'])
    return out


def bench_ws(dev, reps, warmup):
    from htd_amd.configs import build_baseline_detector
    model = build_baseline_detector('faster_rcnn_gn_ws')
    shapes = {}
    for m in model.modules():
        if type(m).__name__ == 'ConvWS2d':
            key = (m.weight.size(0), m.weight.numel() // m.weight.size(0))
            shapes[key] = shapes.get(key, 0) + 1
    out = dict(table='ws', layers=sum(shapes.values()), rows=[])
    total_f = total_b = 0.0
    for (Co, K), count in sorted(shapes.items()):
        w, g = torch.randn(Co, K, device=dev) * 0.05, torch.randn(Co, K, device=dev)
        o, gw = torch.empty_like(w), torch.empty_like(w)
        mean, inv = torch.empty(Co, device=dev), torch.empty(Co, device=dev)
        f = timed(lambda: capi.call('htd_weight_standardize_fwd', P_(w), P_(o), P_(mean), P_(inv), Co, K, 1e-5, S_()), reps, warmup)
        b = timed(lambda: capi.call('htd_weight_standardize_bwd', P_(w), P_(mean), P_(inv), P_(g), P_(gw), Co, K, 1e-5, S_()), reps,
                  warmup)
        total_f, total_b = total_f + count * f, total_b + count * b
        out['rows'].append(dict(Co=Co, K=K, layers=count, fwd_us=round(f, 1), bwd_us=round(b, 1)))
    out['model_fwd_us'], out['model_bwd_us'] = round(total_f, 1), round(total_b, 1)
    return out


def bench_step(dev, steps, warmup, batch):
    from htd_amd.configs import build_baseline_detector
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(kind):
        torch.manual_seed(0)
        return Trainer(build_baseline_detector(kind).to(dev).train(), lr=0.0)        # lr 0: the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = {k: trainer(k) for k in ('faster_rcnn', 'faster_rcnn_gn_ws')}
    times = {k: [] for k in legs}
    for tr in legs.values():
        for _ in range(warmup):
            tr.train_step(data)
    torch.cuda.synchronize()
    for _ in range(steps):                                          # alternate the legs step by step
        for k, tr in legs.items():
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=['maps', 'ws', 'step'])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_group_norm.py measures on the GPU only'
    dev = torch.device('cuda:0')
    capi.lib()
    for t in args.tables or ['maps', 'ws', 'step']:
        if t == 'maps':
            print(json.dumps(bench_maps(dev, args.reps, 10, args.batch)), flush=True)
        elif t == 'ws':
            print(json.dumps(bench_ws(dev, args.reps, 10)), flush=True)
        elif t == 'step':
            print(json.dumps(bench_step(dev, args.steps, args.warmup, args.batch)), flush=True)
        else:
            raise SystemExit(f'unknown table {t}')


if __name__ == '__main__':
    main()
