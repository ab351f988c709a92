"""What the dense heads' tools (bench_retinanet / ghm / fcos / atss / gfl / vfnet / fovea .py) share, each written once: the timers,
the head and its seeded maps, the HBM-floor row, the fused / tensor-path head table, the alternated train-step table and the
command line.  A tool keeps its docstring, its bench_kernel, its extra tables and its `__main__` line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from htd_amd import capi  # noqa: E402

HBM_COPY_TBS = 6.29           # float4 copy on the MI355X (8.0 TB/s on paper)
SIZES = ((100, 168), (50, 84), (25, 42), (13, 21), (7, 11))
STRIDES = (8, 16, 32, 64, 128)


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


def head_from_config(config_fn, dev):
    """The bbox_head of config_fn(), built with the config's train_cfg and test_cfg."""
    from htd_amd import detector  # noqa: F401
    from htd_amd.registry import build_head
    cfg = config_fn()
    spec = cfg.model.bbox_head.to_dict()
    spec.update(train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    return build_head(spec).to(dev)


def seeded_maps(specs, batch, dev, g=None):
    """specs: per kind of map (channels, f(normal draw, level) -> CPU map) -> per kind the channels_last device maps of the five
    levels of SIZES, drawn kind after kind, level after level from one generator (seed 0 unless g is given)."""
    g = torch.Generator().manual_seed(0) if g is None else g
    return [[f(torch.randn(batch, c, h, w, generator=g), l).to(dev).contiguous(memory_format=torch.channels_last)
             for l, (h, w) in enumerate(SIZES)] for c, f in specs]


def floor_row(timing, bytes_):
    """A kernel's timing beside the HBM floor of its mandatory traffic at HBM_COPY_TBS."""
    floor = bytes_ / (HBM_COPY_TBS * 1e12) * 1e6
    timing.update(mandatory_MB=round(bytes_ / 1e6, 2), hbm_floor_us=round(floor, 2), fraction_of_floor=round(floor / timing['median_us'], 3))
    return timing


def head_table(head, run_loss, reps, warmup, after=None, **fields):
    """The head table: run_loss() (head.loss forward + backward on fresh leaves) with the fused path and with the tensor path,
    legs alternated.  after(out, step): the tool's own additions while both legs are still at hand."""
    def step(fused):
        def run():
            head.fused_loss = fused
            run_loss()
        return run
    out = dict(table='head', **fields)
    out.update(alternated(dict(fused=step(True), tensor_path=step(False)), reps, warmup))
    out['fused_no_slower'] = out['fused']['median_us'] <= out['tensor_path']['median_us']
    if after is not None:
        after(out, step)
    head.fused_loss = True
    return out


def build_detector(kind):
    from htd_amd import configs
    if kind in ('retinanet', 'retinanet_ghm'):
        return getattr(configs, f'build_{kind}_detector')()
    if kind in ('fovea', 'fovea_align'):
        return configs.build_fovea_detector(50, align=kind == 'fovea_align')
    return configs.build_baseline_detector(kind)


def step_table(dev, model_name, legs, pairs, steps, warmup, batch):
    """The step table: legs ((key, kind of detector, fused), ...) of the R50 fp32 synthetic train step in one process, alternated
    step by step; fused_no_slower over pairs ((fused key, tensor-path key), ...)."""
    from htd_amd.runner import Trainer, synthetic_batch

    def trainer(kind, fused):
        torch.manual_seed(0)
        model = build_detector(kind)
        model.bbox_head.fused_loss = fused
        if kind == 'fovea_align':
            model.bbox_head.feature_adaption.fused = fused
        return Trainer(model.to(dev).train(), lr=0.0)                # lr 0: every leg times the same weights throughout
    data = synthetic_batch(batch, device=dev, seed=0)
    legs = {key: trainer(kind, fused) for key, kind, fused in legs}
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
    out = dict(table='step', model=model_name, precision='fp32', batch=batch, image='1333x800', steps=steps, warmup=warmup)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = dict(median_ms=round(med, 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), img_per_s=round(batch * 1e3 / med, 2))
    out['fused_no_slower'] = all(out[f]['median_ms'] <= out[t]['median_ms'] for f, t in pairs)
    return out


def main(tool_name, tables, strict=False):
    """tables: {name: (f(dev, count, warmup, batch), f(args) -> (count, warmup))} in the default order.  The present defaults are
    KERNEL, HEAD and STEP below.  strict: exit non-zero if a table says the fused path was slower than the tensor path."""
    ap = argparse.ArgumentParser()
    ap.add_argument('tables', nargs='*', default=list(tables))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), f'{tool_name} measures on the GPU only'
    dev = torch.device('cuda:0')
    capi.lib()
    slower = []
    for t in args.tables or list(tables):
        if t not in tables:
            raise SystemExit(f'unknown table {t}')
        fn, counts = tables[t]
        out = fn(dev, *counts(args), args.batch)
        print(json.dumps(out), flush=True)
        if not out.get('fused_no_slower', True):
            slower.append(t)
    if strict and slower:                       # the fused path must be faster than the tensor path measured beside it
        raise SystemExit(f'the fused path is slower than the tensor path in: {", ".join(slower)}')


KERNEL = lambda args: (args.reps, 10)                       # noqa: E731
HEAD = lambda args: (max(10, args.reps // 5), 3)            # noqa: E731
STEP = lambda args: (args.steps, args.warmup)               # noqa: E731
