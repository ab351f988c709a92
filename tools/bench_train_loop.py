#!/usr/bin/env python
"""Time the train loop (CocoDataset -> build_dataloader -> collate -> Trainer.train_step -> log buffer, with the
checkpoint, logging and evaluation hooks) on a synthetic COCO-shaped set: tools/bench_test_loop.py:write_set's JPEGs at
640x480 and 480x640, trained with R50 at the config's (1333, 800) scale.

    python tools/bench_train_loop.py [--images 64] [--spg 2 4] [--workers 0 2] [--rounds 2]

The weights are seeded, not trained.  Each (samples_per_gpu, workers_per_gpu) trains one epoch over the set through
htd_amd.apis.train_detector (log interval 10, a checkpoint, evaluation on a 16-image set), then runs Trainer.train_step
on the same batches collated beforehand; the two alternate `--rounds` times in one process and the last round is
reported.  One JSON line per run: img/s of the whole loop, seconds waiting on the loader, seconds in the hooks (logging,
checkpoint, evaluation; the reads of the log sums, which wait for the queued steps, count as loop time), ms per
iteration of the loop without the hooks, ms per iteration of the bare train_step, and their difference: the runner's
cost per iteration, loader wait included."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def train_cfg(root, ann, val_root, val_ann, spg, workers, work_dir):
    from htd_amd.configs import htd_config
    cfg = htd_config(50)
    cfg.model.pretrained = None
    cfg.data.train.update(ann_file=ann, img_prefix=os.path.join(root, 'imgs'))
    cfg.data.val.update(ann_file=val_ann, img_prefix=os.path.join(val_root, 'imgs'))
    cfg.data.samples_per_gpu, cfg.data.workers_per_gpu = spg, workers
    cfg.total_epochs, cfg.seed, cfg.work_dir = 1, 1, work_dir
    cfg.log_config = dict(interval=10, hooks=[dict(type='TextLoggerHook')])
    return cfg


def run(model, cfg):
    import torch
    from htd_amd.apis import set_random_seed, train_detector
    from htd_amd.datasets import build_dataloader, build_dataset
    from htd_amd.pipelines import collate
    ds = build_dataset(cfg.data.train.to_dict())
    set_random_seed(1)
    torch.cuda.synchronize()
    runner = train_detector(model, ds, cfg, validate=True, timestamp='bench')
    torch.cuda.synchronize()
    tm = runner.timing
    iters = tm['iters']
    # the bare step on the same kind of batches, collated beforehand
    set_random_seed(1)
    batches = [collate(b, 'cuda:0') for b in build_dataloader(ds, cfg.data.samples_per_gpu, 0, dist=False, shuffle=True,
                                                             seed=1)]
    tr = runner.trainer
    tr.train_step(batches[0])
    torch.cuda.synchronize()
    t = time.perf_counter()
    for b in batches:
        tr.train_step(b)
    torch.cuda.synchronize()
    bare_ms = (time.perf_counter() - t) * 1e3 / len(batches)
    tr.flat.close()
    # the reads of the log sums wait for the queued steps: that wait is step time, the rest of the hooks is not
    hooks_s = tm['hooks_s'] - tm['sync_s']
    loop_ms = (tm['run_s'] - hooks_s) * 1e3 / iters
    return dict(images=len(ds), samples_per_gpu=cfg.data.samples_per_gpu, workers_per_gpu=cfg.data.workers_per_gpu,
                iters=iters, img_per_s=round(iters * cfg.data.samples_per_gpu / tm['run_s'], 2),
                loop_s=round(tm['run_s'], 3), loader_wait_s=round(tm['loader_s'], 3), hooks_s=round(hooks_s, 3),
                loop_ms_per_iter=round(loop_ms, 2), bare_train_step_ms=round(bare_ms, 2),
                runner_overhead_ms=round(loop_ms - bare_ms, 2),
                runner_overhead_pct=round(100 * (loop_ms - bare_ms) / bare_ms, 2),
                loader_wait_ms_per_iter=round(tm['loader_s'] * 1e3 / iters, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--spg', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--workers', type=int, nargs='+', default=[0, 2])
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    assert max(args.workers) <= 4
    import torch
    assert torch.cuda.is_available(), 'bench_train_loop needs the GPU'
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    from bench_test_loop import write_set
    from golden_util import load_seeded_
    from htd_amd.configs import build_htd_detector, htd_config
    with tempfile.TemporaryDirectory() as root:
        ann = write_set(root, args.images)
        val_root = os.path.join(root, 'val')
        val_ann = write_set(val_root, 16, seed=1)
        for spg in args.spg:
            for workers in args.workers:
                out = None
                for r in range(args.rounds):
                    model = load_seeded_(build_htd_detector(cfg=htd_config(50)), 'det.').cuda()
                    out = run(model, train_cfg(root, ann, val_root, val_ann, spg, workers, os.path.join(root, 'work')))
                    del model
                    torch.cuda.empty_cache()
                print(json.dumps(dict(model='r50', **out)), flush=True)


if __name__ == '__main__':
    main()
