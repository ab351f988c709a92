#!/usr/bin/env python
"""Time the COCO bbox evaluation on the device on a val2017-shaped synthetic set (5000 images, 80 categories, ~36.8k
ground truths, 100 detections per image): from bbox2result lists on the host to the 12 stats.

    python tools/bench_coco_eval.py [--images 5000] [--reps 5] [--host]

Prints one JSON line: convert (result lists -> arrays), evaluate (coco_eval: upload, sorts, match, accumulate, copy back,
summarize), the match / accumulate kernel times (device events), summarize alone, the whole CocoEvaluator.evaluate
call, and with --host the numpy restatement of COCOeval (tests/coco_eval_np.py) on the same arrays."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host', action='store_true', help='also time the numpy restatement (minutes at full size)')
    args = ap.parse_args()
    import torch
    from coco_eval_np import coco_eval_np, synthetic_coco
    from htd_amd import capi
    from htd_amd.coco import CocoEvaluator
    from htd_amd.core.evaluation import coco_eval, summarize
    assert torch.cuda.is_available(), 'bench_coco_eval needs the GPU'

    ann, res = synthetic_coco(n_img=args.images, gt_per_img=36781 / 5000, det_per_img=100, seed=0)
    ev = CocoEvaluator(ann, classes=[c['name'] for c in ann['categories']])

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t

    ev.evaluate(res)                                     # warm-up: code objects, allocator, sort kernels
    conv, evals, full, summ, kern = [], [], [], [], {}
    for _ in range(args.reps):
        dt, t = timed(lambda: ev._det_arrays(res))
        conv.append(t)
        capi.profile_begin()
        out, t = timed(lambda: coco_eval(ev.gt, dt, ev.img_ids, ev.cat_ids))
        prof = capi.profile_end()
        evals.append(t)
        for name, (_, ms, *_rest) in prof.items():
            kern.setdefault(name, []).append(ms)
        _, t = timed(lambda: summarize(out['precision'], out['recall'], out['params']['iou_thrs'],
                                       out['params']['max_dets']))
        summ.append(t)
        _, t = timed(lambda: ev.evaluate(res))
        full.append(t)
    med = lambda v: float(np.median(v))
    line = dict(images=args.images, gts=len(ev.gt['id']), dets=int(len(dt['score'])),
                convert_s=med(conv), coco_eval_s=med(evals), summarize_s=med(summ), evaluate_s=med(full),
                match_ms=med(kern.get('htd_coco_match', [0])), accumulate_ms=med(kern.get('htd_coco_accumulate', [0])),
                stats=[round(float(x), 6) for x in out['stats']])
    if args.host:
        dtn = {k: v.numpy() for k, v in dt.items()}
        t = time.perf_counter()
        ref = coco_eval_np(ev.gt, dtn, ev.img_ids, ev.cat_ids)
        line['host_restatement_s'] = time.perf_counter() - t
        line['host_equal'] = bool(all(np.array_equal(out[k], ref[k]) for k in ('precision', 'recall', 'scores', 'stats')))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
