#!/usr/bin/env python
"""Time the Pascal VOC mean AP (eval_map) on the device on a VOC07-test-shaped synthetic set (4952 images, 20 classes,
up to 100 detections per image, distinct scores), in VOC07's 11-point mode.

    python tools/bench_voc_eval.py [--images 4952] [--reps 5] [--no-host]

Prints one JSON line (medians over --reps): `lists_s` from bbox2result lists to mAP, `triple_s` from the device-resident
(dets, labels, image index) triple to mAP, the tpfp / accumulate kernel times from device events, and `numpy_s`, the
serial numpy restatement of the reference's eval_map (tests/voc_eval_np.py) on the same inputs, whose mAP must agree."""
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
    ap.add_argument('--images', type=int, default=4952)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement')
    args = ap.parse_args()
    import torch
    from voc_eval_np import eval_map_np, synthetic_voc
    from htd_amd import capi
    from htd_amd.apis import results_to_tensors
    from htd_amd.core.evaluation import eval_map
    assert torch.cuda.is_available(), 'bench_voc_eval needs the GPU'

    dets, anns = synthetic_voc(args.images, 20, dets_per_img=100, seed=5)
    triple = tuple(t.cuda() for t in results_to_tensors(dets))
    n_det = int(triple[0].shape[0])

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    run_lists = lambda: eval_map(dets, anns, dataset='voc07', logger='silent')
    run_triple = lambda: eval_map(triple, anns, dataset='voc07', logger='silent')
    run_lists()                                                       # warm-up: library load, allocator
    lists = [timed(run_lists) for _ in range(args.reps)]
    trip = [timed(run_triple) for _ in range(args.reps)]
    assert all(x[1][0] == lists[0][1][0] for x in lists + trip)
    capi.profile_begin()
    for _ in range(args.reps):
        run_triple()
    prof = capi.profile_end()
    kern = {k: v[1] / v[0] for k, v in prof.items() if k.startswith('htd_voc')}          # ms per call
    out = dict(images=args.images, classes=20, detections=n_det,
               ground_truths=int(sum(len(a['labels']) + len(a['labels_ignore']) for a in anns)),
               mAP=lists[0][1][0], lists_s=float(np.median([x[0] for x in lists])),
               triple_s=float(np.median([x[0] for x in trip])),
               tpfp_ms=kern.get('htd_voc_tpfp'), accumulate_ms=kern.get('htd_voc_accumulate'))
    if not args.no_host:
        t = time.perf_counter()
        ref = eval_map_np(dets, anns, dataset='voc07')
        out['numpy_s'] = time.perf_counter() - t
        assert ref[0] == out['mAP'], (ref[0], out['mAP'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
