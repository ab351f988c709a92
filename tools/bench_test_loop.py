#!/usr/bin/env python
"""Time the COCO test loop (CocoDataset -> build_dataloader -> collate -> detector -> evaluate) on a synthetic
COCO-shaped set: JPEGs at 640x480 and 480x640 written with PIL to a temporary directory, plus an annotation json.

    python tools/bench_test_loop.py [--images 500] [--spg 1 8] [--workers 0 4] [--models r50 r101 r101_hard]

Models: r50 (hard NMS), r101 (soft-NMS, as the released R101 configs test), r101_hard (the same R101 with hard NMS:
the difference to r101 is the per-image soft-NMS path).  The weights are seeded, not trained; `dets_per_img` says how
many detections the post-processing produced.  Each (model, samples_per_gpu, workers_per_gpu) runs the test pipeline
of the configs (1333 x 800, Pad 32) over every image once, after a 16-image warm-up of the model.  One JSON line per
run: images/s of the whole loop (loader start to the loader's end), and the seconds spent starting the loader
(iter(): spawning the workers), waiting for its batches (its end included), in the model (collate + forward + results on
the host) and in dataset.evaluate."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def write_set(root, n, seed=0):
    """n JPEGs (every other one portrait) with 1-6 boxes each over 80 categories; -> annotation file."""
    from PIL import Image
    from htd_amd.coco import COCO_CLASSES
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'imgs'), exist_ok=True)
    images, anns = [], []
    yy, xx = np.mgrid[0:640, 0:640]
    for i in range(n):
        h, w = (480, 640) if i % 2 == 0 else (640, 480)
        base = ((np.sin(xx[:h, :w] / (7 + i % 13)) + np.cos(yy[:h, :w] / (5 + i % 11))) * 60 + 128)
        img = np.clip(base[..., None] + rs.randint(-40, 40, (1, 1, 3)), 0, 255).astype(np.uint8)
        name = f'{i:012d}.jpg'
        Image.fromarray(img).save(os.path.join(root, 'imgs', name), quality=90)
        images.append(dict(id=i + 1, file_name=name, width=w, height=h))
        for _ in range(rs.randint(1, 7)):
            bw, bh = rs.uniform(16, w / 2), rs.uniform(16, h / 2)
            x, y = rs.uniform(0, w - bw), rs.uniform(0, h - bh)
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(rs.randint(1, 81)),
                             bbox=[x, y, bw, bh], area=bw * bh, iscrowd=0))
    path = os.path.join(root, 'ann.json')
    with open(path, 'w') as f:
        json.dump(dict(images=images, annotations=anns,
                       categories=[dict(id=i + 1, name=c) for i, c in enumerate(COCO_CLASSES)]), f)
    return path


def build_model(name):
    import torch
    from golden_util import load_seeded_
    from htd_amd.configs import build_htd_detector, htd_config
    depth = 50 if name == 'r50' else 101
    cfg = htd_config(depth, soft_nms=(name == 'r101'))
    return cfg, load_seeded_(build_htd_detector(cfg=cfg), 'det.').to(torch.device('cuda:0')).eval()


def run(cfg, model, root, ann, spg, workers):
    import torch
    from htd_amd.datasets import build_dataloader, build_dataset, replace_ImageToTensor
    from htd_amd.pipelines import collate
    dcfg = cfg.data.test.to_dict()
    if spg > 1:
        dcfg['pipeline'] = replace_ImageToTensor(dcfg['pipeline'])
    dcfg.update(ann_file=ann, img_prefix=os.path.join(root, 'imgs'), test_mode=True)
    ds = build_dataset(dcfg)
    results, wait, infer = [], 0.0, 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it = iter(build_dataloader(ds, spg, workers, dist=False, shuffle=False))
    start = time.perf_counter() - t0
    while True:
        a = time.perf_counter()
        try:
            batch = next(it)
        except StopIteration:               # (the workers are shut down here)
            wait += time.perf_counter() - a
            break
        b = time.perf_counter()
        with torch.no_grad():
            results.extend(model(return_loss=False, rescale=True, **collate(batch, 'cuda:0')))
        c = time.perf_counter()             # the results are host arrays: the device work of the batch is done
        wait += b - a
        infer += c - b
    loop = time.perf_counter() - t0
    a = time.perf_counter()
    metrics = ds.evaluate(results)
    ev = time.perf_counter() - a
    ndet = sum(x.shape[0] for r in results for x in r)
    return dict(images=len(ds), samples_per_gpu=spg, workers_per_gpu=workers, img_per_s=round(len(ds) / loop, 2),
                loop_s=round(loop, 3), loader_start_s=round(start, 3), loader_wait_s=round(wait, 3), model_s=round(infer, 3),
                evaluate_s=round(ev, 3), dets_per_img=round(ndet / len(ds), 1), bbox_mAP=metrics.get('bbox_mAP'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=500)
    ap.add_argument('--spg', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--workers', type=int, nargs='+', default=[0, 4])
    ap.add_argument('--models', nargs='+', default=['r50', 'r101', 'r101_hard'])
    args = ap.parse_args()
    assert max(args.workers) <= 4
    import torch
    assert torch.cuda.is_available(), 'bench_test_loop needs the GPU'
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    with tempfile.TemporaryDirectory() as root:
        t = time.perf_counter()
        ann = write_set(root, args.images)
        print(json.dumps(dict(wrote_images=args.images, seconds=round(time.perf_counter() - t, 2))), flush=True)
        warm = write_set(os.path.join(root, 'warm'), 16, seed=1)
        for name in args.models:
            cfg, model = build_model(name)
            run(cfg, model, os.path.join(root, 'warm'), warm, max(args.spg), 0)
            for spg in args.spg:
                for workers in args.workers:
                    out = run(cfg, model, root, ann, spg, workers)
                    print(json.dumps(dict(model=name, **out)), flush=True)
            del model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
