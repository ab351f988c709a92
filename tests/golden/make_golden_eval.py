#!/usr/bin/env python
"""Generate tests/golden/eval_recalls.npz by running the REFERENCE's own core/evaluation/recall.py and
bbox_overlaps.py (loaded by file path, with make_golden's mmcv stand-in and a stub `terminaltables`) on seeded
proposals: ragged images, images without ground truth, (k, 4) and (k, 5) proposals, several proposal counts and
IoU thresholds.  Proposal scores are distinct, because the reference ranks them with numpy's unstable argsort.

    python tests/golden/make_golden_eval.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
from coco_eval_np import pack_recall_case  # noqa: E402

EVAL_DIR = os.path.join(make_golden.REF, 'mmdet', 'core', 'evaluation')
PROPOSAL_NUMS = (5, 20, 100, 300)
IOU_THRS = (0.3, 0.5, 0.6, 0.7, 0.75, 0.9)


class _RaggedNumpy(types.ModuleType):
    """numpy for the reference's recall.py: np.array of a ragged list of IoU matrices gives the object array that
    numpy of the reference's era made (numpy >= 1.24 refuses it without dtype=object)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *a, **k):
        if isinstance(obj, list) and obj and all(isinstance(x, np.ndarray) for x in obj) and not a and not k \
                and len({x.shape for x in obj}) > 1:
            out = np.empty(len(obj), dtype=object)
            for i, x in enumerate(obj):
                out[i] = x
            return out
        return np.array(obj, *a, **k)


def load_reference_recall():
    make_golden.install_mmcv_standin()
    tt = types.ModuleType('terminaltables')
    tt.AsciiTable = lambda data: types.SimpleNamespace(table='')
    sys.modules['terminaltables'] = tt
    pkg = types.ModuleType('ref_evaluation')
    pkg.__path__ = [EVAL_DIR]
    sys.modules['ref_evaluation'] = pkg
    mods = {}
    for name in ('bbox_overlaps', 'recall'):
        spec = importlib.util.spec_from_file_location('ref_evaluation.' + name, os.path.join(EVAL_DIR, name + '.py'))
        m = importlib.util.module_from_spec(spec)
        sys.modules['ref_evaluation.' + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    mods['recall'].np = _RaggedNumpy('numpy')
    return mods['recall']


def seeded_case(seed=7, n_img=12):
    rs = np.random.RandomState(seed)
    gts, props = [], []
    for i in range(n_img):
        g = 0 if i % 5 == 2 else rs.randint(1, 40)                # every fifth image: no ground truth
        xy = rs.uniform(0, 400, (g, 2))
        wh = rs.uniform(4, 150, (g, 2))
        gt = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        k = rs.randint(0, 500) if i % 7 != 3 else 0
        src = gt[rs.randint(0, g, k)] if g else np.zeros((k, 4), np.float32)
        jit = rs.normal(0, 6, (k, 4)).astype(np.float32)
        clutter = rs.rand(k) < 0.4
        xy = rs.uniform(0, 400, (k, 2))
        rnd = np.concatenate([xy, xy + rs.uniform(4, 150, (k, 2))], 1).astype(np.float32)
        p = np.where(clutter[:, None], rnd, src + jit).astype(np.float32)
        p[:, 2:] = np.maximum(p[:, 2:], p[:, :2] + 1)
        if i % 2 == 0:                                            # (k, 5): distinct scores, shuffled
            score = (rs.permutation(k).astype(np.float32) + 1) / (k + 1)
            p = np.concatenate([p, score[:, None]], 1).astype(np.float32)
        gts.append(gt if g else (None if i % 10 == 2 else np.zeros((0, 4))))
        props.append(p)
    return gts, props


def main():
    recall = load_reference_recall()
    gts, props = seeded_case()
    out = dict(pack_recall_case(gts, props), proposal_nums=np.array(PROPOSAL_NUMS), iou_thrs=np.array(IOU_THRS))
    out['recalls'] = recall.eval_recalls(gts, props, list(PROPOSAL_NUMS), list(IOU_THRS), logger='silent')
    out['recalls_default'] = recall.eval_recalls(gts, props, 1000, None, logger='silent')
    np.savez_compressed(os.path.join(HERE, 'eval_recalls.npz'), **out)
    print('eval_recalls.npz:', out['recalls'].round(4))


if __name__ == '__main__':
    main()
