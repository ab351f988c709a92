"""COCO evaluation on the device (csrc/coco_eval.hip through htd_amd.core.evaluation / htd_amd.coco) against the numpy
restatement of COCOeval (tests/coco_eval_np.py), bit for bit, and eval_recalls against the reference's own output
(tests/golden/eval_recalls.npz)."""
import os

import numpy as np
import pytest
import torch

from coco_eval_np import coco_eval_np, synthetic_coco, unpack_recall_case
from test_coco_eval_oracle import hand_cases, known_answer, known_answer_arrays

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _same(dev, ref):
    for k in ('precision', 'recall', 'scores'):
        assert dev[k].shape == ref[k].shape, k
        assert np.array_equal(dev[k], ref[k]), (k, np.argwhere(dev[k] != ref[k])[:5])
    assert np.array_equal(dev['stats'], ref['stats']), (dev['stats'], ref['stats'])


def _synthetic(**kw):
    from htd_amd.coco import CocoEvaluator
    ann, res = synthetic_coco(**kw)
    ev = CocoEvaluator(ann, classes=[c['name'] for c in ann['categories']])
    return ev, res


@pytest.mark.parametrize('case', sorted(hand_cases()))
def test_hand_cases(case):
    from htd_amd.core.evaluation import coco_eval
    args = hand_cases()[case]
    _same(coco_eval(*args), coco_eval_np(*args))


def test_reference_known_answer():
    from htd_amd.coco import CocoEvaluator
    from htd_amd.core.evaluation import coco_eval
    args = known_answer_arrays()
    _same(coco_eval(*args), coco_eval_np(*args))
    ann, res = known_answer()
    out = CocoEvaluator(ann, classes=('car',)).evaluate(res, classwise=True)
    assert [out[f'bbox_{k}'] for k in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')] == [1.0] * 6
    assert out['bbox_mAP_copypaste'] == '1.000 1.000 1.000 1.000 1.000 1.000'


@pytest.mark.parametrize('max_dets,iou_thrs', [((100, 300, 1000), None), ((1, 10, 100), None),
                                               ((100, 300, 1000), (0.3, 0.5, 0.55, 0.75, 0.9))])
def test_synthetic_bbox(max_dets, iou_thrs):
    from htd_amd.core.evaluation import coco_eval
    ev, res = _synthetic()
    dt = {k: v.numpy() for k, v in ev._det_arrays(res).items()}
    args = (ev.gt, dt, ev.img_ids, ev.cat_ids, iou_thrs)
    _same(coco_eval(*args, max_dets=max_dets), coco_eval_np(*args, max_dets=max_dets))


def test_synthetic_proposal_use_cats_0():
    """useCats = 0 (the 'proposal' metric) with 1000 detections per image: IoU rows computed on the fly."""
    from htd_amd.core.evaluation import coco_eval
    ev, res = _synthetic(n_img=6, n_cat=5, gt_per_img=10, det_per_img=1000, seed=3)
    dt = {k: v.numpy() for k, v in ev._det_arrays(res).items()}
    args = (ev.gt, dt, ev.img_ids, ev.cat_ids)
    _same(coco_eval(*args, use_cats=False), coco_eval_np(*args, use_cats=False))


@pytest.mark.parametrize('use_cats', [True, False])
def test_crowded_images(use_cats):
    """Over a hundred ground truths in a pair: the matched flags no longer fit in LDS and live in the workspace."""
    from htd_amd.core.evaluation import coco_eval
    ev, res = _synthetic(n_img=3, n_cat=2, gt_per_img=220, det_per_img=40, seed=4)
    dt = {k: v.numpy() for k, v in ev._det_arrays(res).items()}
    args = (ev.gt, dt, ev.img_ids, ev.cat_ids)
    _same(coco_eval(*args, use_cats=use_cats), coco_eval_np(*args, use_cats=use_cats))


def test_runs_are_identical():
    from htd_amd.core.evaluation import coco_eval
    ev, res = _synthetic(seed=5)
    dt = ev._det_arrays(res)
    a = coco_eval(ev.gt, dt, ev.img_ids, ev.cat_ids)
    b = coco_eval(ev.gt, dt, ev.img_ids, ev.cat_ids)
    for k in ('precision', 'recall', 'scores', 'stats'):
        assert np.array_equal(a[k], b[k])


def test_tensor_results_match_lists():
    ev, res = _synthetic(n_img=40, seed=9)
    dets = torch.cat([torch.from_numpy(b) for r in res for b in r]).cuda()
    labels = torch.cat([torch.full((len(b),), c) for r in res for c, b in enumerate(r)]).cuda()
    img = torch.cat([torch.full((len(b),), i) for i, r in enumerate(res) for b in r]).cuda()
    assert ev.evaluate((dets, labels, img)) == ev.evaluate(res)


def test_evaluator_end_to_end_on_simple_test(tmp_path):
    """CocoEvaluator.evaluate on simple_test output of the seeded small detector: the reference's keys, and the
    restatement's values."""
    import sys
    from golden_util import demo_inputs, load_seeded_
    from htd_amd.coco import COCO_CLASSES, CocoEvaluator
    from htd_amd.configs import build_htd_detector, htd_config
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    H, W, B = 96, 128, 2
    imgs, gts, labels = demo_inputs(B, H, W, np.random.RandomState(3))
    imgs = (imgs - 0.5) * 4
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), ori_shape=(H, W, 3),
                  scale_factor=np.array([1, 1, 1, 1], dtype=np.float32), flip=False) for _ in range(B)]
    det = load_seeded_(build_htd_detector(cfg=htd_config(50)), 'det.').cuda().eval()
    with torch.no_grad():
        res = det.simple_test(torch.from_numpy(imgs).cuda(), metas)
    cats = [dict(id=i + 1, name=n) for i, n in enumerate(COCO_CLASSES)]
    anns, aid = [], 1
    for b in range(B):
        for box, lab in zip(gts[b], labels[b]):
            w, h = float(box[2] - box[0]), float(box[3] - box[1])
            anns.append(dict(id=aid, image_id=b + 1, category_id=int(lab) + 1, bbox=[float(box[0]), float(box[1]), w, h],
                             area=w * h, iscrowd=0))
            aid += 1
    ann = dict(images=[dict(id=b + 1, width=W, height=H, file_name=f'{b}.jpg') for b in range(B)], annotations=anns,
               categories=cats)
    ev = CocoEvaluator(ann)
    out = ev.evaluate(res, metric='bbox', jsonfile_prefix=str(tmp_path / 'r'), classwise=True)
    # one metric per call: with a metric list the reference reuses the first metric's metric_items for the next
    out.update(ev.evaluate(res, metric='proposal'))
    assert list(out) == ['bbox_mAP', 'bbox_mAP_50', 'bbox_mAP_75', 'bbox_mAP_s', 'bbox_mAP_m', 'bbox_mAP_l',
                         'bbox_mAP_copypaste', 'AR@100', 'AR@300', 'AR@1000', 'AR_s@1000', 'AR_m@1000', 'AR_l@1000']
    assert os.path.exists(str(tmp_path / 'r.bbox.json'))
    dt = {k: v.numpy() for k, v in ev._det_arrays(res).items()}
    ref = coco_eval_np(ev.gt, dt, ev.img_ids, ev.cat_ids)['stats']
    ref_p = coco_eval_np(ev.gt, dt, ev.img_ids, ev.cat_ids, use_cats=False)['stats']
    names = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
    assert [out[f'bbox_{n}'] for n in names] == [float(f'{x:.3f}') for x in ref[:6]]
    assert [out[k] for k in ('AR@100', 'AR@300', 'AR@1000', 'AR_s@1000', 'AR_m@1000', 'AR_l@1000')] == \
        [float(f'{x:.3f}') for x in ref_p[6:]]


def test_eval_recalls_matches_reference():
    from htd_amd.core.evaluation import eval_recalls
    z = np.load(os.path.join(GOLDEN, 'eval_recalls.npz'))
    gts, props = unpack_recall_case(z)
    assert np.array_equal(eval_recalls(gts, props, list(z['proposal_nums']), list(z['iou_thrs']), logger='silent'),
                          z['recalls'])
    assert np.array_equal(eval_recalls(gts, props, 1000, None, logger='silent'), z['recalls_default'])


def test_proposal_fast():
    from coco_eval_np import eval_recalls_np
    from htd_amd.core.evaluation import default_iou_thrs
    ev, res = _synthetic(n_img=30, seed=11)
    props = [np.concatenate([b for b in r]) for r in res]
    out = ev.evaluate(props, metric='proposal_fast', proposal_nums=(10, 100, 300))
    gts = []
    for img_id in ev.img_ids:
        rows = [a['bbox'] for a in ev.anns if a['image_id'] == img_id and not a['iscrowd']]
        gts.append(np.array([[x, y, x + w, y + h] for x, y, w, h in rows], np.float32) if rows else np.zeros((0, 4)))
    ar = eval_recalls_np(gts, props, (10, 100, 300), default_iou_thrs()).mean(axis=1)
    assert [out[f'AR@{n}'] for n in (10, 100, 300)] == list(ar)

