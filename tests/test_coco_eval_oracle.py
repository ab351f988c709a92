"""CPU checks of the COCO evaluation restatement (tests/coco_eval_np.py) against hand-worked answers, the reference's
own known answer (tests/test_data/test_dataset.py:22-120) and the reference's eval_recalls (eval_recalls.npz)."""
import json
import os

import numpy as np
import pytest

from coco_eval_np import coco_eval_np, eval_recalls_np, unpack_recall_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def gts(rows):
    """rows: (image_id, category_id, x, y, w, h, area or None, iscrowd, id)."""
    r = list(rows)
    return dict(image_id=np.array([x[0] for x in r], np.int64), category_id=np.array([x[1] for x in r], np.int64),
                bbox=np.array([x[2:6] for x in r], np.float64).reshape(-1, 4),
                area=np.array([x[4] * x[5] if x[6] is None else x[6] for x in r], np.float64),
                iscrowd=np.array([x[7] for x in r], np.int64), id=np.array([x[8] for x in r], np.int64))


def dts(rows):
    """rows: (image_id, category_id, x, y, w, h, score)."""
    r = list(rows)
    return dict(image_id=np.array([x[0] for x in r], np.int64), category_id=np.array([x[1] for x in r], np.int64),
                bbox=np.array([x[2:6] for x in r], np.float64).reshape(-1, 4),
                score=np.array([x[6] for x in r], np.float64))


def near(a, v):
    """Equal up to pycocotools' eps: a lone true positive has precision 1 / (1 + np.spacing(1))."""
    return bool(np.all(np.abs(np.asarray(a) - v) <= 4 * np.spacing(1)))


def hand_cases():
    """name -> (gt, dt, img_ids, cat_ids); shared with the device test."""
    return {
        # a false positive above the only true positive: precision 1/2 at every recall threshold
        'fp_above_tp': (gts([(1, 1, 10, 10, 20, 20, None, 0, 1)]),
                        dts([(1, 1, 200, 200, 20, 20, .9), (1, 1, 10, 10, 20, 20, .8)]), [1], [1]),
        # three detections inside one crowd region are absorbed by it (ignored), the fourth matches the person
        'crowd': (gts([(1, 1, 0, 0, 100, 100, None, 1, 1), (1, 1, 300, 300, 40, 40, None, 0, 2)]),
                  dts([(1, 1, 10, 10, 30, 30, .99), (1, 1, 40, 40, 30, 30, .98), (1, 1, 5, 60, 20, 20, .97),
                       (1, 1, 300, 300, 40, 40, .5)]), [1], [1]),
        # annotation areas exactly 32^2 and 96^2 belong to both neighbouring ranges; unmatched detections of area
        # exactly 32^2 are not ignored in 'small' or 'medium'
        'area_ties': (gts([(1, 1, 0, 0, 30, 30, 32.0 ** 2, 0, 1), (1, 1, 100, 100, 100, 100, 96.0 ** 2, 0, 2)]),
                      dts([(1, 1, 0, 0, 30, 30, .9), (1, 1, 100, 100, 100, 100, .8), (1, 1, 400, 400, 32, 32, .7)]),
                      [1], [1]),
        # equal scores across images go in ascending image id order (the file lists image 7 first)
        'score_ties': (gts([(7, 1, 0, 0, 50, 50, None, 0, 1), (3, 1, 0, 0, 50, 50, None, 0, 2)]),
                       dts([(7, 1, 300, 300, 50, 50, .5), (3, 1, 0, 0, 50, 50, .5)]), [7, 3], [1]),
        # category 2 has detections and no ground truth: -1, left out of the mean
        'no_gt_category': (gts([(1, 1, 0, 0, 50, 50, None, 0, 1)]),
                           dts([(1, 1, 0, 0, 50, 50, .6), (1, 2, 0, 0, 50, 50, .9)]), [1], [1, 2]),
        # image 2 has detections and no ground truth: false positives
        'no_gt_image': (gts([(1, 1, 0, 0, 50, 50, None, 0, 1)]),
                        dts([(1, 1, 0, 0, 50, 50, .5), (2, 1, 0, 0, 50, 50, .9)]), [1, 2], [1]),
    }


def known_answer():
    """The reference's test_dataset_evaluation data: (annotation dict, bbox2result list)."""
    with open(os.path.join(GOLDEN, 'coco_known_answer.json')) as f:
        ann = json.load(f)
    with open(os.path.join(GOLDEN, 'coco_known_answer_results.json')) as f:
        res = [[np.array(b, np.float64) for b in r] for r in json.load(f)]
    return ann, res


def known_answer_arrays():
    from htd_amd.coco import CocoEvaluator
    ann, res = known_answer()
    ev = CocoEvaluator(ann, classes=('car',))
    return ev.gt, {k: v.numpy() for k, v in ev._det_arrays(res).items()}, ev.img_ids, ev.cat_ids


def test_fp_above_tp():
    out = coco_eval_np(*hand_cases()['fp_above_tp'])
    assert np.all(out['precision'][:, :, 0, 0, :] == 0.5)
    assert np.all(out['recall'][:, 0, 0, :] == 1.0)
    assert out['stats'][1] == 0.5 and out['stats'][0] == 0.5


def test_crowd_absorbs_detections():
    out = coco_eval_np(*hand_cases()['crowd'])
    assert near(out['precision'][:, :, 0, 0, :], 1.0)
    assert near(out['stats'][0], 1.0)
    # the ignored crowd detections hold recall 0; every later point is the true positive's
    assert np.all(out['scores'][:, 0, 0, 0, :] == 0.99) and np.all(out['scores'][:, 1:, 0, 0, :] == 0.5)


def test_area_range_boundaries():
    out = coco_eval_np(*hand_cases()['area_ties'])
    p = out['precision'][0, :, 0, :, -1]                  # IoU .5, every area range, maxDets 1000
    # all: 2 TP then 1 FP; small: gt 1024 (and the unmatched 32x32 detection, area 1024, counts as FP);
    # medium: both ground truths; large: the 96^2 one only (small-range detections ignored there)
    assert near(p[:, 0], 1.0) and near(p[:, 2], 1.0) and near(p[:, 3], 1.0)
    assert near(p[:, 1], 1.0)
    assert np.all(out['recall'][0, 0, :, -1] == 1.0)
    assert near(out['stats'][3:6], 1.0)


def test_equal_scores_follow_image_id():
    out = coco_eval_np(*hand_cases()['score_ties'])
    q = out['precision'][0, :, 0, 0, -1]
    assert near(q[:51], 1.0) and np.all(q[51:] == 0.0)      # image 3's true positive comes first


def test_category_without_ground_truth():
    out = coco_eval_np(*hand_cases()['no_gt_category'])
    assert np.all(out['precision'][:, :, 1] == -1) and np.all(out['recall'][:, 1] == -1)
    assert np.all(out['scores'][:, :, 1] == -1)
    assert near(out['stats'][0], 1.0)


def test_image_without_ground_truth():
    out = coco_eval_np(*hand_cases()['no_gt_image'])
    assert np.all(out['precision'][:, :, 0, 0, :] == 0.5)
    assert out['stats'][0] == 0.5


def test_reference_known_answer():
    """tests/test_data/test_dataset.py: bbox_mAP = mAP_50 = mAP_75 = 1; the boxes cover every area range, so all
    six AP values are 1."""
    out = coco_eval_np(*known_answer_arrays())
    assert [float(f'{x:.3f}') for x in out['stats'][:6]] == [1.0] * 6      # CocoDataset.evaluate's rounding
    assert near(out['stats'][:6], 1.0) and np.all(out['stats'][6:] == 1.0)


def test_eval_recalls_matches_reference():
    z = np.load(os.path.join(GOLDEN, 'eval_recalls.npz'))
    gts_, props = unpack_recall_case(z)
    assert np.array_equal(eval_recalls_np(gts_, props, z['proposal_nums'], z['iou_thrs']), z['recalls'])
    assert np.array_equal(eval_recalls_np(gts_, props, [1000], [0.5]), z['recalls_default'])


def test_evaluator_refuses_segm():
    from htd_amd.coco import CocoEvaluator
    ann, res = known_answer()
    with pytest.raises(KeyError, match='segm'):
        CocoEvaluator(ann, classes=('car',)).evaluate(res, metric='segm')


def test_results2json(tmp_path):
    from htd_amd.coco import CocoEvaluator
    ann, res = known_answer()
    files = CocoEvaluator(ann, classes=('car',)).results2json(res, str(tmp_path / 'r'))
    with open(files['bbox']) as f:
        rows = json.load(f)
    assert files['proposal'] == files['bbox']
    assert rows[1] == dict(image_id=0, bbox=[100.0, 120.0, 30.0, 30.0], score=0.98, category_id=0)
    assert len(rows) == 4
