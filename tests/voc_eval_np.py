"""numpy restatement of mmdet's Pascal VOC mean AP (core/evaluation/mean_ap.py: tpfp_default, eval_map,
average_precision), the checker of htd_amd.core.evaluation.eval_map.  It keeps the reference's arithmetic and dtypes
under numpy 2 (float32 IoUs, areas and precisions, float64 recalls; NEP 50 casts Python thresholds to float32) and
runs serially; every argsort is stable, so score ties keep (image, row) order.  Also the synthetic VOC07-shaped sets
the tests and tools/bench_voc_eval.py use."""
import numpy as np


def iou_f32(det, gt):
    """bbox_overlaps (mode 'iou', eps 1e-6) of det [m, 4] against gt [n, 4], float32 -> [m, n]."""
    det, gt = det.astype(np.float32), gt.astype(np.float32)
    if det.shape[0] == 0 or gt.shape[0] == 0:
        return np.zeros((det.shape[0], gt.shape[0]), np.float32)
    a_d = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    a_g = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    w = np.maximum(np.minimum(det[:, None, 2], gt[None, :, 2]) - np.maximum(det[:, None, 0], gt[None, :, 0]), 0)
    h = np.maximum(np.minimum(det[:, None, 3], gt[None, :, 3]) - np.maximum(det[:, None, 1], gt[None, :, 1]), 0)
    inter = w * h
    union = np.maximum(a_d[:, None] + a_g[None, :] - inter, 1e-6)
    return inter / union


def area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def tp_fp(dets, gts, gts_ignore, iou_thr, area_ranges):
    """-> (tp, fp) float32 [num_scales, m] of one image and class."""
    ranges = area_ranges if area_ranges is not None else [(None, None)]
    m = dets.shape[0]
    tp = np.zeros((len(ranges), m), np.float32)
    fp = np.zeros((len(ranges), m), np.float32)
    allg = np.vstack((gts, gts_ignore))
    ignored = np.arange(allg.shape[0]) >= gts.shape[0]
    d_area = area(dets)
    if allg.shape[0] == 0:
        for k, (lo, hi) in enumerate(ranges):
            fp[k] = 1 if lo is None else ((d_area >= lo) & (d_area < hi))
        return tp, fp
    ious = iou_f32(dets, allg)
    best, arg = ious.max(axis=1), ious.argmax(axis=1)
    g_area = area(allg)
    rank = np.argsort(-dets[:, -1], kind='stable')
    for k, (lo, hi) in enumerate(ranges):
        out_of_range = np.zeros(allg.shape[0], bool) if lo is None else (g_area < lo) | (g_area >= hi)
        taken = np.zeros(allg.shape[0], bool)
        for i in rank:
            if best[i] >= iou_thr:
                g = arg[i]
                if ignored[g] or out_of_range[g]:
                    continue
                if taken[g]:
                    fp[k, i] = 1
                else:
                    taken[g] = True
                    tp[k, i] = 1
            elif lo is None or (d_area[i] >= lo and d_area[i] < hi):
                fp[k, i] = 1
    return tp, fp


def average_precision(rec, prec, mode):
    """rec / prec [num_scales, n] -> float32 [num_scales], the reference's division by 11 per loop iteration kept."""
    S = rec.shape[0]
    ap = np.zeros(S, np.float32)
    if mode == 'area':
        mrec = np.hstack((np.zeros((S, 1)), rec, np.ones((S, 1))))
        mpre = np.hstack((np.zeros((S, 1)), prec, np.zeros((S, 1))))
        mpre = np.maximum.accumulate(mpre[:, ::-1], axis=1)[:, ::-1]
        for s in range(S):
            j = np.flatnonzero(mrec[s, 1:] != mrec[s, :-1])
            ap[s] = np.sum((mrec[s, j + 1] - mrec[s, j]) * mpre[s, j + 1])
        return ap
    for s in range(S):
        for t in np.arange(0, 1 + 1e-3, 0.1):
            sel = prec[s, rec[s] >= t]
            ap[s] += sel.max() if sel.size else 0
        ap /= 11                     # the whole array, inside the loop: scale s ends up divided S - s times
    return ap


def eval_map_np(det_results, annotations, scale_ranges=None, iou_thr=0.5, dataset=None):
    """-> (mean_ap, per-class dicts) as mean_ap.py:eval_map returns them."""
    K = len(det_results[0])
    S = 1 if scale_ranges is None else len(scale_ranges)
    ranges = None if scale_ranges is None else [(a ** 2, b ** 2) for a, b in scale_ranges]
    mode = '11points' if isinstance(dataset, str) and dataset == 'voc07' else 'area'
    out = []
    for c in range(K):
        dets = [np.asarray(r[c], np.float32).reshape(-1, 5) for r in det_results]
        gts, ign = [], []
        for a in annotations:
            gts.append(a['bboxes'][a['labels'] == c])
            if a.get('labels_ignore', None) is not None:
                ign.append(a['bboxes_ignore'][a['labels_ignore'] == c])
            else:
                ign.append(np.empty((0, 4), np.float32))
        pairs = [tp_fp(d, g, gi, iou_thr, ranges) for d, g, gi in zip(dets, gts, ign)]
        n_gt = np.zeros(S, dtype=int)
        for g in gts:
            if ranges is None:
                n_gt[0] += g.shape[0]
            else:
                ga = area(g)
                for k, (lo, hi) in enumerate(ranges):
                    n_gt[k] += np.sum((ga >= lo) & (ga < hi))
        alld = np.vstack(dets)
        order = np.argsort(-alld[:, -1], kind='stable')
        tp = np.cumsum(np.hstack([p[0] for p in pairs])[:, order], axis=1)
        fp = np.cumsum(np.hstack([p[1] for p in pairs])[:, order], axis=1)
        eps = np.finfo(np.float32).eps
        rec = tp / np.maximum(n_gt[:, None], eps)
        prec = tp / np.maximum(tp + fp, eps)
        if scale_ranges is None:
            rec, prec, n_gt = rec[0, :], prec[0, :], n_gt.item()
            ap = average_precision(rec[None], prec[None], mode)[0]
        else:
            ap = average_precision(rec, prec, mode)
        out.append(dict(num_gts=n_gt, num_dets=alld.shape[0], recall=rec, precision=prec, ap=ap))
    if scale_ranges is not None:
        all_ap = np.vstack([x['ap'] for x in out])
        all_n = np.vstack([x['num_gts'] for x in out])
        mean_ap = [all_ap[all_n[:, s] > 0, s].mean() if np.any(all_n[:, s] > 0) else 0.0 for s in range(S)]
    else:
        aps = [x['ap'] for x in out if x['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    return mean_ap, out


# ------------------------------------------------------------------------------------------------ synthetic sets
def synthetic_voc(n_img, n_cls=20, dets_per_img=100, seed=0, ties=False, ignore_frac=0.1, empty_every=0):
    """(det_results, annotations): ground truths of a few classes per image (some ignored), detections jittered from
    them or random clutter.  ties=False: all scores distinct; ties=True: scores on a coarse grid, so many tie."""
    rs = np.random.RandomState(seed)
    dets_all, anns = [], []
    n_total = n_img * dets_per_img
    pool = (rs.permutation(n_total) + 1).astype(np.float64) / (n_total + 1) if not ties else None
    used = 0
    for i in range(n_img):
        g = 0 if empty_every and i % empty_every == empty_every - 1 else rs.randint(1, 8)
        xy = rs.uniform(0, 400, (g, 2))
        wh = rs.uniform(8, 200, (g, 2))
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        labels = rs.randint(0, n_cls, g).astype(np.int64)
        ign = rs.rand(g) < ignore_frac
        anns.append(dict(bboxes=boxes[~ign], labels=labels[~ign], bboxes_ignore=boxes[ign],
                         labels_ignore=labels[ign]))
        n = rs.randint(dets_per_img // 2, dets_per_img + 1)
        src = rs.randint(0, max(g, 1), n)
        clutter = (rs.rand(n) < 0.5) | (g == 0)
        xy = rs.uniform(0, 400, (n, 2))
        rnd = np.concatenate([xy, xy + rs.uniform(8, 200, (n, 2))], 1)
        near = boxes[src] + rs.normal(0, 8, (n, 4)) if g else rnd
        b = np.where(clutter[:, None], rnd, near).astype(np.float32)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        lab = np.where(clutter | (rs.rand(n) < 0.1), rs.randint(0, n_cls, n), labels[src] if g else 0)
        if ties:
            score = (rs.randint(1, 20, n) / 20.0).astype(np.float32)
        else:
            score = pool[used:used + n].astype(np.float32)
            used += n
        d = np.concatenate([b, score[:, None]], 1).astype(np.float32)
        dets_all.append([d[lab == c] for c in range(n_cls)])
    return dets_all, anns


def drop_class(det_results, annotations, no_dets=(), no_gts=()):
    """Remove every detection of the classes in no_dets and every ground truth of those in no_gts."""
    dets = [[np.zeros((0, 5), np.float32) if c in no_dets else a for c, a in enumerate(r)] for r in det_results]
    anns = []
    for a in annotations:
        k, ki = ~np.isin(a['labels'], no_gts), ~np.isin(a['labels_ignore'], no_gts)
        anns.append(dict(bboxes=a['bboxes'][k], labels=a['labels'][k], bboxes_ignore=a['bboxes_ignore'][ki],
                         labels_ignore=a['labels_ignore'][ki]))
    return dets, anns


def pack_inputs(det_results, annotations, prefix=''):
    """Flat arrays of a case (an npz cannot hold ragged lists)."""
    K = len(det_results[0])
    cnt = np.array([[len(a) for a in r] for r in det_results], np.int64)
    dets = np.concatenate([a.reshape(-1, 5) for r in det_results for a in r]).astype(np.float32)
    out = {'dets': dets, 'det_cnt': cnt, 'num_classes': np.array(K)}
    for key in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
        out[key] = np.concatenate([a[key] for a in annotations])
        out[key + '_cnt'] = np.array([len(a[key]) for a in annotations], np.int64)
    return {prefix + k: v for k, v in out.items()}


def unpack_inputs(z, prefix=''):
    cnt = z[prefix + 'det_cnt']
    parts = np.split(z[prefix + 'dets'], np.cumsum(cnt.reshape(-1))[:-1])
    K = cnt.shape[1]
    det_results = [parts[i * K:(i + 1) * K] for i in range(cnt.shape[0])]
    anns = [dict() for _ in range(cnt.shape[0])]
    for key in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
        for a, v in zip(anns, np.split(z[prefix + key], np.cumsum(z[prefix + key + '_cnt'])[:-1])):
            a[key] = v
    return det_results, anns


def pack_result(mean_ap, results, prefix=''):
    """mean_ap and the per-class dicts as flat arrays: recall / precision concatenated along the detections."""
    out = dict(mean_ap=np.asarray(mean_ap), mean_ap_is_list=np.array(isinstance(mean_ap, list)),
               num_gts=np.array([r['num_gts'] for r in results]), num_dets=np.array([r['num_dets'] for r in results]),
               ap=np.array([r['ap'] for r in results]),
               recall=np.concatenate([np.atleast_2d(r['recall']) for r in results], axis=-1),
               precision=np.concatenate([np.atleast_2d(r['precision']) for r in results], axis=-1))
    return {prefix + k: v for k, v in out.items()}


def assert_same_result(got, want):
    """Bit-for-bit equality of two eval_map returns, types and dtypes included."""
    (m1, r1), (m2, r2) = got, want
    assert type(m1) is type(m2), (type(m1), type(m2))
    if isinstance(m1, list):
        assert [type(x) for x in m1] == [type(x) for x in m2]
        assert np.array_equal(np.array(m1), np.array(m2)), (m1, m2)
    else:
        assert m1 == m2, (m1, m2)
    assert len(r1) == len(r2)
    for c, (a, b) in enumerate(zip(r1, r2)):
        assert a['num_dets'] == b['num_dets'], c
        assert type(a['num_gts']) is type(b['num_gts']) and np.array_equal(a['num_gts'], b['num_gts']), c
        for k in ('recall', 'precision', 'ap'):
            x, y = a[k], b[k]
            assert type(x) is type(y) and x.dtype == y.dtype and x.shape == y.shape, (c, k, x.dtype, y.dtype)
            assert np.array_equal(x, y), (c, k, np.argwhere(x != y)[:5] if np.ndim(x) else (x, y))


def assert_matches_packed(got, z, prefix=''):
    """An eval_map return against pack_result arrays (values and dtypes)."""
    mean_ap, results = got
    p = pack_result(mean_ap, results)
    for k, v in p.items():
        w = z[prefix + k]
        assert v.dtype == w.dtype and v.shape == w.shape, (k, v.dtype, w.dtype, v.shape, w.shape)
        assert np.array_equal(v, w), (k, np.argwhere(v != w)[:5] if v.ndim else (v, w))
