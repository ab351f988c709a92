"""COCO bbox / proposal evaluation, Pascal VOC mean AP and proposal recall on the device.

coco_eval() is pycocotools' COCOeval.evaluate + accumulate + summarize as CocoDataset.evaluate drives them
(datasets/coco.py:363-545): the greedy matching and the accumulation run as HIP kernels (csrc/coco_eval.hip), the sort
and grouping of the detections is a few stable device sorts here, and the 12 summary numbers are taken on the host
from the device arrays with pycocotools' own slices.  eval_recalls() is core/evaluation/recall.py:eval_recalls with
the IoU and the greedy assignment on the device.  pycocotools is not needed.  eval_map() is
core/evaluation/mean_ap.py:eval_map in process (no worker pool): TP/FP and the precision / recall accumulation run as
HIP kernels (csrc/voc_eval.hip), and the host sums each class's 'area' terms in numpy's order.
"""
from collections.abc import Sequence

import numpy as np
import torch

from .. import capi

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def default_iou_thrs():
    """CocoDataset.evaluate's (coco.py:402-403) and COCOeval's IoU thresholds."""
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def default_rec_thrs():
    """COCOeval Params.recThrs."""
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def _device(device):
    dev = torch.device(device if device is not None else 'cuda')
    if dev.type != 'cuda':
        raise ValueError(f'the COCO evaluation kernels run on the GPU, got device {dev}')
    return dev


def _t(x, dtype, dev):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(dev).contiguous()


def _lookup(values, table, dev):
    """(position of each value in the host array `table`, found mask)."""
    table = np.asarray(table, np.int64)
    if table.size == 0:
        return torch.zeros_like(values), torch.zeros_like(values, dtype=torch.bool)
    order = np.argsort(table, kind='stable')
    srt = torch.from_numpy(table[order]).to(dev)
    pos = torch.searchsorted(srt, values).clamp_(max=len(table) - 1)
    return torch.from_numpy(order).to(dev)[pos], srt[pos] == values


def _offsets(sorted_keys, n, dev):
    """[n+1] int64: where each key 0..n starts in `sorted_keys`."""
    return torch.searchsorted(sorted_keys, torch.arange(n + 1, device=dev, dtype=sorted_keys.dtype)).contiguous()


def coco_eval(gt, dt, img_ids, cat_ids, iou_thrs=None, rec_thrs=None, max_dets=(100, 300, 1000), use_cats=True,
              device=None):
    """COCOeval (iouType 'bbox') on the device.

    gt: dict of arrays or tensors in annotation-file order: image_id, category_id [n], bbox [n,4] xywh, area [n]
        (the annotation's 'area'), iscrowd [n], id [n].
    dt: dict in result-file order: image_id, category_id [n], bbox [n,4] xywh float64, score [n] float64.
    img_ids / cat_ids: Params.imgIds / catIds (sorted and made unique as COCOeval.evaluate does; with use_cats=False
    the pooling follows cat_ids as given).  max_dets: Params.maxDets (sorted).
    Returns dict(precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M] float64 numpy, stats [12], and the
    parameters used).
    """
    dev = _device(device)
    iou_thrs = np.asarray(default_iou_thrs() if iou_thrs is None else iou_thrs, dtype=np.float64).reshape(-1)
    rec_thrs = np.asarray(default_rec_thrs() if rec_thrs is None else rec_thrs, dtype=np.float64).reshape(-1)
    max_dets = sorted(int(m) for m in max_dets)
    imgs = np.unique(np.asarray(img_ids, np.int64))
    cats = np.unique(np.asarray(cat_ids, np.int64)) if use_cats else np.asarray(cat_ids, np.int64).reshape(-1)
    if not use_cats and len(np.unique(cats)) != len(cats):
        raise ValueError('coco_eval: cat_ids must be unique')
    I, Kc = len(imgs), len(cats)
    K = Kc if use_cats else 1
    A, T, R, M = len(AREA_RNG), len(iou_thrs), len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    params = dict(iou_thrs=iou_thrs, rec_thrs=rec_thrs, max_dets=max_dets, img_ids=imgs, cat_ids=cats,
                  use_cats=use_cats, area_rng=AREA_RNG)
    if K == 0 or I == 0:
        return dict(precision=precision, recall=recall, scores=scores, params=params,
                    stats=summarize(precision, recall, iou_thrs, max_dets))
    P_, S_ = capi.ptr, capi.current_stream_ptr
    with torch.cuda.device(dev):
        # ---- ground truths: grouped by pair, COCOeval's order inside (file order, pooled in cat_ids order)
        g_img, ok_i = _lookup(_t(gt['image_id'], torch.int64, dev), imgs, dev)
        g_cat, ok_c = _lookup(_t(gt['category_id'], torch.int64, dev), cats, dev)
        keep = (ok_i & ok_c).nonzero().squeeze(1)
        g_img, g_cat = g_img[keep], g_cat[keep]
        g_pair = g_cat * I + g_img if use_cats else g_img
        go = keep[torch.argsort(g_pair * Kc + g_cat, stable=True)]
        g_pair = torch.sort(g_pair).values
        gt_box = _t(gt['bbox'], torch.float64, dev).reshape(-1, 4)[go].contiguous()
        gt_area = _t(gt['area'], torch.float64, dev)[go].contiguous()
        gt_crowd = (_t(gt['iscrowd'], torch.int64, dev)[go] != 0).to(torch.uint8).contiguous()
        gt_id = _t(gt['id'], torch.int64, dev)[go].contiguous()

        # ---- detections: by pair, score descending (stable), cut to maxDets[-1] per pair
        score_all = _t(dt['score'], torch.float64, dev)
        d_img, ok_i = _lookup(_t(dt['image_id'], torch.int64, dev), imgs, dev)
        d_cat, ok_c = _lookup(_t(dt['category_id'], torch.int64, dev), cats, dev)
        keep = (ok_i & ok_c).nonzero().squeeze(1)
        d_img, d_cat = d_img[keep], d_cat[keep]
        d_pair = d_cat * I + d_img if use_cats else d_img
        o = torch.argsort(d_pair * Kc + d_cat, stable=True)
        o = o[torch.argsort(-score_all[keep[o]], stable=True)]
        o = o[torch.argsort(d_pair[o], stable=True)]
        d_pair = d_pair[o]
        rank = torch.arange(len(o), device=dev) - torch.searchsorted(d_pair, d_pair)
        cut = (rank < max_dets[-1]).nonzero().squeeze(1)
        do = keep[o[cut]]
        d_pair, rank = d_pair[cut].contiguous(), rank[cut].to(torch.int32).contiguous()
        dt_box = _t(dt['bbox'], torch.float64, dev).reshape(-1, 4)[do].contiguous()
        dt_score = score_all[do].contiguous()

        pairs = torch.unique(torch.cat([g_pair, d_pair]))
        P = len(pairs)
        n_gt, n_dt = len(g_pair), len(d_pair)
        pair_gt = torch.searchsorted(g_pair, pairs)
        pair_gt = torch.cat([pair_gt, pair_gt.new_tensor([n_gt])]).contiguous()
        pair_dt = torch.searchsorted(d_pair, pairs)
        pair_dt = torch.cat([pair_dt, pair_dt.new_tensor([n_dt])]).contiguous()
        area_rng = torch.tensor(AREA_RNG, dtype=torch.float64, device=dev).contiguous()
        thr_t = torch.from_numpy(iou_thrs).to(dev)
        dt_flags = torch.empty((n_dt, A, T), dtype=torch.uint8, device=dev)
        npig = torch.empty((max(P, 1), A), dtype=torch.int32, device=dev)
        ws = torch.empty(capi.lib().htd_coco_match_workspace_bytes(n_gt, A, T), dtype=torch.uint8, device=dev)
        capi.call('htd_coco_match', P_(gt_box), P_(gt_area), P_(gt_crowd), P_(gt_id), P_(dt_box), P_(pair_gt),
                  P_(pair_dt), P, P_(area_rng), A, P_(thr_t), T, P_(dt_flags), P_(npig), P_(ws), S_())

        # ---- accumulate: each category's detections by score, then image, then rank within the image
        p_cat = pairs // I if use_cats else torch.zeros_like(pairs)
        d_cat = d_pair // I if use_cats else torch.zeros_like(d_pair)
        order = torch.argsort(-dt_score, stable=True)
        order = order[torch.argsort(d_cat[order], stable=True)].contiguous()
        cat_dt = _offsets(d_cat[order], K, dev)
        cat_pair = _offsets(p_cat, K, dev)
        md = torch.tensor(max_dets, dtype=torch.int32, device=dev)
        rec_t = torch.from_numpy(rec_thrs).to(dev)
        prec_d = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        rec_d = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        sc_d = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        ws = torch.empty(capi.lib().htd_coco_accumulate_workspace_bytes(n_dt, A, M), dtype=torch.uint8, device=dev)
        capi.call('htd_coco_accumulate', P_(dt_flags), P_(order), P_(rank), P_(dt_score), P_(cat_dt), P_(cat_pair),
                  P_(npig), K, A, P_(md), M, T, P_(rec_t), R, P_(prec_d), P_(rec_d), P_(sc_d), P_(ws), S_())
        precision, recall, scores = prec_d.cpu().numpy(), rec_d.cpu().numpy(), sc_d.cpu().numpy()
    return dict(precision=precision, recall=recall, scores=scores, params=params,
                stats=summarize(precision, recall, iou_thrs, max_dets))


def summarize(precision, recall, iou_thrs, max_dets):
    """COCOeval.summarize (_summarizeDets) on the host: the same slices and mean(s[s > -1]), unrounded."""
    iou_thrs = np.asarray(iou_thrs)
    max_dets = list(max_dets)

    def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
        aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
        mind = [i for i, mDet in enumerate(max_dets) if mDet == maxDets]
        if ap == 1:
            s = precision
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=max_dets[2])
    stats[2] = _summarize(1, iouThr=.75, maxDets=max_dets[2])
    stats[3] = _summarize(1, areaRng='small', maxDets=max_dets[2])
    stats[4] = _summarize(1, areaRng='medium', maxDets=max_dets[2])
    stats[5] = _summarize(1, areaRng='large', maxDets=max_dets[2])
    stats[6] = _summarize(0, maxDets=max_dets[0])
    stats[7] = _summarize(0, maxDets=max_dets[1])
    stats[8] = _summarize(0, maxDets=max_dets[2])
    stats[9] = _summarize(0, areaRng='small', maxDets=max_dets[2])
    stats[10] = _summarize(0, areaRng='medium', maxDets=max_dets[2])
    stats[11] = _summarize(0, areaRng='large', maxDets=max_dets[2])
    return stats


# ------------------------------------------------------------------------------------------------ eval_recalls
def set_recall_param(proposal_nums, iou_thrs):
    """recall.py:set_recall_param."""
    if isinstance(proposal_nums, Sequence):
        _proposal_nums = np.array(proposal_nums)
    elif isinstance(proposal_nums, int):
        _proposal_nums = np.array([proposal_nums])
    else:
        _proposal_nums = proposal_nums
    if iou_thrs is None:
        _iou_thrs = np.array([0.5])
    elif isinstance(iou_thrs, Sequence):
        _iou_thrs = np.array(iou_thrs)
    elif isinstance(iou_thrs, float):
        _iou_thrs = np.array([iou_thrs])
    else:
        _iou_thrs = iou_thrs
    return _proposal_nums, _iou_thrs


def print_log(msg, logger=None):
    if logger is None:
        print(msg)
    elif logger == 'silent':
        return
    elif isinstance(logger, str):
        import logging
        logging.getLogger(logger).info(msg)
    else:
        logger.info(msg)


def print_recall_summary(recalls, proposal_nums, iou_thrs, row_idxs=None, col_idxs=None, logger=None):
    """recall.py:print_recall_summary, as a plain-text table."""
    proposal_nums = np.array(proposal_nums, dtype=np.int32)
    iou_thrs = np.array(iou_thrs)
    row_idxs = np.arange(proposal_nums.size) if row_idxs is None else row_idxs
    col_idxs = np.arange(iou_thrs.size) if col_idxs is None else col_idxs
    rows = [[''] + [str(x) for x in iou_thrs[col_idxs].tolist()]]
    for i, num in enumerate(proposal_nums[row_idxs]):
        rows.append([str(num)] + [f'{val:.3f}' for val in recalls[row_idxs[i], col_idxs].tolist()])
    print_log('\n' + format_table(rows), logger=logger)


def format_table(rows):
    widths = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    line = lambda r: ' | '.join(s.ljust(w) for s, w in zip(r, widths))
    return '\n'.join([line(rows[0]), '-+-'.join('-' * w for w in widths)] + [line(r) for r in rows[1:]])


def eval_recalls(gts, proposals, proposal_nums=None, iou_thrs=0.5, logger=None, device=None):
    """recall.py:eval_recalls on the device: recalls [len(proposal_nums), len(iou_thrs)] float64.

    gts: list of (n, 4) arrays (or None); proposals: list of (k, 4) or (k, 5) arrays or tensors; (k, 5) proposals
    are ranked by score (descending; the reference's unstable argsort, so ties are only defined without them)."""
    img_num = len(gts)
    assert img_num == len(proposals)
    proposal_nums, iou_thrs = set_recall_param(proposal_nums, iou_thrs)
    dev = _device(device)
    nums = [int(n) for n in np.asarray(proposal_nums).reshape(-1)]
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    with torch.cuda.device(dev):
        g_list, p_list, s_list, g_cnt, p_cnt = [], [], [], [], []
        for i in range(img_num):
            g = gts[i]
            g = torch.zeros((0, 4)) if g is None or g.shape[0] == 0 else torch.as_tensor(g)[:, :4]
            p = torch.as_tensor(proposals[i])
            scored = p.dim() == 2 and p.shape[1] == 5
            # unscored proposals keep their order: rank by position
            s = p[:, 4].double() if scored else -torch.arange(p.shape[0], dtype=torch.float64, device=p.device)
            g_list.append(g.to(dev, torch.float32))
            p_list.append(p[:, :4].to(dev, torch.float32))
            s_list.append(s.to(dev))
            g_cnt.append(g.shape[0])
            p_cnt.append(p.shape[0])
        n_gt = int(sum(g_cnt))
        gtb = torch.cat(g_list).contiguous() if g_list else torch.zeros((0, 4), device=dev)
        props = torch.cat(p_list) if p_list else torch.zeros((0, 4), device=dev)
        score = torch.cat(s_list) if s_list else torch.zeros(0, dtype=torch.float64, device=dev)
        img = torch.repeat_interleave(torch.arange(img_num, device=dev), torch.tensor(p_cnt, device=dev))
        o = torch.argsort(-score, stable=True)
        o = o[torch.argsort(img[o], stable=True)]
        img = img[o]
        rank = torch.arange(len(o), device=dev) - torch.searchsorted(img, img)
        cut = (rank < nums[-1]).nonzero().squeeze(1)       # prop_num = min(k, proposal_nums[-1])
        props = props[o[cut]].contiguous()
        img = img[cut]
        gt_off = torch.tensor(np.concatenate([[0], np.cumsum(g_cnt)]).astype(np.int64), device=dev)
        prop_off = _offsets(img, img_num, dev)
        if max((g * min(p, nums[-1]) for g, p in zip(g_cnt, p_cnt)), default=0) >= 2 ** 32 - 1:
            raise ValueError('eval_recalls: too many ground truths x proposals in one image')
        num_t = torch.tensor(nums, dtype=torch.int32, device=dev)
        gt_ious = torch.empty((len(nums), n_gt), dtype=torch.float32, device=dev)
        ws = torch.empty(capi.lib().htd_eval_recalls_workspace_bytes(n_gt, len(props), len(nums)), dtype=torch.uint8,
                         device=dev)
        capi.call('htd_eval_recalls', capi.ptr(gtb), capi.ptr(gt_off), capi.ptr(props), capi.ptr(prop_off), img_num,
                  n_gt, len(props), capi.ptr(num_t), len(nums), capi.ptr(gt_ious), capi.ptr(ws),
                  capi.current_stream_ptr())
        thr_t = torch.from_numpy(thrs).to(dev)
        counts = (gt_ious.double()[:, None, :] >= thr_t[None, :, None]).sum(-1).cpu().numpy()
    recalls = counts / float(n_gt)
    print_recall_summary(recalls, proposal_nums, iou_thrs, logger=logger)
    return recalls


# ------------------------------------------------------------------------------------------------ eval_map (VOC)
def voc_classes():
    """class_names.py:voc_classes."""
    return ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
            'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']


def coco_classes():
    """class_names.py:coco_classes: the COCO names with '_' for ' '."""
    from ..coco import COCO_CLASSES
    return [c.replace(' ', '_') for c in COCO_CLASSES]


_VOC_ALIASES = ('voc', 'pascal_voc', 'voc07', 'voc12')
_COCO_ALIASES = ('coco', 'mscoco', 'ms_coco')
_OTHER_ALIASES = ('det', 'imagenet_det', 'ilsvrc_det', 'vid', 'imagenet_vid', 'ilsvrc_vid', 'WIDERFaceDataset',
                  'wider_face', 'WDIERFace', 'cityscapes')


def get_classes(dataset):
    """class_names.py:get_classes for the Pascal VOC and COCO aliases; the reference's other aliases raise
    NotImplementedError."""
    if not isinstance(dataset, str):
        raise TypeError(f'dataset must a str, but got {type(dataset)}')
    if dataset in _VOC_ALIASES:
        return voc_classes()
    if dataset in _COCO_ALIASES:
        return coco_classes()
    if dataset in _OTHER_ALIASES:
        raise NotImplementedError(f'get_classes: the class names of {dataset!r} are not included')
    raise ValueError(f'Unrecognized dataset: {dataset}')


def _f32_bound(v):
    """The float32 t such that, for every float32 x, x >= t (and x < t) exactly when numpy's `x >= v` (`x < v`) holds
    for a float32 array x: a Python number is cast to float32 (NEP 50); a 64-bit numpy scalar makes the comparison
    float64, which the next float32 up reproduces."""
    if isinstance(v, np.generic) and np.result_type(np.float32, v) != np.float32:
        t = np.float32(v)
        if float(t) < float(v):
            t = np.nextafter(t, np.float32(np.inf))
        return t
    return np.float32(v)


def _as_np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _map_gts(annotations, K):
    """-> host arrays: gts [n, 4] float32 grouped by pair (class * I + image), non-ignored before ignored, each in
    annotation order; gt_off [K * I + 1]; n_keep [K * I]."""
    I = len(annotations)
    boxes, keys, ign = [], [], []
    for i, ann in enumerate(annotations):
        parts = [(ann['bboxes'], ann['labels'], 0)]
        if ann.get('labels_ignore', None) is not None:
            parts.append((ann['bboxes_ignore'], ann['labels_ignore'], 1))
        for b, lab, flag in parts:
            lab = _as_np(lab).reshape(-1).astype(np.int64)
            b = _as_np(b).astype(np.float32).reshape(-1, 4)
            ok = (lab >= 0) & (lab < K)
            boxes.append(b[ok])
            keys.append(lab[ok] * I + i)
            ign.append(np.full(int(ok.sum()), flag, np.int64))
    boxes = np.concatenate(boxes) if boxes else np.zeros((0, 4), np.float32)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    ign = np.concatenate(ign) if ign else np.zeros(0, np.int64)
    order = np.argsort(keys * 2 + ign, kind='stable')
    keys = keys[order]
    gt_off = np.searchsorted(keys, np.arange(K * I + 1), side='left').astype(np.int64)
    n_keep = np.bincount(keys[ign[order] == 0], minlength=K * I).astype(np.int32)
    return np.ascontiguousarray(boxes[order]), gt_off, n_keep


def _map_dets(det_results, I, K, dev):
    """-> device dets [n, 5] float32 grouped by pair (class * I + image) in row order, det_off [K * I + 1], and a
    device flag (or None) set when a label or image index of the triple form lies out of range.  Out-of-range rows
    are clamped into range so that every kernel stays in bounds; the caller raises once the flag is read back with
    the results."""
    if isinstance(det_results, (tuple, list)) and len(det_results) == 3 and isinstance(det_results[0], torch.Tensor):
        dets, labels, index = det_results
        dets = dets.to(dev, torch.float32).reshape(-1, 5)
        labels, index = labels.to(dev, torch.int64).reshape(-1), index.to(dev, torch.int64).reshape(-1)
        bad = ((labels < 0) | (labels >= K) | (index < 0) | (index >= I)).any().to(torch.uint8).reshape(1)
        key = labels.clamp(0, K - 1) * I + index.clamp(0, I - 1)
        order = torch.argsort(key, stable=True)
        key = key[order]
        det_off = torch.searchsorted(key, torch.arange(K * I + 1, device=dev, dtype=torch.int64))
        return dets[order].contiguous(), det_off.contiguous(), bad
    if len(det_results) != I:
        raise ValueError(f'eval_map: {len(det_results)} results for {I} images')
    arrs, lens = [], np.zeros(K * I, np.int64)
    for c in range(K):
        for i in range(I):
            a = _as_np(det_results[i][c])
            if a.size:
                a = a.reshape(-1, 5)
                arrs.append(a)
                lens[c * I + i] = a.shape[0]
    dets = np.concatenate(arrs).astype(np.float32, copy=False) if arrs else np.zeros((0, 5), np.float32)
    det_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return torch.from_numpy(np.ascontiguousarray(dets)).to(dev), torch.from_numpy(det_off).to(dev), None


def map_device_arrays(det_results, annotations, num_classes, area_ranges=None, iou_thr=0.5, device=None):
    """The device part of eval_map: -> dict of host numpy arrays, all read back in one copy:
    cls_off [K+1], recall [S][n] float64 and precision [S][n] float32 (class k at cls_off[k]..cls_off[k+1], score
    descending, ties in (image, row) order), terms [S][n + K] float64 ('area' terms of class k from cls_off[k] + k),
    n_terms / num_gts [K][S] int32, ap11 [K][S] float32."""
    dev = _device(device)
    I, K = len(annotations), int(num_classes)
    S = 1 if area_ranges is None else len(area_ranges)
    if K <= 0 or I <= 0 or S <= 0:
        raise ValueError(f'eval_map: {K} classes, {I} images, {S} scale ranges')
    P_, S_ = capi.ptr, capi.current_stream_ptr
    with torch.cuda.device(dev):
        dets, det_off, bad = _map_dets(det_results, I, K, dev)
        gts, gt_off, n_keep = _map_gts(annotations, K)
        gts, gt_off, n_keep = (torch.from_numpy(x).to(dev) for x in (gts, gt_off, n_keep))
        rng = None
        if area_ranges is not None:
            rng = torch.from_numpy(np.array([[_f32_bound(lo), _f32_bound(hi)] for lo, hi in area_ranges],
                                            np.float32)).to(dev)
        n = dets.shape[0]
        flags = torch.empty((n, S), dtype=torch.uint8, device=dev)
        pair_gts = torch.empty((K * I, S), dtype=torch.int32, device=dev)
        ws = torch.empty(capi.lib().htd_voc_tpfp_workspace_bytes(n), dtype=torch.uint8, device=dev)
        capi.call('htd_voc_tpfp', P_(dets), P_(det_off), P_(gts), P_(gt_off), P_(n_keep), K * I, P_(rng), S,
                  float(_f32_bound(iou_thr)), P_(flags), P_(pair_gts), P_(ws), S_())

        # the class's rows by score descending, ties in (image, row) order; -score + 0 sorts -0.0 with +0.0
        cls_off = det_off[::I].contiguous()
        cls = torch.repeat_interleave(torch.arange(K, device=dev), cls_off[1:] - cls_off[:-1], output_size=n)
        order = torch.argsort(-dets[:, 4] + 0.0, stable=True)
        order = order[torch.argsort(cls[order], stable=True)].contiguous()
        thr11 = torch.from_numpy(np.arange(0, 1 + 1e-3, 0.1)).to(dev)
        sizes = [('recall', S * n, np.float64), ('terms', S * (n + K), np.float64), ('precision', S * n, np.float32),
                 ('ap11', K * S, np.float32), ('n_terms', K * S, np.int32), ('num_gts', K * S, np.int32),
                 ('cls_off', K + 1, np.int64), ('bad', 1, np.uint8)]
        offs, total = {}, 0
        for name, count, dt in sizes:
            offs[name] = (total, count, dt)
            total += -(-count * np.dtype(dt).itemsize // 8) * 8
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        view = {name: out[o:o + c * np.dtype(dt).itemsize] for name, (o, c, dt) in offs.items()}
        view['cls_off'].view(torch.int64).copy_(cls_off)
        if bad is not None:
            view['bad'].copy_(bad)
        else:
            view['bad'].zero_()
        env = torch.empty(capi.lib().htd_voc_accumulate_workspace_bytes(n, S), dtype=torch.uint8, device=dev)
        capi.call('htd_voc_accumulate', P_(flags), P_(order), P_(cls_off), P_(pair_gts), K, I, S, n, P_(thr11),
                  P_(view['recall']), P_(view['precision']), P_(view['terms']), P_(view['n_terms']),
                  P_(view['num_gts']), P_(view['ap11']), P_(env), S_())
        host = out.cpu().numpy()
    res = {name: host[o:o + c * np.dtype(dt).itemsize].view(dt) for name, (o, c, dt) in offs.items()}
    if res.pop('bad')[0]:
        raise ValueError(f'eval_map: labels must lie in [0, {K}) and image indices in [0, {I})')
    res['recall'] = res['recall'].reshape(S, n)
    res['precision'] = res['precision'].reshape(S, n)
    res['terms'] = res['terms'].reshape(S, n + K)
    for k in ('ap11', 'n_terms', 'num_gts'):
        res[k] = res[k].reshape(K, S)
    return res


def _num_classes(det_results, dataset, num_classes):
    if num_classes is not None:
        return int(num_classes)
    if isinstance(det_results, (tuple, list)) and len(det_results) == 3 and isinstance(det_results[0], torch.Tensor):
        if isinstance(dataset, str):
            return len(get_classes(dataset))
        if dataset is not None:
            return len(dataset)
        raise ValueError('eval_map: the (dets, labels, index) form needs num_classes= or a dataset naming the classes')
    return len(det_results[0])


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5, dataset=None, logger=None, tpfp_fn=None,
             nproc=4, num_classes=None, device=None):
    """mean_ap.py:eval_map on the device, in process: -> (mean_ap, [per-class dict(num_gts, num_dets, recall,
    precision, ap)]) with the reference's types and dtypes.

    det_results: bbox2result lists (one list of (n, 5) arrays per image), or the (dets (N, 5), labels (N,), image index
    (N,)) triple of apis.results_to_tensors (then num_classes=, or `dataset` naming the classes, gives the class count).
    annotations: per image dict(bboxes, labels[, bboxes_ignore, labels_ignore]).  Comparisons follow numpy 2 (NEP 50):
    the float32 IoU maximum against float32(iou_thr) and float32 areas against float32 range ends, so iou_thr=0.7
    matches an IoU of float32(0.7) = 0.69999999, which numpy 1.x compared in float64 would not.  Score ties, which the
    reference leaves to numpy's unstable argsort, keep (image, row) order.  nproc is accepted and ignored; tpfp_fn and
    the ImageNet protocols ('det', 'vid') raise NotImplementedError."""
    if tpfp_fn is not None:
        raise NotImplementedError('eval_map: a custom tpfp_fn is not supported, the device runs tpfp_default')
    if isinstance(dataset, str) and dataset in ('det', 'vid'):
        raise NotImplementedError('eval_map: the ImageNet protocol (tpfp_imagenet) is not supported')
    num_imgs = len(annotations)
    K = _num_classes(det_results, dataset, num_classes)
    num_scales = len(scale_ranges) if scale_ranges is not None else 1
    area_ranges = [(rg[0] ** 2, rg[1] ** 2) for rg in scale_ranges] if scale_ranges is not None else None
    r = map_device_arrays(det_results, annotations, K, area_ranges, iou_thr, device)
    mode = 'area' if not (isinstance(dataset, str) and dataset == 'voc07') else '11points'
    eval_results = []
    for c in range(K):
        lo, hi = int(r['cls_off'][c]), int(r['cls_off'][c + 1])
        recalls = r['recall'][:, lo:hi].copy()
        precisions = r['precision'][:, lo:hi].copy()
        num_gts = r['num_gts'][c].astype(int)
        if mode == 'area':
            ap = np.zeros(num_scales, dtype=np.float32)
            for s in range(num_scales):
                ap[s] = np.sum(r['terms'][s, lo + c:lo + c + int(r['n_terms'][c, s])])
        else:
            ap = r['ap11'][c].copy()
        if scale_ranges is None:
            recalls, precisions, num_gts, ap = recalls[0], precisions[0], num_gts.item(), ap[0]
        eval_results.append(dict(num_gts=num_gts, num_dets=hi - lo, recall=recalls, precision=precisions, ap=ap))
    if scale_ranges is not None:
        all_ap = np.vstack([x['ap'] for x in eval_results])
        all_num_gts = np.vstack([x['num_gts'] for x in eval_results])
        mean_ap = [all_ap[all_num_gts[:, i] > 0, i].mean() if np.any(all_num_gts[:, i] > 0) else 0.0
                   for i in range(num_scales)]
    else:
        aps = [x['ap'] for x in eval_results if x['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    print_map_summary(mean_ap, eval_results, dataset, area_ranges, logger=logger)
    return mean_ap, eval_results


def print_map_summary(mean_ap, results, dataset=None, scale_ranges=None, logger=None):
    """mean_ap.py:print_map_summary: per scale range, a table of gts / dets / recall / ap per class and the mAP."""
    if logger == 'silent':
        return
    num_scales = len(results[0]['ap']) if isinstance(results[0]['ap'], np.ndarray) else 1
    if scale_ranges is not None:
        assert len(scale_ranges) == num_scales
    num_classes = len(results)
    recalls = np.zeros((num_scales, num_classes), dtype=np.float32)
    aps = np.zeros((num_scales, num_classes), dtype=np.float32)
    num_gts = np.zeros((num_scales, num_classes), dtype=int)
    for i, cls_result in enumerate(results):
        if cls_result['recall'].size > 0:
            recalls[:, i] = np.array(cls_result['recall'], ndmin=2)[:, -1]
        aps[:, i] = cls_result['ap']
        num_gts[:, i] = cls_result['num_gts']
    if dataset is None:
        label_names = [str(i) for i in range(num_classes)]
    elif isinstance(dataset, str):
        label_names = get_classes(dataset)
    else:
        label_names = dataset
    if not isinstance(mean_ap, list):
        mean_ap = [mean_ap]
    for i in range(num_scales):
        if scale_ranges is not None:
            print_log(f'Scale range {scale_ranges[i]}', logger=logger)
        rows = [['class', 'gts', 'dets', 'recall', 'ap']]
        for j in range(num_classes):
            rows.append([str(label_names[j]), str(num_gts[i, j]), str(results[j]['num_dets']), f'{recalls[i, j]:.3f}',
                         f'{aps[i, j]:.3f}'])
        rows.append(['mAP', '', '', '', f'{mean_ap[i]:.3f}'])
        print_log('\n' + format_table(rows), logger=logger)
