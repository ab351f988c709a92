"""COCO bbox / proposal evaluation and proposal recall on the device.

coco_eval() is pycocotools' COCOeval.evaluate + accumulate + summarize as CocoDataset.evaluate drives them
(datasets/coco.py:363-545): the greedy matching and the accumulation run as HIP kernels (csrc/coco_eval.hip), the sort
and grouping of the detections is a few stable device sorts here, and the 12 summary numbers are taken on the host
from the device arrays with pycocotools' own slices.  eval_recalls() is core/evaluation/recall.py:eval_recalls with
the IoU and the greedy assignment on the device.  pycocotools is not needed.
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
