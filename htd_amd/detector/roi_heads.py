"""StandardRoIHead and CascadeRoIHead: the RoI heads of the Faster R-CNN and Cascade R-CNN baselines.

Reference: roi_heads/standard_roi_head.py:9-311 with test_mixins.py:52-96, roi_heads/cascade_roi_head.py:12-507
(+ base_roi_head.py:8-106).  Same registry names, kwargs, sub-module names (bbox_roi_extractor / bbox_head, indexed per stage in
the cascade), loss keys (loss_cls, acc, loss_bbox; s{i}.* in the cascade) and return structures.  They train on fixed-size
tensors without a host/device synchronisation when the configuration allows it (forward_train_static), fall back to the
per-image lists otherwise, and post-process a whole test batch in one pass.  HTDRoIHead (htd_roi_head.py) is a CascadeRoIHead:
the module functions, _BBoxRoIHead and the cascade's constructor, gates and stage loops here are its own too.

Outside this path, each raising an error that names the key: mask branches, shared_head, aug_test.
"""
import torch
import torch.nn as nn

from .. import mmcv_ops as M
from ..core import bbox2result, bbox2roi
from ..core.misc import arange_cached, const_tensor
from ..registry import HEADS, build_assigner, build_head, build_roi_extractor, build_sampler


def _batched_sampling_ok(assigner, sampler, gt_bboxes_ignore):
    """MaxIoUAssigner without ignore regions + RandomSampler: what batched_assign_and_sample / static_assign_and_sample cover."""
    return all(g is None for g in gt_bboxes_ignore) and assigner.ignore_iof_thr <= 0 and \
        isinstance(assigner.neg_iou_thr, float) and type(sampler).__name__ == 'RandomSampler'


def assign_and_sample(assigner, sampler, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore):
    """Per-image reference order when a permutation source is installed (parity tests replay the CPU RNG); otherwise all
    images at once with a single device->host copy (core.bbox.batched_assign_and_sample)."""
    from ..core import bbox as _bbox
    if _bbox._randperm is _bbox._device_randperm and _batched_sampling_ok(assigner, sampler, gt_bboxes_ignore):
        return _bbox.batched_assign_and_sample(assigner, sampler, proposal_list, gt_bboxes, gt_labels)[0]
    out = []
    for j in range(len(proposal_list)):
        assign_result = assigner.assign(proposal_list[j], gt_bboxes[j], gt_bboxes_ignore[j], gt_labels[j])
        out.append(sampler.sample(assign_result, proposal_list[j], gt_bboxes[j], gt_labels[j]))
    return out


def static_targets(head, S):
    """bbox_head.get_targets (bbox_head.py:85-146) on the fixed slots of a StaticSamples: unused slots carry weight 0.  A head
    with reg_decoded_bbox gets the gt boxes of its positives instead of encoded deltas, zeros everywhere else."""
    from ..core.bbox import roi_targets_device
    labels, lw, bt, bw = roi_targets_device(S.boxes.view(-1, 4), S.pos_gt_bboxes.view(-1, 4), S.pos_gt_labels.view(-1),
                                            S.is_pos.view(-1), S.valid.view(-1), head.num_classes, head.bbox_coder.means,
                                            head.bbox_coder.stds)
    if head.reg_decoded_bbox:
        bt = S.pos_gt_bboxes.view(-1, 4).float() * bw            # bw: 1 on the positives, 0 elsewhere
    return labels, lw, bt, bw


def batched_targets(head, sampling_results, cfg):
    """BBoxHead.get_targets (bbox_head.py:85-139) for the whole batch in a handful of launches: rows are [pos_i ; neg_i] per
    image, positives carry their gt label and encoded deltas (their gt box for a head with reg_decoded_bbox), everything has
    weight 1 (pos_weight <= 0), negatives the background label."""
    if cfg.pos_weight > 0:
        return head.get_targets(sampling_results, None, None, cfg)
    npos = [r.pos_bboxes.size(0) for r in sampling_results]
    nneg = [r.neg_bboxes.size(0) for r in sampling_results]
    N = sum(npos) + sum(nneg)
    dev = sampling_results[0].pos_bboxes.device
    pos_rows, start = [], 0
    for a, b in zip(npos, nneg):
        pos_rows.append(torch.arange(start, start + a, device=dev))
        start += a + b
    pos_rows = torch.cat(pos_rows)
    pos_b = torch.cat([r.pos_bboxes for r in sampling_results])
    labels = pos_b.new_full((N, ), head.num_classes, dtype=torch.long)
    bbox_targets = pos_b.new_zeros(N, 4)
    bbox_weights = pos_b.new_zeros(N, 4)
    if pos_rows.numel():
        labels[pos_rows] = torch.cat([r.pos_gt_labels for r in sampling_results])
        pos_gt = torch.cat([r.pos_gt_bboxes for r in sampling_results])
        # a head in decoded mode regresses against the gt box itself (bbox_head.py:118-124)
        bbox_targets[pos_rows] = pos_gt if head.reg_decoded_bbox else head.bbox_coder.encode(pos_b, pos_gt)
        bbox_weights.index_fill_(0, pos_rows, 1.0)
    return labels, pos_b.new_ones(N), bbox_targets, bbox_weights


def static_refine(head, S, bbox_pred, lim):
    """BBoxHead.refine_bboxes (bbox_head.py:227-304) on the fixed slots of a StaticSamples, for a class-agnostic regressor:
    decode, clip to lim (B,2) [w,h], drop the gt-born rows.  -> boxes (B,n,4), keep (B,n): the next stage's candidates."""
    from ..core.bbox import delta2bbox_clip_device
    B, n = S.valid.shape
    with torch.no_grad():
        keep = S.valid & ~S.pos_is_gt
        boxes = delta2bbox_clip_device(S.boxes.view(-1, 4), bbox_pred, head.bbox_coder.means, head.bbox_coder.stds, lim,
                                       keep.view(-1), n).view(B, n, 4)
    return boxes, keep


def _static_stage_ok(head, assigner, sampler, cfg):
    """One stage of the sync-free training path: batched assignment and sampling, unit sample weights, and a decoded-box head
    only with a loss the fused kernel takes."""
    return _batched_sampling_ok(assigner, sampler, ()) and cfg.pos_weight <= 0 and \
        (not head.reg_decoded_bbox or head.fused_loss_config_ok())


def _refine_rows(head, rois, bbox_pred, sampling_results, img_metas):
    """BBoxHead.refine_bboxes (bbox_head.py:227-304) for a class-agnostic regressor: one decode for the whole batch (per-row
    image limits), then per image the rows that were ground truth -- they lead each image's block because gt candidates come
    first and sampled indices are ascending -- are dropped with a slice.  -> None when the head needs the reference's form."""
    if not head.reg_class_agnostic or not head.bbox_coder.clip_border:
        return None
    from ..core.bbox import delta2bbox
    boxes = delta2bbox(rois[:, 1:], bbox_pred, head.bbox_coder.means, head.bbox_coder.stds, None)
    lim = const_tensor([[m['img_shape'][1], m['img_shape'][0]] * 2 for m in img_metas], boxes.device, boxes.dtype)      # (B,4) w,h,w,h
    boxes = torch.min(boxes.clamp(min=0), lim[rois[:, 0].long()])
    if all(hasattr(r, 'num_pos_gt') for r in sampling_results):
        n_gt = [r.num_pos_gt for r in sampling_results]
    else:
        n_gt = [int(v) for v in torch.stack([r.pos_is_gt.sum() for r in sampling_results]).tolist()]
    out, start = [], 0
    for r, g in zip(sampling_results, n_gt):
        n = r.pos_bboxes.size(0) + r.neg_bboxes.size(0)
        out.append(boxes[start + g:start + n])
        start += n
    return out


class _BBoxRoIHead(nn.Module):
    """What every RoI head shares: the unsupported keys, the sampling switches and the whole-batch test post-processing."""
    batched_test = True      # post-process the whole batch in one pass (False: the per-image loop of the reference)

    def _reject_unsupported(self, mask_roi_extractor, mask_head, shared_head):
        name = type(self).__name__
        if mask_head is not None:
            raise NotImplementedError(f'roi_head.mask_head: {name} has no mask branch')
        if mask_roi_extractor is not None:
            raise NotImplementedError(f'roi_head.mask_roi_extractor: {name} has no mask branch')
        if shared_head is not None:
            raise NotImplementedError(f'roi_head.shared_head: {name} does not support a shared head')

    @property
    def with_bbox(self):
        return getattr(self, 'bbox_head', None) is not None

    @property
    def with_mask(self):
        return False

    @property
    def with_shared_head(self):
        return False

    def _static_enabled(self, gt_bboxes_ignore):
        from ..core import bbox as _bbox
        if not getattr(self, 'static_shapes', True) or _bbox._randperm is not _bbox._device_randperm:
            return False
        return gt_bboxes_ignore is None or all(g is None for g in gt_bboxes_ignore)

    def _batched_test_ok(self, heads, rois, img_metas, rescale):
        if not (self.batched_test and rois.is_cuda and len(img_metas) > 1):
            return False
        if not all(getattr(h, 'with_reg', False) for h in heads):
            return False                                            # get_bboxes without deltas clips by scalar img_shape
        if dict(self.test_cfg.nms).get('type', 'nms') != 'nms':
            return False                                            # soft-NMS decays sequentially per class: per image
        kinds = {isinstance(m['scale_factor'], float) for m in img_metas}
        return not rescale or len(kinds) == 1

    @staticmethod
    def _row_limits(rois, img_metas):
        """-> (image of every row, its (h, w) clip limits)."""
        img_of = rois[:, 0].long()
        hw = torch.tensor([[float(m['img_shape'][0]), float(m['img_shape'][1])] for m in img_metas],
                          dtype=rois.dtype).to(rois.device, non_blocking=True)[img_of]
        return img_of, hw

    def _get_bboxes_images(self, head, rois, cls_score, bbox_pred, img_of, hw, img_metas, rescale):
        """BBoxHead.get_bboxes (bbox_heads/bbox_head.py:309-341) of every image at once, for (n, 4) and (n, 4 * C) boxes alike;
        results equal the per-image calls bit for bit."""
        from ..core.post_processing import multiclass_nms_images
        bboxes, scores = head.get_bboxes(rois, cls_score, bbox_pred, hw, None, rescale=False, cfg=None)
        if rescale and bboxes.size(0) > 0:
            if isinstance(img_metas[0]['scale_factor'], float):
                # tensor / python scalar multiplies by the fp32 reciprocal on the device; same here, per row
                inv = (1.0 / torch.tensor([m['scale_factor'] for m in img_metas], dtype=torch.float32))
                bboxes = bboxes * inv.to(bboxes.device, non_blocking=True)[img_of][:, None]
            else:
                sf = torch.tensor([[float(v) for v in m['scale_factor']] for m in img_metas], dtype=torch.float32)
                sf = sf.to(bboxes.device, non_blocking=True)[img_of]
                bboxes = (bboxes.view(bboxes.size(0), -1, 4) / sf[:, None, :]).view(bboxes.size(0), -1)
        return multiclass_nms_images(bboxes, scores, img_of, len(img_metas), self.test_cfg.score_thr, self.test_cfg.nms,
                                     self.test_cfg.max_per_img)

    def _results(self, det_bboxes, det_labels, num_classes):
        from ..core.bbox import bbox2result_many
        if self.batched_test:
            return bbox2result_many(det_bboxes, det_labels, num_classes)
        return [bbox2result(b, l, num_classes) for b, l in zip(det_bboxes, det_labels)]

    def aug_test(self, features, proposal_list, img_metas, rescale=False):
        raise NotImplementedError(f'aug_test: {type(self).__name__} has no test-time augmentation (MultiScaleFlipAug with one '
                                  'scale and flip=False goes through simple_test)')


@HEADS.register_module()
class StandardRoIHead(_BBoxRoIHead):
    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None, shared_head=None,
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self._reject_unsupported(mask_roi_extractor, mask_head, shared_head)
        assert bbox_roi_extractor is not None and bbox_head is not None
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.bbox_roi_extractor = build_roi_extractor(bbox_roi_extractor)
        self.bbox_head = build_head(bbox_head)
        self.bbox_assigner = self.bbox_sampler = None
        if self.train_cfg:
            self.bbox_assigner = build_assigner(self.train_cfg.assigner)
            self.bbox_sampler = build_sampler(self.train_cfg.sampler, context=self)

    def init_weights(self, pretrained=None):
        self.bbox_roi_extractor.init_weights()
        self.bbox_head.init_weights()

    def _bbox_forward(self, x, rois):
        bbox_feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        cls_score, bbox_pred = self.bbox_head(bbox_feats)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)

    # ------------------------------------------------------------------ train
    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        if gt_masks is not None:
            raise NotImplementedError('gt_masks: StandardRoIHead has no mask branch')
        if gt_bboxes_ignore is None:
            gt_bboxes_ignore = [None for _ in range(len(img_metas))]
        sampling_results = assign_and_sample(self.bbox_assigner, self.bbox_sampler, proposal_list, gt_bboxes, gt_labels,
                                             gt_bboxes_ignore)
        rois = bbox2roi([res.bboxes for res in sampling_results])
        res = self._bbox_forward(x, rois)
        targets = batched_targets(self.bbox_head, sampling_results, self.train_cfg)
        return dict(self.bbox_head.loss(res['cls_score'], res['bbox_pred'], rois, *targets))

    # ------------------------------------------------------------------ train, static shapes
    def can_train_static(self, gt_bboxes_ignore=None):
        """MaxIoUAssigner without ignore regions, RandomSampler, unit sample weights."""
        return self._static_enabled(gt_bboxes_ignore) and self.bbox_assigner is not None and \
            _static_stage_ok(self.bbox_head, self.bbox_assigner, self.bbox_sampler, self.train_cfg)

    def forward_train_static(self, x, img_metas, proposals, n_keep, gt_bboxes, gt_labels):
        """forward_train on fixed-size tensors: proposals (B,P,5) zero-padded past n_keep (B,) [device].  Numerically the
        per-image path with the same samples; nothing is read back to the host."""
        from ..core.bbox import static_assign_and_sample
        P = proposals.size(1)
        pvalid = arange_cached(P, proposals.device)[None, :] < n_keep[:, None]
        S = static_assign_and_sample(self.bbox_assigner, self.bbox_sampler, proposals[..., :4], pvalid, gt_bboxes, gt_labels)
        rois = S.rois
        res = self._bbox_forward(x, rois)
        losses = self.bbox_head.loss(res['cls_score'], res['bbox_pred'], rois, *static_targets(self.bbox_head, S),
                                     num_samples=S.valid.sum())
        self._last_static = (S, )             # exposed for tests
        return dict(losses)

    # ------------------------------------------------------------------ test
    def simple_test_bboxes(self, x, img_metas, proposals, rcnn_test_cfg=None, rescale=False):
        """test_mixins.py:52-96 -> (det_bboxes list, det_labels list) on the device."""
        assert rcnn_test_cfg is None or rcnn_test_cfg is self.test_cfg
        rois = bbox2roi(proposals)
        res = self._bbox_forward(x, rois)
        head = self.bbox_head
        if self._batched_test_ok([head], rois, img_metas, rescale):
            img_of, hw = self._row_limits(rois, img_metas)
            return self._get_bboxes_images(head, rois, res['cls_score'], res['bbox_pred'], img_of, hw, img_metas, rescale)
        n_per = tuple(len(p) for p in proposals)
        bbox_pred = res['bbox_pred'].split(n_per) if res['bbox_pred'] is not None else (None, ) * len(proposals)
        det_bboxes, det_labels = [], []
        for i, (r, c, p) in enumerate(zip(rois.split(n_per), res['cls_score'].split(n_per), bbox_pred)):
            b, l = head.get_bboxes(r, c, p, img_metas[i]['img_shape'], img_metas[i]['scale_factor'], rescale=rescale,
                                   cfg=self.test_cfg)
            det_bboxes.append(b)
            det_labels.append(l)
        return det_bboxes, det_labels

    def simple_test(self, x, proposal_list, img_metas, proposals=None, rescale=False):
        det_bboxes, det_labels = self.simple_test_bboxes(x, img_metas, proposal_list, self.test_cfg, rescale=rescale)
        return self._results(det_bboxes, det_labels, self.bbox_head.num_classes)


@HEADS.register_module()
class CascadeRoIHead(_BBoxRoIHead):
    def __init__(self, num_stages, stage_loss_weights, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None,
                 mask_head=None, shared_head=None, train_cfg=None, test_cfg=None):
        super().__init__()
        self._reject_unsupported(mask_roi_extractor, mask_head, shared_head)
        assert bbox_roi_extractor is not None and bbox_head is not None
        self.num_stages, self.stage_loss_weights = num_stages, stage_loss_weights
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.bbox_roi_extractor = nn.ModuleList()
        self.bbox_head = nn.ModuleList()
        if not isinstance(bbox_roi_extractor, list):
            bbox_roi_extractor = [bbox_roi_extractor for _ in range(num_stages)]
        if not isinstance(bbox_head, list):
            bbox_head = [bbox_head for _ in range(num_stages)]
        assert len(bbox_roi_extractor) == len(bbox_head) == num_stages
        for ext, head in zip(bbox_roi_extractor, bbox_head):
            self.bbox_roi_extractor.append(build_roi_extractor(ext))
            self.bbox_head.append(build_head(head))
        self.bbox_assigner, self.bbox_sampler = [], []
        if self.train_cfg is not None:
            for idx, rcnn_train_cfg in enumerate(self.train_cfg):
                self.bbox_assigner.append(build_assigner(rcnn_train_cfg.assigner))
                self.current_stage = idx
                self.bbox_sampler.append(build_sampler(rcnn_train_cfg.sampler, context=self))

    def init_weights(self, pretrained=None):
        for i in range(self.num_stages):
            self.bbox_roi_extractor[i].init_weights()
            self.bbox_head[i].init_weights()

    def _bbox_forward(self, stage, x, rois):
        """x: the pyramid levels, or (training) a mmcv_ops.PyramidTaps over them -- the RoIAlign consumers of a step then share
        one gradient map per level instead of summing one per stage."""
        extractor = self.bbox_roi_extractor[stage]
        bbox_feats = extractor(x if isinstance(x, M.PyramidTaps) else x[:extractor.num_inputs], rois)
        cls_score, bbox_pred = self.bbox_head[stage](bbox_feats)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)

    def _bbox_forward_train(self, stage, x, rois, sampling_results, **kw):
        """A stage's forward in the per-image training loop; a head that treats the sampled positives apart overrides it."""
        return self._bbox_forward(stage, x, rois, **kw)

    def _taps(self, x):
        same = len({e.num_inputs for e in self.bbox_roi_extractor}) == 1
        return M.PyramidTaps(x[:self.bbox_roi_extractor[0].num_inputs]) if same and x[0].is_cuda else x

    def _add_stage_losses(self, losses, stage, loss_bbox):
        lw = self.stage_loss_weights[stage]
        for name, value in loss_bbox.items():
            losses[f's{stage}.{name}'] = value * lw if 'loss' in name else value

    # ------------------------------------------------------------------ train
    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None, **kw):
        """kw: handed on to every stage's _bbox_forward."""
        if gt_masks is not None:
            raise NotImplementedError('gt_masks: CascadeRoIHead has no mask branch')
        losses = dict()
        if gt_bboxes_ignore is None:
            gt_bboxes_ignore = [None for _ in range(len(img_metas))]
        feats = self._taps(x)
        for i in range(self.num_stages):
            self.current_stage = i
            head = self.bbox_head[i]
            sampling_results = assign_and_sample(self.bbox_assigner[i], self.bbox_sampler[i], proposal_list, gt_bboxes,
                                                 gt_labels, gt_bboxes_ignore)
            rois = bbox2roi([res.bboxes for res in sampling_results])
            res = self._bbox_forward_train(i, feats, rois, sampling_results, **kw)
            targets = batched_targets(head, sampling_results, self.train_cfg[i])
            self._add_stage_losses(losses, i, head.loss(res['cls_score'], res['bbox_pred'], rois, *targets))
            if i < self.num_stages - 1:
                with torch.no_grad():
                    proposal_list = _refine_rows(head, rois, res['bbox_pred'], sampling_results, img_metas)
                    if proposal_list is None:
                        # background rows take the arg-max foreground class (cascade_roi_head.py:276-286)
                        roi_labels = torch.where(targets[0] == head.num_classes, res['cls_score'][:, :-1].argmax(1), targets[0])
                        proposal_list = head.refine_bboxes(rois, roi_labels, res['bbox_pred'],
                                                           [r.pos_is_gt for r in sampling_results], img_metas)
        return losses

    # ------------------------------------------------------------------ train, static shapes
    def can_train_static(self, gt_bboxes_ignore=None):
        """Every stage on batched sampling with unit weights, and every stage that hands boxes on a class-agnostic regressor
        with clip_border (delta2bbox_clip_device decodes (n, 4) deltas)."""
        if not self._static_enabled(gt_bboxes_ignore) or len(self.bbox_assigner) != self.num_stages:
            return False
        if not all(_static_stage_ok(h, a, s, c) for h, a, s, c in zip(self.bbox_head, self.bbox_assigner, self.bbox_sampler,
                                                                      self.train_cfg)):
            return False
        return all(h.reg_class_agnostic and h.bbox_coder.clip_border for h in list(self.bbox_head)[:-1])

    def forward_train_static(self, x, img_metas, proposals, n_keep, gt_bboxes, gt_labels):
        """forward_train on fixed-size tensors: proposals (B,P,5) zero-padded past n_keep (B,) [device].  Numerically the
        per-image path with the same samples; nothing is read back to the host."""
        from ..core.bbox import static_assign_and_sample
        losses = dict()
        dev = proposals.device
        boxes = proposals[..., :4]
        keep = arange_cached(proposals.size(1), dev)[None, :] < n_keep[:, None]
        lim = const_tensor([[m['img_shape'][1], m['img_shape'][0]] for m in img_metas], dev, torch.float32)
        feats = self._taps(x)
        trail = []
        for i in range(self.num_stages):
            self.current_stage = i
            head = self.bbox_head[i]
            S = static_assign_and_sample(self.bbox_assigner[i], self.bbox_sampler[i], boxes, keep, gt_bboxes, gt_labels)
            trail.append(S)
            rois = S.rois
            res = self._bbox_forward(i, feats, rois)
            self._add_stage_losses(losses, i, head.loss(res['cls_score'], res['bbox_pred'], rois, *static_targets(head, S),
                                                        num_samples=S.valid.sum()))
            if i < self.num_stages - 1:
                boxes, keep = static_refine(head, S, res['bbox_pred'], lim)
        self._last_static = tuple(trail)      # exposed for tests
        return losses

    # ------------------------------------------------------------------ test
    def simple_test_bboxes(self, x, proposal_list, img_metas, rescale=False, **kw):
        """cascade_roi_head.py:290-350 -> (det_bboxes list, det_labels list) on the device: the logits averaged over the stages,
        the last stage's deltas decoded on the boxes the stages before it refined.  kw: handed on to every _bbox_forward."""
        rois = bbox2roi(proposal_list)
        n_per = tuple(len(p) for p in proposal_list)
        batched = self._batched_test_ok(self.bbox_head, rois, img_metas, rescale)
        if batched:
            # every row carries its image's clip limits / scale: the same arithmetic as the per-image calls, one pass
            img_of, hw = self._row_limits(rois, img_metas)
        ms_scores = []
        for i in range(self.num_stages):
            res = self._bbox_forward(i, x, rois, **kw)
            ms_scores.append(res['cls_score'])
            if i < self.num_stages - 1:
                label = res['cls_score'][:, :-1].argmax(dim=1)
                if batched:
                    rois = self.bbox_head[i].regress_by_class(rois, label, res['bbox_pred'], dict(img_shape=hw))
                else:
                    rois = torch.cat([self.bbox_head[i].regress_by_class(r, l, p, m) for r, l, p, m in
                                      zip(rois.split(n_per), label.split(n_per), res['bbox_pred'].split(n_per), img_metas)])
        cls_score = sum(ms_scores[1:], ms_scores[0]) / float(len(ms_scores))
        head = self.bbox_head[-1]
        if batched:
            return self._get_bboxes_images(head, rois, cls_score, res['bbox_pred'], img_of, hw, img_metas, rescale)
        det_bboxes, det_labels = [], []
        for i, (r, c, p) in enumerate(zip(rois.split(n_per), cls_score.split(n_per), res['bbox_pred'].split(n_per))):
            b, l = head.get_bboxes(r, c, p, img_metas[i]['img_shape'], img_metas[i]['scale_factor'], rescale=rescale,
                                   cfg=self.test_cfg)
            det_bboxes.append(b)
            det_labels.append(l)
        return det_bboxes, det_labels

    def simple_test(self, x, proposal_list, img_metas, rescale=False):
        det_bboxes, det_labels = self.simple_test_bboxes(x, proposal_list, img_metas, rescale)
        return self._results(det_bboxes, det_labels, self.bbox_head[-1].num_classes)
