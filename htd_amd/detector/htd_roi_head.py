"""HTDRoIHead: the two-stage decoupled RoI head (driver of SFA, stage 1, BA and PGraph).

Reference: roi_heads/htd_roi_head.py:12-476 (+ base_roi_head.py:8-106).  Same registry name, kwargs,
sub-module names (bbox_roi_extractor.{0,1}, bbox_head.{0,1}, glbctx_head), loss keys
(loss_global, s0.loss_cls, s0.acc, s0.loss_bbox, s1.*) and return structures.

Deliberate fixes ('F'): stage-2 positives are taken from EVERY image of the batch
(the reference hard-codes image ids 0 and 1, :158-169,181-182 -- identical for B <= 2); `_fuse_global`
does not round-trip through the host.
"""
import os

import torch

from .. import mmcv_ops as M
from ..core import bbox2result, bbox2roi
from ..core.misc import arange_cached, const_tensor
from ..registry import HEADS, build_head
from .roi_heads import CascadeRoIHead, static_refine, static_targets


POS_BUCKET = max(1, int(os.environ.get('HTD_POS_BUCKET', '16')))    # stage-2 regression rows: multiples of this


@HEADS.register_module()
class HTDRoIHead(CascadeRoIHead):
    """A two-stage cascade whose second stage splits classification from regression (the latter on the positives only) and whose
    RoI features carry a global-context vector.  Construction, sampling, targets, refinement, the static-path gates and the
    whole-batch test post-processing are CascadeRoIHead's."""

    def __init__(self, num_stages, stage_loss_weights, with_global=False, **kwargs):
        super().__init__(num_stages, stage_loss_weights, **kwargs)
        self.with_global = with_global
        if with_global:
            self.glbctx_head = build_head(dict(type='GlobalContextHead', num_ins=5, num_convs=4, in_channels=256,
                                               conv_out_channels=256, num_classes=self.bbox_head[0].num_classes + 1,
                                               loss_weight=3.0))

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained)
        if self.with_global:
            self.glbctx_head.init_weights()

    def _fuse_global(self, roi_feats, global_feat, rois):
        assert roi_feats.size(0) == rois.size(0)
        return M.fuse_global(roi_feats, rois, global_feat)

    def _global(self, x, gt_labels=None):
        """-> (global feature or None, the dict of losses a train step starts from: loss_global when gt_labels are given)."""
        if not self.with_global:
            return None, dict()
        mc_pred, global_feat = self.glbctx_head(x)
        if gt_labels is None:
            return global_feat, dict()
        return global_feat, dict(loss_global=self.glbctx_head.loss(mc_pred, gt_labels))

    # ------------------------------------------------------------------ per-stage forward
    def _bbox_forward(self, stage, x, rois, global_feat=None, sampling_results=None):
        """x: the pyramid levels, or (training) a mmcv_ops.PyramidTaps over them -- the three RoIAlign consumers of a step
        (both extractors and BA) then share one gradient map per level instead of summing three."""
        extractor, enhanced_extractor = self.bbox_roi_extractor[0], self.bbox_roi_extractor[1]
        feats = x if isinstance(x, M.PyramidTaps) else x[:extractor.num_inputs]
        bbox_feats = extractor(feats, rois)
        if stage == 0:
            if self.with_global:
                bbox_feats = self._fuse_global(bbox_feats, global_feat, rois)
            cls_score, bbox_pred = self.bbox_head[0](bbox_feats)
            return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)
        head = self.bbox_head[stage]
        if sampling_results:
            # training: BA + reg branch on the positives only; rows of `rois` are [pos_i, neg_i] per image
            pos_rois = bbox2roi([res.pos_bboxes for res in sampling_results])
            pos_rows, start = [], 0
            for res in sampling_results:
                npos = res.pos_bboxes.size(0)
                pos_rows.append(torch.arange(start, start + npos, device=rois.device))
                start += npos + res.neg_bboxes.size(0)
            pos_rows = torch.cat(pos_rows)
            enhanced = enhanced_extractor(feats, pos_rois)
            pos_bbox_feat = torch.index_select(bbox_feats, 0, pos_rows)
            per_img = tuple(r.pos_bboxes.size(0) + r.neg_bboxes.size(0) for r in sampling_results)
            cls_score, bbox_pred = head(bbox_feats, pos_bbox_feat, feats, rois, self.bbox_head[0].fc_cls, enhanced,
                                        pos_rois, global_feat if self.with_global else None, rois_per_img=per_img)
            full = cls_score.new_zeros(cls_score.size(0), 4).index_put((pos_rows, ), bbox_pred)
            return dict(cls_score=cls_score, bbox_pred=full)
        enhanced = enhanced_extractor(feats, rois)
        cls_score, bbox_pred = head(bbox_feats, bbox_feats, feats, rois, self.bbox_head[0].fc_cls, enhanced, rois,
                                    global_feat if self.with_global else None)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred)

    def _bbox_forward_train(self, stage, x, rois, sampling_results, global_feat=None):
        return self._bbox_forward(stage, x, rois, global_feat, sampling_results)

    # ------------------------------------------------------------------ train
    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        global_feat, losses = self._global(x, gt_labels)
        losses.update(super().forward_train(x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore,
                                            global_feat=global_feat))
        return losses

    # ------------------------------------------------------------------ train, static shapes
    def forward_train_static(self, x, img_metas, proposals, n_keep, gt_bboxes, gt_labels):
        """forward_train (htd_roi_head.py:240-349) on fixed-size tensors: proposals (B,P,5) zero-padded past
        n_keep (B,) [device].  Numerically the per-image path with the same samples.  The only host read is the
        number of stage-2 positives, fetched asynchronously behind queued device work."""
        from ..core.bbox import static_assign_and_sample
        B, P = proposals.shape[:2]
        dev = proposals.device
        pvalid = arange_cached(P, dev)[None, :] < n_keep[:, None]
        S0 = static_assign_and_sample(self.bbox_assigner[0], self.bbox_sampler[0], proposals[..., :4], pvalid,
                                      gt_bboxes, gt_labels)
        global_feat, losses = self._global(x, gt_labels)
        # ---------------- stage 1: common head
        rois = S0.rois
        taps = self._taps(x)
        res = self._bbox_forward(0, taps, rois, global_feat)
        t0 = static_targets(self.bbox_head[0], S0)
        self._add_stage_losses(losses, 0, self.bbox_head[0].loss(res['cls_score'], res['bbox_pred'], rois, *t0,
                                                                 num_samples=S0.valid.sum()))
        lim = const_tensor([[m['img_shape'][1], m['img_shape'][0]] for m in img_metas], dev, torch.float32)
        boxes, keep = static_refine(self.bbox_head[0], S0, res['bbox_pred'], lim)
        # ---------------- stage 2: graph reasoning
        S1 = static_assign_and_sample(self.bbox_assigner[1], self.bbox_sampler[1], boxes, keep, gt_bboxes, gt_labels)
        rois = S1.rois
        n = S1.valid.size(1)
        extractor, enhanced_extractor = self.bbox_roi_extractor[0], self.bbox_roi_extractor[1]
        feats = taps if isinstance(taps, M.PyramidTaps) else x[:extractor.num_inputs]
        bbox_feats = extractor(feats, rois)
        # The regression branch runs on the positives only.  Their count is the one number of the step the host
        # needs: it is copied to pinned memory asynchronously now and read AFTER the classification branch has been
        # queued, so the device still has that work to do while the host waits for the copy (no idle gap), and the
        # host never waits for more than the sampling kernels.
        npos_host = torch.empty(B, dtype=S1.npos.dtype).pin_memory()
        npos_host.copy_(S1.npos, non_blocking=True)
        npos_ready = torch.cuda.Event()
        npos_ready.record()
        head = self.bbox_head[1]
        gf = global_feat if self.with_global else None
        # the positives' rows of bbox_feats are read after the classification branch is queued: through the alias that branch's
        # first node leaves in the stash, so that their gradient joins its sum in place (mmcv_ops.PlainAndFusedFunction)
        stash = M.RowStash() if (gf is not None and bbox_feats.is_cuda and torch.is_grad_enabled()) else None
        cls_score = head.forward_cls(bbox_feats, feats, rois, self.bbox_head[0].fc_cls, gf, rois_per_img=(n, ) * B,
                                     roi_valid=S1.valid.view(-1), row_stash=stash)
        t1 = static_targets(head, S1)             # needs no count: queued before the host stops for it
        full = cls_score.new_zeros(cls_score.size(0), 4)
        nvalid1 = S1.valid.sum()
        npos_ready.synchronize()
        npos = [int(v) for v in npos_host.tolist()]
        if sum(npos) > 0:
            # The count changes from step to step, and with it the size of every tensor of the regression branch: the caching
            # allocator then keeps a block per size it has seen (+277 MB of reserve per 500 steps with the optimizer
            # on).  The row list is therefore padded to a multiple of POS_BUCKET with slots that are NOT positives (the first
            # image's next slots: negatives or unused ones); their predictions land in rows whose regression weight is zero
            # (bbox_head.py:165-183), so losses and gradients are unchanged and the sizes repeat.
            take = list(npos)
            pad = (-sum(npos)) % POS_BUCKET
            for b in range(B):
                extra = min(pad, n - take[b])
                take[b] += extra
                pad -= extra
            pos_rows = torch.cat([torch.arange(b * n, b * n + k, device=dev) for b, k in enumerate(take)])
            pos_rois = torch.index_select(rois, 0, pos_rows)
            enhanced = enhanced_extractor(feats, pos_rois)
            pos_feats = M.select_rows_via(stash, pos_rows) if (stash is not None and stash.alias is not None) else \
                torch.index_select(bbox_feats, 0, pos_rows)
            bbox_pred = head.forward_reg(pos_feats, enhanced, pos_rois, gf)
            full = full.index_copy(0, pos_rows, bbox_pred)
        # no positive in the whole batch: the regression branch gets no gradient this step (zeros in the flat buffer)
        self._add_stage_losses(losses, 1, head.loss(cls_score, full, rois, *t1, num_samples=nvalid1))
        self._last_static = (S0, S1)          # exposed for tests
        return losses

    # ------------------------------------------------------------------ test
    def simple_test_bboxes(self, x, proposal_list, img_metas, rescale=False):
        """-> (det_bboxes list, det_labels list) on the device."""
        return super().simple_test_bboxes(x, proposal_list, img_metas, rescale, global_feat=self._global(x)[0])

    def aug_test(self, features, proposal_list, img_metas, rescale=False):
        """roi_heads/htd_roi_head.py:388-433: the merged proposals of one image go through both stages on every
        augmentation's pyramid; boxes are mapped back, averaged with the scores, and take ONE multi-class NMS.
        Like the reference, the result is in the original image scale whatever `rescale` says."""
        from ..core.bbox import bbox_mapping
        from ..core.post_processing import merge_aug_bboxes, multiclass_nms
        aug_bboxes, aug_scores = [], []
        for x, img_meta in zip(features, img_metas):
            m = img_meta[0]                                         # one image per batch in aug test
            proposals = bbox_mapping(proposal_list[0][:, :4], m['img_shape'], m['scale_factor'], m['flip'],
                                     m['flip_direction'])
            global_feat = self._global(x)[0]
            rois = bbox2roi([proposals])
            ms_scores = []
            for i in range(self.num_stages):
                res = self._bbox_forward(i, x, rois, global_feat)
                ms_scores.append(res['cls_score'])
                if i < self.num_stages - 1:
                    label = res['cls_score'][:, :-1].argmax(dim=1)
                    rois = self.bbox_head[i].regress_by_class(rois, label, res['bbox_pred'], m)
            cls_score = sum(ms_scores) / float(len(ms_scores))
            bboxes, scores = self.bbox_head[-1].get_bboxes(rois, cls_score, res['bbox_pred'], m['img_shape'],
                                                           m['scale_factor'], rescale=False, cfg=None)
            aug_bboxes.append(bboxes)
            aug_scores.append(scores)
        merged_bboxes, merged_scores = merge_aug_bboxes(aug_bboxes, aug_scores, img_metas, self.test_cfg)
        det_bboxes, det_labels = multiclass_nms(merged_bboxes, merged_scores, self.test_cfg.score_thr, self.test_cfg.nms,
                                                self.test_cfg.max_per_img)
        return [bbox2result(det_bboxes, det_labels, self.bbox_head[-1].num_classes)]
