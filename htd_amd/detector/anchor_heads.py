"""Anchor-based dense heads of single-stage detectors: AnchorHead, RetinaHead, ATSSHead and GFLHead (with its Integral layer).

Reference: dense_heads/anchor_head.py:14-682 (AnchorHead: forward, get_anchors, get_targets, loss, get_bboxes),
base_dense_head.py:22-59 (forward_train), retina_head.py:8-114 (RetinaHead), atss_head.py:15-650 (ATSSHead), gfl_head.py:15-632
(Integral, GFLHead).  Same registry names, constructor kwargs, state_dict keys (cls_convs / reg_convs / retina_cls / retina_reg;
atss_cls / atss_reg / atss_centerness / scales.N.scale; gfl_cls / gfl_reg / integral.project) and return structures.  AnchorHead is also the base of RPNHead
(detector/rpn_head.py), as in the reference: anchors, per-image targets (gt_labels None: foreground is class 0), the
reference-order loss are written once, here; forward_train, simple_test, the two convolution towers (`_build_towers`,
`_init_towers`, `_run_towers`), the fused losses' rule on the maps (`_fused_maps_ok`) and the cache of constants of the pyramid's
map shapes (`_shape_key` makes their key, `_cached` fetches them) come from BaseDenseHead (detector/base_dense_head.py), which the
anchor-free heads share: `_anchors_inside`, the RPN's proposal constants and the level-concatenated priors of `_get_bboxes` all go
through the two.

The anchors and their targets live in two mixins, so that the FCOS-shaped VFNetHead inherits them like the anchor heads do.
`AnchorTargets` (AnchorHead's first base) has `get_anchors`, `_anchors_inside`, the per-image routine `_anchor_targets_single`,
the batch routine `_anchor_targets` (both with the ATSS family's returns: the anchors first) and `_loss_targets`, the head of
every `loss_tensor`; its hooks are `_assign` (the assigner's call) and `_pos_bbox_targets`.  `ATSSTargets`, on top of it, is what
ATSSHead, GFLHead and VFNetHead add: ATSSAssigner's call with the per-level inside counts, `_atss_consts`, the assigner's half of
the fused-loss rule (`_atss_fused_ok`) and the head of their fused losses (`_atss_fused_targets`).  `get_targets` keeps the
reference's return structure in every class: six entries in AnchorHead, seven in ATSSHead and GFLHead.

`loss` has two forms, like RPNHead.loss.  The tensor form follows the reference's order of operations (per image targets, per
level losses) and works with any loss modules, `reg_decoded_bbox`, ignore boxes and on the CPU.  The fused form -- FocalLoss with
L1Loss / SmoothL1Loss, or GHMC with GHMR, on delta targets, no ignore boxes, fp32 GPU tensors -- assigns the whole batch against
the shared anchors (htd_max_iou_assign), counts the positives on the device (htd_retina_avg_factor) and takes both losses and
both gradients of all levels in one launch (htd_retina_loss; htd_ghm_head_loss is three: histogram, weights, loss) that reads
the convolution outputs where they are: no labels / label_weights /
bbox_targets / bbox_weights tensors, no permute or concatenation of the logits, no host read.

`get_bboxes` of RetinaHead, ATSSHead and GFLHead is BaseDenseHead._get_bboxes (the dispatch, the per-image loop and the batched
form, written once for all dense heads); a head gives its priors (`_bbox_priors`: the anchors, GFLHead their centres) and its
decode (`_bbox_decode`), ATSSHead passes its centerness maps as score factors and GFLHead takes keys and distances from its one
htd_gfl_decode launch (`_keys_and_preds`).
"""
import os

import torch
import torch.nn as nn

from ..core import anchor_inside_flags, images_to_levels, multi_apply, reduce_mean, unmap
from ..core.misc import const_tensor
from .. import mmcv_ops as M
from ..registry import HEADS, build_anchor_generator, build_assigner, build_bbox_coder, build_loss, build_sampler
from .base_dense_head import BaseDenseHead
from .bricks import Conv2d, normal_init
from .losses import GHM_KERNEL_BINS, GHMC, GHMR

RETINA_FUSED = os.environ.get('HTD_RETINA_FUSED', '1') != '0'       # 0: the tensor-path loss (A/B runs)
ATSS_FUSED = os.environ.get('HTD_ATSS_FUSED', '1') != '0'           # the same switch for ATSSHead
ATSS_EPS = 1e-12                                                    # atss_head.py:12
GFL_FUSED = os.environ.get('HTD_GFL_FUSED', '1') != '0'             # the same switch for GFLHead


def bias_init_with_prob(prior_prob):
    """mmcv.cnn.bias_init_with_prob: the bias that makes sigmoid(bias) = prior_prob."""
    import math
    return float(-math.log((1 - prior_prob) / prior_prob))


class AnchorTargets:
    """The anchors of a pyramid and their per-image targets (anchor_head.py:142-371, atss_head.py:471-643), for any head with
    an `anchor_generator`, `assigner`, `sampler`, `train_cfg`, `num_classes`, `cls_out_channels` and `use_sigmoid_cls`: AnchorHead
    and, through ATSSTargets, the FCOS-shaped VFNetHead.  Two hooks: `_assign` and `_pos_bbox_targets`."""

    def get_anchors(self, featmap_sizes, img_metas, device='cuda'):
        mlvl = self.anchor_generator.grid_anchors(featmap_sizes, device)
        anchor_list = [mlvl for _ in img_metas]
        valid_flag_list = [self.anchor_generator.valid_flags(featmap_sizes, m['pad_shape'], device) for m in img_metas]
        return anchor_list, valid_flag_list

    def _anchors_inside(self, featmap_sizes, img_metas, dev):
        """(A, 4) level-concatenated anchors and the (B, A) mask of anchors that are valid and inside their image
        (anchor_head.py:200-207, core/anchor/utils.py:20-46): constants of (feature-map sizes, image shapes), cached under
        exactly those."""
        border = self.train_cfg.allowed_border

        def make():
            anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=dev)
            flat_anchors = torch.cat(anchor_list[0])
            valid = torch.stack([torch.cat(v) for v in valid_flag_list])
            if border >= 0:
                lim = const_tensor([[m['img_shape'][1], m['img_shape'][0]] for m in img_metas], dev, flat_anchors.dtype)
                valid = valid & (flat_anchors[None, :, 0] >= -border) & (flat_anchors[None, :, 1] >= -border) & \
                    (flat_anchors[None, :, 2] < lim[:, 0:1] + border) & (flat_anchors[None, :, 3] < lim[:, 1:2] + border)
            return flat_anchors, valid
        key = (self._shape_key(featmap_sizes), tuple((tuple(m['img_shape'][:2]), tuple(m['pad_shape'][:2])) for m in img_metas),
               str(dev), border)
        return self._cached('_inside_cache', 64, key, make)

    def _assign(self, anchors, num_level_anchors, inside, gt_bboxes, gt_bboxes_ignore, gt_labels):
        """MaxIoUAssigner and its kin; a sampling head assigns without labels (anchor_head.py:209-211)."""
        return self.assigner.assign(anchors, gt_bboxes, gt_bboxes_ignore, None if self.sampling else gt_labels)

    def _pos_bbox_targets(self, sr):
        """The regression targets of the positives of a sampling result: the coder's deltas, the gt boxes under
        reg_decoded_bbox (GFLHead and VFNetHead: always the gt boxes)."""
        return sr.pos_gt_bboxes if self.reg_decoded_bbox else self.bbox_coder.encode(sr.pos_bboxes, sr.pos_gt_bboxes)

    def _anchor_targets_single(self, flat_anchors, valid_flags, num_level_anchors, gt_bboxes, gt_bboxes_ignore, gt_labels,
                               img_meta, label_channels=1, unmap_outputs=True):
        """anchor_head.py:172-269 and atss_head.py:535-643 (gfl_head.py:521-625) for one image -> (anchors, labels,
        label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds).  Only the RPN gives gt_labels as None: foreground is
        class 0."""
        inside = anchor_inside_flags(flat_anchors, valid_flags, img_meta['img_shape'][:2], self.train_cfg.allowed_border)
        if not inside.any():
            return (None, ) * 7
        anchors = flat_anchors[inside, :]
        assign_result = self._assign(anchors, num_level_anchors, inside, gt_bboxes, gt_bboxes_ignore, gt_labels)
        sr = self.sampler.sample(assign_result, anchors, gt_bboxes)
        n = anchors.shape[0]
        bbox_targets = torch.zeros_like(anchors)
        bbox_weights = torch.zeros_like(anchors)
        labels = anchors.new_full((n, ), self.num_classes, dtype=torch.long)
        label_weights = anchors.new_zeros(n, dtype=torch.float)
        pos_inds, neg_inds = sr.pos_inds, sr.neg_inds
        if len(pos_inds) > 0:
            bbox_targets[pos_inds, :] = self._pos_bbox_targets(sr)
            bbox_weights[pos_inds, :] = 1.0
            labels[pos_inds] = 0 if gt_labels is None else gt_labels[sr.pos_assigned_gt_inds]
            label_weights[pos_inds] = 1.0 if self.train_cfg.pos_weight <= 0 else self.train_cfg.pos_weight
        if len(neg_inds) > 0:
            label_weights[neg_inds] = 1.0
        if unmap_outputs:
            total = flat_anchors.size(0)
            anchors = unmap(anchors, total, inside)
            labels = unmap(labels, total, inside, fill=self.num_classes)
            label_weights = unmap(label_weights, total, inside)
            bbox_targets = unmap(bbox_targets, total, inside)
            bbox_weights = unmap(bbox_weights, total, inside)
        return anchors, labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds

    def _anchor_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list=None,
                        gt_labels_list=None, label_channels=1, unmap_outputs=True):
        """anchor_head.py:271-371 and atss_head.py:471-533 -> (anchors, labels, label_weights, bbox_targets, bbox_weights per
        level, num_total_pos, num_total_neg), or None when an image has no anchor inside."""
        num_imgs = len(img_metas)
        assert len(anchor_list) == len(valid_flag_list) == num_imgs
        num_level_anchors = [a.size(0) for a in anchor_list[0]]
        concat_anchors = [torch.cat(a) for a in anchor_list]
        concat_valid = [torch.cat(v) for v in valid_flag_list]
        if gt_bboxes_ignore_list is None:
            gt_bboxes_ignore_list = [None] * num_imgs
        if gt_labels_list is None:
            gt_labels_list = [None] * num_imgs
        res = [self._anchor_targets_single(concat_anchors[i], concat_valid[i], num_level_anchors, gt_bboxes_list[i],
                                           gt_bboxes_ignore_list[i], gt_labels_list[i], img_metas[i], label_channels,
                                           unmap_outputs) for i in range(num_imgs)]
        if any(r[0] is None for r in res):
            return None
        num_total_pos = sum(max(r[5].numel(), 1) for r in res)
        num_total_neg = sum(max(r[6].numel(), 1) for r in res)
        lv = [images_to_levels([r[k] for r in res], num_level_anchors) for k in range(5)]
        return lv[0], lv[1], lv[2], lv[3], lv[4], num_total_pos, num_total_neg

    def _loss_targets(self, cls_scores, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore):
        """The head of every tensor-form loss (anchor_head.py:450-466): the anchors of the maps and the targets of the batch
        -> (anchor_list, what `_anchor_targets` returns)."""
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=cls_scores[0].device)
        label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
        return anchor_list, self._anchor_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas,
                                                 gt_bboxes_ignore_list=gt_bboxes_ignore, gt_labels_list=gt_labels,
                                                 label_channels=label_channels)


class ATSSTargets(AnchorTargets):
    """What ATSSHead, GFLHead and VFNetHead share beyond AnchorTargets: ATSSAssigner's call, the constants, the assigner's half
    of the fused-loss rule and the head of the fused loss (htd_atss_targets)."""

    def get_num_level_anchors_inside(self, num_level_anchors, inside_flags):
        return [int(flags.sum()) for flags in torch.split(inside_flags, num_level_anchors)]

    def _assign(self, anchors, num_level_anchors, inside, gt_bboxes, gt_bboxes_ignore, gt_labels):
        return self.assigner.assign(anchors, self.get_num_level_anchors_inside(num_level_anchors, inside), gt_bboxes,
                                    gt_bboxes_ignore, gt_labels)

    def _get_target_single(self, *args, **kwargs):
        """The per-image routine under the reference's name (atss_head.py:535, gfl_head.py:521)."""
        return self._anchor_targets_single(*args, **kwargs)

    def get_targets(self, *args, **kwargs):
        """atss_head.py:471-533, gfl_head.py:455-519 -> (anchors, labels, label_weights, bbox_targets, bbox_weights per level,
        num_total_pos, num_total_neg)."""
        return self._anchor_targets(*args, **kwargs)

    def _atss_consts(self, featmap_sizes, img_metas, dev):
        """-> (A, 4) level-concatenated anchors and whether every anchor of every image is valid and inside (a host bool, read
        once per (map sizes, image shapes))."""
        def make():
            flat_anchors, inside = self._anchors_inside(featmap_sizes, img_metas, dev)
            return flat_anchors.float().contiguous(), bool(inside.all())
        key = (self._shape_key(featmap_sizes), tuple((tuple(m['img_shape'][:2]), tuple(m['pad_shape'][:2])) for m in img_metas),
               str(dev), self.train_cfg.allowed_border)
        return self._cached('_atss_cache', 64, key, make)

    def _atss_fused_ok(self, cls_scores, gt_labels, gt_bboxes_ignore, img_metas):
        """htd_atss_targets covers one anchor per location (several tie in distance), ATSSAssigner with topk <= 16 and no ignore
        threshold, no ignore boxes, label weight 1 on positives (pos_weight <= 0: the kernels have no other) and -- last, a host
        read on a cache miss -- every anchor valid and inside."""
        a = getattr(self, 'assigner', None)
        return gt_labels is not None and gt_bboxes_ignore is None and self.num_anchors == 1 and \
            type(a).__name__ == 'ATSSAssigner' and a.ignore_iof_thr <= 0 and a.topk <= 16 and self.train_cfg.pos_weight <= 0 and \
            self._atss_consts([f.size()[-2:] for f in cls_scores], img_metas, cls_scores[0].device)[1]

    def _atss_fused_targets(self, cls_scores, gt_bboxes, gt_labels, img_metas, means_stds=(), reduce_norm=True):
        """The head of every fused ATSS-family loss: the batch assigned in one launch, nothing read back -> flat anchors, padded
        gts and labels, assigned, ctr_targets (of the coder given by `means_stds`: ATSSHead alone), num_pos, norm."""
        import torch.distributed as dist
        from ..core.bbox import pad_gt_batch
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        flat_anchors, _ = self._atss_consts(featmap_sizes, img_metas, cls_scores[0].device)
        gts, gt_valid, labels = pad_gt_batch(gt_bboxes, gt_labels)
        assigned, ctr_targets, num_pos, norm = M.atss_targets(flat_anchors, [int(h * w) for h, w in featmap_sizes], gts, gt_valid,
                                                              self.assigner.topk, *means_stds)
        if reduce_norm and dist.is_available() and dist.is_initialized():
            # atss_head.py:271-273,288, gfl_head.py:347-350: both factors averaged over the processes, the sample count at least 1
            norm = reduce_mean(norm)
            norm = torch.cat([norm[:2].clamp(min=1.0), norm[2:]])
        return flat_anchors, gts, labels, assigned, ctr_targets, num_pos, norm


@HEADS.register_module()
class AnchorHead(AnchorTargets, BaseDenseHead):
    def __init__(self, num_classes, in_channels, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', scales=[8, 16, 32], ratios=[0.5, 1.0, 2.0],
                                       strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True, target_means=(.0, .0, .0, .0),
                                 target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False,
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), train_cfg=None, test_cfg=None):
        super().__init__()
        self.in_channels, self.num_classes, self.feat_channels = in_channels, num_classes, feat_channels
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.sampling = loss_cls['type'] not in ['FocalLoss', 'GHMC', 'QualityFocalLoss']       # anchor_head.py:60-66
        self.cls_out_channels = num_classes if self.use_sigmoid_cls else num_classes + 1
        if self.cls_out_channels <= 0:
            raise ValueError(f'num_classes={num_classes} is too small')
        self.reg_decoded_bbox = reg_decoded_bbox
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        if self.train_cfg:
            self.assigner = build_assigner(self.train_cfg.assigner)
            if self.sampling and hasattr(self.train_cfg, 'sampler'):
                sampler_cfg = self.train_cfg.sampler
            else:
                sampler_cfg = dict(type='PseudoSampler')
            self.sampler = build_sampler(sampler_cfg, context=self)
        self.fp16_enabled = False
        self.anchor_generator = build_anchor_generator(anchor_generator)
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        self._init_layers()

    def _init_layers(self):
        self.conv_cls = Conv2d(self.in_channels, self.num_anchors * self.cls_out_channels, 1)
        self.conv_reg = Conv2d(self.in_channels, self.num_anchors * 4, 1)

    def init_weights(self):
        normal_init(self.conv_cls, std=0.01)
        normal_init(self.conv_reg, std=0.01)

    # ------------------------------------------------------------------ forward
    def forward_single(self, x):
        return self.conv_cls(x), self.conv_reg(x)

    def forward(self, feats):
        return multi_apply(self.forward_single, feats)

    # ------------------------------------------------------------------ targets
    def get_targets(self, *args, **kwargs):
        """anchor_head.py:271-371 -> (labels, label_weights, bbox_targets, bbox_weights per level, num_total_pos,
        num_total_neg): `_anchor_targets` without the anchors."""
        targets = self._anchor_targets(*args, **kwargs)
        return None if targets is None else targets[1:]

    # ------------------------------------------------------------------ loss
    def loss_single(self, cls_score, bbox_pred, anchors, labels, label_weights, bbox_targets, bbox_weights, num_total_samples):
        """anchor_head.py:373-418."""
        labels = labels.reshape(-1)
        label_weights = label_weights.reshape(-1)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
        loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples)
        bbox_targets = bbox_targets.reshape(-1, 4)
        bbox_weights = bbox_weights.reshape(-1, 4)
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4)
        if self.reg_decoded_bbox:
            bbox_pred = self.bbox_coder.decode(anchors.reshape(-1, 4), bbox_pred)
        loss_bbox = self.loss_bbox(bbox_pred, bbox_targets, bbox_weights, avg_factor=num_total_samples)
        return loss_cls, loss_bbox

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        if self._fused_loss_ok(cls_scores, bbox_preds, gt_bboxes, gt_labels, gt_bboxes_ignore):
            return self.loss_fused(cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas)
        return self.loss_tensor(cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)

    def loss_tensor(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """anchor_head.py:420-488, in the reference's order of operations."""
        anchor_list, targets = self._loss_targets(cls_scores, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        if targets is None:
            return None
        _, labels, label_weights, bbox_targets, bbox_weights, num_total_pos, num_total_neg = targets
        num_total_samples = num_total_pos + num_total_neg if self.sampling else num_total_pos
        num_level_anchors = [a.size(0) for a in anchor_list[0]]
        all_anchors = images_to_levels([torch.cat(a) for a in anchor_list], num_level_anchors)
        losses_cls, losses_bbox = multi_apply(self.loss_single, cls_scores, bbox_preds, all_anchors, labels, label_weights,
                                              bbox_targets, bbox_weights, num_total_samples=num_total_samples)
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox)

    def _fused_loss_ok(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, gt_bboxes_ignore):
        """htd_retina_loss covers FocalLoss + L1Loss / SmoothL1Loss on delta targets without ignore boxes, fp32 on the GPU;
        htd_ghm_head_loss covers GHMC + GHMR (at most 64 bins each) under the same conditions.  Any other pair, mixed ones such
        as GHMC + L1Loss included, takes the tensor path."""
        lc, lb = self.loss_cls, self.loss_bbox
        a = getattr(self, 'assigner', None)
        focal = type(lc).__name__ == 'FocalLoss' and lc.reduction == 'mean' and \
            type(lb).__name__ in ('SmoothL1Loss', 'L1Loss') and lb.reduction == 'mean'
        return getattr(self, 'fused_loss', RETINA_FUSED) and gt_labels is not None and gt_bboxes_ignore is None and \
            (focal or self._ghm_pair()) and not self.reg_decoded_bbox and \
            type(a).__name__ == 'MaxIoUAssigner' and a.ignore_iof_thr <= 0 and isinstance(a.neg_iou_thr, float) and \
            (a.gt_max_assign_all or not a.match_low_quality) and self._fused_maps_ok(cls_scores, bbox_preds)

    def _ghm_pair(self):
        lc, lb = self.loss_cls, self.loss_bbox
        return type(lc) is GHMC and type(lb) is GHMR and lc.bins <= GHM_KERNEL_BINS and lb.bins <= GHM_KERNEL_BINS and \
            lc.edges.is_cuda and lb.edges.is_cuda

    def loss_fused(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas):
        from ..core.bbox import batched_max_iou_assign, pad_gt_batch
        dev = cls_scores[0].device
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        flat_anchors, inside = self._anchors_inside(featmap_sizes, img_metas, dev)
        gts, gt_valid, labels = pad_gt_batch(gt_bboxes, gt_labels)
        assigned, _ = batched_max_iou_assign(self.assigner, flat_anchors, inside, gts, gt_valid)
        if self._ghm_pair():
            # GHM takes its own normalisers (per level: the valid elements, the weight sum): no avg_factor
            self._last_assigned = (assigned, None, None)
            loss_cls, loss_bbox = M.ghm_head_loss(
                cls_scores, bbox_preds, self.num_anchors, self.cls_out_channels, flat_anchors, gts, labels, assigned,
                tuple(self.bbox_coder.means), tuple(self.bbox_coder.stds), self.loss_cls, self.loss_bbox)
            return dict(loss_cls=[loss_cls], loss_bbox=[loss_bbox])
        num_pos, avg = M.retina_avg_factor(assigned)
        self._last_assigned = (assigned, num_pos, avg)          # exposed for tests
        lb = self.loss_bbox
        l1 = type(lb).__name__ == 'L1Loss'
        loss_cls, loss_bbox = M.retina_loss(
            cls_scores, bbox_preds, self.num_anchors, self.cls_out_channels, flat_anchors, gts, labels, assigned, avg,
            tuple(self.bbox_coder.means), tuple(self.bbox_coder.stds), self.loss_cls.gamma, self.loss_cls.alpha,
            self.train_cfg.pos_weight, 1 if l1 else 0, 0.0 if l1 else lb.beta, self.loss_cls.loss_weight, lb.loss_weight)
        return dict(loss_cls=[loss_cls], loss_bbox=[loss_bbox])

    # ------------------------------------------------------------------ boxes
    @property
    def strides(self):
        return self.anchor_generator.strides

    def _bbox_priors(self, featmap_sizes, dtype, device):
        return self.anchor_generator.grid_anchors(featmap_sizes, device=device)

    def _bbox_decode(self, anchors, deltas, img_shape):
        return self.bbox_coder.decode(anchors, deltas, max_shape=img_shape)

    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True):
        """anchor_head.py:490-664 -> list (per image) of (dets (k, 5), labels (k,)): BaseDenseHead._get_bboxes with the anchors
        as priors and the coder's decode.  Softmax heads take the per-image loop."""
        return self._get_bboxes(cls_scores, bbox_preds, None, img_metas, cfg, rescale, with_nms)


@HEADS.register_module()
class RetinaHead(AnchorHead):
    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None, norm_cfg=None,
                 anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4, scales_per_octave=3, ratios=[0.5, 1.0, 2.0],
                                       strides=[8, 16, 32, 64, 128]), **kwargs):
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        super().__init__(num_classes, in_channels, anchor_generator=anchor_generator, **kwargs)

    def _init_layers(self):
        self.relu = nn.ReLU(inplace=True)
        self._build_towers('cls_convs', 'reg_convs', interleaved=True)
        self.retina_cls = Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.retina_reg = Conv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)

    def init_weights(self):
        self._init_towers()
        normal_init(self.retina_cls, std=0.01, bias=bias_init_with_prob(0.01))
        normal_init(self.retina_reg, std=0.01)

    def forward_single(self, x):
        cls_feat, reg_feat = self._run_towers(x)
        return self.retina_cls(cls_feat), self.retina_reg(reg_feat)


@HEADS.register_module()
class ATSSHead(ATSSTargets, AnchorHead):
    """dense_heads/atss_head.py:15-650: the towers of RetinaHead under GroupNorm, a centerness branch on the regression tower,
    one learnable scale per level, ATSSAssigner in place of MaxIoUAssigner and a centerness-weighted IoU-family box loss on
    decoded boxes.

    `loss` has two forms, like AnchorHead.loss, and `_fused_loss_ok` is the one rule between them.  `loss_tensor` is the
    reference's order of operations (get_targets / _get_target_single on the inside-flag subset, loss_single per level, the two
    averaging factors through reduce_mean) and works on the CPU, in fp64, with several anchors per location and with ignore
    boxes.  `loss_fused` assigns the whole batch and leaves the centerness targets and the averaging factors on the device
    (htd_atss_targets), and takes the three losses and the three gradient maps of all levels in one more launch (htd_atss_loss)
    that reads the maps where they are: no permute, concatenation or gather of the predictions, no nonzero(), no host read.

    `get_bboxes` is BaseDenseHead._get_bboxes with the anchors as priors, the coder's decode and the centerness as score factor."""

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), **kwargs):
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        super().__init__(num_classes, in_channels, **kwargs)
        self.sampling = False
        if self.train_cfg:
            self.assigner = build_assigner(self.train_cfg.assigner)
            self.sampler = build_sampler(dict(type='PseudoSampler'), context=self)
        self.loss_centerness = build_loss(loss_centerness)

    def _init_layers(self):
        from .anchor_free_heads import Scale
        self.relu = nn.ReLU(inplace=True)
        self._build_towers('cls_convs', 'reg_convs', interleaved=True)
        self.atss_cls = Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.atss_reg = Conv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)
        self.atss_centerness = Conv2d(self.feat_channels, self.num_anchors * 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.anchor_generator.strides])

    def init_weights(self):
        self._init_towers()
        normal_init(self.atss_cls, std=0.01, bias=bias_init_with_prob(0.01))
        normal_init(self.atss_reg, std=0.01)
        normal_init(self.atss_centerness, std=0.01)

    # ------------------------------------------------------------------ forward
    def forward(self, feats):
        return multi_apply(self.forward_single, feats, self.scales)

    def forward_single(self, x, scale):
        """atss_head.py:116-143 -> cls_score, bbox_pred (scaled, no exp), centerness (on the regression tower)."""
        cls_feat, reg_feat = self._run_towers(x)
        return self.atss_cls(cls_feat), scale(self.atss_reg(reg_feat)).float(), self.atss_centerness(reg_feat)

    # ------------------------------------------------------------------ targets
    def centerness_target(self, anchors, bbox_targets):
        """atss_head.py:297-313 (positives only: elsewhere there may be NaN)."""
        gts = self.bbox_coder.decode(anchors, bbox_targets)
        anchors_cx, anchors_cy = (anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2
        left_right = torch.stack([anchors_cx - gts[:, 0], gts[:, 2] - anchors_cx], dim=1)
        top_bottom = torch.stack([anchors_cy - gts[:, 1], gts[:, 3] - anchors_cy], dim=1)
        return torch.sqrt((left_right.min(dim=-1)[0] / left_right.max(dim=-1)[0]) *
                          (top_bottom.min(dim=-1)[0] / top_bottom.max(dim=-1)[0]))

    def _pos_bbox_targets(self, sr):
        """The coder's deltas, whatever reg_decoded_bbox says (atss_head.py:606-611): centerness_target decodes them."""
        return self.bbox_coder.encode(sr.pos_bboxes, sr.pos_gt_bboxes)

    # ------------------------------------------------------------------ loss
    def loss_single(self, anchors, cls_score, bbox_pred, centerness, labels, label_weights, bbox_targets, num_total_samples):
        """atss_head.py:145-218."""
        anchors = anchors.reshape(-1, 4)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels).contiguous()
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4)
        centerness = centerness.permute(0, 2, 3, 1).reshape(-1)
        bbox_targets = bbox_targets.reshape(-1, 4)
        labels = labels.reshape(-1)
        label_weights = label_weights.reshape(-1)
        loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples)
        pos_inds = ((labels >= 0) & (labels < self.num_classes)).nonzero().squeeze(1)
        if len(pos_inds) > 0:
            pos_bbox_targets, pos_bbox_pred = bbox_targets[pos_inds], bbox_pred[pos_inds]
            pos_anchors, pos_centerness = anchors[pos_inds], centerness[pos_inds]
            centerness_targets = self.centerness_target(pos_anchors, pos_bbox_targets)
            loss_bbox = self.loss_bbox(self.bbox_coder.decode(pos_anchors, pos_bbox_pred),
                                       self.bbox_coder.decode(pos_anchors, pos_bbox_targets), weight=centerness_targets,
                                       avg_factor=1.0)
            loss_centerness = self.loss_centerness(pos_centerness, centerness_targets, avg_factor=num_total_samples)
        else:
            loss_bbox = bbox_pred.sum() * 0
            loss_centerness = centerness.sum() * 0
            centerness_targets = bbox_targets.new_tensor(0.)
        return loss_cls, loss_bbox, loss_centerness, centerness_targets.sum()

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        if self._fused_loss_ok(cls_scores, bbox_preds, centernesses, gt_labels, gt_bboxes_ignore, img_metas):
            return self.loss_fused(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas)
        return self.loss_tensor(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)

    def loss_tensor(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """atss_head.py:220-295, in the reference's order of operations."""
        _, targets = self._loss_targets(cls_scores, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        if targets is None:
            return None
        anchors, labels, label_weights, bbox_targets, _, num_total_pos, _ = targets
        num_total_samples = float(reduce_mean(torch.tensor(float(num_total_pos), device=cls_scores[0].device)))
        num_total_samples = max(num_total_samples, 1.0)
        losses_cls, losses_bbox, loss_centerness, bbox_avg_factor = multi_apply(
            self.loss_single, anchors, cls_scores, bbox_preds, centernesses, labels, label_weights, bbox_targets,
            num_total_samples=num_total_samples)
        bbox_avg_factor = float(reduce_mean(sum(bbox_avg_factor)))
        if bbox_avg_factor < ATSS_EPS:
            bbox_avg_factor = 1
        losses_bbox = [x / bbox_avg_factor for x in losses_bbox]
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox, loss_centerness=loss_centerness)

    def _fused_loss_ok(self, cls_scores, bbox_preds, centernesses, gt_labels, gt_bboxes_ignore, img_metas):
        """htd_atss_targets / htd_atss_loss cover sigmoid FocalLoss + IoULoss / GIoULoss + sigmoid CrossEntropyLoss without class
        weight, all with mean reduction, and a DeltaXYWHBBoxCoder, on maps that `_fused_maps_ok` takes, under the assigner's
        conditions (`_atss_fused_ok`)."""
        lc, lb, lt = self.loss_cls, self.loss_bbox, self.loss_centerness
        return getattr(self, 'fused_loss', ATSS_FUSED) and \
            type(lc).__name__ == 'FocalLoss' and lc.use_sigmoid and lc.reduction == 'mean' and \
            type(lb).__name__ in M.FCOS_BOX_KINDS and lb.reduction == 'mean' and \
            type(lt).__name__ == 'CrossEntropyLoss' and lt.use_sigmoid and lt.reduction == 'mean' and lt.class_weight is None and \
            type(self.bbox_coder).__name__ == 'DeltaXYWHBBoxCoder' and not self.reg_decoded_bbox and \
            self._fused_maps_ok(cls_scores, bbox_preds, centernesses) and \
            self._atss_fused_ok(cls_scores, gt_labels, gt_bboxes_ignore, img_metas)

    def loss_fused(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas):
        means, stds = tuple(self.bbox_coder.means), tuple(self.bbox_coder.stds)
        flat_anchors, gts, labels, assigned, ctr_targets, num_pos, norm = self._atss_fused_targets(
            cls_scores, gt_bboxes, gt_labels, img_metas, (means, stds))
        self._last_targets = (assigned, ctr_targets, num_pos, norm)            # exposed for tests
        lc, lb = self.loss_cls, self.loss_bbox
        loss_cls, loss_bbox, loss_centerness = M.atss_loss(
            cls_scores, bbox_preds, centernesses, self.anchor_generator.strides, flat_anchors, gts, labels, assigned, ctr_targets,
            norm, means, stds, M.FCOS_BOX_KINDS[type(lb).__name__], lb.eps, lc.gamma, lc.alpha, lc.loss_weight, lb.loss_weight,
            self.loss_centerness.loss_weight)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness)

    # ------------------------------------------------------------------ boxes
    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg=None, rescale=False, with_nms=True):
        """atss_head.py:316-469 -> list (per image) of (dets (k, 5), labels (k,)), the centerness as score factor of the ranking
        and of the NMS.  Several anchors per location take the per-image loop with the reference's own tensor operations."""
        return self._get_bboxes(cls_scores, bbox_preds, centernesses, img_metas, cfg, rescale, with_nms)


class Integral(nn.Module):
    """gfl_head.py:15-48: the expectation sum_i P(y_i) y_i of the discrete distribution over {0, 1, ..., reg_max} that a softmax
    of each side's reg_max + 1 logits gives: (N, 4 * (reg_max + 1)) -> (N, 4).  `project` is part of the state dict."""

    def __init__(self, reg_max=16):
        super().__init__()
        self.reg_max = reg_max
        self.register_buffer('project', torch.linspace(0, self.reg_max, self.reg_max + 1))

    def forward(self, x):
        x = torch.softmax(x.reshape(-1, self.reg_max + 1), dim=1)
        return torch.nn.functional.linear(x, self.project.type_as(x)).reshape(-1, 4)


@HEADS.register_module()
class GFLHead(ATSSTargets, AnchorHead):
    """dense_heads/gfl_head.py:51-632: ATSSHead's towers, assigner and one-anchor pyramid with a joint class / quality score
    under QualityFocalLoss in place of the centerness branch, and a discrete distribution of reg_max + 1 bins per side under
    DistributionFocalLoss, plus an IoU-family loss on its integral, in place of the four deltas.  The targets are the gt boxes.

    `loss` has two forms, like ATSSHead.loss, and `_fused_loss_ok` is the one rule between them.  `loss_tensor` is the reference's
    order of operations and works on the CPU, in fp64 and with ignore boxes.  `loss_fused` assigns the batch with
    htd_atss_targets, takes the weights, the IoU scores and their sum in one pass (htd_gfl_quality) and the three losses with
    both gradient maps of all levels in one more launch (htd_gfl_loss): no permute, concatenation, gather or nonzero() of the
    predictions, no host read.

    Two pieces of reference behaviour are kept in both forms.  The averaging factor of the box and DFL losses (the sum of the
    positives' weights, gfl_head.py:364-367) is not clamped: a batch without a positive gives loss_bbox = loss_dfl = 0 / 0 = NaN
    and a NaN regression gradient beside a finite loss_cls.  And the DFL targets are clamped to [0, reg_max - 0.1]
    (bbox2distance's max_dis and eps) before `label.long()` splits them into bins."""

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25), reg_max=16, **kwargs):
        self.stacked_convs, self.conv_cfg, self.norm_cfg, self.reg_max = stacked_convs, conv_cfg, norm_cfg, reg_max
        super().__init__(num_classes, in_channels, **kwargs)
        self.sampling = False
        if self.train_cfg:
            self.assigner = build_assigner(self.train_cfg.assigner)
            self.sampler = build_sampler(dict(type='PseudoSampler'), context=self)
        self.integral = Integral(self.reg_max)
        self.loss_dfl = build_loss(loss_dfl)

    def _init_layers(self):
        from .anchor_free_heads import Scale
        self.relu = nn.ReLU(inplace=True)
        self._build_towers('cls_convs', 'reg_convs', interleaved=True)
        assert self.num_anchors == 1, 'anchor free version'
        self.gfl_cls = Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)
        self.gfl_reg = Conv2d(self.feat_channels, 4 * (self.reg_max + 1), 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.anchor_generator.strides])

    def init_weights(self):
        self._init_towers()
        normal_init(self.gfl_cls, std=0.01, bias=bias_init_with_prob(0.01))
        normal_init(self.gfl_reg, std=0.01)

    # ------------------------------------------------------------------ forward
    def forward(self, feats):
        return multi_apply(self.forward_single, feats, self.scales)

    def forward_single(self, x, scale):
        """gfl_head.py:170-194 -> cls_score (class / quality logits), bbox_pred (scaled distribution logits)."""
        cls_feat, reg_feat = self._run_towers(x)
        return self.gfl_cls(cls_feat), scale(self.gfl_reg(reg_feat)).float()

    def anchor_center(self, anchors):
        """gfl_head.py:196-207: (N, 4) anchors -> (N, 2) centres."""
        return torch.stack([(anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2], dim=-1)

    # ------------------------------------------------------------------ targets (ATSSTargets', with the gt boxes as targets)
    def _pos_bbox_targets(self, sr):
        return sr.pos_gt_bboxes

    # ------------------------------------------------------------------ loss
    def loss_single(self, anchors, cls_score, bbox_pred, labels, label_weights, bbox_targets, stride, num_total_samples):
        """gfl_head.py:209-295."""
        from ..core.bbox import bbox2distance, bbox_overlaps, distance2bbox
        assert stride[0] == stride[1], 'h stride is not equal to w stride!'
        anchors = anchors.reshape(-1, 4)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4 * (self.reg_max + 1))
        bbox_targets = bbox_targets.reshape(-1, 4)
        labels = labels.reshape(-1)
        label_weights = label_weights.reshape(-1)
        pos_inds = ((labels >= 0) & (labels < self.num_classes)).nonzero().squeeze(1)
        # in the dtype of the logits (the reference takes label_weights' fp32, the same wherever it runs): an fp64 run keeps its
        # fp64 IoU scores, as the fixture's fp64 run of the reference does with its label weights cast
        score = cls_score.new_zeros(labels.shape)
        if len(pos_inds) > 0:
            pos_bbox_targets, pos_bbox_pred = bbox_targets[pos_inds], bbox_pred[pos_inds]
            pos_anchor_centers = self.anchor_center(anchors[pos_inds]) / stride[0]
            weight_targets = cls_score.detach().sigmoid().max(dim=1)[0][pos_inds]
            pos_decode_bbox_pred = distance2bbox(pos_anchor_centers, self.integral(pos_bbox_pred))
            pos_decode_bbox_targets = pos_bbox_targets / stride[0]
            score[pos_inds] = bbox_overlaps(pos_decode_bbox_pred.detach(), pos_decode_bbox_targets, is_aligned=True).to(score.dtype)
            pred_corners = pos_bbox_pred.reshape(-1, self.reg_max + 1)
            target_corners = bbox2distance(pos_anchor_centers, pos_decode_bbox_targets, self.reg_max).reshape(-1)
            loss_bbox = self.loss_bbox(pos_decode_bbox_pred, pos_decode_bbox_targets, weight=weight_targets, avg_factor=1.0)
            loss_dfl = self.loss_dfl(pred_corners, target_corners, weight=weight_targets[:, None].expand(-1, 4).reshape(-1),
                                     avg_factor=4.0)
        else:
            loss_bbox = bbox_pred.sum() * 0
            loss_dfl = bbox_pred.sum() * 0
            weight_targets = bbox_pred.new_tensor(0.)
        loss_cls = self.loss_cls(cls_score, (labels, score), weight=label_weights, avg_factor=num_total_samples)
        return loss_cls, loss_bbox, loss_dfl, weight_targets.sum()

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        if self._fused_loss_ok(cls_scores, bbox_preds, gt_labels, gt_bboxes_ignore, img_metas):
            return self.loss_fused(cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas)
        return self.loss_tensor(cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)

    def loss_tensor(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """gfl_head.py:297-369, in the reference's order of operations; the averaging factor is not clamped."""
        _, targets = self._loss_targets(cls_scores, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        if targets is None:
            return None
        anchors, labels, label_weights, bbox_targets, _, num_total_pos, _ = targets
        num_total_samples = float(reduce_mean(torch.tensor(float(num_total_pos), device=cls_scores[0].device)))
        num_total_samples = max(num_total_samples, 1.0)
        losses_cls, losses_bbox, losses_dfl, avg_factor = multi_apply(
            self.loss_single, anchors, cls_scores, bbox_preds, labels, label_weights, bbox_targets, self.anchor_generator.strides,
            num_total_samples=num_total_samples)
        avg_factor = float(reduce_mean(sum(avg_factor)))
        losses_bbox = [x / avg_factor for x in losses_bbox]
        losses_dfl = [x / avg_factor for x in losses_dfl]
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox, loss_dfl=losses_dfl)

    def _fused_loss_ok(self, cls_scores, bbox_preds, gt_labels, gt_bboxes_ignore, img_metas):
        """htd_atss_targets / htd_gfl_quality / htd_gfl_loss cover QualityFocalLoss + DistributionFocalLoss + IoULoss / GIoULoss
        all with mean reduction and reg_max <= 31, on maps that `_fused_maps_ok` takes, under the assigner's conditions
        (`_atss_fused_ok`)."""
        lc, lb, ld = self.loss_cls, self.loss_bbox, self.loss_dfl
        return getattr(self, 'fused_loss', GFL_FUSED) and \
            type(lc).__name__ == 'QualityFocalLoss' and lc.use_sigmoid and lc.reduction == 'mean' and \
            type(lb).__name__ in M.FCOS_BOX_KINDS and lb.reduction == 'mean' and \
            type(ld).__name__ == 'DistributionFocalLoss' and ld.reduction == 'mean' and 1 <= self.reg_max <= 31 and \
            self._fused_maps_ok(cls_scores, bbox_preds) and self._atss_fused_ok(cls_scores, gt_labels, gt_bboxes_ignore, img_metas)

    def loss_fused(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas):
        import torch.distributed as dist
        flat_anchors, gts, labels, assigned, _, num_pos, norm = self._atss_fused_targets(cls_scores, gt_bboxes, gt_labels, img_metas)
        strides = self.anchor_generator.strides
        weight, score, wsum = M.gfl_quality([c.detach() for c in cls_scores], [r.detach() for r in bbox_preds], strides,
                                            self.reg_max, flat_anchors, gts, assigned)
        if dist.is_available() and dist.is_initialized():
            wsum = reduce_mean(wsum)            # gfl_head.py:364-365
        self._last_targets = (assigned, num_pos, norm)          # exposed for tests
        self._last_quality = (weight, score, wsum)
        lc, lb = self.loss_cls, self.loss_bbox
        loss_cls, loss_bbox, loss_dfl = M.gfl_loss(
            cls_scores, bbox_preds, strides, self.reg_max, flat_anchors, gts, labels, assigned, weight, score, norm, wsum,
            M.FCOS_BOX_KINDS[type(lb).__name__], lb.eps, lc.beta, lc.loss_weight, lb.loss_weight, self.loss_dfl.loss_weight)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_dfl=loss_dfl)

    # ------------------------------------------------------------------ boxes
    def _device_keys_ok(self, cls_scores, bbox_preds, score_factors=None):
        """htd_gfl_decode takes fp32 channels_last GPU maps of at most 8 levels; anything else, NCHW-contiguous maps included,
        takes the tensor operations."""
        return cls_scores[0].is_cuda and len(cls_scores) <= 8 and 1 <= self.reg_max <= 31 and \
            all(t.dtype == torch.float32 and M.nhwc_channel_stride(t) is not None for t in list(cls_scores) + list(bbox_preds))

    def _bbox_priors(self, featmap_sizes, dtype, device):
        return [self.anchor_center(a) for a in self.anchor_generator.grid_anchors(featmap_sizes, device=device)]

    def _bbox_decode(self, centres, dists, img_shape):
        from ..core.bbox import distance2bbox
        return distance2bbox(centres, dists, max_shape=img_shape)

    def _keys_and_preds(self, cls_scores, bbox_preds, score_factors, want_keys):
        """-> (B, A) max_c sigmoid(score) and (B, A, 4) integral * stride: one htd_gfl_decode launch gives both, so it runs
        whether or not a level is cut; the reference's tensor operations elsewhere."""
        if self._device_keys_ok(cls_scores, bbox_preds):
            return M.gfl_decode(cls_scores, bbox_preds, self.strides, self.reg_max)
        B = cls_scores[0].size(0)
        keys = [c.permute(0, 2, 3, 1).reshape(B, -1, self.cls_out_channels).sigmoid().max(dim=-1)[0] for c in cls_scores]
        dists = [(self.integral(r.permute(0, 2, 3, 1)) * s[0]).reshape(B, -1, 4) for r, s in zip(bbox_preds, self.strides)]
        return torch.cat(keys, 1), torch.cat(dists, 1)

    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True):
        """gfl_head.py:371-455 over a batch -> list (per image) of (dets (k, 5), labels (k,)): BaseDenseHead._get_bboxes with the
        anchor centres as priors and distance2bbox as decode."""
        return self._get_bboxes(cls_scores, bbox_preds, None, img_metas, cfg, rescale, with_nms)
