"""VFNetHead: the IoU-aware dense head of VarifocalNet.

Reference: dense_heads/vfnet_head.py:18-794 (towers and predictors :144-177, forward_single :217-273, star_dcn_offset :275-314,
loss :317-463, get_bboxes :465-597, the points :599-620, the ATSS / FCOS targets :622-788, _load_from_state_dict :790-794).  Same
registry name, constructor kwargs and defaults, `reg_denoms`, `dcn_base_offset`, state_dict keys (cls_convs.N.conv/gn,
reg_convs.N..., vfnet_reg_conv.conv/gn, vfnet_reg, scales.N.scale, vfnet_reg_refine_dconv.weight, vfnet_reg_refine,
scales_refine.N.scale, vfnet_cls_dconv.weight, vfnet_cls) and return structures.

The head is FCOS-shaped (the towers, one Scale per level, points) and inherits the anchors, their targets and the ATSS half of
the fused loss from the mixin ATSSHead and GFLHead take them from (`VFNetHead(ATSSTargets, FCOSHead)`); the targets of the
positives are the gt boxes themselves (no coder).  Its two deformable convolutions
(htd_amd.dcn.deform_conv2d with the ReLU in the epilogue) share one offset tensor that is not predicted but built from the
initial box: on fp32 GPU maps one autograd function around htd_vfnet_star_fwd / _bwd turns the scaled regression logits into
`bbox_pred` and `dcn_offset` together; `star_dcn_offset` is the reference's tensor form (CPU, fp64).

`loss` has two forms, like GFLHead.loss, and `_fused_loss_ok` is the one rule between them.  `loss_tensor` is the reference's
order of operations (both target kinds, use_vfl off, center sampling, the `num_pos == 0` branch, sync_num_pos).  `loss_fused`
assigns the batch with htd_atss_targets, takes both IoUs of every positive and the three sums that the averaging factors are in
one pass (htd_vfnet_quality) and the three losses with the three gradient maps of all levels in one more launch
(htd_vfnet_loss): no permute, concatenation, gather or nonzero() of the predictions, no host read.  The number of positives is
that of the whole batch, clamped once -- not AnchorHead's sum of per-image counts clamped per image, which htd_atss_targets
leaves in norm[0].

`get_bboxes` is BaseDenseHead._get_bboxes, which all dense heads share, on the refined distances: ranked by max_c sigmoid(cls)
without a score factor (FCOSHead passes one, this head does not), FCOSHead's priors and decode.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from ..core import bbox2distance, bbox_overlaps, distance2bbox, multi_apply, reduce_mean
from .. import mmcv_ops as M
from ..dcn import DeformConv2d, deform_conv2d
from ..registry import HEADS, build_anchor_generator, build_assigner, build_loss, build_sampler
from .anchor_free_heads import INF, AnchorFreeHead, FCOSHead, Scale
from .anchor_heads import ATSSTargets, bias_init_with_prob
from .bricks import Conv2d, ConvModule, normal_init

VFNET_FUSED = os.environ.get('HTD_VFNET_FUSED', '1') != '0'         # 0: the tensor-path loss and star offsets (A/B runs)


@HEADS.register_module()
class VFNetHead(ATSSTargets, FCOSHead):
    def __init__(self, num_classes, in_channels, regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)),
                 center_sampling=False, center_sample_radius=1.5, sync_num_pos=True, gradient_mul=0.1, bbox_norm_type='reg_denom',
                 loss_cls_fl=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0), use_vfl=True,
                 loss_cls=dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True, loss_weight=1.0),
                 loss_bbox=dict(type='GIoULoss', loss_weight=1.5), loss_bbox_refine=dict(type='GIoULoss', loss_weight=2.0),
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), use_atss=True,
                 anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                       center_offset=0.0, strides=[8, 16, 32, 64, 128]), **kwargs):
        # dcn base offsets (vfnet_head.py:100-110): (y, x) of the 3 x 3 taps, tap-major
        self.num_dconv_points = 9
        self.dcn_kernel = int(np.sqrt(self.num_dconv_points))
        self.dcn_pad = int((self.dcn_kernel - 1) / 2)
        dcn_base = np.arange(-self.dcn_pad, self.dcn_pad + 1).astype(np.float64)
        dcn_base_offset = np.stack([np.repeat(dcn_base, self.dcn_kernel), np.tile(dcn_base, self.dcn_kernel)], axis=1).reshape(-1)
        self.dcn_base_offset = torch.tensor(dcn_base_offset).view(1, -1, 1, 1)
        if bbox_norm_type not in ('reg_denom', 'stride'):
            raise NotImplementedError(f"bbox_norm_type must be 'reg_denom' or 'stride', got {bbox_norm_type!r}")
        self.bbox_norm_type = bbox_norm_type

        AnchorFreeHead.__init__(self, num_classes, in_channels, norm_cfg=norm_cfg, **kwargs)
        self.regress_ranges = regress_ranges
        self.reg_denoms = [regress_range[-1] for regress_range in regress_ranges]
        self.reg_denoms[-1] = self.reg_denoms[-2] * 2
        self.center_sampling, self.center_sample_radius = center_sampling, center_sample_radius
        self.norm_on_bbox = False
        self.sync_num_pos, self.gradient_mul, self.use_vfl = sync_num_pos, gradient_mul, use_vfl
        self.loss_cls = build_loss(loss_cls if use_vfl else loss_cls_fl)
        self.loss_bbox = build_loss(loss_bbox)
        self.loss_bbox_refine = build_loss(loss_bbox_refine)

        # for getting ATSS targets
        self.use_atss = use_atss
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.anchor_generator = build_anchor_generator(anchor_generator)
        self.anchor_center_offset = anchor_generator['center_offset']
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        self.sampling = False
        if self.train_cfg:
            self.assigner = build_assigner(self.train_cfg.assigner)
            self.sampler = build_sampler(dict(type='PseudoSampler'), context=self)

    def _init_layers(self):
        self._build_towers('cls_convs', 'reg_convs')
        self.relu = nn.ReLU(inplace=True)
        self.vfnet_reg_conv = ConvModule(self.feat_channels, self.feat_channels, 3, stride=1, padding=1, conv_cfg=self.conv_cfg,
                                         norm_cfg=self.norm_cfg, bias=self.conv_bias)
        self.vfnet_reg = Conv2d(self.feat_channels, 4, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])
        self.vfnet_reg_refine_dconv = DeformConv2d(self.feat_channels, self.feat_channels, self.dcn_kernel, 1, padding=self.dcn_pad)
        self.vfnet_reg_refine = Conv2d(self.feat_channels, 4, 3, padding=1)
        self.scales_refine = nn.ModuleList([Scale(1.0) for _ in self.strides])
        self.vfnet_cls_dconv = DeformConv2d(self.feat_channels, self.feat_channels, self.dcn_kernel, 1, padding=self.dcn_pad)
        self.vfnet_cls = Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)

    def init_weights(self):
        self._init_towers()
        normal_init(self.vfnet_reg_conv.conv, std=0.01)
        normal_init(self.vfnet_reg, std=0.01)
        normal_init(self.vfnet_reg_refine_dconv, std=0.01)
        normal_init(self.vfnet_reg_refine, std=0.01)
        normal_init(self.vfnet_cls_dconv, std=0.01)
        normal_init(self.vfnet_cls, std=0.01, bias=bias_init_with_prob(0.01))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """vfnet_head.py:790-794: not AnchorFreeHead's pre-2.0 rename (it would turn vfnet_cls / vfnet_reg into conv_cls /
        conv_reg); the head owns no parameters of its own, its children load theirs."""
        pass

    # ------------------------------------------------------------------ forward
    def forward(self, feats):
        return multi_apply(self.forward_single, feats, self.scales, self.scales_refine, self.strides, self.reg_denoms)

    def _star_kernel_ok(self, x):
        return getattr(self, 'fused_loss', VFNET_FUSED) and x.is_cuda and x.dtype == torch.float32

    def forward_single(self, x, scale, scale_refine, stride, reg_denom):
        """vfnet_head.py:217-273 -> cls_score, bbox_pred, bbox_pred_refine (both distances in image units)."""
        cls_feat, reg_feat = self._run_towers(x)
        # predict the bbox_pred of different level
        reg_feat_init = self.vfnet_reg_conv(reg_feat)
        denom = reg_denom if self.bbox_norm_type == 'reg_denom' else stride
        logits = scale(self.vfnet_reg(reg_feat_init)).float()
        if self._star_kernel_ok(logits):
            bbox_pred, dcn_offset = M.vfnet_star(logits, denom, stride, self.gradient_mul)
        else:
            bbox_pred = logits.exp() * denom
            dcn_offset = self.star_dcn_offset(bbox_pred, self.gradient_mul, stride).to(reg_feat.dtype)
        # refine the bbox_pred
        reg_feat = self._dconv(self.vfnet_reg_refine_dconv, reg_feat, dcn_offset)
        bbox_pred_refine = scale_refine(self.vfnet_reg_refine(reg_feat)).float().exp()
        bbox_pred_refine = bbox_pred_refine * bbox_pred.detach()
        # predict the iou-aware cls score
        cls_feat = self._dconv(self.vfnet_cls_dconv, cls_feat, dcn_offset)
        cls_score = self.vfnet_cls(cls_feat)
        return cls_score, bbox_pred, bbox_pred_refine

    @staticmethod
    def _dconv(m, x, offset):
        """relu(DeformConv2d(x, offset)), the activation in the epilogue of the convolution's GEMM."""
        return deform_conv2d(x, offset, m.weight, m.stride, m.padding, m.dilation, m.groups, m.deform_groups, relu=True)

    def star_dcn_offset(self, bbox_pred, gradient_mul, stride):
        """vfnet_head.py:275-314, the tensor form: (N, 4, H, W) distances (l, t, r, b) -> (N, 18, H, W) offsets that put the
        nine taps on the corners, the edge midpoints and the centre of the box."""
        dcn_base_offset = self.dcn_base_offset.type_as(bbox_pred)
        bbox_pred_grad_mul = (1 - gradient_mul) * bbox_pred.detach() + gradient_mul * bbox_pred
        bbox_pred_grad_mul = bbox_pred_grad_mul / stride            # map to the feature map scale
        N, C, H, W = bbox_pred.size()
        x1, y1, x2, y2 = (bbox_pred_grad_mul[:, k, :, :] for k in range(4))
        offset = bbox_pred.new_zeros(N, 2 * self.num_dconv_points, H, W)
        offset[:, 0, :, :] = -1.0 * y1
        offset[:, 1, :, :] = -1.0 * x1
        offset[:, 2, :, :] = -1.0 * y1
        offset[:, 4, :, :] = -1.0 * y1
        offset[:, 5, :, :] = x2
        offset[:, 7, :, :] = -1.0 * x1
        offset[:, 11, :, :] = x2
        offset[:, 12, :, :] = y2
        offset[:, 13, :, :] = -1.0 * x1
        offset[:, 14, :, :] = y2
        offset[:, 16, :, :] = y2
        offset[:, 17, :, :] = x2
        return offset - dcn_base_offset

    # ------------------------------------------------------------------ points and targets
    def _get_points_single(self, featmap_size, stride, dtype, device, flatten=False):
        """vfnet_head.py:599-620: the anchors' centres under ATSS, FCOS's cell centres otherwise."""
        h, w = featmap_size
        x_range = torch.arange(0, w * stride, stride, dtype=dtype, device=device)
        y_range = torch.arange(0, h * stride, stride, dtype=dtype, device=device)
        y, x = torch.meshgrid(y_range, x_range, indexing='ij')
        points = torch.stack((x.reshape(-1), y.reshape(-1)), dim=-1)
        return points + (stride * self.anchor_center_offset if self.use_atss else stride // 2)

    def _pos_bbox_targets(self, sr):
        return sr.pos_gt_bboxes

    def _get_target_single(self, *args, **kwargs):
        """vfnet_head.py:657-662: ATSSTargets' per-image routine under use_atss, FCOSHead's (which its get_targets calls)
        otherwise."""
        if self.use_atss:
            return super()._get_target_single(*args, **kwargs)
        return FCOSHead._get_target_single(self, *args, **kwargs)

    def get_targets(self, cls_scores, mlvl_points, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore):
        """vfnet_head.py:622-655 -> (labels per level, label_weights or None, bbox_targets (l, t, r, b) per level, bbox_weights or
        None)."""
        if self.use_atss:
            return self.get_atss_targets(cls_scores, mlvl_points, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        self.norm_on_bbox = False
        return self.get_fcos_targets(mlvl_points, gt_bboxes, gt_labels)

    def get_fcos_targets(self, points, gt_bboxes_list, gt_labels_list):
        labels, bbox_targets = FCOSHead.get_targets(self, points, gt_bboxes_list, gt_labels_list)
        return labels, None, bbox_targets, None

    def get_atss_targets(self, cls_scores, mlvl_points, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """vfnet_head.py:690-763."""
        _, targets = self._loss_targets(cls_scores, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        if targets is None:
            return None
        _, labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, _, _ = targets
        bbox_targets_list = [t.reshape(-1, 4) for t in bbox_targets_list]
        bbox_targets_list = self.transform_bbox_targets(bbox_targets_list, mlvl_points, len(img_metas))
        labels_list = [labels.reshape(-1) for labels in labels_list]
        label_weights = torch.cat([w.reshape(-1) for w in label_weights_list])
        bbox_weights = torch.cat([w.reshape(-1) for w in bbox_weights_list])
        return labels_list, label_weights, bbox_targets_list, bbox_weights

    def transform_bbox_targets(self, decoded_bboxes, mlvl_points, num_imgs):
        """vfnet_head.py:765-788: (x1, y1, x2, y2) targets -> (l, t, r, b) of their points."""
        assert len(decoded_bboxes) == len(mlvl_points)
        return [bbox2distance(points.repeat(num_imgs, 1), boxes) for points, boxes in zip(mlvl_points, decoded_bboxes)]

    # ------------------------------------------------------------------ loss
    def loss(self, cls_scores, bbox_preds, bbox_preds_refine, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        if self._fused_loss_ok(cls_scores, bbox_preds, bbox_preds_refine, gt_labels, gt_bboxes_ignore, img_metas):
            return self.loss_fused(cls_scores, bbox_preds, bbox_preds_refine, gt_bboxes, gt_labels, img_metas)
        return self.loss_tensor(cls_scores, bbox_preds, bbox_preds_refine, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)

    def loss_tensor(self, cls_scores, bbox_preds, bbox_preds_refine, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """vfnet_head.py:317-463, in the reference's order of operations."""
        assert len(cls_scores) == len(bbox_preds) == len(bbox_preds_refine)
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        all_level_points = self.get_points(featmap_sizes, bbox_preds[0].dtype, bbox_preds[0].device)
        labels, label_weights, bbox_targets, bbox_weights = self.get_targets(cls_scores, all_level_points, gt_bboxes, gt_labels,
                                                                             img_metas, gt_bboxes_ignore)
        num_imgs = cls_scores[0].size(0)
        flatten_cls_scores = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels).contiguous() for c in cls_scores])
        flatten_bbox_preds = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4).contiguous() for b in bbox_preds])
        flatten_bbox_preds_refine = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4).contiguous() for b in bbox_preds_refine])
        flatten_labels, flatten_bbox_targets = torch.cat(labels), torch.cat(bbox_targets)
        flatten_points = torch.cat([points.repeat(num_imgs, 1) for points in all_level_points])
        bg_class_ind = self.num_classes
        pos_inds = torch.where(((flatten_labels >= 0) & (flatten_labels < bg_class_ind)) > 0)[0]
        num_pos = len(pos_inds)
        pos_bbox_preds, pos_bbox_preds_refine = flatten_bbox_preds[pos_inds], flatten_bbox_preds_refine[pos_inds]
        pos_labels = flatten_labels[pos_inds]
        if self.sync_num_pos:
            num_pos_avg_per_gpu = max(reduce_mean(pos_inds.new_tensor(num_pos).float()).item(), 1.0)
        else:
            num_pos_avg_per_gpu = num_pos
        if num_pos > 0:
            pos_bbox_targets, pos_points = flatten_bbox_targets[pos_inds], flatten_points[pos_inds]
            pos_decoded_bbox_preds = distance2bbox(pos_points, pos_bbox_preds)
            pos_decoded_target_preds = distance2bbox(pos_points, pos_bbox_targets).detach()
            iou_targets_ini = bbox_overlaps(pos_decoded_bbox_preds, pos_decoded_target_preds, is_aligned=True).clamp(min=1e-6)
            bbox_weights_ini = iou_targets_ini.clone().detach()
            bbox_avg_factor_ini = max(reduce_mean(bbox_weights_ini.sum()).item(), 1.0)
            loss_bbox = self.loss_bbox(pos_decoded_bbox_preds, pos_decoded_target_preds, weight=bbox_weights_ini,
                                       avg_factor=bbox_avg_factor_ini)
            pos_decoded_bbox_preds_refine = distance2bbox(pos_points, pos_bbox_preds_refine)
            iou_targets_rf = bbox_overlaps(pos_decoded_bbox_preds_refine, pos_decoded_target_preds, is_aligned=True).clamp(min=1e-6)
            bbox_weights_rf = iou_targets_rf.clone().detach()
            bbox_avg_factor_rf = max(reduce_mean(bbox_weights_rf.sum()).item(), 1.0)
            loss_bbox_refine = self.loss_bbox_refine(pos_decoded_bbox_preds_refine, pos_decoded_target_preds,
                                                     weight=bbox_weights_rf, avg_factor=bbox_avg_factor_rf)
            if self.use_vfl:                    # build IoU-aware cls_score targets
                cls_iou_targets = torch.zeros_like(flatten_cls_scores)
                cls_iou_targets[pos_inds, pos_labels] = iou_targets_rf.clone().detach()
        else:
            loss_bbox = pos_bbox_preds.sum() * 0
            loss_bbox_refine = pos_bbox_preds_refine.sum() * 0
            if self.use_vfl:
                cls_iou_targets = torch.zeros_like(flatten_cls_scores)
        if self.use_vfl:
            loss_cls = self.loss_cls(flatten_cls_scores, cls_iou_targets, avg_factor=num_pos_avg_per_gpu)
        else:
            loss_cls = self.loss_cls(flatten_cls_scores, flatten_labels, weight=label_weights, avg_factor=num_pos_avg_per_gpu)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_bbox_rf=loss_bbox_refine)

    def _fused_loss_ok(self, cls_scores, bbox_preds, bbox_preds_refine, gt_labels, gt_bboxes_ignore, img_metas):
        """htd_atss_targets / htd_vfnet_quality / htd_vfnet_loss cover ATSS targets under sigmoid VarifocalLoss and two IoULoss /
        GIoULoss, all with mean reduction, the number of positives synchronised (its clamp to 1 is part of the kernel), on maps
        that `_fused_maps_ok` takes, under the assigner's conditions (`_atss_fused_ok`)."""
        lc, lb, lr = self.loss_cls, self.loss_bbox, self.loss_bbox_refine
        return getattr(self, 'fused_loss', VFNET_FUSED) and self.use_atss and self.use_vfl and self.sync_num_pos and \
            type(lc).__name__ == 'VarifocalLoss' and lc.use_sigmoid and lc.reduction == 'mean' and \
            type(lb).__name__ in M.FCOS_BOX_KINDS and lb.reduction == 'mean' and \
            type(lr).__name__ in M.FCOS_BOX_KINDS and lr.reduction == 'mean' and \
            self._fused_maps_ok(cls_scores, bbox_preds, bbox_preds_refine) and \
            self._atss_fused_ok(cls_scores, gt_labels, gt_bboxes_ignore, img_metas)

    def loss_fused(self, cls_scores, bbox_preds, bbox_preds_refine, gt_bboxes, gt_labels, img_metas):
        import torch.distributed as dist
        assert len(cls_scores) == len(bbox_preds) == len(bbox_preds_refine)
        # `norm` stays this process's own: the head takes none of it, it averages the sums of its quality pass below
        flat_anchors, gts, labels, assigned, _, num_pos, norm = self._atss_fused_targets(cls_scores, gt_bboxes, gt_labels, img_metas,
                                                                                        reduce_norm=False)
        iou_ini, iou_rf, sums = M.vfnet_quality([r.detach() for r in bbox_preds], [r.detach() for r in bbox_preds_refine],
                                                flat_anchors, gts, assigned)
        if dist.is_available() and dist.is_initialized():
            # vfnet_head.py:393-396,412-414,428-430: the three factors averaged over the processes (the kernel clamps each to 1)
            sums = reduce_mean(sums)
        self._last_targets = (assigned, num_pos, norm)          # exposed for tests
        self._last_quality = (iou_ini, iou_rf, sums)
        lc, lb, lr = self.loss_cls, self.loss_bbox, self.loss_bbox_refine
        loss_cls, loss_bbox, loss_bbox_rf = M.vfnet_loss(
            cls_scores, bbox_preds, bbox_preds_refine, flat_anchors, gts, labels, assigned, iou_ini, iou_rf, sums,
            M.FCOS_BOX_KINDS[type(lb).__name__], M.FCOS_BOX_KINDS[type(lr).__name__], lb.eps, lr.eps, lc.alpha, lc.gamma,
            lc.iou_weighted, lc.loss_weight, lb.loss_weight, lr.loss_weight)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_bbox_rf=loss_bbox_rf)

    # ------------------------------------------------------------------ boxes
    _prior_deps = property(lambda self: (self.use_atss, ))      # the points sit on the anchor centres under use_atss

    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, bbox_preds_refine, img_metas, cfg=None, rescale=None, with_nms=True):
        """vfnet_head.py:465-597 -> list (per image) of (dets (k, 5), labels (k,)) from the refined boxes, ranked by max_c
        sigmoid(cls) without a score factor."""
        assert len(bbox_preds) == len(bbox_preds_refine)
        return self._get_bboxes(cls_scores, bbox_preds_refine, None, img_metas, cfg, rescale, with_nms)
