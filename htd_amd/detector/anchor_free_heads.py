"""Anchor-free dense heads: AnchorFreeHead and FCOSHead.

Reference: dense_heads/anchor_free_head.py:14-340 (towers, predictors, the pre-2.0 key rename, get_points),
dense_heads/fcos_head.py:14-576 (forward_single, loss, get_bboxes, get_targets, centerness_target), mmcv.cnn.Scale.  Same registry
names, constructor kwargs, state_dict keys (cls_convs.N.conv/gn, reg_convs.N..., conv_cls, conv_reg, conv_centerness,
scales.N.scale) and return structures.  forward_train, simple_test, the towers (built tower by tower: `_build_towers`), the
fused losses' rule on the maps and the shape-keyed caches come from BaseDenseHead, which the anchor heads extend too.

`FCOSHead.loss` has two forms, like AnchorHead.loss, and `_fused_loss_ok` is the one rule between them.  `loss_tensor` is the
reference's order of operations (get_points, get_targets / _get_target_single, centerness_target, distance2bbox, the three loss
modules, the `num_pos == 0` branch) and works on the CPU, in fp64 and with any loss modules.  `loss_fused` -- FocalLoss, IoULoss
or GIoULoss, sigmoid CrossEntropyLoss, all with mean reduction, fp32 channels_last GPU maps -- assigns the whole batch in one launch
that computes the points itself (htd_fcos_targets: no (points, gts) matrices, the three averaging factors left on the device) and
takes the three losses and the three gradient maps of all levels in one more (htd_fcos_loss) that reads the maps where they are: no
permute, concatenation or gather of the predictions, no nonzero(), no host read.

`get_bboxes` is BaseDenseHead._get_bboxes, which all dense heads share, with the points as priors, distance2bbox as decode and the
centerness maps as score factors of the ranking (htd_fcos_keys) and of the NMS.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..core import distance2bbox, multi_apply
from .. import mmcv_ops as M
from ..registry import HEADS, build_loss
from .anchor_heads import bias_init_with_prob
from .base_dense_head import BaseDenseHead
from .bricks import Conv2d, normal_init

FCOS_FUSED = os.environ.get('HTD_FCOS_FUSED', '1') != '0'           # 0: the tensor-path loss (A/B runs)
INF = 1e8


class Scale(nn.Module):
    """mmcv.cnn.Scale: one learnable scalar."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


@HEADS.register_module()
class AnchorFreeHead(BaseDenseHead):
    _version = 1

    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64),
                 dcn_on_last_conv=False, conv_bias='auto',
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0), conv_cfg=None, norm_cfg=None, train_cfg=None, test_cfg=None):
        super().__init__()
        self.num_classes = self.cls_out_channels = num_classes
        self.in_channels, self.feat_channels, self.stacked_convs = in_channels, feat_channels, stacked_convs
        self.strides, self.dcn_on_last_conv = strides, dcn_on_last_conv
        assert conv_bias == 'auto' or isinstance(conv_bias, bool)
        self.conv_bias = conv_bias
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.fp16_enabled = False
        self._init_layers()

    def _init_layers(self):
        self._build_towers('cls_convs', 'reg_convs')
        self.conv_cls = Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)
        self.conv_reg = Conv2d(self.feat_channels, 4, 3, padding=1)

    def init_weights(self):
        self._init_towers()
        normal_init(self.conv_cls, std=0.01, bias=bias_init_with_prob(0.01))
        normal_init(self.conv_reg, std=0.01)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """anchor_free_head.py:143-179: a state dict without version metadata has the pre-2.0 predictor names
        (fcos_cls / fcos_reg / fcos_centerness -> conv_cls / conv_reg / conv_centerness)."""
        if local_metadata.get('version', None) is None:
            for key in [k for k in state_dict.keys() if k.startswith(prefix)]:
                parts = key[len(prefix):].split('.')
                new = None
                if parts[0].endswith('cls'):
                    new = 'conv_cls'
                elif parts[0].endswith('reg'):
                    new = 'conv_reg'
                elif parts[0].endswith('centerness'):
                    new = 'conv_centerness'
                if new is not None and new != parts[0]:
                    state_dict[prefix + '.'.join([new] + parts[1:])] = state_dict.pop(key)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, feats):
        return multi_apply(self.forward_single, feats)[:2]

    def forward_single(self, x):
        """-> cls_score, bbox_pred and the two tower outputs (FCOS puts the centerness on one of them)."""
        cls_feat, reg_feat = self._run_towers(x)
        return self.conv_cls(cls_feat), self.conv_reg(reg_feat), cls_feat, reg_feat

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        raise NotImplementedError

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=None):
        raise NotImplementedError

    def get_targets(self, points, gt_bboxes_list, gt_labels_list):
        raise NotImplementedError

    def _get_points_single(self, featmap_size, stride, dtype, device, flatten=False):
        h, w = featmap_size
        y, x = torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device),
                              indexing='ij')
        return (y.flatten(), x.flatten()) if flatten else (y, x)

    def get_points(self, featmap_sizes, dtype, device, flatten=False):
        return [self._get_points_single(featmap_sizes[i], self.strides[i], dtype, device, flatten)
                for i in range(len(featmap_sizes))]


@HEADS.register_module()
class FCOSHead(AnchorFreeHead):
    def __init__(self, num_classes, in_channels, regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)),
                 center_sampling=False, center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False,
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), **kwargs):
        self.regress_ranges = regress_ranges
        self.center_sampling, self.center_sample_radius = center_sampling, center_sample_radius
        self.norm_on_bbox, self.centerness_on_reg = norm_on_bbox, centerness_on_reg
        super().__init__(num_classes, in_channels, loss_cls=loss_cls, loss_bbox=loss_bbox, norm_cfg=norm_cfg, **kwargs)
        self.loss_centerness = build_loss(loss_centerness)

    def _init_layers(self):
        super()._init_layers()
        self.conv_centerness = Conv2d(self.feat_channels, 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])

    def init_weights(self):
        super().init_weights()
        normal_init(self.conv_centerness, std=0.01)

    # ------------------------------------------------------------------ forward
    def forward(self, feats):
        return multi_apply(self.forward_single, feats, self.scales, self.strides)

    def forward_single(self, x, scale, stride):
        """fcos_head.py:127-156."""
        cls_score, bbox_pred, cls_feat, reg_feat = super().forward_single(x)
        centerness = self.conv_centerness(reg_feat if self.centerness_on_reg else cls_feat)
        bbox_pred = scale(bbox_pred).float()
        if self.norm_on_bbox:
            bbox_pred = F.relu(bbox_pred)
            if not self.training:
                bbox_pred = bbox_pred * stride
        else:
            bbox_pred = bbox_pred.exp()
        return cls_score, bbox_pred, centerness

    # ------------------------------------------------------------------ targets
    def _get_points_single(self, featmap_size, stride, dtype, device, flatten=False):
        y, x = super()._get_points_single(featmap_size, stride, dtype, device)
        return torch.stack((x.reshape(-1) * stride, y.reshape(-1) * stride), dim=-1) + stride // 2

    def get_targets(self, points, gt_bboxes_list, gt_labels_list):
        """fcos_head.py:415-474 -> (labels per level, bbox_targets per level), each level's rows image after image."""
        assert len(points) == len(self.regress_ranges)
        num_levels = len(points)
        expanded = [points[i].new_tensor(self.regress_ranges[i])[None].expand_as(points[i]) for i in range(num_levels)]
        concat_ranges, concat_points = torch.cat(expanded, dim=0), torch.cat(points, dim=0)
        num_points = [p.size(0) for p in points]
        labels_list, bbox_targets_list = multi_apply(self._get_target_single, gt_bboxes_list, gt_labels_list, points=concat_points,
                                                     regress_ranges=concat_ranges, num_points_per_lvl=num_points)
        labels_list = [labels.split(num_points, 0) for labels in labels_list]
        bbox_targets_list = [t.split(num_points, 0) for t in bbox_targets_list]
        lvl_labels, lvl_targets = [], []
        for i in range(num_levels):
            lvl_labels.append(torch.cat([labels[i] for labels in labels_list]))
            t = torch.cat([t[i] for t in bbox_targets_list])
            lvl_targets.append(t / self.strides[i] if self.norm_on_bbox else t)
        return lvl_labels, lvl_targets

    def _get_target_single(self, gt_bboxes, gt_labels, points, regress_ranges, num_points_per_lvl):
        """fcos_head.py:476-558 for one image."""
        num_points, num_gts = points.size(0), gt_labels.size(0)
        if num_gts == 0:
            return gt_labels.new_full((num_points, ), self.num_classes), gt_bboxes.new_zeros((num_points, 4))
        areas = (gt_bboxes[:, 2] - gt_bboxes[:, 0]) * (gt_bboxes[:, 3] - gt_bboxes[:, 1])
        areas = areas[None].repeat(num_points, 1)
        regress_ranges = regress_ranges[:, None, :].expand(num_points, num_gts, 2)
        gt_bboxes = gt_bboxes[None].expand(num_points, num_gts, 4)
        xs = points[:, 0][:, None].expand(num_points, num_gts)
        ys = points[:, 1][:, None].expand(num_points, num_gts)
        left, right = xs - gt_bboxes[..., 0], gt_bboxes[..., 2] - xs
        top, bottom = ys - gt_bboxes[..., 1], gt_bboxes[..., 3] - ys
        bbox_targets = torch.stack((left, top, right, bottom), -1)
        if self.center_sampling:
            radius = self.center_sample_radius
            center_xs = (gt_bboxes[..., 0] + gt_bboxes[..., 2]) / 2
            center_ys = (gt_bboxes[..., 1] + gt_bboxes[..., 3]) / 2
            stride = center_xs.new_zeros(center_xs.shape)
            lvl_begin = 0
            for lvl_idx, n in enumerate(num_points_per_lvl):
                stride[lvl_begin:lvl_begin + n] = self.strides[lvl_idx] * radius
                lvl_begin += n
            x_mins, y_mins, x_maxs, y_maxs = center_xs - stride, center_ys - stride, center_xs + stride, center_ys + stride
            c0 = torch.where(x_mins > gt_bboxes[..., 0], x_mins, gt_bboxes[..., 0])
            c1 = torch.where(y_mins > gt_bboxes[..., 1], y_mins, gt_bboxes[..., 1])
            c2 = torch.where(x_maxs > gt_bboxes[..., 2], gt_bboxes[..., 2], x_maxs)
            c3 = torch.where(y_maxs > gt_bboxes[..., 3], gt_bboxes[..., 3], y_maxs)
            center_bbox = torch.stack((xs - c0, ys - c1, c2 - xs, c3 - ys), -1)
            inside_gt_bbox_mask = center_bbox.min(-1)[0] > 0
        else:
            inside_gt_bbox_mask = bbox_targets.min(-1)[0] > 0
        max_regress_distance = bbox_targets.max(-1)[0]
        inside_regress_range = (max_regress_distance >= regress_ranges[..., 0]) & (max_regress_distance <= regress_ranges[..., 1])
        areas[inside_gt_bbox_mask == 0] = INF
        areas[inside_regress_range == 0] = INF
        min_area, min_area_inds = areas.min(dim=1)
        labels = gt_labels[min_area_inds]
        labels[min_area == INF] = self.num_classes
        bbox_targets = bbox_targets[range(num_points), min_area_inds]
        return labels, bbox_targets

    def centerness_target(self, pos_bbox_targets):
        """fcos_head.py:560-576."""
        left_right, top_bottom = pos_bbox_targets[:, [0, 2]], pos_bbox_targets[:, [1, 3]]
        return torch.sqrt((left_right.min(dim=-1)[0] / left_right.max(dim=-1)[0]) *
                          (top_bottom.min(dim=-1)[0] / top_bottom.max(dim=-1)[0]))

    # ------------------------------------------------------------------ loss
    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        if self._fused_loss_ok(cls_scores, bbox_preds, centernesses):
            return self.loss_fused(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas)
        return self.loss_tensor(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)

    def _fused_loss_ok(self, cls_scores, bbox_preds, centernesses):
        """htd_fcos_loss covers FocalLoss + IoULoss / GIoULoss + sigmoid CrossEntropyLoss without class weight, all with mean
        reduction, on maps that `_fused_maps_ok` takes."""
        lc, lb, lt = self.loss_cls, self.loss_bbox, self.loss_centerness
        return getattr(self, 'fused_loss', FCOS_FUSED) and \
            type(lc).__name__ == 'FocalLoss' and lc.reduction == 'mean' and \
            type(lb).__name__ in M.FCOS_BOX_KINDS and lb.reduction == 'mean' and \
            type(lt).__name__ == 'CrossEntropyLoss' and lt.use_sigmoid and lt.reduction == 'mean' and lt.class_weight is None and \
            self._fused_maps_ok(cls_scores, bbox_preds, centernesses)

    def loss_tensor(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """fcos_head.py:159-253, in the reference's order of operations."""
        assert len(cls_scores) == len(bbox_preds) == len(centernesses)
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        all_level_points = self.get_points(featmap_sizes, bbox_preds[0].dtype, bbox_preds[0].device)
        labels, bbox_targets = self.get_targets(all_level_points, gt_bboxes, gt_labels)
        num_imgs = cls_scores[0].size(0)
        flatten_cls_scores = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels) for c in cls_scores])
        flatten_bbox_preds = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds])
        flatten_centerness = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in centernesses])
        flatten_labels, flatten_bbox_targets = torch.cat(labels), torch.cat(bbox_targets)
        flatten_points = torch.cat([points.repeat(num_imgs, 1) for points in all_level_points])
        bg_class_ind = self.num_classes
        pos_inds = ((flatten_labels >= 0) & (flatten_labels < bg_class_ind)).nonzero().reshape(-1)
        num_pos = len(pos_inds)
        loss_cls = self.loss_cls(flatten_cls_scores, flatten_labels, avg_factor=num_pos + num_imgs)
        pos_bbox_preds, pos_centerness = flatten_bbox_preds[pos_inds], flatten_centerness[pos_inds]
        if num_pos > 0:
            pos_bbox_targets = flatten_bbox_targets[pos_inds]
            pos_centerness_targets = self.centerness_target(pos_bbox_targets)
            pos_points = flatten_points[pos_inds]
            loss_bbox = self.loss_bbox(distance2bbox(pos_points, pos_bbox_preds), distance2bbox(pos_points, pos_bbox_targets),
                                       weight=pos_centerness_targets, avg_factor=pos_centerness_targets.sum())
            loss_centerness = self.loss_centerness(pos_centerness, pos_centerness_targets)
        else:
            loss_bbox, loss_centerness = pos_bbox_preds.sum(), pos_centerness.sum()
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness)

    def loss_fused(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas):
        from ..core.bbox import pad_gt_batch
        assert len(cls_scores) == len(bbox_preds) == len(centernesses) == len(self.strides)
        gts, gt_valid, labels = pad_gt_batch(gt_bboxes, gt_labels)
        targets = M.fcos_targets([f.size()[-2:] for f in cls_scores], self.strides, self.regress_ranges, gts, gt_valid,
                                 self.center_sampling, self.center_sample_radius, self.norm_on_bbox)
        assigned, bbox_targets, ctr_targets, num_pos, norm = targets
        self._last_targets = targets            # exposed for tests
        lc, lb = self.loss_cls, self.loss_bbox
        loss_cls, loss_bbox, loss_centerness = M.fcos_loss(
            cls_scores, bbox_preds, centernesses, self.strides, labels, assigned, bbox_targets, ctr_targets, norm,
            M.FCOS_BOX_KINDS[type(lb).__name__], lb.eps, lc.gamma, lc.alpha, lc.loss_weight, lb.loss_weight,
            self.loss_centerness.loss_weight)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness)

    # ------------------------------------------------------------------ boxes
    def _bbox_priors(self, featmap_sizes, dtype, device):
        return self.get_points(featmap_sizes, dtype, device)

    def _bbox_decode(self, points, distances, img_shape):
        return distance2bbox(points, distances, max_shape=img_shape)

    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg=None, rescale=False, with_nms=True):
        """fcos_head.py:255-401 -> list (per image) of (dets (k, 5), labels (k,)), the centerness as score factor of the ranking
        and of the NMS."""
        return self._get_bboxes(cls_scores, bbox_preds, centernesses, img_metas, cfg, rescale, with_nms)
