"""FoveaHead and FeatureAlign: the anchor-free head of FoveaBox.

Reference: dense_heads/fovea_head.py:13-341 (FeatureAlign :13-39, layers :65-103, forward_single :110-121, the points :123-125,
loss :127-175, get_targets / _get_target_single :177-258, get_bboxes :260-341).  Same registry name, constructor kwargs and
defaults, state_dict keys (cls_convs.N.conv/gn, reg_convs.N..., conv_cls, conv_reg, feature_adaption.conv_offset.weight,
feature_adaption.conv_adaption.weight) and return structures.

The target rule paints, level by level, the shrunk rectangle of every gt whose `gt_areas` = sqrt(w * h) lies in the level's scale
range, larger ones first, so a point goes to the smallest gt_areas that holds it.  The reference's `torch.sort(-gt_areas)` is not
stable and leaves equal sizes undefined; here they are defined: among equal gt_areas the higher gt index wins, what a stable sort
paints last.  The targets of background points are exactly 0 (the reference leaves uninitialised memory there; no loss reads it).

`loss` has two forms, like FCOSHead.loss, and `_fused_loss_ok` is the one rule between them.  `loss_tensor` is the reference's
order of operations and works on the CPU, in fp64 and with any loss modules.  `loss_fused` -- FocalLoss with SmoothL1Loss, both
with mean reduction, fp32 channels_last GPU maps -- assigns the whole batch in one launch (htd_fovea_targets: no sort, no
per-gt slicing, the two averaging factors left on the device) and takes both losses and both gradient maps of all levels in one
more (htd_fovea_loss): no permute, concatenation, gather or nonzero() of the predictions, no host read.

`FeatureAlign` (the `with_deform` form) feeds each level's input through a deformable convolution whose offsets are a bias-free
1 x 1 convolution of exp(bbox_pred); on fp32 channels_last GPU maps one autograd function around htd_fovea_align_fwd / _bwd turns
the regression logits into the offsets, elsewhere `conv_offset(shape)` is the reference's tensor form.

`get_bboxes` is BaseDenseHead._get_bboxes, which all dense heads share: it ranks by max_c sigmoid(cls) without a score factor, the
priors are rows of x, y, stride and base edge, and the decode takes the exp() of the kept predictions.
"""
import os

import torch
import torch.nn as nn

from .. import mmcv_ops as M
from ..dcn import DeformConv2d, deform_conv2d
from ..registry import HEADS
from .anchor_free_heads import AnchorFreeHead
from .bricks import Conv2d, ConvModule, normal_init

FOVEA_FUSED = os.environ.get('HTD_FOVEA_FUSED', '1') != '0'         # 0: the tensor-path loss and offsets (A/B runs)


class FeatureAlign(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, deform_groups=4):
        super().__init__()
        offset_channels = kernel_size * kernel_size * 2
        self.conv_offset = nn.Conv2d(4, deform_groups * offset_channels, 1, bias=False)
        self.conv_adaption = DeformConv2d(in_channels, out_channels, kernel_size=kernel_size, padding=(kernel_size - 1) // 2,
                                          deform_groups=deform_groups)
        self.relu = nn.ReLU(inplace=True)
        self.deform_groups, self.kernel_size = deform_groups, kernel_size

    def init_weights(self):
        normal_init(self.conv_offset, std=0.1)
        normal_init(self.conv_adaption, std=0.01)

    def _kernel_ok(self, logits):
        return logits is not None and getattr(self, 'fused', FOVEA_FUSED) and logits.is_cuda and \
            logits.dtype == torch.float32 and self.conv_offset.weight.dtype == torch.float32 and self.kernel_size == 3 and \
            1 <= self.deform_groups <= 8 and M.nhwc_channel_stride(logits) is not None

    def offsets(self, shape=None, logits=None):
        """conv_offset(shape) with shape = exp(logits): the kernels when the logits are given as fp32 channels_last GPU maps,
        the tensor form otherwise."""
        if self._kernel_ok(logits):
            return M.fovea_align(logits, self.conv_offset.weight)
        return self.conv_offset(logits.exp() if shape is None else shape)

    def forward(self, x, shape=None, logits=None):
        """fovea_head.py:36-39; `logits` (bbox_pred itself, in place of shape = bbox_pred.exp()) lets the offsets take the kernels."""
        offset = self.offsets(shape, logits)
        m = self.conv_adaption
        if x.is_cuda:                       # the ReLU in the epilogue of the convolution's GEMM
            return deform_conv2d(x, offset, m.weight, m.stride, m.padding, m.dilation, m.groups, m.deform_groups, relu=True)
        return self.relu(m(x, offset))


@HEADS.register_module()
class FoveaHead(AnchorFreeHead):
    def __init__(self, num_classes, in_channels, base_edge_list=(16, 32, 64, 128, 256),
                 scale_ranges=((8, 32), (16, 64), (32, 128), (64, 256), (128, 512)), sigma=0.4, with_deform=False, deform_groups=4,
                 **kwargs):
        self.base_edge_list, self.scale_ranges, self.sigma = base_edge_list, scale_ranges, sigma
        self.with_deform, self.deform_groups = with_deform, deform_groups
        super().__init__(num_classes, in_channels, **kwargs)

    def _init_layers(self):
        """fovea_head.py:65-103."""
        self._build_towers('reg_convs')
        self.conv_reg = Conv2d(self.feat_channels, 4, 3, padding=1)
        if not self.with_deform:
            self._build_towers('cls_convs')
            self.conv_cls = Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)
        else:
            wide = self.feat_channels * 4
            self.cls_convs = nn.ModuleList([
                ConvModule(self.feat_channels, wide, 3, stride=1, padding=1, conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                           bias=self.norm_cfg is None),
                ConvModule(wide, wide, 1, stride=1, padding=0, conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                           bias=self.norm_cfg is None)])
            self.feature_adaption = FeatureAlign(self.feat_channels, self.feat_channels, kernel_size=3,
                                                 deform_groups=self.deform_groups)
            self.conv_cls = Conv2d(int(wide), self.cls_out_channels, 3, padding=1)

    def init_weights(self):
        super().init_weights()
        if self.with_deform:
            self.feature_adaption.init_weights()

    # ------------------------------------------------------------------ forward
    def forward_single(self, x):
        """fovea_head.py:110-121 -> cls_score, bbox_pred (log distances in units of the level's base edge)."""
        if x.dtype != torch.float32:             # a bf16 pyramid: the towers and all box / loss arithmetic stay fp32
            x = x.float()
        cls_feat = reg_feat = x
        for reg_layer in self.reg_convs:
            reg_feat = reg_layer(reg_feat)
        bbox_pred = self.conv_reg(reg_feat)
        if self.with_deform:
            cls_feat = self.feature_adaption(cls_feat, logits=bbox_pred)
        for cls_layer in self.cls_convs:
            cls_feat = cls_layer(cls_feat)
        return self.conv_cls(cls_feat), bbox_pred

    def _get_points_single(self, *args, **kwargs):
        y, x = super()._get_points_single(*args, **kwargs)
        return y + 0.5, x + 0.5

    # ------------------------------------------------------------------ targets
    def get_targets(self, gt_bbox_list, gt_label_list, featmap_sizes, points):
        """fovea_head.py:177-197 -> (labels, bbox_targets), level after level and within a level image after image."""
        per_image = [self._get_target_single(boxes, labels, featmap_size_list=featmap_sizes, point_list=points)
                     for boxes, labels in zip(gt_bbox_list, gt_label_list)]
        num_levels = len(featmap_sizes)
        labels = [lab[lvl].flatten() for lvl in range(num_levels) for lab, _ in per_image]
        targets = [tgt[lvl].reshape(-1, 4) for lvl in range(num_levels) for _, tgt in per_image]
        return torch.cat(labels), torch.cat(targets)

    def _fovea_rects(self, boxes, height, width):
        """fovea_head.py:228-242: (K, 4) boxes in map units -> (K, 4) int64 left, right, top, down of the shrunk rectangles, clamped
        to the map.  Every operation is rounded on its own; `1 -+ sigma` is a Python float that meets the tensor's dtype."""
        half_w = 0.5 * (boxes[:, 2] - boxes[:, 0])
        half_h = 0.5 * (boxes[:, 3] - boxes[:, 1])
        inner, outer = 1 - self.sigma, 1 + self.sigma
        left = torch.ceil(boxes[:, 0] + inner * half_w - 0.5).long().clamp(0, width - 1)
        right = torch.floor(boxes[:, 0] + outer * half_w - 0.5).long().clamp(0, width - 1)
        top = torch.ceil(boxes[:, 1] + inner * half_h - 0.5).long().clamp(0, height - 1)
        down = torch.floor(boxes[:, 1] + outer * half_h - 0.5).long().clamp(0, height - 1)
        return torch.stack([left, right, top, down], 1)

    def _get_target_single(self, gt_bboxes_raw, gt_labels_raw, featmap_size_list=None, point_list=None):
        """fovea_head.py:199-258 for one image -> per level labels (h, w) and log targets (h, w, 4).  The rectangles are painted
        in descending order of gt_areas under a stable sort (equal sizes: the higher index last, so it wins); the targets start
        as ones, so the background holds log 1 = 0."""
        w_raw = gt_bboxes_raw[:, 2] - gt_bboxes_raw[:, 0]
        h_raw = gt_bboxes_raw[:, 3] - gt_bboxes_raw[:, 1]
        gt_areas = torch.sqrt(w_raw * h_raw)
        label_list, bbox_target_list = [], []
        levels = zip(self.base_edge_list, self.scale_ranges, self.strides, featmap_size_list, point_list)
        for base_len, (lower_bound, upper_bound), stride, featmap_size, (y, x) in levels:
            height, width = int(featmap_size[0]), int(featmap_size[1])
            labels = gt_labels_raw.new_full((height, width), self.num_classes)
            bbox_targets = gt_bboxes_raw.new_ones(height, width, 4)
            on_level = ((gt_areas >= lower_bound) & (gt_areas <= upper_bound)).nonzero().flatten()
            if len(on_level) > 0:
                order = on_level[torch.sort(-gt_areas[on_level], stable=True)[1]]           # largest first
                rects = self._fovea_rects(gt_bboxes_raw[order, :] / stride, height, width).tolist()
                sx, sy = stride * x, stride * y
                for (left, right, top, down), label, box in zip(rects, gt_labels_raw[order], gt_bboxes_raw[order, :]):
                    rows, cols = slice(top, down + 1), slice(left, right + 1)      # empty when left > right or top > down
                    labels[rows, cols] = label
                    bbox_targets[rows, cols, 0] = (sx[rows, cols] - box[0]) / base_len
                    bbox_targets[rows, cols, 1] = (sy[rows, cols] - box[1]) / base_len
                    bbox_targets[rows, cols, 2] = (box[2] - sx[rows, cols]) / base_len
                    bbox_targets[rows, cols, 3] = (box[3] - sy[rows, cols]) / base_len
                bbox_targets = bbox_targets.clamp(min=1. / 16, max=16.)
            label_list.append(labels)
            bbox_target_list.append(torch.log(bbox_targets))
        return label_list, bbox_target_list

    # ------------------------------------------------------------------ loss
    def loss(self, cls_scores, bbox_preds, gt_bbox_list, gt_label_list, img_metas, gt_bboxes_ignore=None):
        if self._fused_loss_ok(cls_scores, bbox_preds):
            return self.loss_fused(cls_scores, bbox_preds, gt_bbox_list, gt_label_list, img_metas)
        return self.loss_tensor(cls_scores, bbox_preds, gt_bbox_list, gt_label_list, img_metas, gt_bboxes_ignore)

    def _fused_loss_ok(self, cls_scores, bbox_preds):
        """htd_fovea_loss covers FocalLoss + SmoothL1Loss, both with mean reduction, on maps that `_fused_maps_ok` takes."""
        lc, lb = self.loss_cls, self.loss_bbox
        return getattr(self, 'fused_loss', FOVEA_FUSED) and \
            type(lc).__name__ == 'FocalLoss' and lc.reduction == 'mean' and \
            type(lb).__name__ == 'SmoothL1Loss' and lb.reduction == 'mean' and lb.beta > 0 and \
            0 <= self.sigma <= 1 and self._fused_maps_ok(cls_scores, bbox_preds)

    def loss_tensor(self, cls_scores, bbox_preds, gt_bbox_list, gt_label_list, img_metas, gt_bboxes_ignore=None):
        """fovea_head.py:127-175, in the reference's order of operations."""
        assert len(cls_scores) == len(bbox_preds)
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        points = self.get_points(featmap_sizes, bbox_preds[0].dtype, bbox_preds[0].device)
        num_imgs = cls_scores[0].size(0)
        flatten_cls_scores = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels) for c in cls_scores])
        flatten_bbox_preds = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds])
        flatten_labels, flatten_bbox_targets = self.get_targets(gt_bbox_list, gt_label_list, featmap_sizes, points)
        # FG cat_id: [0, num_classes -1], BG cat_id: num_classes
        pos_inds = ((flatten_labels >= 0) & (flatten_labels < self.num_classes)).nonzero().view(-1)
        num_pos = len(pos_inds)
        loss_cls = self.loss_cls(flatten_cls_scores, flatten_labels, avg_factor=num_pos + num_imgs)
        if num_pos > 0:
            pos_bbox_preds = flatten_bbox_preds[pos_inds]
            pos_bbox_targets = flatten_bbox_targets[pos_inds]
            pos_weights = pos_bbox_targets.new_zeros(pos_bbox_targets.size()) + 1.0
            loss_bbox = self.loss_bbox(pos_bbox_preds, pos_bbox_targets, pos_weights, avg_factor=num_pos)
        else:
            loss_bbox = flatten_bbox_preds.sum() * 0           # exactly 0, with zero gradient maps
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox)

    def loss_fused(self, cls_scores, bbox_preds, gt_bbox_list, gt_label_list, img_metas):
        from ..core.bbox import pad_gt_batch
        assert len(cls_scores) == len(bbox_preds) == len(self.strides)
        gts, gt_valid, labels = pad_gt_batch(gt_bbox_list, gt_label_list)
        targets = M.fovea_targets([f.size()[-2:] for f in cls_scores], self.strides, self.base_edge_list, self.scale_ranges,
                                  self.sigma, gts, gt_valid)
        assigned, bbox_targets, num_pos, norm = targets
        self._last_targets = targets            # exposed for tests
        lc, lb = self.loss_cls, self.loss_bbox
        loss_cls, loss_bbox = M.fovea_loss(cls_scores, bbox_preds, labels, assigned, bbox_targets, norm, lb.beta, lc.gamma, lc.alpha,
                                           lc.loss_weight, lb.loss_weight)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox)

    # ------------------------------------------------------------------ boxes
    def _bbox_priors(self, featmap_sizes, dtype, device):
        """per level (n_l, 4) rows of x, y, stride and base edge: the reference's per-level numbers, one copy per point."""
        points = self.get_points(featmap_sizes, dtype, device, flatten=True)
        return [torch.stack([x, y, torch.full_like(x, stride), torch.full_like(x, base_len)], -1)
                for (y, x), stride, base_len in zip(points, self.strides, self.base_edge_list)]

    def _bbox_decode(self, priors, bbox_pred, img_shape):
        """fovea_head.py:311,319-327."""
        x, y, stride, base_len = priors.unbind(-1)
        bbox_pred = bbox_pred.exp()
        x1 = (stride * x - base_len * bbox_pred[:, 0]).clamp(min=0, max=img_shape[1] - 1)
        y1 = (stride * y - base_len * bbox_pred[:, 1]).clamp(min=0, max=img_shape[0] - 1)
        x2 = (stride * x + base_len * bbox_pred[:, 2]).clamp(min=0, max=img_shape[1] - 1)
        y2 = (stride * y + base_len * bbox_pred[:, 3]).clamp(min=0, max=img_shape[0] - 1)
        return torch.stack([x1, y1, x2, y2], -1)

    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=None, with_nms=True):
        """fovea_head.py:260-341 -> list (per image) of (dets (k, 5), labels (k,))."""
        return self._get_bboxes(cls_scores, bbox_preds, None, img_metas, cfg, rescale, with_nms)
