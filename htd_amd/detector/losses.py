"""Losses of the HTD path: CrossEntropyLoss (softmax / sigmoid), SmoothL1Loss, L1Loss, the IoU family on decoded boxes
(IoULoss, BoundedIoULoss, GIoULoss, DIoULoss, CIoULoss), FocalLoss, QualityFocalLoss, DistributionFocalLoss, GHMC, GHMR, accuracy.
Reference: mmdet/models/losses/{cross_entropy_loss.py:9-202, smooth_l1_loss.py:8-136, iou_loss.py:11-418,
utils.py:26-52, focal_loss.py:10-157, gfocal_loss.py:8-185, ghm_loss.py:8-172, accuracy.py:4-48}.  Same constructor kwargs and forward signature
(weight, avg_factor, reduction_override; the GHM pair has the reference's own, ghm_loss.py:50, :127)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..registry import LOSSES
from ..core.misc import const_tensor


def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        if reduction == 'mean':
            return loss.mean()
        return loss.sum() if reduction == 'sum' else loss
    if reduction == 'mean':
        return loss.sum() / avg_factor
    if reduction != 'none':
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss


def cross_entropy(pred, label, weight=None, reduction='mean', avg_factor=None, class_weight=None):
    loss = F.cross_entropy(pred, label, weight=class_weight, reduction='none')
    return weight_reduce_loss(loss, None if weight is None else weight.float(), reduction, avg_factor)


def binary_cross_entropy(pred, label, weight=None, reduction='mean', avg_factor=None, class_weight=None):
    if pred.dim() != label.dim():
        # integer labels -> one-hot columns; out-of-range labels (background) give an all-zero row
        C = pred.size(-1)
        onehot = (label.view(-1, 1) == torch.arange(C, device=label.device).view(1, -1))
        label = onehot
        weight = None if weight is None else weight.view(-1, 1).expand(weight.size(0), C)
    loss = F.binary_cross_entropy_with_logits(pred, label.float(), pos_weight=class_weight, reduction='none')
    return weight_reduce_loss(loss, None if weight is None else weight.float(), reduction, avg_factor)


@LOSSES.register_module()
class CrossEntropyLoss(nn.Module):
    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0):
        super().__init__()
        assert not use_mask, 'mask cross-entropy is outside the HTD path'
        self.use_sigmoid, self.use_mask, self.reduction = use_sigmoid, use_mask, reduction
        self.loss_weight, self.class_weight = loss_weight, class_weight
        self.cls_criterion = binary_cross_entropy if use_sigmoid else cross_entropy

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        cw = const_tensor(self.class_weight, cls_score.device, cls_score.dtype) if self.class_weight is not None else None
        return self.loss_weight * self.cls_criterion(cls_score, label, weight, class_weight=cw, reduction=reduction,
                                                     avg_factor=avg_factor, **kwargs)


def smooth_l1_loss(pred, target, weight=None, beta=1.0, reduction='mean', avg_factor=None):
    assert beta > 0
    assert pred.size() == target.size() and target.numel() > 0
    diff = torch.abs(pred - target)
    loss = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


@LOSSES.register_module()
class SmoothL1Loss(nn.Module):
    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * smooth_l1_loss(pred, target, weight, beta=self.beta, reduction=reduction,
                                                 avg_factor=avg_factor, **kwargs)


def l1_loss(pred, target, weight=None, reduction='mean', avg_factor=None):
    assert pred.size() == target.size() and target.numel() > 0
    return weight_reduce_loss(torch.abs(pred - target), weight, reduction, avg_factor)


@LOSSES.register_module()
class L1Loss(nn.Module):
    """smooth_l1_loss.py:97-136: |pred - target|; zero with a zero gradient where pred == target (autograd's slope of |x| at 0)."""

    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * l1_loss(pred, target, weight, reduction=reduction, avg_factor=avg_factor)


# ---------------------------------------------------------------- IoU family (iou_loss.py), per-row losses on (n, 4) boxes
def iou_loss(pred, target, eps=1e-6):
    """-log(IoU) in the reference's own edit (iou_loss.py:27-29): IoUs of at most 0.1 are lifted by 0.1 before the log."""
    from ..core.bbox import bbox_overlaps
    ious = bbox_overlaps(pred, target, is_aligned=True).clamp(min=eps)
    ious = torch.where(ious > 0.1, ious, 0.1 + ious)
    return -ious.log()


def bounded_iou_loss(pred, target, beta=0.2, eps=1e-3):
    """iou_loss.py:34-75 -> (n, 4): smooth-L1 of the bounded IoU of centre x / y and width / height."""
    pred_ctrx, pred_ctry = (pred[:, 0] + pred[:, 2]) * 0.5, (pred[:, 1] + pred[:, 3]) * 0.5
    pred_w, pred_h = pred[:, 2] - pred[:, 0], pred[:, 3] - pred[:, 1]
    with torch.no_grad():
        target_ctrx, target_ctry = (target[:, 0] + target[:, 2]) * 0.5, (target[:, 1] + target[:, 3]) * 0.5
        target_w, target_h = target[:, 2] - target[:, 0], target[:, 3] - target[:, 1]
    dx, dy = target_ctrx - pred_ctrx, target_ctry - pred_ctry
    loss_dx = 1 - torch.max((target_w - 2 * dx.abs()) / (target_w + 2 * dx.abs() + eps), torch.zeros_like(dx))
    loss_dy = 1 - torch.max((target_h - 2 * dy.abs()) / (target_h + 2 * dy.abs() + eps), torch.zeros_like(dy))
    loss_dw = 1 - torch.min(target_w / (pred_w + eps), pred_w / (target_w + eps))
    loss_dh = 1 - torch.min(target_h / (pred_h + eps), pred_h / (target_h + eps))
    loss_comb = torch.stack([loss_dx, loss_dy, loss_dw, loss_dh], dim=-1).view(loss_dx.size(0), -1)
    return torch.where(loss_comb < beta, 0.5 * loss_comb * loss_comb / beta, loss_comb - 0.5 * beta)


def giou_loss(pred, target, eps=1e-7):
    from ..core.bbox import bbox_overlaps
    return 1 - bbox_overlaps(pred, target, mode='giou', is_aligned=True, eps=eps)


def _iou_and_centre_term(pred, target, eps):
    """The part diou_loss and ciou_loss share (iou_loss.py:112-143, 167-201): IoU with eps added to the union, and the squared
    centre distance over the squared diagonal of the enclosing box (eps added)."""
    wh = (torch.min(pred[:, 2:], target[:, 2:]) - torch.max(pred[:, :2], target[:, :2])).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    ap = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    ag = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    ious = overlap / (ap + ag - overlap + eps)
    enclose_wh = (torch.max(pred[:, 2:], target[:, 2:]) - torch.min(pred[:, :2], target[:, :2])).clamp(min=0)
    c2 = enclose_wh[:, 0]**2 + enclose_wh[:, 1]**2 + eps
    left = ((target[:, 0] + target[:, 2]) - (pred[:, 0] + pred[:, 2]))**2 / 4
    right = ((target[:, 1] + target[:, 3]) - (pred[:, 1] + pred[:, 3]))**2 / 4
    return ious, (left + right) / c2


def diou_loss(pred, target, eps=1e-7):
    ious, centre = _iou_and_centre_term(pred, target, eps)
    return 1 - (ious - centre)


def ciou_loss(pred, target, eps=1e-7):
    ious, centre = _iou_and_centre_term(pred, target, eps)
    w1, h1 = pred[:, 2] - pred[:, 0], pred[:, 3] - pred[:, 1] + eps          # eps on the heights only (iou_loss.py:196-197)
    w2, h2 = target[:, 2] - target[:, 0], target[:, 3] - target[:, 1] + eps
    v = (4 / math.pi**2) * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)
    # v == 0 makes the aspect term 0 with zero slope.  With pred == target (a gt-born positive with zero deltas) the fp32 IoU
    # rounds to 1 and the reference divides 0 by 0 there; the limit is taken instead (what its fp64 run gives), so every per-row
    # loss of finite boxes is finite and a zero weight really removes the row.  Everywhere else this is the same arithmetic.
    den = torch.where(v > 0, 1 - ious + v, torch.ones_like(v))
    return 1 - (ious - (centre + v**2 / den))


class _BoxLoss(nn.Module):
    """Common forward of the five modules (iou_loss.py:212-418).  The reference leaves early with (pred * weight).sum() when no
    weight is positive, which costs a host sync (`torch.any`); the weighted sum below gives the same exact 0 with zero
    gradients because every per-row loss of finite boxes is finite, so it is not reproduced."""
    per_row = True          # loss of shape (n,): an (n, 4) weight is reduced to its row mean

    def __init__(self, eps=1e-6, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.eps, self.reduction, self.loss_weight = eps, reduction, loss_weight

    def _loss(self, pred, target):
        raise NotImplementedError

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if self.per_row and weight is not None and weight.dim() > 1:
            assert weight.shape == pred.shape
            weight = weight.mean(-1)
        return self.loss_weight * weight_reduce_loss(self._loss(pred, target), weight, reduction, avg_factor)


@LOSSES.register_module()
class IoULoss(_BoxLoss):
    kind = 0

    def _loss(self, pred, target):
        return iou_loss(pred, target, eps=self.eps)


@LOSSES.register_module()
class BoundedIoULoss(_BoxLoss):
    kind, per_row = 1, False

    def __init__(self, beta=0.2, eps=1e-3, reduction='mean', loss_weight=1.0):
        super().__init__(eps, reduction, loss_weight)
        self.beta = beta

    def _loss(self, pred, target):
        return bounded_iou_loss(pred, target, beta=self.beta, eps=self.eps)


@LOSSES.register_module()
class GIoULoss(_BoxLoss):
    kind = 2

    def _loss(self, pred, target):
        return giou_loss(pred, target, eps=self.eps)


@LOSSES.register_module()
class DIoULoss(_BoxLoss):
    kind = 3

    def _loss(self, pred, target):
        return diou_loss(pred, target, eps=self.eps)


@LOSSES.register_module()
class CIoULoss(_BoxLoss):
    kind = 4

    def _loss(self, pred, target):
        return ciou_loss(pred, target, eps=self.eps)


# ---------------------------------------------------------------- focal loss (focal_loss.py:10-157)
def py_sigmoid_focal_loss(pred, target, weight=None, gamma=2.0, alpha=0.25, reduction='mean', avg_factor=None):
    """focal_loss.py:10-41, the reference's own arithmetic: pred (N, C) logits, target (N, C) one-hot."""
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction='none') * focal_weight
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


def sigmoid_focal_loss(pred, target, weight=None, gamma=2.0, alpha=0.25, reduction='mean', avg_factor=None):
    """focal_loss.py:44-87: pred (N, C) logits, target (N,) class indices with C = background, weight (N,), (N, C) or (N * C,).
    fp32 GPU tensors go through htd_sigmoid_focal_loss (a per-row weight and the sum inside the launch); everything else
    through the tensor formula on the one-hot target."""
    from .. import mmcv_ops as M
    N, C = pred.shape
    device_op = pred.is_cuda and pred.dtype == torch.float32
    if device_op and reduction != 'none' and (weight is None or weight.shape == (N, )):
        total = M.sigmoid_focal_loss(pred, target, gamma, alpha, None if weight is None else weight.float(), 'sum')
        if avg_factor is None:
            return total / max(N * C, 1) if reduction == 'mean' else total
        if reduction == 'mean':
            return total / avg_factor
        raise ValueError('avg_factor can not be used with reduction="sum"')
    if device_op:
        loss = M.sigmoid_focal_loss(pred, target, gamma, alpha, None, 'none')
    else:
        onehot = target.view(-1, 1) == torch.arange(C, device=target.device).view(1, -1)
        loss = py_sigmoid_focal_loss(pred, onehot, None, gamma, alpha, 'none')
    if weight is not None:
        if weight.shape != loss.shape:
            if weight.size(0) == loss.size(0):
                weight = weight.view(-1, 1)          # one weight per prior
            else:
                assert weight.numel() == loss.numel()
                weight = weight.view(loss.size(0), -1)
        assert weight.ndim == loss.ndim
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


@LOSSES.register_module()
class FocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, 'Only sigmoid focal loss supported now.'
        self.use_sigmoid, self.gamma, self.alpha = use_sigmoid, gamma, alpha
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * sigmoid_focal_loss(pred, target, weight, gamma=self.gamma, alpha=self.alpha,
                                                     reduction=reduction, avg_factor=avg_factor)


# ---------------------------------------------------------------- generalized focal losses (gfocal_loss.py:8-185)
def quality_focal_loss(pred, target, weight=None, beta=2.0, reduction='mean', avg_factor=None):
    """gfocal_loss.py:8-49 under weighted_loss: pred (N, C) joint class / quality logits, target = (label (N,) with C =
    background, score (N,) the quality of a positive's own class).  Every (row, class) is supervised by 0 under the modulating
    factor sigmoid^beta; a positive's own class by its score under |score - sigmoid|^beta.  Neither factor is detached.
    -> per-row sums, then weight (N,), reduction and avg_factor as weight_reduce_loss has them."""
    assert len(target) == 2, 'target for QFL must be a tuple of two elements: category label and quality label'
    label, score = target
    pred_sigmoid = pred.sigmoid()
    loss = F.binary_cross_entropy_with_logits(pred, pred_sigmoid.new_zeros(pred.shape), reduction='none') * pred_sigmoid.pow(beta)
    pos = ((label >= 0) & (label < pred.size(1))).nonzero().squeeze(1)
    pos_label = label[pos].long()
    scale_factor = score[pos] - pred_sigmoid[pos, pos_label]
    loss[pos, pos_label] = F.binary_cross_entropy_with_logits(pred[pos, pos_label], score[pos], reduction='none') * \
        scale_factor.abs().pow(beta)
    return weight_reduce_loss(loss.sum(dim=1, keepdim=False), weight, reduction, avg_factor)


def distribution_focal_loss(pred, label, weight=None, reduction='mean', avg_factor=None):
    """gfocal_loss.py:52-74 under weighted_loss: pred (N, n + 1) logits of the bins 0 .. n, label (N,) target distances in
    [0, n): the cross-entropies of the two neighbouring bins weighted by the distance to the other."""
    dis_left = label.long()
    dis_right = dis_left + 1
    weight_left = dis_right.float() - label
    weight_right = label - dis_left.float()
    loss = F.cross_entropy(pred, dis_left, reduction='none') * weight_left + \
        F.cross_entropy(pred, dis_right, reduction='none') * weight_right
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


@LOSSES.register_module()
class QualityFocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, beta=2.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, 'Only sigmoid in QFL supported now.'
        self.use_sigmoid, self.beta, self.reduction, self.loss_weight = use_sigmoid, beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * quality_focal_loss(pred, target, weight, beta=self.beta, reduction=reduction,
                                                     avg_factor=avg_factor)


@LOSSES.register_module()
class DistributionFocalLoss(nn.Module):
    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * distribution_focal_loss(pred, target, weight, reduction=reduction, avg_factor=avg_factor)


# ---------------------------------------------------------------- varifocal loss (varifocal_loss.py:8-131)
def varifocal_loss(pred, target, weight=None, alpha=0.75, gamma=2.0, iou_weighted=True, reduction='mean', avg_factor=None):
    """varifocal_loss.py:8-53: pred (N, C) logits, target (N, C) the IoU-aware classification score (the IoU at a positive's
    own class, 0 elsewhere).  An element with a positive target is weighted by the target (or by 1 without iou_weighted), every
    other one by alpha * |sigmoid - target|^gamma; then weight, reduction and avg_factor as weight_reduce_loss has them."""
    assert pred.size() == target.size()
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    positive = (target > 0.0).float()
    focal_weight = (target * positive if iou_weighted else positive) + \
        alpha * (pred_sigmoid - target).abs().pow(gamma) * (target <= 0.0).float()
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction='none') * focal_weight
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


@LOSSES.register_module()
class VarifocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, 'Only sigmoid varifocal loss supported now.'
        assert alpha >= 0.0
        self.use_sigmoid, self.alpha, self.gamma, self.iou_weighted = use_sigmoid, alpha, gamma, iou_weighted
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if not self.use_sigmoid:
            raise NotImplementedError
        return self.loss_weight * varifocal_loss(pred, target, weight, alpha=self.alpha, gamma=self.gamma,
                                                 iou_weighted=self.iou_weighted, reduction=reduction, avg_factor=avg_factor)


# ---------------------------------------------------------------- gradient harmonising losses (ghm_loss.py:8-172)
GHM_KERNEL_BINS = 64            # bins the kernels of csrc/ghm_loss.hip take


def _expand_onehot_labels(labels, label_weights, label_channels):
    """ghm_loss.py:8-16 without its nonzero(): (N,) class indices -> (N, C) binary targets (an index outside 0 .. C - 1, the
    background, gives an all-zero row) and the (N,) weights repeated along the classes."""
    onehot = labels.view(-1, 1) == torch.arange(label_channels, device=labels.device).view(1, -1)
    return onehot.to(labels.dtype), label_weights.view(-1, 1).expand(label_weights.size(0), label_channels)


def _ghm_weights(g, valid, tot, edges, bins, momentum, acc_sum):
    """The element weights of both GHM losses (ghm_loss.py:70-90, :151-168) without a host read: the bin of every valid
    element from the fp32 `edges` (edges[i] <= g < edges[i + 1]), integer bin counts, the moving average in the reference's
    own arithmetic -- fp32 `mmt * acc_sum[i]` plus the double `(1 - mmt) * num` rounded to fp32 -- applied to the filled bins
    only, and tot / acc / n per bin (tot / num with momentum 0, formed in double as the reference's Python floats are).
    tot: 0-dim float64 tensor, already clamped to >= 1.  -> (weights like g, counts (bins,) int64, n 0-dim int64)."""
    idx = torch.bucketize(g, edges.to(g.dtype), right=True) - 1
    idx = torch.where(valid & (idx >= 0) & (idx < bins), idx, torch.full_like(idx, bins))      # `bins`: in no bin
    counts = torch.stack([(idx == i).sum() for i in range(bins)])
    filled = counts > 0
    n = filled.sum()
    if momentum > 0:
        moved = momentum * acc_sum + ((1 - momentum) * counts.double()).float()
        acc_sum.copy_(torch.where(filled, moved, acc_sum))
        per_bin = (acc_sum.reciprocal() * tot.float()).to(g.dtype)         # `tot / tensor` is reciprocal() * tot in torch
    else:
        per_bin = (tot / counts.double().clamp(min=1)).to(g.dtype)
    per_bin = torch.where(filled, per_bin, torch.zeros_like(per_bin)) / n.clamp(min=1)
    return torch.cat([per_bin, per_bin.new_zeros(1)])[idx], counts, n


@LOSSES.register_module()
class GHMC(nn.Module):
    """ghm_loss.py:20-94.  forward(pred (N, C) logits, target (N,) class indices or (N, C) binary, label_weight (N,) or
    (N, C): an element is valid where its weight is > 0).  `avg_factor` and any further argument are ignored, as there.
    An fp32 GPU matrix with (N,) labels and (N,) weights goes through htd_ghmc_loss (bins <= 64); everything else through
    the tensor formulation, which reads nothing back to the host either.  `last` keeps (counts, tot, n) of the latest call."""

    def __init__(self, bins=10, momentum=0, use_sigmoid=True, loss_weight=1.0):
        super().__init__()
        self.bins, self.momentum = bins, momentum
        edges = torch.arange(bins + 1).float() / bins
        edges[-1] += 1e-6
        self.register_buffer('edges', edges)
        if momentum > 0:
            self.register_buffer('acc_sum', torch.zeros(bins))
        self.use_sigmoid = use_sigmoid
        if not self.use_sigmoid:
            raise NotImplementedError
        self.loss_weight = loss_weight

    def forward(self, pred, target, label_weight, *args, **kwargs):
        if pred.dim() != target.dim() and pred.is_cuda and pred.dtype == torch.float32 and label_weight.dim() == 1 and \
                self.bins <= GHM_KERNEL_BINS and self.edges.is_cuda:
            from .. import mmcv_ops as M
            return M.ghmc_loss(pred, target, label_weight, self.edges, self.bins, self.momentum,
                               self.acc_sum if self.momentum > 0 else None, self.loss_weight)
        if pred.dim() != target.dim():
            target, label_weight = _expand_onehot_labels(target, label_weight, pred.size(-1))
        target, label_weight = target.to(pred.dtype), label_weight.float()
        g = torch.abs(pred.sigmoid().detach() - target)
        valid = label_weight > 0
        tot = valid.sum().clamp(min=1).double()
        weights, counts, n = _ghm_weights(g, valid, tot, self.edges, self.bins, self.momentum, getattr(self, 'acc_sum', None))
        self.last = (counts, tot, n)
        loss = F.binary_cross_entropy_with_logits(pred, target, weights, reduction='sum') / tot.to(pred.dtype)
        return loss * self.loss_weight


@LOSSES.register_module()
class GHMR(nn.Module):
    """ghm_loss.py:98-172.  forward(pred, target, label_weight, avg_factor=None) on tensors of one shape; tot is the weight
    sum, `avg_factor` is ignored."""

    def __init__(self, mu=0.02, bins=10, momentum=0, loss_weight=1.0):
        super().__init__()
        self.mu, self.bins, self.momentum = mu, bins, momentum
        edges = torch.arange(bins + 1).float() / bins
        edges[-1] = 1e3
        self.register_buffer('edges', edges)
        if momentum > 0:
            self.register_buffer('acc_sum', torch.zeros(bins))
        self.loss_weight = loss_weight

    def forward(self, pred, target, label_weight, avg_factor=None):
        mu = self.mu
        diff = pred - target
        loss = torch.sqrt(diff * diff + mu * mu) - mu
        g = torch.abs(diff / torch.sqrt(mu * mu + diff * diff)).detach()
        valid = label_weight > 0
        tot = label_weight.float().sum().clamp(min=1).double()
        weights, counts, n = _ghm_weights(g, valid, tot, self.edges, self.bins, self.momentum, getattr(self, 'acc_sum', None))
        self.last = (counts, tot, n)
        return (loss * weights).sum() / tot.to(pred.dtype) * self.loss_weight


DECODED_BOX_LOSSES = (IoULoss, BoundedIoULoss, GIoULoss, DIoULoss, CIoULoss)       # index = `kind` of htd_roi_head_loss_decoded


def accuracy(pred, target, topk=1, thresh=None):
    assert isinstance(topk, (int, tuple))
    single = isinstance(topk, int)
    topk = (topk, ) if single else topk
    if pred.size(0) == 0:
        accu = [pred.new_tensor(0.) for _ in topk]
        return accu[0] if single else accu
    assert pred.ndim == 2 and target.ndim == 1 and pred.size(0) == target.size(0)
    maxk = max(topk)
    assert maxk <= pred.size(1), f'maxk {maxk} exceeds pred dimension {pred.size(1)}'
    pred_value, pred_label = pred.topk(maxk, dim=1)
    pred_label = pred_label.t()
    correct = pred_label.eq(target.view(1, -1).expand_as(pred_label))
    if thresh is not None:
        correct = correct & (pred_value > thresh).t()
    res = [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / pred.size(0)) for k in topk]
    return res[0] if single else res
