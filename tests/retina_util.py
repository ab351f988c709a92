"""Shared by tests/golden/make_golden_retinanet.py, tests/test_retinanet.py and tests/test_gpu_retinanet.py: the inputs of the
RetinaNet fixture (tests/golden/retinanet.npz), re-created from seeds so the fixture holds results only."""
import torch

import dense_fixture_util as D
from dense_fixture_util import CFG_KEYS, LEVEL_SIZES  # noqa: F401
from golden_util import seeded_tensor

CONFIG = 'configs/retinanet/retinanet_r50_fpn_1x_coco.py'
EXTRA_GRAD_KEYS = ('neck.fpn_convs.3.conv.weight', 'neck.fpn_convs.4.conv.weight', 'bbox_head.cls_convs.0.conv.weight',
                   'bbox_head.reg_convs.3.conv.weight', 'bbox_head.retina_cls.weight', 'bbox_head.retina_cls.bias',
                   'bbox_head.retina_reg.weight', 'bbox_head.retina_reg.bias')
FOCAL_PARAMS = ((2.0, 0.25), (1.5, 0.25), (2.0, 0.5), (1.5, 0.5))          # (gamma, alpha)
AVG = 37.0
CLS_BIAS_SHIFT = 5.0


# the fixture's weights (dense_fixture_util): the classification layer scaled by the factor the fixture records and its bias lowered
# by CLS_BIAS_SHIFT (plainly seeded, its logits saturate the sigmoid: the ranking keys crowd at 1 and every score passes the
# threshold; a RetinaNet starts from sigmoid(bias) = 0.01)
FIXTURE = dict(edits=(('bbox_head.retina_cls.weight', 'mul', 'cls_scale'), ('bbox_head.retina_cls.bias', 'sub', CLS_BIAS_SHIFT)))


def load_fixture_weights_(det, cls_scale):
    return D.load_fixture_weights(det, **FIXTURE, cls_scale=cls_scale)


def fixture_state(keys, shapes, cls_scale):
    return D.fixture_state(keys, shapes, **FIXTURE, cls_scale=cls_scale)


def grad_keys(det):
    return D.grad_keys(det, EXTRA_GRAD_KEYS)


def focal_rows(n=64, C=80):
    """pred (n, C) fp32, labels (n,) int64 with C = background, weight (n,): logits at +-30 and +-90 in the label's column and
    beside it, background rows, rows of weight 0."""
    pred = seeded_tensor(f'retina.focal.pred.{n}.{C}', (n, C), scale=2.0)
    u = seeded_tensor(f'retina.focal.u.{n}.{C}', (n, 2), kind='rand')
    labels = torch.where(u[:, 0] < 0.6, (u[:, 1] * C).long().clamp(max=C - 1), torch.full((n, ), C, dtype=torch.long))
    if n > 1:
        labels[1] = C
    weight = 0.5 + seeded_tensor(f'retina.focal.w.{n}.{C}', (n, ), kind='rand')
    weight[3::5] = 0.
    extremes = (30., -30., 90., -90.)
    for i, v in enumerate(extremes):
        r = (2 * i) % n
        c = int(labels[r]) if int(labels[r]) < C else 0
        pred[r, c] = v                          # in the target column (or a background row's first column)
        pred[(2 * i + 1) % n, (c + 1) % C] = v  # and in a column that is not the target
    return pred, labels, weight


def onehot(labels, C):
    return labels.view(-1, 1) == torch.arange(C).view(1, -1)


def head_maps(B=2, C=80, na=9, sizes=LEVEL_SIZES, tag='retina.head'):
    """Seeded head outputs: per level (B, na * C, h, w) logits and (B, na * 4, h, w) deltas, fp32 on the CPU."""
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, na * C, h, w), scale=2.0) - 2.0 for l, (h, w) in enumerate(sizes)]
    reg = [seeded_tensor(f'{tag}.reg{l}', (B, na * 4, h, w), scale=0.5) for l, (h, w) in enumerate(sizes)]
    return cls, reg


def focal_ref(pred, labels, weight, gamma, alpha, dtype=torch.float64):
    """The reference's arithmetic (focal_loss.py:33-39) with autograd in a chosen precision -> (element losses, gradient of their
    sum); fp32 gives the reference's own rounding error on a case."""
    x = pred.detach().cpu().to(dtype).requires_grad_()
    t = onehot(labels.cpu(), x.size(1)).to(dtype)
    s = x.sigmoid()
    pt = (1 - s) * t + s * (1 - t)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none') * (alpha * t + (1 - alpha) * (1 - t)) * \
        pt.pow(gamma)
    if weight is not None:
        loss = loss * weight.cpu().to(dtype).view(-1, 1)
    g, = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), g


# ---------------------------------------------------------------------------- the head-kernel case
HEAD_CASE_SIZES = ((4, 5), (2, 3), (1, 2), (1, 1), (1, 1))
HEAD_CASE_STRIDES = (8, 16, 32, 64, 128)


def head_case(B=3, C=80, na=9, K=4, reg_pad=4, sizes=HEAD_CASE_SIZES, strides=HEAD_CASE_STRIDES, scale=1.0, tag='retina.case'):
    """Inputs of htd_retina_loss on five small levels (32 x 40 images): anchors of the RetinaNet generator, K = 4 gt slots with
    image 1 empty, image 2's gts far from every anchor's reach (no positive: the max(., 1) clamp) and the last 30 anchors of
    image 0 invalid.  -> dict of CPU tensors; `assigned` comes from the tensor form of MaxIoUAssigner (0.5 / 0.4 / 0, low-quality
    matches on), with image 2's matches removed by hand."""
    from htd_amd.core.anchor import AnchorGenerator
    from htd_amd.core.bbox import MaxIoUAssigner, _batched_max_iou_assign_tensor
    gen = AnchorGenerator(strides=list(strides), ratios=[0.5, 1.0, 2.0], octave_base_scale=4, scales_per_octave=3)
    anchors = torch.cat(gen.grid_anchors(sizes, device='cpu'))
    A = anchors.size(0)
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, na * C, h, w), scale=2.0) - 1.0 for l, (h, w) in enumerate(sizes)]
    reg = [seeded_tensor(f'{tag}.reg{l}', (B, na * 4 + reg_pad, h, w), scale=0.5) for l, (h, w) in enumerate(sizes)]
    gts = torch.zeros(B, K, 4)
    gts[0] = torch.tensor([[2., 3., 30., 28.], [10., 8., 36., 20.], [0., 0., 14., 12.], [20., 18., 39., 31.]])
    if B > 2:
        gts[2, :2] = torch.tensor([[4., 4., 26., 30.], [12., 2., 38., 24.]])
    gts = gts * scale                       # (`scale`: the same boxes on a larger image, for the cases with more rows)
    gt_valid = torch.tensor([[1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0]], dtype=torch.bool)[:B]
    gt_labels = torch.tensor([[3, 79, 0, 41], [0, 0, 0, 0], [7, 12, 0, 0]])[:B]
    inside = torch.ones(B, A, dtype=torch.bool)
    inside[0, -30:] = False
    assigner = MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0., ignore_iof_thr=-1)
    assigned, _ = _batched_max_iou_assign_tensor(assigner, anchors, inside, gts, gt_valid)
    if B > 2:
        assigned[2] = assigned[2].clamp(max=0)
    return dict(cls=cls, reg=reg, anchors=anchors, gts=gts, gt_labels=gt_labels, assigned=assigned, na=na, C=C, reg_pad=reg_pad)


def head_ref(case, gamma, alpha, pos_weight, box_loss, beta, cls_weight, box_weight, dtype=torch.float64,
             means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """The tensor formulation of the head loss in `dtype` -> dict(sums (2,), avg, gcls list, greg list (without padding))."""
    from htd_amd.core.bbox import bbox2delta
    na, C = case['na'], case['C']
    cls = [c.detach().to(dtype).requires_grad_() for c in case['cls']]
    reg = [r[:, :na * 4].detach().to(dtype).requires_grad_() for r in case['reg']]
    assigned, anchors = case['assigned'], case['anchors'].to(dtype)
    B, A = assigned.shape
    x = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1, C) for c in cls], 1)
    d = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, 4) for r in reg], 1)
    pos = assigned > 0
    gi = (assigned - 1).clamp(min=0)
    labels = torch.where(pos, torch.gather(case['gt_labels'], 1, gi), torch.full_like(assigned, C))
    lw = (assigned >= 0).to(dtype) * torch.where(pos & (pos_weight > 0), torch.full((), float(max(pos_weight, 0.)), dtype=dtype),
                                                  torch.ones((), dtype=dtype))
    t = onehot(labels.reshape(-1), C).to(dtype)
    xf = x.reshape(-1, C)
    s = xf.sigmoid()
    pt = (1 - s) * t + s * (1 - t)
    focal = torch.nn.functional.binary_cross_entropy_with_logits(xf, t, reduction='none') * \
        (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma) * lw.reshape(-1, 1)
    gt_of = torch.gather(case['gts'].to(dtype), 1, gi[..., None].expand(B, A, 4))
    safe = torch.where(pos[..., None], gt_of, anchors[None].expand(B, A, 4))
    tgt = bbox2delta(anchors[None].expand(B, A, 4).reshape(-1, 4), safe.reshape(-1, 4), means, stds).view(B, A, 4)
    diff = (d - tgt).abs()
    box = diff if box_loss == 1 else torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    box = box * pos[..., None].to(dtype)
    avg = float(sum(max(int(n), 1) for n in pos.sum(1)))
    s_cls, s_box = focal.sum(), box.sum()
    (cls_weight * s_cls / avg + box_weight * s_box / avg).backward()
    return dict(sums=torch.stack([s_cls.detach(), s_box.detach()]), avg=avg, num_pos=pos.sum(1),
                gcls=[c.grad for c in cls], greg=[r.grad if r.grad is not None else torch.zeros_like(r) for r in reg])
