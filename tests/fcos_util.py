"""Shared by tests/golden/make_golden_fcos.py, tests/test_fcos.py and tests/test_gpu_fcos.py: the inputs of the FCOS fixture
(tests/golden/fcos.npz), re-created from seeds so the fixture holds results only, and restatements of the reference's target
assignment and loss in a chosen precision (pinned against the fixture by tests/test_fcos.py) for the cases of the GPU tests that
the fixture does not hold."""
import torch

import dense_fixture_util as D
from dense_fixture_util import CFG_KEYS, LEVEL_SIZES, STRIDES, levels_to_images, maps_to_rows, pad_gts  # noqa: F401
from golden_util import seeded_tensor

CONFIGS = dict(gn_head='configs/fcos/fcos_r50_caffe_fpn_gn-head_4x4_1x_coco.py',
               center='configs/fcos/fcos_center-normbbox-centeronreg-giou_r50_caffe_fpn_gn-head_4x4_1x_coco.py')
VARIANT_OF = dict(gn_head='gn-head', center='center-normbbox-centeronreg-giou')
EXTRA_GRAD_KEYS = ('neck.fpn_convs.3.conv.weight', 'neck.fpn_convs.4.conv.weight', 'bbox_head.cls_convs.0.conv.weight',
                   'bbox_head.reg_convs.3.conv.weight', 'bbox_head.conv_cls.weight', 'bbox_head.conv_cls.bias',
                   'bbox_head.conv_reg.weight', 'bbox_head.conv_reg.bias', 'bbox_head.conv_centerness.weight',
                   'bbox_head.conv_centerness.bias', 'bbox_head.scales.0.scale', 'bbox_head.scales.1.scale',
                   'bbox_head.scales.2.scale', 'bbox_head.scales.3.scale', 'bbox_head.scales.4.scale',
                   'bbox_head.cls_convs.1.gn.weight')
REG_BIAS_SHIFT = 2.5      # distances around exp(2.5) = 12 pixels: plainly seeded, the boxes of neighbouring points never overlap
INF = 1e8
RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF))         # the head's default
SMALL_RANGES = ((-1, 16), (16, 32), (32, 64), (64, 128), (128, INF))       # scaled to the 128 x 160 pyramid
# the two head-level variants: (box loss, center_sampling, norm_on_bbox, centerness_on_reg)
HEAD_VARIANTS = dict(iou=dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)),
                     giou=dict(loss_bbox=dict(type='GIoULoss', loss_weight=1.0), center_sampling=True, norm_on_bbox=True,
                               centerness_on_reg=True))
CASE_RADIUS = 0.75       # of the targets case: its ranges end at two strides, where the default 1.5 never clips a centre box
HEAD_TEST_CFG = dict(nms_pre=50, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
TARGET_COMBOS = ((False, False), (True, False), (False, True), (True, True))         # (center_sampling, norm_on_bbox)


def head_cfg(variant, num_classes=80, **extra):
    d = dict(type='FCOSHead', num_classes=num_classes, in_channels=256, stacked_convs=4, feat_channels=256, strides=list(STRIDES),
             loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
             loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
    d.update(HEAD_VARIANTS[variant])
    d.update(extra)
    return d


# the fixture's weights (dense_fixture_util): the level scales at 1 + a quarter of a seeded normal, the classification and centerness
# layers scaled and the classification bias lowered by the two figures the fixture records (plainly seeded, the logits saturate
# the sigmoid, the ranking keys crowd and thousands of scores lie around the score threshold)
FIXTURE = dict(scales=('scales', ),
               edits=(('bbox_head.conv_cls.weight', 'mul', 'scale'), ('bbox_head.conv_centerness.weight', 'mul', 'scale'),
                      ('bbox_head.conv_cls.bias', 'sub', 'bias_shift'), ('bbox_head.conv_reg.bias', 'add', REG_BIAS_SHIFT)))


def load_fixture_weights_(det, scale, bias_shift):
    return D.load_fixture_weights(det, **FIXTURE, scale=scale, bias_shift=bias_shift)


def fixture_state(keys, shapes, scale, bias_shift):
    return D.fixture_state(keys, shapes, **FIXTURE, scale=scale, bias_shift=bias_shift)


def grad_keys(det):
    return D.grad_keys(det, EXTRA_GRAD_KEYS)


def head_maps(variant, B=2, C=80, sizes=LEVEL_SIZES, strides=STRIDES, tag='fcos.head'):
    """Seeded head outputs, fp32 on the CPU: per level (B, C, h, w) logits, (B, 4, h, w) positive distances (pixels; stride
    units under norm_on_bbox, as the training forward gives them) and (B, 1, h, w) centerness logits."""
    norm = HEAD_VARIANTS[variant].get('norm_on_bbox', False)
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, C, h, w), scale=2.0) - 2.0 for l, (h, w) in enumerate(sizes)]
    reg = [(seeded_tensor(f'{tag}.reg{l}', (B, 4, h, w), scale=0.5)).exp() * (1.5 if norm else 1.5 * strides[l])
           for l, (h, w) in enumerate(sizes)]
    ctr = [seeded_tensor(f'{tag}.ctr{l}', (B, 1, h, w), scale=1.5) for l, (h, w) in enumerate(sizes)]
    return cls, reg, ctr


def targets_case():
    """Synthetic gts on the 128 x 160 pyramid with SMALL_RANGES -> (gts list, labels list).  Image 0: a box reaching past the
    image on every side, nested boxes, two boxes of equal area over the same points (30,40,70,60 / 40,30,60,70), a box whose left
    edge passes through the points of column x = 24; image 1: empty; images 2 and 3: boxes whose largest distance from a point
    falls exactly on each bound of the ranges (16 and 64 / 32 and 128), from below and from above."""
    g0 = [[-70., -10., 200., 140.], [10., 5., 150., 125.], [20., 30., 100., 100.], [60., 60., 100., 90.], [118., 8., 134., 24.],
          [30., 40., 70., 60.], [40., 30., 60., 70.], [24., 72., 56., 104.]]
    g2 = [[8., 8., 28., 28.], [8., 8., 40., 40.], [40., 40., 112., 112.], [32., 32., 160., 160.]]
    g3 = [[16., 16., 56., 56.], [16., 16., 80., 80.], [24., 24., 160., 160.], [-64., -64., 192., 192.]]
    gts = [torch.tensor(g0), torch.zeros(0, 4), torch.tensor(g2), torch.tensor(g3)]
    labels = [torch.tensor([3, 79, 0, 41, 7, 12, 12, 5]), torch.zeros(0, dtype=torch.long), torch.tensor([1, 2, 3, 4]),
              torch.tensor([9, 8, 7, 6])]
    return gts, labels


def points_of(sizes, strides, dtype=torch.float32):
    """(P, 2) level-major points (x, y) = (column, row) * stride + stride // 2, and (P,) the level of each."""
    pts, lvl = [], []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        y, x = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing='ij')
        pts.append(torch.stack((x.reshape(-1) * s, y.reshape(-1) * s), -1) + s // 2)
        lvl.append(torch.full((h * w, ), l, dtype=torch.long))
    return torch.cat(pts), torch.cat(lvl)


def targets_ref(sizes, strides, ranges, gts, valid, center_sampling=False, radius=1.5, norm_on_bbox=False, dtype=torch.float32):
    """fcos_head.py:476-576 restated on padded gts (B, K, 4) / valid (B, K) in `dtype`, one rounded operation at a time as the
    reference's tensors take them -> assigned (B, P) int32 (0 background, k + 1 = gt k), bbox_targets (B, P, 4), ctr_targets
    (B, P) (0 on background), all level-major."""
    pts, lvl = points_of(sizes, strides, dtype)
    P, (B, K) = pts.size(0), valid.shape
    g = gts.to(dtype)[:, None]                                                  # (B, 1, K, 4)
    xs, ys = pts[None, :, None, 0], pts[None, :, None, 1]
    left, right, top, bottom = xs - g[..., 0], g[..., 2] - xs, ys - g[..., 1], g[..., 3] - ys
    t = torch.stack((left, top, right, bottom), -1)                             # (B, P, K, 4)
    if center_sampling:
        cx, cy = (g[..., 0] + g[..., 2]) / 2, (g[..., 1] + g[..., 3]) / 2
        sr = torch.tensor([s * radius for s in strides], dtype=dtype)[lvl][None, :, None]
        x0, y0, x1, y1 = cx - sr, cy - sr, cx + sr, cy + sr
        c0, c1 = torch.where(x0 > g[..., 0], x0, g[..., 0]), torch.where(y0 > g[..., 1], y0, g[..., 1])
        c2, c3 = torch.where(x1 > g[..., 2], g[..., 2], x1), torch.where(y1 > g[..., 3], g[..., 3], y1)
        inside = torch.stack((xs - c0, ys - c1, c2 - xs, c3 - ys), -1).min(-1)[0] > 0
    else:
        inside = t.min(-1)[0] > 0
    far = t.max(-1)[0]
    rng = torch.tensor([list(r) for r in ranges], dtype=dtype)[lvl]
    in_range = (far >= rng[None, :, None, 0]) & (far <= rng[None, :, None, 1])
    areas = ((g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])).expand(B, P, K).clone()
    areas[~(inside & in_range)] = INF
    areas[~valid[:, None, :].expand(B, P, K)] = float('inf')                    # padding slots never win, whatever the others hold
    min_area, k = areas.min(-1)
    has_gt = valid.any(1)[:, None]
    pos = (min_area != INF) & has_gt
    bt = torch.gather(t, 2, k[..., None, None].expand(B, P, 1, 4))[:, :, 0]
    bt = torch.where(has_gt[..., None], bt, torch.zeros_like(bt))
    if norm_on_bbox:
        bt = bt / torch.tensor([float(s) for s in strides], dtype=dtype)[lvl][None, :, None]
    lr, tb = bt[..., [0, 2]], bt[..., [1, 3]]
    ctr = torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0]))
    ctr = torch.where(pos, ctr, torch.zeros_like(ctr))
    return torch.where(pos, k + 1, torch.zeros_like(k)).to(torch.int32), bt, ctr


def loss_ref(cls, reg, ctr, strides, gt_labels, assigned, bbox_targets, ctr_targets, kind='iou', gamma=2.0, alpha=0.25,
             weights=(1., 1., 1.), eps=1e-6, dtype=torch.float64):
    """FCOSHead.loss (fcos_head.py:196-253) with FocalLoss, IoULoss (the reference's edited form) or GIoULoss and the sigmoid
    CrossEntropyLoss restated on the outputs of the assignment, with autograd in `dtype` -> dict(losses (3,), gcls / greg / gctr
    lists); fp32 gives the formula's own rounding error on a case."""
    cls = [c.detach().cpu().to(dtype).requires_grad_() for c in cls]
    reg = [r.detach().cpu().to(dtype).requires_grad_() for r in reg]
    ctr = [c.detach().cpu().to(dtype).requires_grad_() for c in ctr]
    assigned, gt_labels = assigned.cpu().long(), gt_labels.cpu()
    B, P = assigned.shape
    C = cls[0].size(1)
    x, d, z = maps_to_rows(cls), maps_to_rows(reg), maps_to_rows(ctr)[..., 0]
    pos = assigned > 0
    num_pos = int(pos.sum())
    labels = torch.where(pos, torch.gather(gt_labels, 1, (assigned - 1).clamp(min=0)), torch.full_like(assigned, C))
    t = (labels.reshape(-1, 1) == torch.arange(C).view(1, -1)).to(dtype)
    xf = x.reshape(-1, C)
    s = xf.sigmoid()
    pt = (1 - s) * t + s * (1 - t)
    focal = torch.nn.functional.binary_cross_entropy_with_logits(xf, t, reduction='none') * (alpha * t + (1 - alpha) * (1 - t)) * \
        pt.pow(gamma)
    loss_cls = weights[0] * focal.sum() / (num_pos + B)
    pts, _ = points_of([c.shape[-2:] for c in cls], strides, dtype)
    pp = pts[None].expand(B, P, 2)[pos]
    w = ctr_targets.cpu().to(dtype)[pos]
    if num_pos > 0:
        def boxes(dist):
            return torch.stack((pp[:, 0] - dist[:, 0], pp[:, 1] - dist[:, 1], pp[:, 0] + dist[:, 2], pp[:, 1] + dist[:, 3]), -1)
        a, b = boxes(d[pos]), boxes(bbox_targets.cpu().to(dtype)[pos])
        wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
        overlap = wh[:, 0] * wh[:, 1]
        union = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - overlap
        union = torch.max(union, union.new_tensor(eps))
        ious = overlap / union
        if kind == 'iou':
            ious = ious.clamp(min=eps)
            per = -torch.where(ious > 0.1, ious, 0.1 + ious).log()
        else:
            ewh = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
            earea = torch.max(ewh[:, 0] * ewh[:, 1], union.new_tensor(eps))
            per = 1 - (ious - (earea - union) / earea)
        loss_bbox = weights[1] * (per * w).sum() / w.sum()
        loss_ctr = weights[2] * torch.nn.functional.binary_cross_entropy_with_logits(z[pos], w, reduction='sum') / num_pos
    else:
        loss_bbox, loss_ctr = d[pos].sum(), z[pos].sum()
    (loss_cls + loss_bbox + loss_ctr).backward()
    zero = lambda m: m.grad if m.grad is not None else torch.zeros_like(m)
    return dict(losses=torch.stack([loss_cls.detach(), loss_bbox.detach(), loss_ctr.detach()]), gcls=[zero(m) for m in cls],
                greg=[zero(m) for m in reg], gctr=[zero(m) for m in ctr])
