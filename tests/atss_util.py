"""Shared by tests/golden/make_golden_atss.py, tests/test_atss.py and tests/test_gpu_atss.py: the inputs of the ATSS fixture
(tests/golden/atss.npz), re-created from seeds so the fixture holds results only, the hand-placed assignment cases, and the
reference's centerness arithmetic restated in fp32 for the checks of the kernel's centerness targets."""
import numpy as np
import torch

import dense_fixture_util as D
from dense_fixture_util import CFG_KEYS, LEVEL_SIZES, STRIDES, levels_to_images, maps_to_rows, pad_gts  # noqa: F401
from golden_util import seeded_tensor

CONFIGS = dict(r50='configs/atss/atss_r50_fpn_1x_coco.py', r101='configs/atss/atss_r101_fpn_1x_coco.py')
EXTRA_GRAD_KEYS = ('neck.fpn_convs.3.conv.weight', 'neck.fpn_convs.4.conv.weight', 'bbox_head.cls_convs.0.conv.weight',
                   'bbox_head.reg_convs.3.conv.weight', 'bbox_head.atss_cls.weight', 'bbox_head.atss_cls.bias',
                   'bbox_head.atss_reg.weight', 'bbox_head.atss_reg.bias', 'bbox_head.atss_centerness.weight',
                   'bbox_head.atss_centerness.bias', 'bbox_head.scales.0.scale', 'bbox_head.scales.1.scale',
                   'bbox_head.scales.2.scale', 'bbox_head.scales.3.scale', 'bbox_head.scales.4.scale',
                   'bbox_head.cls_convs.1.gn.weight')
LEVEL_ANCHORS = tuple(h * w for h, w in LEVEL_SIZES)                       # 320, 80, 20, 6, 2: the last two hold fewer than topk
TOPK = 9
MEANS, STDS = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
REG_SCALE = 0.25         # of the seeded regression layer: deltas of a few tenths, boxes of about the anchors' size
HEAD_VARIANTS = dict(giou=dict(loss_bbox=dict(type='GIoULoss', loss_weight=2.0)),
                     iou=dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)))
# nms_pre: the value nearest 50 at which the ranking keys of head_maps() leave a gap of 1e-3 at both cuts (levels 0 and 1)
HEAD_TEST_CFG = dict(nms_pre=47, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
TRAIN_CFG = dict(assigner=dict(type='ATSSAssigner', topk=TOPK), allowed_border=-1, pos_weight=-1, debug=False)


GT_X_SCALE = 0.95       # (first of a short search: see detector_inputs)


def detector_inputs():
    """baselines_util.detector_inputs() with the x coordinates of the boxes scaled by GT_X_SCALE: two of the seeded boxes have
    their centres almost on the diagonal of the anchor grid, where two anchors lie at nearly the same distance (6e-4 relative)
    around the ninth place; scaled, every such gap of the batch is above the 1e-3 the generator asserts."""
    from baselines_util import detector_inputs as base
    imgs, metas, gts, labels = base()
    return imgs, metas, [(g * np.array([GT_X_SCALE, 1, GT_X_SCALE, 1], dtype=np.float32)).astype(np.float32) for g in gts], labels


def head_cfg(variant, num_classes=80, **extra):
    d = dict(type='ATSSHead', num_classes=num_classes, in_channels=256, stacked_convs=4, feat_channels=256,
             anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                   strides=list(STRIDES)),
             bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=list(MEANS), target_stds=list(STDS)),
             loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
             loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
    d.update(HEAD_VARIANTS[variant])
    d.update(extra)
    return d


# the fixture's weights (dense_fixture_util): the level scales at 1 + a quarter of a seeded normal, the classification and centerness
# layers scaled and the classification bias lowered by the two figures the fixture records (plainly seeded, the logits saturate
# the sigmoid, the ranking keys crowd and thousands of scores lie around the score threshold), the regression layer by REG_SCALE
FIXTURE = dict(scales=('scales', ),
               edits=(('bbox_head.atss_cls.weight', 'mul', 'scale'), ('bbox_head.atss_centerness.weight', 'mul', 'scale'),
                      ('bbox_head.atss_cls.bias', 'sub', 'bias_shift'), ('bbox_head.atss_reg.weight', 'mul', REG_SCALE),
                      ('bbox_head.atss_reg.bias', 'mul', REG_SCALE)))


def load_fixture_weights_(det, scale, bias_shift):
    return D.load_fixture_weights(det, **FIXTURE, scale=scale, bias_shift=bias_shift)


def fixture_state(keys, shapes, scale, bias_shift):
    return D.fixture_state(keys, shapes, **FIXTURE, scale=scale, bias_shift=bias_shift)


def grad_keys(det):
    return D.grad_keys(det, EXTRA_GRAD_KEYS)


def head_maps(variant=None, B=2, C=80, sizes=LEVEL_SIZES, tag='atss.head'):
    """Seeded head outputs, fp32 on the CPU: per level (B, C, h, w) logits, (B, 4, h, w) deltas and (B, 1, h, w) centerness
    logits (the same for both variants)."""
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, C, h, w), scale=2.0) - 2.0 for l, (h, w) in enumerate(sizes)]
    reg = [seeded_tensor(f'{tag}.reg{l}', (B, 4, h, w), scale=1.5) for l, (h, w) in enumerate(sizes)]
    ctr = [seeded_tensor(f'{tag}.ctr{l}', (B, 1, h, w), scale=1.5) for l, (h, w) in enumerate(sizes)]
    return cls, reg, ctr


def anchors_of(sizes=LEVEL_SIZES, strides=STRIDES, scale=8, dtype=torch.float32):
    """(A, 4) level-major square anchors of `scale` strides centred on the grid nodes (column, row) * stride: what
    AnchorGenerator(ratios=[1.0], octave_base_scale=8, scales_per_octave=1) makes."""
    out = []
    for (h, w), s in zip(sizes, strides):
        y, x = torch.meshgrid(torch.arange(h, dtype=dtype) * s, torch.arange(w, dtype=dtype) * s, indexing='ij')
        c = torch.stack((x.reshape(-1), y.reshape(-1)), -1)
        half = scale * s / 2
        out.append(torch.cat([c - half, c + half], -1))
    return torch.cat(out)


def assignment_case():
    """Hand-placed gts on the 128 x 160 pyramid -> (gts list, labels list) of 4 images.
    Image 0: a gt centred on the map corner (0, 0) (its nearest anchors are a clipped 3 x 3 window); one centred below the last
    anchor row (y = 120) at y = 141.2; two overlapping gts that share positive anchors; a gt so small that no candidate centre
    lies inside it (no positive); a gt centred exactly on the grid node (64, 64) of levels 0 to 2 (distances tie inside the
    selected nine).
    Image 1: a gt beyond the right border that no anchor of levels 0 to 2 touches (every candidate IoU of those levels is 0;
    on this pyramid the coarse anchors cover the fine ones, so the levels of all-zero IoU are the fine ones), and a large gt.
    Image 2: no gt.  Image 3: a small gt and three of about the anchor sizes of levels 2, 3 and 4, which take their positives
    there (the shorter lists of the other images are padded)."""
    g0 = [[-22., -20., 22., 20.], [57.6, 119.4, 103.6, 163.], [37., 29., 101.6, 87.8], [47., 35., 114.2, 96.4],
          [33.2, 33.4, 39.2, 39.6], [43., 45., 85., 83.]]
    g1 = [[291., 41., 333., 83.], [11., 7., 150.2, 122.4]]
    g3 = [[69., 21., 132.2, 100.6], [-45.4, -55.2, 204.6, 185.4], [-170.4, -180.2, 330.6, 300.4], [-400.4, -420.2, 560.6, 520.4]]
    gts = [torch.tensor(g0), torch.tensor(g1), torch.zeros(0, 4), torch.tensor(g3)]
    labels = [torch.tensor([3, 79, 0, 41, 7, 12]), torch.tensor([1, 2]), torch.zeros(0, dtype=torch.long), torch.tensor([9, 8, 7, 6])]
    return gts, labels


def twin_case():
    """Two identical gts (the lower index takes the shared positives) beside a third: compared against the reference only if the
    reference took the lower index too (the fixture records whether: `twin.ref_lower`)."""
    return [torch.tensor([[35., 27., 100.2, 94.4], [35., 27., 100.2, 94.4], [91., 51., 140.2, 118.4]])], [torch.tensor([5, 6, 7])]


def tie_case():
    """A gt centred at (68, 64): level 0 has four anchors at the same distance around the ninth place, levels 1 and 2 two
    each.  torch.topk leaves such ties undefined, so this case is held against ATSSAssigner (rule: distance, then index), not
    against the reference."""
    return [torch.tensor([[38., 34., 98., 94.]])], [torch.tensor([4])]


# Two cases on pyramids of their own -> name: (map sizes, strides, gts of one image).
# 'equal': two anchors of one level that hold the gt whole, so both IoUs are the same fp32 value, the deviation is 0 and the threshold
#          equals them: `>=` makes both positive, `>` none.
# 'std':   three anchors whose largest IoU lies between mean + biased and mean + unbiased deviation (1.5 % of the threshold from
#          either): the unbiased deviation gives no positive, the biased one would give one.
EXTRA_CASES = dict(equal=(((1, 2), ), (128, ), torch.tensor([[-40., -30., 168., 30.]])),
                   std=(((1, 3), ), (64, ), torch.tensor([[-224.7, -233.9, 245.7, 256.9]])))


def _rounded(fn, x):
    """fn in fp64 rounded to fp32: the correctly rounded fp32 function (the kernel's logarithm and exponential)."""
    return fn(x.double()).float()


def target_ltrb(anchors, gts, means=MEANS, stds=STDS, rounded=False, wh_ratio_clip=16 / 1000):
    """ATSSHead.centerness_target's l, t, r, b of delta2bbox(anchor, bbox2delta(anchor, gt)) (delta_xywh_bbox_coder.py:98-118,
    171-197, atss_head.py:297-306) in fp32, one operation at a time: anchors, gts (n, 4) -> (n, 4).  rounded: the logarithm and
    the exponential correctly rounded instead of torch's own."""
    a, g = anchors.float(), gts.float()
    log = (lambda x: _rounded(torch.log, x)) if rounded else torch.log
    exp = (lambda x: _rounded(torch.exp, x)) if rounded else torch.exp
    px, py, pw, ph = (a[:, 0] + a[:, 2]) * 0.5, (a[:, 1] + a[:, 3]) * 0.5, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    gx, gy, gw, gh = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    d = torch.stack([(gx - px) / pw, (gy - py) / ph, log(gw / pw), log(gh / ph)], -1)
    m, s = torch.tensor(means, dtype=torch.float32)[None], torch.tensor(stds, dtype=torch.float32)[None]
    d = (d - m) / s
    d = d * s + m
    max_ratio = float(np.abs(np.log(wh_ratio_clip)))
    w2, h2 = pw * exp(d[:, 2].clamp(min=-max_ratio, max=max_ratio)), ph * exp(d[:, 3].clamp(min=-max_ratio, max=max_ratio))
    x2, y2 = px + pw * d[:, 0], py + ph * d[:, 1]
    cx, cy = (a[:, 2] + a[:, 0]) / 2, (a[:, 3] + a[:, 1]) / 2
    return torch.stack([cx - (x2 - w2 * 0.5), cy - (y2 - h2 * 0.5), (x2 + w2 * 0.5) - cx, (y2 + h2 * 0.5) - cy], -1)


def batch_ltrb(anchors, padded_gts, assigned, rounded=False):
    """target_ltrb of every positive of assigned (B, A) (k + 1 = gt k) -> (B, A, 4), ones where the anchor is background."""
    B, A = assigned.shape
    out = torch.ones(B, A, 4)
    pos = assigned > 0
    b, i = pos.nonzero(as_tuple=True)
    out[pos] = target_ltrb(anchors[i], padded_gts[b, assigned[pos].long() - 1], rounded=rounded)
    return out


def centerness_of(ltrb):
    lr, tb = ltrb[..., [0, 2]], ltrb[..., [1, 3]]
    return torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0]))
