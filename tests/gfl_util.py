"""Shared by tests/golden/make_golden_gfl.py, tests/test_gfl.py and tests/test_gpu_gfl.py: the inputs of the GFL fixture
(tests/golden/gfl.npz), re-created from seeds so the fixture holds results only.  The images, boxes, level sizes and anchors are
atss_util's."""
import torch

import atss_util as AU
from atss_util import (LEVEL_ANCHORS, LEVEL_SIZES, STRIDES, TOPK, TRAIN_CFG, anchors_of, detector_inputs, maps_to_rows,  # noqa: F401
                       pad_gts)
import dense_fixture_util as D
from golden_util import seeded_tensor

CONFIGS = dict(r50='configs/gfl/gfl_r50_fpn_1x_coco.py', r101_mstrain='configs/gfl/gfl_r101_fpn_mstrain_2x_coco.py')
CONFIG_ARGS = dict(r50=dict(depth=50), r101_mstrain=dict(depth=101, mstrain=True))
# the reference's gfl_r50_fpn_mstrain_2x_coco.py names a base file its tree does not hold (gfl_r50_fpn_1x_polyp.py); its sibling
# of the same directory stands in for it when the configs are merged
MISSING_BASE = {'./gfl_r50_fpn_1x_polyp.py': './gfl_r50_fpn_1x_coco.py'}
CFG_KEYS = AU.CFG_KEYS          # and 'train_pipeline' = data.train.pipeline
EXTRA_GRAD_KEYS = ('neck.fpn_convs.3.conv.weight', 'neck.fpn_convs.4.conv.weight', 'bbox_head.cls_convs.0.conv.weight',
                   'bbox_head.reg_convs.3.conv.weight', 'bbox_head.gfl_cls.weight', 'bbox_head.gfl_cls.bias',
                   'bbox_head.gfl_reg.weight', 'bbox_head.gfl_reg.bias', 'bbox_head.scales.0.scale', 'bbox_head.scales.1.scale',
                   'bbox_head.scales.2.scale', 'bbox_head.scales.3.scale', 'bbox_head.scales.4.scale',
                   'bbox_head.cls_convs.1.gn.weight')
# variant -> what it changes of the head: the box loss, reg_max (7: target sides above 6.9 take the clamp), QFL's beta
HEAD_VARIANTS = dict(giou=dict(loss_bbox=dict(type='GIoULoss', loss_weight=2.0)),
                     iou=dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)),
                     giou_r7=dict(loss_bbox=dict(type='GIoULoss', loss_weight=2.0), reg_max=7),
                     giou_b15=dict(loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                                   loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=1.5, loss_weight=1.0)))
# nms_pre and HEAD_TAG: what make_golden_gfl.search_head_tag() finds (asserted there): the first seed tag, and the cut nearest 50, at
# which the ranking keys max_c sigmoid(cls) of head_maps() leave a gap of 1e-3 at both cuts (levels 0 and 1) of both images
HEAD_TAG = 'gfl.head.v6'
HEAD_TEST_CFG = dict(nms_pre=66, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
REG_SCALE = 0.25         # of the seeded regression layer of the detector fixture


def head_cfg(variant, num_classes=80, **extra):
    d = dict(type='GFLHead', num_classes=num_classes, in_channels=256, stacked_convs=4, feat_channels=256,
             anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                   strides=list(STRIDES)),
             loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0),
             loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25), reg_max=16)
    d.update(HEAD_VARIANTS[variant])
    d.update(extra)
    return d


def reg_max_of(variant):
    return HEAD_VARIANTS[variant].get('reg_max', 16)


def head_maps(variant='giou', B=2, C=80, sizes=LEVEL_SIZES, reg_max=None, tag=HEAD_TAG):
    """Seeded head outputs, fp32 on the CPU: per level (B, C, h, w) class / quality logits and (B, 4 * (reg_max + 1), h, w)
    distribution logits (one set per reg_max)."""
    R = reg_max_of(variant) if reg_max is None else reg_max
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, C, h, w), scale=2.0) - 2.0 for l, (h, w) in enumerate(sizes)]
    reg = [seeded_tensor(f'{tag}.reg{l}.{R}', (B, 4 * (R + 1), h, w), scale=1.5) for l, (h, w) in enumerate(sizes)]
    return cls, reg


def target_distances(anchors, padded_gts, assigned, strides=STRIDES, level_anchors=LEVEL_ANCHORS):
    """bbox2distance(anchor centre / stride, gt / stride) of every positive of assigned (B, A), unclamped, in the reference's
    fp32 order -> (B, A, 4), zeros where the anchor is background."""
    B, A = assigned.shape
    stride = torch.cat([torch.full((n, ), float(s)) for n, s in zip(level_anchors, strides)])
    out = torch.zeros(B, A, 4)
    pos = assigned > 0
    b, i = pos.nonzero(as_tuple=True)
    a, g, s = anchors[i].float(), padded_gts[b, assigned[pos].long() - 1].float(), stride[i]
    cx, cy = ((a[:, 2] + a[:, 0]) / 2) / s, ((a[:, 3] + a[:, 1]) / 2) / s
    t = g / s[:, None]
    out[pos] = torch.stack([cx - t[:, 0], cy - t[:, 1], t[:, 2] - cx, t[:, 3] - cy], -1)
    return out


# the fixture's weights (dense_fixture_util): the level scales at 1 + a quarter of a seeded normal, the classification layer scaled
# and its bias lowered by the two figures the fixture records (plainly seeded, the logits saturate the sigmoid and the ranking
# keys crowd), the regression layer scaled by REG_SCALE; the integral's projection stays 0 .. reg_max
FIXTURE = dict(scales=('scales', ),
               constants={'bbox_head.integral.project': lambda shape: torch.linspace(0, shape[0] - 1, shape[0])},
               edits=(('bbox_head.gfl_cls.weight', 'mul', 'scale'), ('bbox_head.gfl_cls.bias', 'sub', 'bias_shift'),
                      ('bbox_head.gfl_reg.weight', 'mul', REG_SCALE), ('bbox_head.gfl_reg.bias', 'mul', REG_SCALE)))


def load_fixture_weights_(det, scale, bias_shift):
    return D.load_fixture_weights(det, **FIXTURE, scale=scale, bias_shift=bias_shift)


def fixture_state(keys, shapes, scale, bias_shift):
    return D.fixture_state(keys, shapes, **FIXTURE, scale=scale, bias_shift=bias_shift)


def grad_keys(det):
    return D.grad_keys(det, EXTRA_GRAD_KEYS)


def loss_module_case():
    """Small seeded inputs of the loss-module entries of the fixture: QFL on (12, 5) logits with 5 positive rows, DFL on (10, 8)
    logits with targets in [0, 7), one weight per row each."""
    pred = seeded_tensor('gfl.qfl.pred', (12, 5), scale=2.0).double()
    label = torch.tensor([5, 0, 5, 3, 5, 5, 1, 5, 4, 5, 2, 5])
    score = seeded_tensor('gfl.qfl.score', (12, ), kind='rand').double() * (label < 5)
    weight = seeded_tensor('gfl.qfl.weight', (12, ), kind='rand').double() + 0.5
    dpred = seeded_tensor('gfl.dfl.pred', (10, 8), scale=2.0).double()
    dlabel = seeded_tensor('gfl.dfl.label', (10, ), kind='rand', scale=6.9).double()
    dweight = seeded_tensor('gfl.dfl.weight', (10, ), kind='rand').double() + 0.5
    return dict(pred=pred, label=label, score=score, weight=weight, dpred=dpred, dlabel=dlabel, dweight=dweight)


LOSS_MODES = (('mean', None, False), ('mean', 3.5, True), ('sum', None, True), ('none', None, True), ('none', None, False))


def distance_case():
    """points, boxes of the bbox2distance entries: some sides negative, some beyond max_dis = 7."""
    pts = seeded_tensor('gfl.b2d.pts', (9, 2), kind='rand', scale=10.0).double()
    half = seeded_tensor('gfl.b2d.half', (9, 4), kind='randn', scale=5.0).double() + 3.0
    box = torch.stack([pts[:, 0] - half[:, 0], pts[:, 1] - half[:, 1], pts[:, 0] + half[:, 2], pts[:, 1] + half[:, 3]], -1)
    return pts, box
