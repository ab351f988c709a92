"""Shared by tests/golden/make_golden_vfnet.py, tests/test_vfnet.py and tests/test_gpu_vfnet.py: the inputs of the VFNet fixture
(tests/golden/vfnet.npz), re-created from seeds so the fixture holds results only.  The images, boxes, level sizes and anchors
are atss_util's (its anchors are centred on the grid nodes: centre offset 0, VFNet's)."""
import torch

import atss_util as AU
from atss_util import (LEVEL_ANCHORS, LEVEL_SIZES, STRIDES, TOPK, TRAIN_CFG, anchors_of, detector_inputs, maps_to_rows,  # noqa: F401
                       pad_gts)
import dense_fixture_util as D
from golden_util import seeded_tensor

CONFIGS = dict(r50='configs/vfnet/vfnet_r50_fpn_1x_coco.py', r101_mstrain='configs/vfnet/vfnet_r101_fpn_mstrain_2x_coco.py')
CONFIG_ARGS = dict(r50=dict(depth=50), r101_mstrain=dict(depth=101, mstrain=True))
CFG_KEYS = AU.CFG_KEYS          # and 'train_pipeline' = data.train.pipeline
REG_DENOMS = (64, 128, 256, 512, 1024)
EXTRA_GRAD_KEYS = ('neck.fpn_convs.3.conv.weight', 'neck.fpn_convs.4.conv.weight', 'bbox_head.cls_convs.0.conv.weight',
                   'bbox_head.reg_convs.2.conv.weight', 'bbox_head.vfnet_reg_conv.conv.weight', 'bbox_head.vfnet_reg.weight',
                   'bbox_head.vfnet_reg.bias', 'bbox_head.vfnet_reg_refine_dconv.weight', 'bbox_head.vfnet_reg_refine.weight',
                   'bbox_head.vfnet_reg_refine.bias', 'bbox_head.vfnet_cls_dconv.weight', 'bbox_head.vfnet_cls.weight',
                   'bbox_head.vfnet_cls.bias', 'bbox_head.scales.0.scale', 'bbox_head.scales.1.scale', 'bbox_head.scales.2.scale',
                   'bbox_head.scales_refine.0.scale', 'bbox_head.scales_refine.1.scale', 'bbox_head.cls_convs.1.gn.weight')
GIOU = dict(loss_bbox=dict(type='GIoULoss', loss_weight=1.5), loss_bbox_refine=dict(type='GIoULoss', loss_weight=2.0))


def _vfl(**kw):
    return dict(dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True, loss_weight=1.0), **kw)


# variant -> what it changes of the head: the box losses, the varifocal loss, the normalisation of the distances (which the seeded
# maps of head_maps() follow: exp(logits) * reg_denom or * stride)
HEAD_VARIANTS = dict(giou=dict(GIOU),
                     iou=dict(loss_bbox=dict(type='IoULoss', loss_weight=1.5), loss_bbox_refine=dict(type='IoULoss', loss_weight=2.0)),
                     noiouw=dict(GIOU, loss_cls=_vfl(iou_weighted=False)),
                     g15=dict(GIOU, loss_cls=_vfl(gamma=1.5, alpha=0.5)),
                     stride=dict(GIOU, bbox_norm_type='stride'))
# nms_pre and HEAD_TAG: what make_golden_vfnet.search_head_tag() finds (asserted there): the first seed tag, and the cut nearest
# 50, at which the ranking keys max_c sigmoid(cls) of head_maps() leave a gap of 1e-3 at both cuts (levels 0 and 1) of both images
HEAD_TAG = 'vfnet.head'
HEAD_TEST_CFG = dict(nms_pre=48, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
# (image, level, row, column) of a positive whose initial box head_maps() moves off its gt (negative left distance): its IoU is 0
# and takes the clamp to 1e-6.  The generator asserts that the location is a positive.
NO_OVERLAP = (0, 0, 11, 10)
REG_SCALE = 0.25         # of the seeded regression layers of the detector fixture


def head_cfg(variant, num_classes=80, **extra):
    d = dict(type='VFNetHead', num_classes=num_classes, in_channels=256, stacked_convs=3, feat_channels=256,
             strides=list(STRIDES), center_sampling=False, dcn_on_last_conv=False, use_atss=True, use_vfl=True,
             loss_cls=_vfl())
    d.update(HEAD_VARIANTS[variant])
    d.update(extra)
    return d


def denoms_of(variant, strides=STRIDES):
    if HEAD_VARIANTS[variant].get('bbox_norm_type', 'reg_denom') == 'stride':
        return tuple(strides)
    return tuple(REG_DENOMS) + tuple(1024 * 2 ** (i + 1) for i in range(len(strides) - len(REG_DENOMS)))


def head_maps(variant='giou', B=2, C=80, sizes=LEVEL_SIZES, strides=STRIDES, tag=HEAD_TAG, no_overlap=True):
    """Seeded head outputs, fp32 on the CPU: per level (B, C, h, w) IoU-aware class logits, (B, 4, h, w) initial distances
    exp(logits) * denom and (B, 4, h, w) refined distances = the initial ones times exp(other logits), as forward_single makes
    them.  no_overlap: the initial box at NO_OVERLAP lies off its gt."""
    denoms = denoms_of(variant, strides)
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, C, h, w), scale=2.0) - 4.0 for l, (h, w) in enumerate(sizes)]
    reg = [(seeded_tensor(f'{tag}.reg{l}', (B, 4, h, w), scale=0.5) - (0.0 if denoms[l] <= strides[l] else 1.5)).exp() * float(denoms[l])
           for l, (h, w) in enumerate(sizes)]
    ref = [r * seeded_tensor(f'{tag}.ref{l}', tuple(r.shape), scale=0.3).exp() for l, r in enumerate(reg)]
    if no_overlap and sizes == LEVEL_SIZES and B == 2:
        b, l, y, x = NO_OVERLAP
        reg[l][b, :, y, x] = torch.tensor([-1000., 3., 1010., 3.])
    return cls, reg, ref


# the fixture's weights (dense_fixture_util): the level scales of both groups at 1 + a quarter of a seeded normal, the
# classification layer scaled and its bias lowered by the two figures the fixture records (plainly seeded, the logits saturate
# the sigmoid and the ranking keys crowd), both regression layers scaled by REG_SCALE
FIXTURE = dict(scales=('scales', 'scales_refine'),
               edits=(('bbox_head.vfnet_cls.weight', 'mul', 'scale'), ('bbox_head.vfnet_cls.bias', 'sub', 'bias_shift'),
                      ('bbox_head.vfnet_reg.weight', 'mul', REG_SCALE), ('bbox_head.vfnet_reg.bias', 'mul', REG_SCALE),
                      ('bbox_head.vfnet_reg_refine.weight', 'mul', REG_SCALE), ('bbox_head.vfnet_reg_refine.bias', 'mul', REG_SCALE)))


def load_fixture_weights_(det, scale, bias_shift):
    return D.load_fixture_weights(det, **FIXTURE, scale=scale, bias_shift=bias_shift)


def fixture_state(keys, shapes, scale, bias_shift):
    return D.fixture_state(keys, shapes, **FIXTURE, scale=scale, bias_shift=bias_shift)


def grad_keys(det):
    return D.grad_keys(det, EXTRA_GRAD_KEYS)


def loss_module_case():
    """Small seeded inputs of the VarifocalLoss entries of the fixture: (12, 5) logits, IoU targets at one class of seven rows
    (zero elsewhere), one weight per element."""
    pred = seeded_tensor('vfnet.vfl.pred', (12, 5), scale=2.0).double()
    target = torch.zeros(12, 5, dtype=torch.float64)
    rows, cols = torch.tensor([1, 3, 4, 6, 8, 10, 11]), torch.tensor([0, 3, 1, 1, 4, 2, 0])
    target[rows, cols] = seeded_tensor('vfnet.vfl.iou', (7, ), kind='rand').double() * 0.9 + 0.05
    weight = seeded_tensor('vfnet.vfl.weight', (12, 5), kind='rand').double() + 0.5
    return dict(pred=pred, target=target, weight=weight)


LOSS_MODES = (('mean', None, False), ('mean', 3.5, True), ('sum', None, True), ('none', None, True), ('none', None, False))
LOSS_MODULES = dict(vfl=dict(alpha=0.75, gamma=2.0, iou_weighted=True, loss_weight=1.5),
                    vfl15=dict(alpha=0.5, gamma=1.5, iou_weighted=True, loss_weight=1.0),
                    vflnow=dict(alpha=0.75, gamma=2.0, iou_weighted=False, loss_weight=1.0))


def star_case(shape=(2, 4, 3, 5), tag='vfnet.star'):
    """Scaled regression logits of the star-offset entries."""
    return seeded_tensor(f'{tag}.{"x".join(str(s) for s in shape)}', shape, scale=0.7)
