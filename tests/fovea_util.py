"""Shared by tests/golden/make_golden_fovea.py, tests/test_fovea.py and tests/test_gpu_fovea.py: the inputs of the FoveaBox fixture
(tests/golden/fovea.npz), re-created from seeds so the fixture holds results only, and the fp64 formulas of the loss and of the
FeatureAlign offsets that the GPU tests measure the kernels against."""
import torch

import dense_fixture_util as D
from dense_fixture_util import CFG_KEYS, LEVEL_SIZES, STRIDES, levels_to_images, maps_to_rows, pad_gts  # noqa: F401
from golden_util import seeded_tensor

CONFIGS = dict(plain='configs/foveabox/fovea_r50_fpn_4x4_1x_coco.py',
               align='configs/foveabox/fovea_align_r50_fpn_gn-head_4x4_2x_coco.py',
               align_r101_mstrain='configs/foveabox/fovea_align_r101_fpn_gn-head_mstrain_640-800_4x4_2x_coco.py')
CONFIG_ARGS = dict(plain=dict(depth=50), align=dict(depth=50, align=True, schedule='2x'),
                   align_r101_mstrain=dict(depth=101, align=True, mstrain=True, schedule='2x'))
DETECTOR_CONFIGS = ('plain', 'align')           # the two the fixture runs
# (CFG_KEYS and 'train_pipeline' = data.train.pipeline)
EXTRA_GRAD_KEYS = ('neck.fpn_convs.3.conv.weight', 'neck.fpn_convs.4.conv.weight', 'bbox_head.cls_convs.0.conv.weight',
                   'bbox_head.cls_convs.1.conv.weight', 'bbox_head.reg_convs.3.conv.weight', 'bbox_head.conv_cls.weight',
                   'bbox_head.conv_cls.bias', 'bbox_head.conv_reg.weight', 'bbox_head.conv_reg.bias',
                   'bbox_head.feature_adaption.conv_offset.weight', 'bbox_head.feature_adaption.conv_adaption.weight',
                   'bbox_head.cls_convs.1.gn.weight')
BASE_EDGES = (16, 32, 64, 128, 256)
LEVEL_POINTS = tuple(h * w for h, w in LEVEL_SIZES)
CONFIG_RANGES = ((1, 64), (32, 128), (64, 256), (128, 512), (256, 2048))   # of the reference's configs
DEFAULT_RANGES = ((8, 32), (16, 64), (32, 128), (64, 256), (128, 512))     # of the head's constructor: the targets case
SIGMA = 0.4
HEAD_LOSSES = dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.50, alpha=0.4, loss_weight=1.0),
                   loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))
HEAD_TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)      # + nms_pre of the fixture
REG_SCALE = 0.25         # of the seeded regression layer of the detector fixture: distances within a few base edges


def head_cfg(num_classes=80, **extra):
    d = dict(type='FoveaHead', num_classes=num_classes, in_channels=256, stacked_convs=4, feat_channels=256, strides=list(STRIDES),
             base_edge_list=list(BASE_EDGES), scale_ranges=CONFIG_RANGES, sigma=SIGMA, with_deform=False)
    d.update(HEAD_LOSSES)
    d.update(extra)
    return d


# the fixture's weights (dense_fixture_util): the classification layer scaled and its bias lowered by the two figures the fixture
# records (plainly seeded, the logits saturate the sigmoid and the ranking keys crowd), the regression layer scaled by REG_SCALE
FIXTURE = dict(edits=(('bbox_head.conv_cls.weight', 'mul', 'scale'), ('bbox_head.conv_cls.bias', 'sub', 'bias_shift'),
                      ('bbox_head.conv_reg.weight', 'mul', REG_SCALE)))


def load_fixture_weights_(det, scale, bias_shift):
    return D.load_fixture_weights(det, **FIXTURE, scale=scale, bias_shift=bias_shift)


def fixture_state(keys, shapes, scale, bias_shift):
    return D.fixture_state(keys, shapes, **FIXTURE, scale=scale, bias_shift=bias_shift)


def grad_keys(det):
    return D.grad_keys(det, EXTRA_GRAD_KEYS)


def head_maps(B=2, C=80, sizes=LEVEL_SIZES, tag='fovea.head'):
    """Seeded head outputs, fp32 on the CPU: per level (B, C, h, w) logits (unsaturated: the ranking keys max_c sigmoid spread
    around 0.4) and (B, 4, h, w) log distances."""
    cls = [seeded_tensor(f'{tag}.cls{l}', (B, C, h, w), scale=1.0) - 3.0 for l, (h, w) in enumerate(sizes)]
    reg = [seeded_tensor(f'{tag}.reg{l}', (B, 4, h, w), scale=0.5) for l, (h, w) in enumerate(sizes)]
    return cls, reg


def targets_case():
    """Synthetic gts on the 128 x 160 pyramid under DEFAULT_RANGES -> (gts list, labels list) of 4 images.  Image 0, by index:
    0 a 24 x 24 box nested in 1, a 64 x 64 box (both on level 1, the smaller one first in index order: the painting order, not
    the index, must decide); 2 / 3 / 4 boxes wholly right of, below and left of the image; 5 a 10 x 10 box whose rectangle on level
    0 is empty; 6 an 8 x 8 box (gt_areas on the lower bound of level 0); 7 a 600 x 1.5 strip whose targets take both clamps; 8 a
    400 x 400 box for level 4; 9 a 128 x 128 box (the upper bound of level 2, the lower one of level 4).  Image 1: no gt.
    Image 2: a 32 x 32 box (the upper bound of level 0, the lower one of level 2) and a box of a size that is no square.
    Image 3: the whole image and a 24 x 24 box."""
    g0 = [[40., 40., 64., 64.], [16., 16., 80., 80.], [200., 40., 224., 64.], [40., 150., 64., 174.], [-60., 40., -36., 64.],
          [20., 84., 30., 94.], [96., 8., 104., 16.], [-400., 43.5, 200., 45.], [-100., -150., 300., 250.], [10., -20., 138., 108.]]
    g2 = [[8., 8., 40., 40.], [50., 30., 150., 110.]]
    g3 = [[0., 0., 160., 128.], [100., 60., 124., 84.]]
    gts = [torch.tensor(g0), torch.zeros(0, 4), torch.tensor(g2), torch.tensor(g3)]
    labels = [torch.tensor([3, 79, 0, 41, 7, 12, 12, 5, 9, 30]), torch.zeros(0, dtype=torch.long), torch.tensor([1, 2]),
              torch.tensor([9, 8])]
    return gts, labels


def tie_case(n=20):
    """n nested gts of one image with equal gt_areas (64) whose rectangles on level 1 all hold the point (row 3, column 3): boxes
    of 64 x 64, 128 x 32 and 32 x 128 around (56, 56), shuffled by a fixed rule.  -> (gts (n, 4), labels (n,))."""
    shapes = ((64., 64.), (128., 32.), (32., 128.))
    rows = []
    for i in range(n):
        w, h = shapes[(i * 7) % 3]
        rows.append([56. - w / 2, 56. - h / 2, 56. + w / 2, 56. + h / 2])
    return torch.tensor(rows), torch.arange(n) % 80


def sqrt_tie_case():
    """Two gts of different area whose gt_areas round to the same fp32 root: 64 x 64 (area 4096, index 0) and (64 + 2^-17) x 64
    (area 4096 + 2^-11, index 1; its root 64 * (1 + 2^-24 - ...) rounds to 64).  The reference compares the rounded roots, so
    they tie and index 1 wins every point (their rectangles are equal); a compare of the areas would give them to index 0."""
    gts = torch.tensor([[24., 24., 88., 88.], [24., 24., 88. + 2.0 ** -17, 88.]])
    assert float(gts[1, 2] - gts[1, 0]) == 64 + 2.0 ** -17
    return gts, torch.tensor([5, 6])


def flat_to_images(flat, B, sizes=LEVEL_POINTS):
    """FoveaHead.get_targets' flat tensors (level after level, within a level image after image) -> (B, P, ...)."""
    out, at = [], 0
    for n in sizes:
        out.append(flat[at:at + B * n].reshape(B, n, *flat.shape[1:]))
        at += B * n
    assert at == flat.size(0)
    return torch.cat(out, 1)


def head_targets(head, gts, dtype=torch.float32, sizes=LEVEL_SIZES):
    """get_targets with labels = gt index -> assigned (B, P) (0 background, k + 1 = gt k) and bbox_targets (B, P, 4) with zeros
    under the background (the reference leaves uninitialised memory there)."""
    B = len(gts)
    points = head.get_points(sizes, dtype, 'cpu')
    labels, bt = head.get_targets([g.to(dtype) for g in gts], [torch.arange(len(g)) for g in gts], sizes, points)
    n = [h * w for h, w in sizes]
    labels, bt = flat_to_images(labels, B, n), flat_to_images(bt, B, n)
    pos = labels < head.num_classes
    return torch.where(pos, labels + 1, torch.zeros_like(labels)), torch.where(pos[..., None], bt, torch.zeros_like(bt))


def loss_ref(cls, reg, gt_labels, assigned, bbox_targets, gamma=1.5, alpha=0.4, beta=0.11, weights=(1., 1.), dtype=torch.float64):
    """FoveaHead.loss (fovea_head.py:127-175) with FocalLoss and SmoothL1Loss restated on the outputs of the assignment, with
    autograd in `dtype` -> dict(losses (2,), gcls / greg lists); fp32 gives the formula's own rounding error on a case."""
    cls = [c.detach().cpu().to(dtype).requires_grad_() for c in cls]
    reg = [r.detach().cpu().to(dtype).requires_grad_() for r in reg]
    assigned, gt_labels = assigned.cpu().long(), gt_labels.cpu()
    B, P = assigned.shape
    C = cls[0].size(1)
    x, d = maps_to_rows(cls), maps_to_rows(reg)
    pos = assigned > 0
    num_pos = int(pos.sum())
    if gt_labels.size(1):
        labels = torch.where(pos, torch.gather(gt_labels, 1, (assigned - 1).clamp(min=0)), torch.full_like(assigned, C))
    else:
        labels = torch.full_like(assigned, C)
    t = (labels.reshape(-1, 1) == torch.arange(C).view(1, -1)).to(dtype)
    xf = x.reshape(-1, C)
    s = xf.sigmoid()
    pt = (1 - s) * t + s * (1 - t)
    focal = torch.nn.functional.binary_cross_entropy_with_logits(xf, t, reduction='none') * (alpha * t + (1 - alpha) * (1 - t)) * \
        pt.pow(gamma)
    loss_cls = weights[0] * focal.sum() / (num_pos + B)
    if num_pos > 0:
        diff = (d[pos] - bbox_targets.cpu().to(dtype)[pos]).abs()
        loss_bbox = weights[1] * torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta).sum() / num_pos
    else:
        loss_bbox = d.sum() * 0
    (loss_cls + loss_bbox).backward()
    return dict(losses=torch.stack([loss_cls.detach(), loss_bbox.detach()]), gcls=[m.grad for m in cls], greg=[m.grad for m in reg])


def align_ref(x, weight, g_off, dtype=torch.float64):
    """FeatureAlign's offsets conv_offset(exp(x)) and their backward under the incoming gradient g_off, in `dtype` on the CPU ->
    (offset, g_x, g_weight)."""
    x = x.detach().cpu().to(dtype).requires_grad_()
    w = weight.detach().cpu().to(dtype).requires_grad_()
    off = torch.nn.functional.conv2d(x.exp(), w)
    (off * g_off.detach().cpu().to(dtype)).sum().backward()
    return off.detach(), x.grad, w.grad
