"""FCOS without a GPU: the two configurations against the reference's merged configs, the state dict and the pre-2.0 key rename,
get_targets / centerness_target / the tensor-path loss / the per-image get_bboxes against the reference's own run
(tests/golden/fcos.npz, recipe in tests/golden/make_golden_fcos.py), the restatements of fcos_util that the GPU tests lean on, and
the new entry points of the C ABI."""
import json
import os

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import T
import fcos_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def build_head(variant='iou', **extra):
    from htd_amd.registry import build_head as build
    import htd_amd.detector  # noqa: F401
    return build(U.head_cfg(variant, **extra))


def inputs():
    return D.inputs('cpu', BU.detector_inputs)[1:]


@pytest.mark.parametrize('which', list(U.CONFIGS))
def test_fcos_config_equals_the_reference_merged_config(which):
    from htd_amd.configs import fcos_config
    ref = json.load(open(os.path.join(GOLDEN, os.path.basename(U.CONFIGS[which])[:-3] + '_cfg.json')))
    cfg = fcos_config(50, U.VARIANT_OF[which])
    mine = json.loads(json.dumps({k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in U.CFG_KEYS}))
    assert mine == ref
    with pytest.raises(ValueError):
        fcos_config(34)
    with pytest.raises(ValueError, match='variant'):
        fcos_config(50, 'plain')


def test_state_dict_keys_and_shapes_equal_the_fixture(golden):
    from htd_amd.configs import build_baseline_detector
    g = golden('fcos')
    det = build_baseline_detector('fcos')
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_keys']]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == g['state_shapes'].tolist()
    assert type(det).__name__ == 'FCOS' and type(det.bbox_head).__name__ == 'FCOSHead'
    b = det.bbox_head.conv_cls.bias
    assert torch.allclose(b.sigmoid(), torch.full_like(b, 0.01))             # bias_init_with_prob(0.01)
    assert all(float(s.scale.detach()) == 1.0 and s.scale.dim() == 0 for s in det.bbox_head.scales)
    assert det.bbox_head.cls_convs[0].conv.bias is None                      # conv_bias='auto' under GroupNorm
    with pytest.raises(NotImplementedError):
        det.aug_test([], [])
    from htd_amd.apis import _num_classes
    assert _num_classes(det) == 80
    center = build_baseline_detector('fcos_center')
    h = center.bbox_head
    assert h.center_sampling and h.norm_on_bbox and h.centerness_on_reg and type(h.loss_bbox).__name__ == 'GIoULoss'
    assert h.cls_convs[0].conv.bias is not None and center.test_cfg.nms.iou_threshold == 0.6


def test_dense_heads_share_one_base():
    from htd_amd.detector.anchor_free_heads import AnchorFreeHead, FCOSHead
    from htd_amd.detector.anchor_heads import AnchorHead, RetinaHead
    from htd_amd.detector.base_dense_head import BaseDenseHead
    from htd_amd.detector.rpn_head import RPNHead
    from htd_amd.registry import HEADS
    for cls in (AnchorHead, RetinaHead, RPNHead, AnchorFreeHead, FCOSHead):
        assert issubclass(cls, BaseDenseHead)
        assert cls._cached is BaseDenseHead._cached and cls._shape_key is BaseDenseHead._shape_key
        assert cls.simple_test is BaseDenseHead.simple_test
    for cls in (AnchorHead, RetinaHead, AnchorFreeHead, FCOSHead):
        assert cls.forward_train is BaseDenseHead.forward_train
    assert HEADS.get('FCOSHead') is FCOSHead and HEADS.get('AnchorFreeHead') is AnchorFreeHead
    assert BaseDenseHead._shape_key([(4, 5), torch.Size([2, 3])]) == ((4, 5), (2, 3))


def test_old_predictor_keys_are_renamed_on_load():
    head = build_head('giou', num_classes=3, in_channels=8, feat_channels=8, stacked_convs=1,
                      norm_cfg=dict(type='GN', num_groups=4, requires_grad=True))
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    old = {k.replace('conv_cls', 'fcos_cls').replace('conv_reg', 'fcos_reg').replace('conv_centerness', 'fcos_centerness'):
           v + 1.0 for k, v in sd.items()}                       # a plain dict: no version metadata, as a pre-2.0 checkpoint
    assert any(k.startswith('fcos_cls') for k in old) and 'reg_convs.0.conv.weight' in old
    wrapper = torch.nn.Module()
    wrapper.bbox_head = head
    missing, unexpected = wrapper.load_state_dict({'bbox_head.' + k: v for k, v in old.items()}, strict=True)
    assert not missing and not unexpected
    for k, v in head.state_dict().items():
        torch.testing.assert_close(v, sd[k] + 1.0, rtol=0, atol=0)
    # a current state dict (with version metadata) loads as it is
    head.load_state_dict(head.state_dict(), strict=True)


def test_dcn_on_last_conv_builds_or_names_the_key():
    kw = dict(num_classes=3, in_channels=8, feat_channels=8, stacked_convs=2, norm_cfg=dict(type='GN', num_groups=4))
    from htd_amd.detector.bricks import build_conv_layer
    try:
        build_conv_layer(dict(type='DCNv2'), 8, 8, 3, stride=1, padding=1, bias=False)
        builds = True
    except (KeyError, TypeError):
        builds = False
    if builds:
        head = build_head('iou', dcn_on_last_conv=True, **kw)
        assert type(head.cls_convs[1].conv).__name__ != type(head.cls_convs[0].conv).__name__
    else:
        with pytest.raises(NotImplementedError, match='dcn_on_last_conv'):
            build_head('iou', dcn_on_last_conv=True, **kw)


def test_check_supported_names_paramwise_cfg():
    from htd_amd.apis import check_supported
    from htd_amd.configs import fcos_config, retinanet_config
    check_supported(retinanet_config())
    for variant in U.VARIANT_OF.values():
        cfg = fcos_config(50, variant)
        cfg.optimizer_config.grad_clip = None
        with pytest.raises(NotImplementedError, match='paramwise_cfg'):
            check_supported(cfg)


def head_targets(head, gts, dtype=torch.float32):
    """get_targets with labels = gt index and centerness_target -> assigned (B, P), bbox_targets (B, P, 4), ctr (B, P)."""
    B = len(gts)
    points = head.get_points(U.LEVEL_SIZES, dtype, 'cpu')
    labels, bt = head.get_targets(points, [x.to(dtype) for x in gts], [torch.arange(len(x)) for x in gts])
    labels, bt = U.levels_to_images(labels, B), U.levels_to_images(bt, B)
    pos = labels < head.num_classes
    ctr = torch.zeros(bt.shape[:2], dtype=dtype)
    ctr[pos] = head.centerness_target(bt[pos])
    return torch.where(pos, labels + 1, torch.zeros_like(labels)), bt, ctr


@pytest.mark.parametrize('c', range(len(U.TARGET_COMBOS)))
def test_get_targets_equal_the_reference_on_the_targets_case(golden, c):
    """Edges, ties, nested boxes, boxes past the image, an empty image and distances on the range bounds: the head's tensor form
    and the restatement of fcos_util both equal the reference's fp32 run exactly."""
    g = golden('fcos')
    cs, norm = U.TARGET_COMBOS[c]
    gts, _ = U.targets_case()
    head = build_head('iou', regress_ranges=U.SMALL_RANGES, center_sampling=cs, norm_on_bbox=norm, center_sample_radius=U.CASE_RADIUS)
    padded, valid, _ = U.pad_gts(gts)
    for assigned, bt, ctr in (head_targets(head, gts),
                              U.targets_ref(U.LEVEL_SIZES, U.STRIDES, U.SMALL_RANGES, padded, valid, cs, U.CASE_RADIUS, norm)):
        assert torch.equal(assigned.long(), T(g[f'tc.{c}.assigned']).long())
        assert torch.equal(bt, T(g[f'tc.{c}.bbox_targets']))
        assert torch.equal(ctr, T(g[f'tc.{c}.ctr_targets']))
    assert int((assigned[1] > 0).sum()) == 0 and int((assigned > 0).sum()) > 0


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_tensor_path_loss_on_the_cpu_matches_the_reference(golden, v):
    """FCOSHead.loss (tensor path) on the seeded maps against the reference head's own result: targets exactly, losses and
    gradients in fp64 to 1e-10, fp32 within 4 x the reference's own fp32 error; the restatement fcos_util.loss_ref likewise (its
    centerness term is true fp64, the reference's rounds the targets and the loss to fp32: 1e-6)."""
    g = golden('fcos')
    p = f'head.{v}.'
    metas, gts, labels = inputs()
    head = build_head(v)
    assigned, bt, ctr = head_targets(head, gts)
    assert torch.equal(assigned.long(), T(g[p + 'assigned']).long())
    assert torch.equal(bt, T(g[p + 'bbox_targets'])) and torch.equal(ctr, T(g[p + 'ctr_targets']))
    padded, valid, plab = U.pad_gts(gts, labels)
    kw = U.HEAD_VARIANTS[v]
    a2, bt2, ctr2 = U.targets_ref(U.LEVEL_SIZES, U.STRIDES, U.RANGES, padded, valid, kw.get('center_sampling', False), 1.5,
                                  kw.get('norm_on_bbox', False))
    assert torch.equal(a2.long(), assigned) and torch.equal(bt2, bt) and torch.equal(ctr2, ctr)
    lab = torch.where(assigned > 0, torch.gather(plab, 1, (assigned - 1).clamp(min=0)), torch.full_like(assigned, 80))
    assert torch.equal(lab, T(g[p + 'labels']).long())
    err = g[p + 'err32']
    for dt, tag in ((torch.float64, '64'), (torch.float32, '32')):
        maps = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        ls = head.loss(*maps, [x.to(dt) for x in gts], labels, metas)
        assert set(ls) == {'loss_cls', 'loss_bbox', 'loss_centerness'}
        mine = torch.stack([ls['loss_cls'], ls['loss_bbox'], ls['loss_centerness']])
        mine.sum().backward()
        grads = [U.maps_to_rows([m.grad for m in ms]) for ms in maps]
        if dt == torch.float64:
            np.testing.assert_allclose(mine.detach().numpy(), g[p + 'loss64'], rtol=1e-10)
            np.testing.assert_allclose(grads[1].numpy(), g[p + 'greg64'], rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(grads[2][..., 0].numpy(), g[p + 'gctr64'], rtol=1e-9, atol=1e-15)
            sums, sample = BU.digest(grads[0])
            np.testing.assert_allclose(sums, g[p + 'gcls64.sums'], rtol=1e-9)
            np.testing.assert_allclose(sample, g[p + 'gcls64.sample'], rtol=1e-9, atol=1e-15)
        else:
            for i in range(3):
                assert abs(float(mine[i].detach()) - float(g[p + 'loss64'][i])) <= 4 * max(float(err[i]), 2.0 ** -23 * float(g[p + 'loss64'][i]))
            for grad, want, e in ((grads[1], g[p + 'greg64'], err[4]), (grads[2][..., 0], g[p + 'gctr64'], err[5])):
                assert float((grad.double() - T(want)).abs().max()) <= 4 * max(float(e), 2.0 ** -23 * float(np.abs(want).max()))
    # the restatement takes the fp32 targets the kernels take (the reference's fp64 run forms them in fp64): the focal term equal,
    # the box term and its gradient within the reference's own fp32 error, the centerness term within fp32 rounding
    r = U.loss_ref(*U.head_maps(v), U.STRIDES, plab, assigned, bt, ctr, kind=v)
    np.testing.assert_allclose(float(r['losses'][0]), g[p + 'loss64'][0], rtol=1e-10)
    assert abs(float(r['losses'][1]) - float(g[p + 'loss64'][1])) <= float(err[1])
    np.testing.assert_allclose(float(r['losses'][2]), g[p + 'loss64'][2], rtol=1e-6)
    assert float((U.maps_to_rows(r['greg']) - T(g[p + 'greg64'])).abs().max()) <= float(err[4])
    np.testing.assert_allclose(U.maps_to_rows(r['gctr'])[..., 0].numpy(), g[p + 'gctr64'], rtol=0, atol=1e-6 * np.abs(g[p + 'gctr64']).max())
    np.testing.assert_allclose(BU.digest(U.maps_to_rows(r['gcls']))[0], g[p + 'gcls64.sums'], rtol=1e-9)


def test_tensor_path_loss_without_positives_is_the_sum_branch():
    """fcos_head.py:246-248: no positive point -> the box and centerness losses are 0 * the (empty) predictions."""
    metas, gts, labels = inputs()
    head = build_head('iou')
    maps = [[m.double().requires_grad_() for m in ms] for ms in U.head_maps('iou')]
    ls = head.loss(*maps, [x.new_zeros(0, 4).double() for x in gts], [x.new_zeros(0) for x in labels], metas)
    assert float(ls['loss_bbox']) == 0 and float(ls['loss_centerness']) == 0 and float(ls['loss_cls']) > 0
    (ls['loss_cls'] + ls['loss_bbox'] + ls['loss_centerness']).backward()
    assert all(float(m.grad.abs().max()) == 0 for ms in maps[1:] for m in ms)
    r = U.loss_ref(*U.head_maps('iou'), U.STRIDES, torch.zeros(2, 1, dtype=torch.long), torch.zeros(2, 428, dtype=torch.int32),
                   torch.zeros(2, 428, 4), torch.zeros(2, 428))
    np.testing.assert_allclose(float(r['losses'][0]), float(ls['loss_cls']), rtol=1e-12)


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_per_image_get_bboxes_on_the_cpu_matches_the_reference(golden, v):
    """The nms_pre cut by the stable descending order of max_c sigmoid(cls) * sigmoid(centerness), distance2bbox clamped to the
    image, the scores with their background column and the centerness: the reference's own output (before the NMS, which is a
    device operation here)."""
    from htd_amd.registry import ConfigDict
    g = golden('fcos')
    metas, _, _ = inputs()
    head = build_head(v)
    res = head.get_bboxes(*U.head_maps(v), metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores, ctrs) in enumerate(res):
        p = f'head.{v}.'
        assert scores.shape == (boxes.size(0), 81) and float(scores[:, -1].abs().max()) == 0
        np.testing.assert_array_equal(boxes.numpy(), g[p + f'boxes{i}'])
        np.testing.assert_array_equal(ctrs.numpy(), g[p + f'ctrs{i}'])
        np.testing.assert_allclose(scores.double().sum(1).numpy(), g[p + f'score_rows{i}'], rtol=1e-12)
        assert float(boxes[:, [0, 2]].max()) <= metas[i]['img_shape'][1] and float(boxes.min()) >= 0


def test_fused_loss_dispatch_rule():
    """CPU maps take the tensor form whatever the modules; the rule itself is about modules, reductions and layouts."""
    head = build_head('iou')
    cls, reg, ctr = U.head_maps('iou')
    assert not head._fused_loss_ok(cls, reg, ctr)
    from htd_amd import mmcv_ops as M
    assert M.FCOS_BOX_KINDS == dict(IoULoss=0, GIoULoss=2)
    m = torch.zeros(2, 1, 4, 5)
    assert M.nhwc_channel_stride(m) == 1 and M.nhwc_channel_stride(torch.zeros(2, 8, 4, 5)) is None
    assert M.nhwc_channel_stride(torch.zeros(2, 8, 4, 5).contiguous(memory_format=torch.channels_last)[:, :3]) == 8


def test_new_abi_symbols_are_declared_and_exported():
    from htd_amd import capi
    names = {n for n, _, _ in capi.declared_functions()}
    want = {'htd_fcos_targets_workspace_bytes', 'htd_fcos_targets', 'htd_fcos_loss_partial_rows', 'htd_fcos_loss',
            'htd_fcos_grad_scale', 'htd_fcos_keys'}
    assert want <= names
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in want)
    assert lib.htd_fcos_loss_partial_rows() > 0 and lib.htd_fcos_loss_partial_rows() % 2 == 0
    assert lib.htd_fcos_targets_workspace_bytes(2, 428) >= 2 * 2 * 12
    header = open(capi.HEADER).read()
    assert 'fcos_head.py:415-558' in header and 'fcos_head.py:159-253' in header and 'fcos_head.py:364-372' in header
