"""VFNet without a GPU: VarifocalLoss against the reference's own results (tests/golden/vfnet.npz, recipe in
tests/golden/make_golden_vfnet.py), the configs against the reference's merged configs, the state dict, VFNetHead.loss_tensor,
star_dcn_offset and the per-image get_bboxes against the reference's own run, the other target kind and class loss, the
no-positive batch and the new entry points of the C ABI.

Tolerances: 1e-10 relative in fp64 -- the fp64 runs take their targets through + - * / only, and the fp64 exp / log of two hosts
agree far below that; the fp32 runs, which depend on the host's fp32 exp / log, take the rule of the fp32 error: 4 x max(the
reference's own |fp32 - fp64| on that case, one fp32 ulp of the largest entry)."""
import json
import os

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T
from golden_util import seeded_tensor
import vfnet_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ('loss_cls', 'loss_bbox', 'loss_bbox_rf')
# head.{v}.err32: |fp32 - fp64| of [3 losses, gcls, greg, gref, iou_ini, iou_rf, gclspos, 3 sums]
E_GCLS, E_GREG, E_GREF, E_INI, E_RF, E_GCLSPOS, E_SUMS = 3, 4, 5, 6, 7, 8, 9


def build_head(variant='giou', **extra):
    from htd_amd.registry import ConfigDict, build_head as build
    import htd_amd.detector  # noqa: F401
    train_cfg = dict(U.TRAIN_CFG)
    train_cfg.update(extra.pop('train_cfg', {}))
    return build(dict(U.head_cfg(variant, **extra), train_cfg=ConfigDict(train_cfg)))


def inputs():
    return D.inputs('cpu', U.detector_inputs)[1:]


def head_losses(ls):
    return torch.stack([ls[k] for k in KEYS])


# ---------------------------------------------------------------------------------------------------- the loss module
def test_varifocal_loss_equals_the_reference(golden):
    """Three parameter sets (gamma 2 / 1.5, iou_weighted on / off) with and without weight, with avg_factor and under each
    reduction: values and gradients; the reference's asserts."""
    import htd_amd.detector  # noqa: F401
    from htd_amd.registry import LOSSES, build_loss
    g = golden('vfnet')
    c = U.loss_module_case()
    assert LOSSES.get('VarifocalLoss') is not None
    for name, kw in U.LOSS_MODULES.items():
        mod = build_loss(dict(type='VarifocalLoss', **kw))
        for i, (reduction, avg, weighted) in enumerate(U.LOSS_MODES):
            x = c['pred'].clone().requires_grad_()
            val = mod(x, c['target'], weight=c['weight'] if weighted else None, avg_factor=avg, reduction_override=reduction)
            val.sum().backward()
            np.testing.assert_allclose(val.detach().numpy(), g[f'{name}.{i}'], rtol=1e-10, err_msg=f'{name}.{i}')
            np.testing.assert_allclose(x.grad.numpy(), g[f'{name}.{i}.grad'], rtol=1e-10, atol=1e-14, err_msg=f'{name}.{i}')
    mod = build_loss(dict(type='VarifocalLoss'))
    assert (mod.use_sigmoid, mod.alpha, mod.gamma, mod.iou_weighted, mod.reduction, mod.loss_weight) == (True, 0.75, 2.0, True, 'mean', 1.0)
    with pytest.raises(AssertionError):
        build_loss(dict(type='VarifocalLoss', use_sigmoid=False))
    with pytest.raises(AssertionError):
        build_loss(dict(type='VarifocalLoss', alpha=-0.1))
    with pytest.raises(AssertionError):
        mod(c['pred'], c['target'], reduction_override='max')
    with pytest.raises(AssertionError):
        mod(c['pred'], c['target'][:, :4])
    with pytest.raises(ValueError):
        mod(c['pred'], c['target'], avg_factor=2.0, reduction_override='sum')
    # the targets are weights only where they are positive
    zero = mod(c['pred'], torch.zeros_like(c['target']), reduction_override='none')
    want = 0.75 * c['pred'].sigmoid() ** 2 * torch.nn.functional.softplus(c['pred'])
    np.testing.assert_allclose(zero.numpy(), want.numpy(), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------- configs, state
@pytest.mark.parametrize('which', list(U.CONFIGS))
def test_vfnet_config_equals_the_reference_merged_config(which):
    from htd_amd.apis import check_supported
    from htd_amd.configs import vfnet_config
    ref = json.load(open(os.path.join(GOLDEN, os.path.basename(U.CONFIGS[which])[:-3] + '_cfg.json')))
    cfg = vfnet_config(**U.CONFIG_ARGS[which])
    mine = {k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in U.CFG_KEYS}
    mine['train_pipeline'] = [p.to_dict() if hasattr(p, 'to_dict') else p for p in cfg.data.train.pipeline]
    assert json.loads(json.dumps(mine)) == ref
    assert ref['optimizer']['paramwise_cfg'] == dict(bias_lr_mult=2.0, bias_decay_mult=0.0)
    with pytest.raises(Exception, match='paramwise_cfg'):
        check_supported(cfg)
    if which == 'r101_mstrain':
        resize = ref['train_pipeline'][2]
        assert resize['multiscale_mode'] == 'range' and resize['img_scale'] == [[1333, 480], [1333, 960]]
        assert ref['lr_config']['step'] == [16, 22] and ref['total_epochs'] == 24 and ref['model']['backbone']['depth'] == 101
    with pytest.raises(ValueError):
        vfnet_config(34)


def test_state_dict_keys_and_shapes_equal_the_fixture(golden):
    from htd_amd.configs import build_baseline_detector
    from htd_amd.registry import DETECTORS, HEADS
    g = golden('vfnet')
    det = build_baseline_detector('vfnet')
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_keys']]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == g['state_shapes'].tolist()
    head = det.bbox_head
    assert type(det) is DETECTORS.get('VFNet') and type(head) is HEADS.get('VFNetHead')
    assert head.reg_denoms == [64, 128, 256, 512, 1024] and len(head.scales) == len(head.scales_refine) == 5
    assert head.dcn_base_offset.shape == (1, 18, 1, 1) and head.dcn_base_offset.dtype == torch.float64
    assert head.dcn_base_offset.flatten().tolist() == [-1, -1, -1, 0, -1, 1, 0, -1, 0, 0, 0, 1, 1, -1, 1, 0, 1, 1]
    assert head.vfnet_reg_refine_dconv.weight.shape == (256, 256, 3, 3) and head.vfnet_cls.weight.size(0) == 80
    assert torch.allclose(head.vfnet_cls.bias.sigmoid(), torch.full_like(head.vfnet_cls.bias, 0.01))
    assert head.num_anchors == 1 and not head.sampling and head.anchor_center_offset == 0.0 and head.gradient_mul == 0.1
    with pytest.raises(NotImplementedError):
        build_head(bbox_norm_type='area')


def test_a_reference_format_checkpoint_loads_without_the_pre_2_0_rename(golden, tmp_path):
    """A `.pth` in the reference's wire format without version metadata: AnchorFreeHead's rename would look for conv_cls /
    conv_reg; VFNetHead loads vfnet_cls / vfnet_reg as they are, strictly."""
    from htd_amd.checkpoint import load_checkpoint
    from htd_amd.configs import build_baseline_detector
    g = golden('vfnet')
    ref = U.fixture_state(g['state_keys'], g['state_shapes'], float(g['cls_scale']), float(g['cls_bias_shift']))
    path = D.save_reference_checkpoint(ref, tmp_path)
    torch.manual_seed(123)
    model = build_baseline_detector('vfnet')
    load_checkpoint(model, path, strict=True)
    sd = model.state_dict()
    assert all(torch.equal(sd[k].float(), v.float()) for k, v in ref.items())
    plain = {k[len('bbox_head.'):]: v for k, v in ref.items() if k.startswith('bbox_head.')}
    missing, unexpected = model.bbox_head.load_state_dict(plain, strict=True)
    assert not missing and not unexpected


# ---------------------------------------------------------------------------------------------------- the head
def test_star_dcn_offset_equals_the_reference(golden):
    g = golden('vfnet')
    head = build_head()
    x = U.star_case().double().requires_grad_()
    off = head.star_dcn_offset(x.exp() * 64, 0.1, 8)
    w = seeded_tensor('vfnet.star.w', tuple(off.shape)).double()
    (off * w).sum().backward()
    np.testing.assert_allclose(off.detach().numpy(), g['star.offset'], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(x.grad.numpy(), g['star.grad'], rtol=1e-10, atol=1e-14)
    # the nine taps land on the corners, the edge midpoints and the centre of the box (tap k at (k // 3 - 1, k % 3 - 1) + offset)
    pred = torch.tensor([3., 5., 7., 11.]).view(1, 4, 1, 1) * 8
    o = head.star_dcn_offset(pred, 1.0, 8).flatten().view(9, 2) + head.dcn_base_offset.float().flatten().view(9, 2)
    assert o.tolist() == [[-5, -3], [-5, 0], [-5, 7], [0, -3], [0, 0], [0, 7], [11, -3], [11, 0], [11, 7]]


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_tensor_path_loss_on_the_cpu_matches_the_reference(golden, v):
    """VFNetHead.loss (tensor path) on the seeded maps against the reference head's own runs: fp32 gts beside fp64 and fp32 maps."""
    g = golden('vfnet')
    p = f'head.{v}.'
    metas, gts, labels = inputs()
    head = build_head(v)
    err = g[p + 'err32']
    pi = T(g['head.pos_index']).long()
    for dt in (torch.float64, torch.float32):
        cls, reg, ref = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        assert not head._fused_loss_ok(cls, reg, ref, labels, None, metas)
        ls = head.loss(cls, reg, ref, gts, labels, metas)
        assert set(ls) == set(KEYS) and all(x.dim() == 0 for x in ls.values())
        mine = head_losses(ls)
        mine.sum().backward()
        gcls, greg, gref = (U.maps_to_rows([m.grad for m in ms]) for ms in (cls, reg, ref))
        if dt == torch.float64:
            np.testing.assert_allclose(mine.detach().numpy(), g[p + 'loss64'], rtol=1e-10)
            np.testing.assert_allclose(greg.numpy(), g[p + 'greg64'], rtol=1e-9, atol=1e-14)
            np.testing.assert_allclose(gref.numpy(), g[p + 'gref64'], rtol=1e-9, atol=1e-14)
            np.testing.assert_allclose(gcls[pi[:, 0], pi[:, 1], pi[:, 2]].numpy(), g[p + 'gclspos64'], rtol=1e-10)
            sums, sample = BU.digest(gcls)
            np.testing.assert_allclose(sums, g[p + 'gcls64.sums'], rtol=1e-10)
            np.testing.assert_allclose(sample, g[p + 'gcls64.sample'], rtol=1e-10, atol=1e-14)
        else:
            for i in range(3):
                want = float(g[p + 'loss64'][i])
                assert abs(float(mine[i].detach()) - want) <= 4 * max(float(err[i]), EPS32 * want), (v, i)
            for mine_g, key, e in ((greg, 'greg64', E_GREG), (gref, 'gref64', E_GREF)):
                want = g[p + key]
                assert float((mine_g.double() - T(want)).abs().max()) <= 4 * max(float(err[e]), EPS32 * float(np.abs(want).max()))
            want = g[p + 'gclspos64']
            assert float((gcls[pi[:, 0], pi[:, 1], pi[:, 2]].double() - T(want)).abs().max()) <= \
                4 * max(float(err[E_GCLSPOS]), EPS32 * float(np.abs(want).max()))
            want = g[p + 'gcls64.sample']
            assert float(np.abs(BU.digest(gcls)[1] - want).max()) <= 4 * max(float(err[E_GCLS]), EPS32 * float(np.abs(want).max()))


def test_the_fixture_holds_a_clamped_iou_and_every_image_a_positive(golden):
    g = golden('vfnet')
    a = T(g['head.assigned']).long()
    assert int((a > 0).sum()) == len(g['head.pos_index']) and int((a > 0).sum(1).min()) > 0
    b, l, y, x = U.NO_OVERLAP
    at = sum(U.LEVEL_ANCHORS[:l]) + y * U.LEVEL_SIZES[l][1] + x
    assert int(a[b, at]) > 0
    for v in U.HEAD_VARIANTS:
        assert float(g[f'head.{v}.iou_ini64'][b, at]) == 1e-6 and float(g[f'head.{v}.iou_rf64'][b, at]) > 1e-3
        assert float(g[f'head.{v}.sums64'][0]) == float((a > 0).sum())


def test_the_other_target_kind_and_class_loss_run_and_match_the_reference(golden):
    """use_atss=False (FCOS targets with centre sampling, points at the cell centres, norm_on_bbox off) and use_vfl=False
    (FocalLoss on the labels with ATSS's label weights)."""
    g = golden('vfnet')
    metas, gts, labels = inputs()
    for name, extra in (('fcos', dict(use_atss=False, center_sampling=True)), ('fl', dict(use_vfl=False))):
        head = build_head('giou', **extra)
        cls, reg, ref = [[m.double() for m in ms] for ms in U.head_maps()]
        assert not head._fused_loss_ok(cls, reg, ref, labels, None, metas)
        boxes = [x.double() for x in gts] if name == 'fcos' else gts           # as the fixture's runs
        mine = head_losses(head.loss(cls, reg, ref, boxes, labels, metas))
        np.testing.assert_allclose(mine.numpy(), g[f'head.{name}.loss64'], rtol=1e-10, err_msg=name)
    head = build_head('giou', use_atss=False)
    assert head.norm_on_bbox is False and type(head.loss_cls).__name__ == 'VarifocalLoss'
    pts = head.get_points(U.LEVEL_SIZES, torch.float32, 'cpu')
    assert pts[0][0].tolist() == [4.0, 4.0] and build_head().get_points(U.LEVEL_SIZES, torch.float32, 'cpu')[0][0].tolist() == [0.0, 0.0]
    assert type(build_head(use_vfl=False).loss_cls).__name__ == 'FocalLoss'


def test_no_positive_batch_gives_zero_box_losses_and_a_finite_class_loss(golden):
    """Each averaging factor is clamped to 1: both box losses are exactly 0 with zero gradients, unlike GFL's 0 / 0."""
    g = golden('vfnet')
    metas, gts, labels = inputs()
    head = build_head()
    cls, reg, ref = [[m.double().requires_grad_() for m in ms] for ms in U.head_maps()]
    ls = head.loss(cls, reg, ref, [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in labels], metas)
    mine = head_losses(ls)
    mine.sum().backward()
    mine = mine.detach()
    want = g['head.nopos.loss']
    assert float(want[1]) == 0 and float(want[2]) == 0 and np.isfinite(want[0])
    assert float(mine[1]) == 0 and float(mine[2]) == 0 and abs(float(mine[0]) - float(want[0])) <= 4 * EPS32 * float(want[0])
    assert all(float(m.grad.abs().max()) == 0 for m in reg + ref) and all(bool(torch.isfinite(m.grad).all()) for m in cls)


def test_per_image_get_bboxes_on_the_cpu_matches_the_reference(golden):
    """The nms_pre cut (biting on levels 0 and 1) by max_c sigmoid(cls), distance2bbox of the refined distances clamped to the
    image, the scores with their background column: the reference's own output before the NMS."""
    from htd_amd.registry import ConfigDict
    g = golden('vfnet')
    metas, _, _ = inputs()
    head = build_head()
    res = head.get_bboxes(*U.head_maps(), metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores) in enumerate(res):
        assert scores.shape == (boxes.size(0), 81) and float(scores[:, -1].abs().max()) == 0
        np.testing.assert_allclose(boxes.numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-4)
        np.testing.assert_allclose(scores.double().sum(1).numpy(), g[f'head.score_rows{i}'], rtol=1e-6)
        assert float(boxes[:, [0, 2]].max()) <= metas[i]['img_shape'][1] and float(boxes.min()) >= 0


def test_new_abi_symbols_are_declared_and_exported():
    from htd_amd import capi
    names = {n for n, _, _ in capi.declared_functions()}
    want = {'htd_vfnet_star_fwd', 'htd_vfnet_star_bwd', 'htd_vfnet_quality_workspace_bytes', 'htd_vfnet_quality',
            'htd_vfnet_loss_partial_rows', 'htd_vfnet_loss', 'htd_vfnet_grad_scale'}
    assert want <= names
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in want)
    assert lib.htd_vfnet_loss_partial_rows() > 0 and lib.htd_vfnet_loss_partial_rows() % 2 == 0
    assert lib.htd_vfnet_quality_workspace_bytes(2, 428) >= 2 * 2 * 3 * 8
    from htd_amd.csrc import build
    assert 'vfnet.hip' in build.sources() and build.EXTRA['vfnet.hip'] == ['-ffp-contract=off']
