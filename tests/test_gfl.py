"""GFL without a GPU: QualityFocalLoss, DistributionFocalLoss, bbox2distance and Integral against the reference's own results
(tests/golden/gfl.npz, recipe in tests/golden/make_golden_gfl.py), the configs against the reference's merged configs, the state
dict, GFLHead.loss_tensor and the per-image get_bboxes against the reference's own run, the no-positive batch and the new entry
points of the C ABI.

Tolerances: 1e-10 relative in fp64 -- the fp64 runs take their targets through + - * / only (no fp32 logarithm, unlike ATSS's
delta targets), and the fp64 exp / log of two hosts agree far below that; the fp32 runs, which depend on the host's fp32 exp /
log, take the rule of the fp32 error: 4 x max(the reference's own |fp32 - fp64| on that case, one fp32 ulp of the largest
entry)."""
import json
import os

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T
import gfl_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def build_head(variant='giou', **extra):
    from htd_amd.registry import ConfigDict, build_head as build
    import htd_amd.detector  # noqa: F401
    train_cfg = dict(U.TRAIN_CFG)
    train_cfg.update(extra.pop('train_cfg', {}))
    return build(dict(U.head_cfg(variant, **extra), train_cfg=ConfigDict(train_cfg)))


def inputs():
    return D.inputs('cpu', U.detector_inputs)[1:]


def head_losses(ls):
    return torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_dfl'])])


# ---------------------------------------------------------------------------------------------------- modules
def test_loss_modules_equal_the_reference(golden):
    """QFL (beta 2 and 1.5) and DFL with and without weight, with avg_factor and under each reduction: values and gradients."""
    import htd_amd.detector  # noqa: F401
    from htd_amd.registry import LOSSES, build_loss
    g = golden('gfl')
    c = U.loss_module_case()
    assert LOSSES.get('QualityFocalLoss') is not None and LOSSES.get('DistributionFocalLoss') is not None
    mods = dict(qfl=(build_loss(dict(type='QualityFocalLoss', beta=2.0, loss_weight=1.5)), c['pred'], (c['label'], c['score']), c['weight']),
                qfl15=(build_loss(dict(type='QualityFocalLoss', beta=1.5)), c['pred'], (c['label'], c['score']), c['weight']),
                dfl=(build_loss(dict(type='DistributionFocalLoss', loss_weight=0.25)), c['dpred'], c['dlabel'], c['dweight']))
    for i, (reduction, avg, weighted) in enumerate(U.LOSS_MODES):
        for name, (mod, pred, target, weight) in mods.items():
            x = pred.clone().requires_grad_()
            val = mod(x, target, weight=weight if weighted else None, avg_factor=avg, reduction_override=reduction)
            val.sum().backward()
            np.testing.assert_allclose(val.detach().numpy(), g[f'{name}.{i}'], rtol=1e-10, err_msg=f'{name}.{i}')
            np.testing.assert_allclose(x.grad.numpy(), g[f'{name}.{i}.grad'], rtol=1e-10, atol=1e-14, err_msg=f'{name}.{i}')
    with pytest.raises(ValueError):
        mods['dfl'][0](c['dpred'], c['dlabel'], avg_factor=2.0, reduction_override='sum')
    with pytest.raises(AssertionError):
        mods['qfl'][0](c['pred'], c['label'])                       # the target is the pair (label, score)
    # the positive's own class is supervised by its score, the other classes and the negatives by 0
    mod = mods['qfl'][0]
    one = mod(c['pred'][1:2], (c['label'][1:2], c['score'][1:2]), reduction_override='none')
    zero = mod(c['pred'][1:2], (torch.tensor([5]), c['score'][1:2]), reduction_override='none')
    assert float((one - zero).abs()) > 1e-3


def test_bbox2distance_and_integral(golden):
    from htd_amd.core import bbox2distance, distance2bbox
    from htd_amd.detector.anchor_heads import Integral
    g = golden('gfl')
    pts, box = U.distance_case()
    np.testing.assert_allclose(bbox2distance(pts, box).numpy(), g['b2d.plain'], rtol=1e-10)
    clamped = bbox2distance(pts, box, max_dis=7)
    np.testing.assert_allclose(clamped.numpy(), g['b2d.max7'], rtol=1e-10)
    assert float(clamped.max()) == 7 - 0.1 and float(clamped.min()) == 0
    np.testing.assert_allclose(distance2bbox(pts, bbox2distance(pts, box)).numpy(), box.numpy(), rtol=1e-10, atol=1e-12)
    integral = Integral(7)
    assert list(integral.state_dict()) == ['project'] and integral.project.tolist() == list(range(8))
    x = c = U.loss_module_case()['dpred']
    want = (torch.softmax(c, 1) * torch.arange(8.)).sum(1)
    out = integral(torch.cat([x, x, x, x], 1))
    assert out.shape == (10, 4)
    np.testing.assert_allclose(out.numpy(), want[:, None].expand(10, 4).numpy(), rtol=1e-12)
    onehot = torch.full((1, 32), -1e4, dtype=torch.float64)
    onehot[0, [3, 8 + 0, 16 + 7, 24 + 5]] = 1e4
    assert integral(onehot).tolist() == [[3.0, 0.0, 7.0, 5.0]]


# ---------------------------------------------------------------------------------------------------- configs, state
@pytest.mark.parametrize('which', list(U.CONFIGS))
def test_gfl_config_equals_the_reference_merged_config(which):
    from htd_amd.apis import check_supported
    from htd_amd.configs import gfl_config
    ref = json.load(open(os.path.join(GOLDEN, os.path.basename(U.CONFIGS[which])[:-3] + '_cfg.json')))
    cfg = gfl_config(**U.CONFIG_ARGS[which])
    mine = {k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in U.CFG_KEYS}
    mine['train_pipeline'] = [p.to_dict() if hasattr(p, 'to_dict') else p for p in cfg.data.train.pipeline]
    assert json.loads(json.dumps(mine)) == ref
    check_supported(cfg)
    if which == 'r101_mstrain':
        resize = ref['train_pipeline'][2]
        assert resize['multiscale_mode'] == 'range' and resize['img_scale'] == [[1333, 480], [1333, 800]]
        assert ref['lr_config']['step'] == [16, 22] and ref['total_epochs'] == 24 and ref['model']['backbone']['depth'] == 101
    with pytest.raises(ValueError):
        gfl_config(34)


def test_state_dict_keys_and_shapes_equal_the_fixture(golden):
    from htd_amd.configs import build_baseline_detector
    from htd_amd.registry import DETECTORS, HEADS
    g = golden('gfl')
    det = build_baseline_detector('gfl')
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_keys']]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == g['state_shapes'].tolist()
    head = det.bbox_head
    assert type(det) is DETECTORS.get('GFL') and type(head) is HEADS.get('GFLHead')
    assert sd['bbox_head.integral.project'].tolist() == list(range(17)) and head.reg_max == 16
    assert head.gfl_reg.weight.size(0) == 68 and head.gfl_cls.weight.size(0) == 80 and len(head.scales) == 5
    assert torch.allclose(head.gfl_cls.bias.sigmoid(), torch.full_like(head.gfl_cls.bias, 0.01))
    assert head.num_anchors == 1 and not head.sampling


def test_targets_are_shared_with_atss_and_hold_the_gt_boxes():
    from htd_amd.detector.anchor_heads import ATSSHead, GFLHead
    from htd_amd.detector.vfnet_head import VFNetHead
    assert GFLHead.get_targets is ATSSHead.get_targets and GFLHead._get_target_single is ATSSHead._get_target_single
    assert GFLHead.get_num_level_anchors_inside is ATSSHead.get_num_level_anchors_inside
    # VFNetHead keeps the reference's own get_targets / _get_target_single (they choose between ATSS and FCOS targets); what
    # they call is the same
    assert VFNetHead.get_num_level_anchors_inside is ATSSHead.get_num_level_anchors_inside
    assert VFNetHead._anchor_targets is ATSSHead._anchor_targets is GFLHead._anchor_targets
    assert VFNetHead._anchor_targets_single is ATSSHead._anchor_targets_single is GFLHead._anchor_targets_single
    assert VFNetHead._pos_bbox_targets is not ATSSHead._pos_bbox_targets                # the gt boxes, as GFLHead's
    metas, gts, labels = inputs()
    head = build_head()
    anchor_list, valid = head.get_anchors(U.LEVEL_SIZES, metas, device='cpu')
    t = head.get_targets(anchor_list, valid, gts, metas, gt_labels_list=labels, label_channels=80)
    bbox_targets, lab = torch.cat(t[3], 1), torch.cat(t[1], 1)
    pos = lab < 80
    assert int(pos.sum()) == 77
    for b in range(2):
        rows = bbox_targets[b][pos[b]]
        assert all(any(torch.equal(r, x) for x in gts[b]) for r in rows)            # gt boxes, not deltas


# ---------------------------------------------------------------------------------------------------- the head
@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_tensor_path_loss_on_the_cpu_matches_the_reference(golden, v):
    """GFLHead.loss (tensor path) on the seeded maps against the reference head's own runs.  The fp64 run takes fp32 gts beside
    fp64 maps, as the fixture's does (the reference's targets mix dtypes under fp64 gts)."""
    g = golden('gfl')
    p = f'head.{v}.'
    metas, gts, labels = inputs()
    head = build_head(v)
    err = g[p + 'err32']
    for dt in (torch.float64, torch.float32):
        cls, reg = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        assert not head._fused_loss_ok(cls, reg, labels, None, metas)
        ls = head.loss(cls, reg, gts, labels, metas)
        assert set(ls) == {'loss_cls', 'loss_bbox', 'loss_dfl'} and all(len(x) == 5 for x in ls.values())
        mine = head_losses(ls)
        mine.sum().backward()
        gcls, greg = (U.maps_to_rows([m.grad for m in ms]) for ms in (cls, reg))
        if dt == torch.float64:
            np.testing.assert_allclose(mine.detach().numpy(), g[p + 'loss64'], rtol=1e-10)
            np.testing.assert_allclose(greg.numpy(), g[p + 'greg64'], rtol=1e-10, atol=1e-14)
            pi = T(g['head.pos_index']).long()
            np.testing.assert_allclose(gcls[pi[:, 0], pi[:, 1], pi[:, 2]].numpy(), g[p + 'gclspos64'], rtol=1e-10)
            sums, sample = BU.digest(gcls)
            np.testing.assert_allclose(sums, g[p + 'gcls64.sums'], rtol=1e-10)
            np.testing.assert_allclose(sample, g[p + 'gcls64.sample'], rtol=1e-10, atol=1e-14)
        else:
            for i in range(3):
                ref = float(g[p + 'loss64'][i])
                assert abs(float(mine[i].detach()) - ref) <= 4 * max(float(err[i]), EPS32 * ref), (v, i)
            want = g[p + 'greg64']
            assert float((greg.double() - T(want)).abs().max()) <= 4 * max(float(err[4]), EPS32 * float(np.abs(want).max()))
            pi = T(g['head.pos_index']).long()
            want = g[p + 'gclspos64']
            assert float((gcls[pi[:, 0], pi[:, 1], pi[:, 2]].double() - T(want)).abs().max()) <= 4 * max(float(err[7]), EPS32 * float(np.abs(want).max()))
            want = g[p + 'gcls64.sample']
            assert float(np.abs(BU.digest(gcls)[1] - want).max()) <= 4 * max(float(err[3]), EPS32 * float(np.abs(want).max()))


def test_the_clamp_of_the_dfl_targets_bites_at_reg_max_7(golden):
    """25 target sides of the head case exceed 6.9: with reg_max 7 they are clamped to 6.9 and split between bins 6 and 7."""
    g = golden('gfl')
    t = T(g['head.tdist'])[T(g['head.assigned']).long() > 0]
    assert int((t > 6.9).sum()) == 25 and float(t.max()) == 9.0 and int((T(g['head.assigned']) > 0).sum()) == 77
    assert abs(float(g['head.giou_r7.loss64'][2]) - float(g['head.giou.loss64'][2])) > 1e-2


def test_no_positive_batch_gives_nan_box_losses_and_a_finite_class_loss(golden):
    """The averaging factor is not clamped: 0 / 0, as the reference computes it."""
    g = golden('gfl')
    metas, gts, labels = inputs()
    head = build_head()
    cls, reg = [[m.double().requires_grad_() for m in ms] for ms in U.head_maps()]
    ls = head.loss(cls, reg, [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in labels], metas)
    mine = head_losses(ls)
    mine.sum().backward()
    mine = mine.detach()
    ref = g['head.nopos.loss']
    assert np.isnan(ref[1:]).all() and np.isfinite(ref[0])
    assert bool(torch.isnan(mine[1:]).all()) and abs(float(mine[0]) - float(ref[0])) <= 4 * EPS32 * float(ref[0])
    assert all(bool(torch.isnan(m.grad).all()) for m in reg) and all(bool(torch.isfinite(m.grad).all()) for m in cls)


def test_per_image_get_bboxes_on_the_cpu_matches_the_reference(golden):
    """The nms_pre cut (biting on levels 0 and 1) by max_c sigmoid(cls), distance2bbox of the integral times the stride clamped to
    the image, the scores with their background column: the reference's own output before the NMS."""
    from htd_amd.registry import ConfigDict
    g = golden('gfl')
    metas, _, _ = inputs()
    head = build_head()
    res = head.get_bboxes(*U.head_maps(), metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores) in enumerate(res):
        assert scores.shape == (boxes.size(0), 81) and float(scores[:, -1].abs().max()) == 0
        np.testing.assert_allclose(boxes.numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-4)       # (exp is the machine's)
        np.testing.assert_allclose(scores.double().sum(1).numpy(), g[f'head.score_rows{i}'], rtol=1e-6)
        assert float(boxes[:, [0, 2]].max()) <= metas[i]['img_shape'][1] and float(boxes.min()) >= 0


def test_dispatch_rule_is_false_on_the_cpu():
    metas, gts, labels = inputs()
    head = build_head()
    assert not head._fused_loss_ok(*U.head_maps(), labels, None, metas)


def test_new_abi_symbols_are_declared_and_exported():
    from htd_amd import capi
    names = {n for n, _, _ in capi.declared_functions()}
    want = {'htd_gfl_quality_workspace_bytes', 'htd_gfl_quality', 'htd_gfl_loss_partial_rows', 'htd_gfl_loss',
            'htd_gfl_grad_scale', 'htd_gfl_decode'}
    assert want <= names
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in want)
    assert lib.htd_gfl_loss_partial_rows() > 0 and lib.htd_gfl_loss_partial_rows() % 2 == 0
    assert lib.htd_gfl_quality_workspace_bytes(2, 428) >= 2 * 2 * 8
    from htd_amd.csrc import build
    assert 'gfl.hip' in build.sources() and build.EXTRA['gfl.hip'] == ['-ffp-contract=off']
