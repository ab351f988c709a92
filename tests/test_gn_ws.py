"""GroupNorm + weight-standardised models, host side: ConvWS2d and weight_standardize against the tensor formula of mmcv's
ConvWS2d (mmcv-knowledge: mmcv 1.2.1 -- torch.std, i.e. the unbiased estimator, and eps added to the std, not under the root),
the registry entries, the reference's GN+WS Faster R-CNN config and state dict (tests/golden/gn_ws.npz and
faster_rcnn_r50_fpn_gn_ws-all_1x_coco_cfg.json, recipe in tests/golden/make_golden_gn_ws.py) and the new C ABI symbols."""
import json
import os

import pytest
import torch

import gn_ws_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def formula64(w, eps):
    """(w - mean) / (std + eps) written out: unbiased variance sum(c^2) / (K - 1), eps beside the root"""
    flat = w.double().reshape(w.size(0), -1)
    K = flat.size(1)
    c = flat - flat.sum(1, keepdim=True) / K
    std = torch.sqrt((c * c).sum(1, keepdim=True) / (K - 1))
    return (c / (std + eps)).view_as(w)


def reference_cfg():
    with open(os.path.join(ROOT, 'tests', 'golden', U.CFG_JSON)) as f:
        return json.load(f)


@pytest.mark.parametrize('shape,eps', [((64, 3, 7, 7), 1e-5), ((8, 16, 3, 3), 1e-5), ((5, 12, 1, 1), 1e-2)])
def test_conv_ws_standardises_with_unbiased_std_and_eps_beside_the_root(shape, eps):
    from htd_amd.detector.bricks import ConvWS2d, build_conv_layer
    conv = build_conv_layer(dict(type='ConvWS'), shape[1], shape[0], shape[2], bias=False) if eps == 1e-5 else \
        ConvWS2d(shape[1], shape[0], shape[2], bias=False, eps=eps)
    assert type(conv) is ConvWS2d and conv.eps == eps and tuple(conv.weight.shape) == shape
    with torch.no_grad():
        conv.weight.copy_(torch.randn(shape, generator=torch.Generator().manual_seed(3)) * 0.05 + 0.02)
    got = conv.standardized_weight()
    want = formula64(conv.weight.detach(), eps)
    got = got.detach()
    assert float((got.double() - want).abs().max()) <= 8 * 2.0 ** -23 * float(want.abs().max())
    # the two look-alikes are far outside that: the biased estimator, and eps under the root
    flat = conv.weight.detach().double().reshape(shape[0], -1)
    c = flat - flat.mean(1, keepdim=True)
    biased = (c / (flat.std(1, keepdim=True, unbiased=False) + eps)).view(shape)
    under = (c / torch.sqrt(flat.var(1, keepdim=True) + eps)).view(shape)
    for other in (biased, under):
        assert float((got.double() - other).abs().max()) > 1e-4 * float(want.abs().max())
    # every row: mean 0, unbiased std 1 / (1 + eps / std)
    rows = got.detach().double().reshape(shape[0], -1)
    assert float(rows.mean(1).abs().max()) < 1e-6
    torch.testing.assert_close(rows.std(1), flat.std(1) / (flat.std(1) + eps), rtol=1e-5, atol=0)


def test_weight_standardize_cpu_gradient_matches_autograd_and_the_kernel_formula():
    """The CPU path is the tensor formula under autograd; the backward kernel's closed form (h = g d - c (sum g c) d^2 / ((K-1) std),
    gw = h - mean(h)) is the same gradient."""
    from htd_amd import mmcv_ops as M
    gen = torch.Generator().manual_seed(11)
    w = (torch.randn(6, 4, 3, 3, generator=gen, dtype=torch.float64) * 0.1 + 0.03).requires_grad_()
    g = torch.randn(6, 4, 3, 3, generator=gen, dtype=torch.float64)
    out = M.weight_standardize(w, 1e-5)
    torch.testing.assert_close(out, formula64(w.detach(), 1e-5), rtol=1e-12, atol=1e-12)
    out.backward(g)
    w2 = w.detach().clone().requires_grad_()
    formula64(w2, 1e-5).backward(g)
    torch.testing.assert_close(w.grad, w2.grad, rtol=1e-10, atol=1e-12)
    K = 36
    flat, gf = w.detach().reshape(6, K), g.reshape(6, K)
    c = flat - flat.mean(1, keepdim=True)
    std = flat.std(1, keepdim=True)
    d = 1 / (std + 1e-5)
    h = gf * d - c * (gf * c).sum(1, keepdim=True) * d * d / ((K - 1) * std)
    torch.testing.assert_close((h - h.mean(1, keepdim=True)).view_as(w), w.grad, rtol=1e-10, atol=1e-12)
    assert torch.autograd.gradcheck(lambda t: M.weight_standardize(t, 1e-5), (w.detach().clone().requires_grad_(), ))


def test_registry_knows_conv_ws_and_the_four_conv_head():
    import htd_amd.detector  # noqa: F401
    from htd_amd.detector.bbox_heads import ConvFCBBoxHead, Shared4Conv1FCBBoxHead
    from htd_amd.detector.bricks import ConvWS2d
    from htd_amd.registry import CONV_LAYERS, HEADS
    assert CONV_LAYERS.get('ConvWS') is ConvWS2d and HEADS.get('Shared4Conv1FCBBoxHead') is Shared4Conv1FCBBoxHead
    head = Shared4Conv1FCBBoxHead(conv_out_channels=256, conv_cfg=dict(type='ConvWS'), norm_cfg=dict(type='GN', num_groups=32),
                                  num_classes=80)
    assert isinstance(head, ConvFCBBoxHead) and len(head.shared_convs) == 4 and len(head.shared_fcs) == 1
    assert all(type(m.conv) is ConvWS2d and isinstance(m.gn, torch.nn.GroupNorm) and m.conv.bias is None for m in head.shared_convs)
    assert head.shared_fcs[0].out_features == 1024 and head.fc_reg.out_features == 320


def test_conv_ws_under_a_batch_norm_is_refused():
    from htd_amd.detector.bricks import ConvWS2d
    from htd_amd.detector.resnet import conv_bn
    conv, bn = ConvWS2d(8, 8, 1, bias=False), torch.nn.BatchNorm2d(8).eval()
    with pytest.raises(NotImplementedError, match='ConvWS'):
        conv_bn(conv, bn, torch.zeros(1, 8, 4, 4))


def test_hand_written_config_equals_the_reference_config():
    from htd_amd.configs import faster_rcnn_gn_ws_config
    ref = reference_cfg()
    mine = json.loads(json.dumps(faster_rcnn_gn_ws_config().to_dict()))
    assert set(ref) <= set(mine)
    for k, v in ref.items():
        assert mine[k] == v, k
    assert ref['model']['backbone']['conv_cfg'] == {'type': 'ConvWS'} and ref['model']['neck']['norm_cfg']['type'] == 'GN'
    assert ref['model']['roi_head']['bbox_head']['type'] == 'Shared4Conv1FCBBoxHead'


def test_reference_config_builds_with_the_reference_state_dict(golden):
    """The JSON of the reference's merged config goes through the registry: ConvWS + GN in the ResNet (gn1, layer2.0.downsample.1),
    the FPN and the Shared4Conv1FCBBoxHead; the state dict has the reference's keys, in its order, with its shapes, and no
    BatchNorm statistics."""
    import htd_amd.detector  # noqa: F401
    from htd_amd.configs import build_baseline_detector
    from htd_amd.detector.bricks import ConvWS2d
    from htd_amd.registry import ConfigDict
    g = golden('gn_ws')
    det = build_baseline_detector(cfg=ConfigDict(reference_cfg()))
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_keys']]
    for (k, v), shape in zip(sd.items(), g['state_shapes']):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]] and not shape[v.dim():].any(), k
    for k in ('backbone.gn1.weight', 'backbone.layer2.0.downsample.1.weight', 'backbone.layer4.2.gn3.bias',
              'neck.lateral_convs.0.gn.weight', 'neck.fpn_convs.3.gn.bias', 'roi_head.bbox_head.shared_convs.3.gn.weight',
              'roi_head.bbox_head.shared_fcs.0.weight'):
        assert k in sd, k
    assert not any('running_' in k or '.bn' in k for k in sd)
    assert sd['roi_head.bbox_head.shared_fcs.0.weight'].shape == (1024, 256 * 49)
    assert isinstance(det.backbone.gn1, torch.nn.GroupNorm) and det.backbone.gn1.num_groups == 32
    assert type(det.backbone.conv1) is ConvWS2d and type(det.neck.fpn_convs[0].conv) is ConvWS2d
    assert all(k in sd for k in U.GRAD_KEYS)
    same = build_baseline_detector('faster_rcnn_gn_ws')
    assert list(same.state_dict().keys()) == list(sd.keys())
    # the stem and layer1 are frozen (frozen_stages = 1), GroupNorm included
    assert not det.backbone.gn1.weight.requires_grad and not det.backbone.layer1[0].gn3.bias.requires_grad
    assert det.backbone.layer2[0].gn1.weight.requires_grad


def test_train_entry_accepts_the_config_file(tmp_path):
    """python -m htd_amd.train on the GN+WS config with pretrained=None, up to the model: the file (the reference's merged
    settings, one `key = value` line each, plus the data section) goes through the entry's own parse_args / load_config --
    runtime defaults, the check for unsupported settings -- and the detector is built from it as main() builds it."""
    import htd_amd.detector  # noqa: F401
    from htd_amd import train
    from htd_amd.configs import faster_rcnn_gn_ws_config
    from htd_amd.registry import build_detector
    settings = reference_cfg()
    settings['model']['pretrained'] = None
    settings['data'] = faster_rcnn_gn_ws_config().data.to_dict()
    path = tmp_path / 'faster_rcnn_r50_fpn_gn_ws-all_1x_coco.py'
    path.write_text(''.join(f'{k} = {v!r}\n' for k, v in settings.items()))
    args = train.parse_args([str(path), '--work-dir', str(tmp_path / 'work')])
    cfg = train.load_config(args)
    assert cfg.model.backbone.conv_cfg.type == 'ConvWS' and cfg.work_dir == str(tmp_path / 'work')
    det = build_detector(cfg.model.to_dict(), train_cfg=cfg.get('train_cfg'), test_cfg=cfg.get('test_cfg'))
    assert type(det).__name__ == 'FasterRCNN' and type(det.roi_head.bbox_head).__name__ == 'Shared4Conv1FCBBoxHead'
    assert type(det.backbone.layer3[0].conv2).__name__ == 'ConvWS2d' and cfg.total_epochs == 12


def test_fixture_records_its_margins(golden):
    """What tests/golden/make_golden_gn_ws.py asserts while writing the fixture, read back: see that script's docstring."""
    g = golden('gn_ws')
    for k in ('assign', 'score', 'nms_rpn', 'nms_rcnn', 'topk'):
        assert f'margin.{k}' in g.files
    assert float(g['margin.assign']) >= 1e-3 and float(g['margin.score']) >= 1e-3
    assert float(g['margin.nms_rpn']) >= 1e-3 and float(g['margin.nms_rcnn']) >= 1e-3 and float(g['margin.topk']) >= 1e-3
    # the reference's fp32 and fp64 runs take the same discrete decisions: same proposals, sampled RoIs and detections
    for k in ('train_s0_rois', 'test_props0', 'test_props1', 'test_dets0', 'test_dets1'):
        assert float(g['err32.' + k]) <= 2e-3, k


def test_new_abi_symbols_are_declared_and_exported():
    from htd_amd import capi
    names = {n for n, _, _ in capi.declared_functions()}
    want = {'htd_group_norm_map_slab', 'htd_group_norm_map_workspace_bytes', 'htd_group_norm_map_fwd', 'htd_group_norm_map_bwd',
            'htd_weight_standardize_fwd', 'htd_weight_standardize_bwd'}
    assert want <= names
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in want)
    assert lib.htd_abi_version() == 8
    assert lib.htd_group_norm_map_slab(200 * 336, 256) > 0
    assert lib.htd_group_norm_map_workspace_bytes(4, 200 * 336, 256, 32) >= 4 * 32 * 16
    assert lib.htd_group_norm_map_slab(100, 2050) != 0 and b'group_norm_map_slab' in lib.htd_last_error()
