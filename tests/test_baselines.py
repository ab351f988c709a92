"""Faster R-CNN and Cascade R-CNN baselines, host side: configs, registry, L1Loss, the class-specific tensor formulation of
BBoxHead.loss, the static-path gates and the CLI, against what the reference's own code gave (tests/golden/baselines.npz, recipe in
tests/golden/make_golden_baselines.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import baselines_util as U
from iou_loss_util import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_JSON = dict(faster_rcnn='faster_rcnn_r50_fpn_1x_coco_cfg.json', cascade_rcnn='cascade_rcnn_r50_fpn_1x_coco_cfg.json')


def reference_cfg(name):
    with open(os.path.join(ROOT, 'tests', 'golden', CFG_JSON[name])) as f:
        return json.load(f)


def hand_cfg(name):
    from htd_amd import configs
    return dict(faster_rcnn=configs.faster_rcnn_config, cascade_rcnn=configs.cascade_rcnn_config)[name]()


@pytest.mark.parametrize('name', U.MODELS)
def test_hand_written_config_equals_the_reference_config(name):
    ref = reference_cfg(name)
    mine = json.loads(json.dumps(hand_cfg(name).to_dict()))
    assert set(ref) <= set(mine)
    for k, v in ref.items():
        assert mine[k] == v, k
    assert mine['data']['train']['type'] == 'CocoDataset'


@pytest.mark.parametrize('name', U.MODELS)
def test_reference_config_builds_with_the_reference_state_dict(golden, name):
    """The JSON of the reference's merged config goes through the registry; the state dict has the reference's keys, in its order,
    with its shapes -- no stage index in StandardRoIHead, one per stage in CascadeRoIHead."""
    import htd_amd.detector  # noqa: F401
    from htd_amd.registry import Config, build_detector
    g = golden('baselines')
    cfg = Config(reference_cfg(name))
    model = cfg.model.to_dict()
    model['pretrained'] = None
    det = build_detector(model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert type(det).__name__ == dict(faster_rcnn='FasterRCNN', cascade_rcnn='CascadeRCNN')[name]
    assert type(det.roi_head).__name__ == dict(faster_rcnn='StandardRoIHead', cascade_rcnn='CascadeRoIHead')[name]
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f'{name}.state_keys']]
    for (k, v), shape in zip(sd.items(), g[f'{name}.state_shapes']):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]] and not shape[v.dim():].any(), k
    keys = [k for k in sd if k.startswith('roi_head.')]
    if name == 'faster_rcnn':
        assert all(k.startswith('roi_head.bbox_head.') and not k.split('.')[2].isdigit() for k in keys)
        assert sd['roi_head.bbox_head.fc_reg.weight'].shape == (320, 1024)
    else:
        assert {k.split('.')[2] for k in keys} == {'0', '1', '2'}
        assert sd['roi_head.bbox_head.2.fc_reg.weight'].shape == (4, 1024)
    # a state dict of the reference's keys and logical shapes loads strictly (the .pth file itself: tests/test_gpu_baselines.py)
    from htd_amd.checkpoint import load_state_dict
    load_state_dict(det, {str(k): torch.zeros([int(v) for v in shape if v]) for k, shape in
                          zip(g[f'{name}.state_keys'], g[f'{name}.state_shapes'])}, strict=True)


def test_builder_and_unsupported_keys():
    from htd_amd.configs import build_baseline_detector, cascade_rcnn_config, faster_rcnn_config
    det = build_baseline_detector('cascade_rcnn')
    assert type(det).__name__ == 'CascadeRCNN' and len(det.roi_head.bbox_head) == 3
    with pytest.raises(ValueError, match='kind'):
        build_baseline_detector('retinanet')
    for make, key, value in ((faster_rcnn_config, 'mask_head', dict(type='FCNMaskHead')),
                             (cascade_rcnn_config, 'mask_roi_extractor', dict(type='SingleRoIExtractor')),
                             (faster_rcnn_config, 'shared_head', dict(type='ResLayer'))):
        cfg = make()
        cfg.model.roi_head[key] = value
        with pytest.raises(NotImplementedError, match=key):
            build_baseline_detector(cfg=cfg)
    for kind in U.MODELS:
        with pytest.raises(NotImplementedError, match='aug_test'):
            build_baseline_detector(kind).roi_head.aug_test([], [], [])


def test_htd_roi_head_is_a_cascade_head_with_the_same_parameter_layout():
    """HTDRoIHead builds on CascadeRoIHead; its sub-modules register in the order that lays out the Trainer's flat buffer and the
    optimizer state of existing checkpoints (extractors, heads, then the global-context head), and the keys the HTD configs do
    not support raise like the baselines' do."""
    from htd_amd.configs import build_htd_detector, htd_config
    from htd_amd.detector.roi_heads import CascadeRoIHead
    det = build_htd_detector(cfg=htd_config(50))
    rh = det.roi_head
    assert isinstance(rh, CascadeRoIHead) and rh.with_bbox and not rh.with_mask and not rh.with_shared_head
    assert [n for n, _ in rh.named_children()] == ['bbox_roi_extractor', 'bbox_head', 'glbctx_head']
    keys = [k for k in det.state_dict() if k.startswith('roi_head.')]
    assert list(det.state_dict())[-len(keys):] == keys and len(keys) == 52
    assert keys[:2] == ['roi_head.bbox_roi_extractor.1.conv1.weight', 'roi_head.bbox_roi_extractor.1.conv1.bias']
    assert list(dict.fromkeys(k.split('.')[1] for k in keys)) == ['bbox_roi_extractor', 'bbox_head', 'glbctx_head']
    assert keys[-1] == 'roi_head.glbctx_head.fc.bias'
    assert keys[-4:-1] == ['roi_head.glbctx_head.convs.3.conv.weight', 'roi_head.glbctx_head.convs.3.conv.bias',
                           'roi_head.glbctx_head.fc.weight']
    assert rh.can_train_static() is True
    for key, value in (('mask_head', dict(type='FCNMaskHead')), ('mask_roi_extractor', dict(type='SingleRoIExtractor')),
                       ('shared_head', dict(type='ResLayer'))):
        cfg = htd_config(50)
        cfg.model.roi_head[key] = value
        with pytest.raises(NotImplementedError, match=key):
            build_htd_detector(cfg=cfg)


def test_l1_loss_matches_the_reference_fp64(golden):
    from htd_amd.detector.losses import L1Loss
    g = golden('baselines')
    pred, target, weight = (t.double() for t in U.l1_rows())
    pred.requires_grad_()
    mod = L1Loss(loss_weight=1.0)
    avg = float(g['l1.avg_factor'])
    red = torch.stack([mod(pred, target, weight), mod(pred, target, weight, avg_factor=avg),
                       mod(pred, target, weight, reduction_override='sum'), mod(pred, target),
                       mod(pred, target, reduction_override='sum')])
    close(red, g['l1.red64'])
    close(mod(pred, target, weight, reduction_override='none'), g['l1.none64'])
    mod(pred, target, weight, avg_factor=avg).backward()
    close(pred.grad, g['l1.gpred64'])
    assert float(pred.grad[::5].abs().max()) == 0.0                    # pred == target: zero loss, zero gradient
    assert float(L1Loss(loss_weight=2.5)(pred, target).detach()) == pytest.approx(2.5 * float(g['l1.red64'][3]), rel=1e-12)
    with pytest.raises(ValueError):
        mod(pred, target, weight, avg_factor=avg, reduction_override='sum')
    # the fp32 module is as close to fp64 as the reference's own fp32 run (4 x its error, one ulp as the floor)
    p32, t32, w32 = U.l1_rows()
    red32 = torch.stack([mod(p32, t32, w32), mod(p32, t32, w32, avg_factor=avg), mod(p32, t32, w32, reduction_override='sum'),
                         mod(p32, t32), mod(p32, t32, reduction_override='sum')]).double().numpy()
    err32 = np.abs(g['l1.red32'].astype(np.float64) - g['l1.red64'])
    assert (np.abs(red32 - g['l1.red64']) <= 4 * np.maximum(err32, 2.0 ** -23 * np.abs(g['l1.red64']))).all()


@pytest.mark.parametrize('variant', ['mixed', 'allbg'])
@pytest.mark.parametrize('agnostic', [False, True], ids=['spec', 'agn'])
@pytest.mark.parametrize('loss', list(U.HEAD_LOSSES))
def test_bbox_head_loss_tensor_formulation_matches_the_reference_fp64(golden, loss, agnostic, variant):
    """BBoxHead.loss with one box per class (gather by label instead of the reference's boolean indexing) and with L1Loss, in fp64
    on the rows of head_case(48, 81): a row of the last class, unused slots, pred == target rows, and the all-background batch."""
    g = golden('baselines')
    cls, full, labels, lw, tgt, bw = U.head_case(48, 81, variant)
    p = f'head.{loss}.{"agn" if agnostic else "spec"}.' + ('' if variant == 'mixed' else 'allbg.')
    head = U.make_head(loss, 80, agnostic)
    pred = U.own_columns(full, labels, 80) if agnostic else full
    out = U.head_loss_fp64(head, cls, pred, labels, lw, tgt, bw)
    close(torch.stack([out['loss_cls'], out['loss_bbox'], out['acc'].reshape(())]), g[p + 'scalars64'])
    gown = out['grad_box'] if agnostic else U.own_columns(out['grad_box'], labels, 80)
    close(gown, g[p + 'gown64'])
    close(out['grad_box'].abs().sum(), g[p + 'gabs64'])               # nothing outside the rows' own columns
    sums, sample = U.digest(out['grad_cls'], 64)
    close(sums, g[p + 'gcls_sums'])
    close(sample, g[p + 'gcls_sample'])
    # the static path's form (num_samples = all slots) gives the same two losses
    ns = U.head_loss_fp64(head, cls, pred, labels, lw, tgt, bw, num_samples=48)
    close(torch.stack([ns['loss_cls'], ns['loss_bbox']]), g[p + 'scalars64'][:2])
    if variant == 'allbg':
        assert float(out['loss_bbox']) == 0.0 and float(out['grad_box'].abs().max()) == 0.0


def test_cascade_head_builds_per_stage_assigners_and_samplers():
    from htd_amd.configs import build_baseline_detector
    rh = build_baseline_detector('cascade_rcnn').roi_head
    assert rh.num_stages == 3 and rh.stage_loss_weights == [1, 0.5, 0.25]
    assert isinstance(rh.bbox_head, torch.nn.ModuleList) and isinstance(rh.bbox_roi_extractor, torch.nn.ModuleList)
    assert [a.pos_iou_thr for a in rh.bbox_assigner] == [0.5, 0.6, 0.7]
    assert [type(s).__name__ for s in rh.bbox_sampler] == ['RandomSampler'] * 3 and all(s.num == 512 for s in rh.bbox_sampler)
    assert [list(h.bbox_coder.stds) for h in rh.bbox_head] == [[0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1],
                                                                [0.033, 0.033, 0.067, 0.067]]
    srh = build_baseline_detector('faster_rcnn').roi_head
    assert srh.bbox_assigner.pos_iou_thr == 0.5 and srh.bbox_sampler.num == 512 and not srh.bbox_head.reg_class_agnostic


def test_static_path_gates():
    from htd_amd.configs import build_baseline_detector, cascade_rcnn_config, faster_rcnn_config
    from htd_amd.detector.losses import L1Loss
    frcnn = build_baseline_detector('faster_rcnn')
    assert frcnn.roi_head.can_train_static() is True and frcnn.roi_head.can_train_static([None, None]) is True
    assert frcnn.roi_head.can_train_static([torch.zeros(1, 4), None]) is False          # ignore regions: per-image path
    assert type(frcnn.rpn_head.loss_bbox) is L1Loss and frcnn.rpn_head._fused_loss_ok()
    assert frcnn.roi_head.bbox_head.fused_loss_config_ok()
    assert build_baseline_detector('cascade_rcnn').roi_head.can_train_static() is True
    cfg = cascade_rcnn_config()
    cfg.model.roi_head.bbox_head[0].reg_class_agnostic = False                          # stage 0 hands on class-specific boxes
    rh = build_baseline_detector(cfg=cfg).roi_head
    assert rh.can_train_static() is False and rh.bbox_head[0].fused_loss_config_ok()
    cfg = cascade_rcnn_config()
    cfg.model.roi_head.bbox_head[2].reg_class_agnostic = False                          # the last stage may be class-specific
    assert build_baseline_detector(cfg=cfg).roi_head.can_train_static() is True
    cfg = faster_rcnn_config()
    cfg.train_cfg.rcnn.sampler.type = 'OHEMSampler'
    try:
        rh = build_baseline_detector(cfg=cfg).roi_head
    except KeyError:
        rh = None                                                                       # not in the registry at all
    assert rh is None or rh.can_train_static() is False
    cfg = faster_rcnn_config()
    cfg.model.roi_head.bbox_head.loss_bbox = dict(type='SmoothL1Loss', beta=1.0, reduction='sum')
    head = build_baseline_detector(cfg=cfg).roi_head.bbox_head
    assert head.fused_loss_config_ok() is False                                         # tensor formulation


def test_refine_rows_equals_the_reference_form():
    """Between cascade stages: the one-pass refinement (decode every row with its image's limits, drop the leading gt-born rows)
    equals BBoxHead.refine_bboxes with background rows taking their arg-max foreground class."""
    from htd_amd.detector.roi_heads import _refine_rows
    head = U.make_head('smooth_l1', 80, True)
    gen = torch.Generator().manual_seed(4)
    metas = [dict(img_shape=(100, 140, 3)), dict(img_shape=(90, 120, 3))]
    res, rois, pos_is_gts = [], [], []
    for b, (n_gt, npos, nneg) in enumerate(((2, 5, 6), (0, 3, 4))):
        xy = torch.rand(npos + nneg, 2, generator=gen) * 90
        boxes = torch.cat([xy, xy + 5 + torch.rand(npos + nneg, 2, generator=gen) * 60], 1)
        flags = torch.zeros(npos, dtype=torch.uint8)
        flags[:n_gt] = 1
        res.append(types.SimpleNamespace(pos_bboxes=boxes[:npos], neg_bboxes=boxes[npos:], pos_is_gt=flags))
        rois.append(torch.cat([torch.full((npos + nneg, 1), float(b)), boxes], 1))
        pos_is_gts.append(flags)
    rois = torch.cat(rois)
    pred = torch.randn(rois.size(0), 4, generator=gen)
    labels = torch.randint(0, 80, (rois.size(0), ), generator=gen)
    want = head.refine_bboxes(rois, labels, pred, pos_is_gts, metas)
    got = _refine_rows(head, rois, pred, res, metas)
    assert len(got) == 2 and [len(x) for x in got] == [9, 7]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert _refine_rows(U.make_head('l1', 80, False), rois, pred.repeat(1, 80), res, metas) is None


@pytest.mark.parametrize('name', U.MODELS)
def test_train_cli_accepts_the_config(name, tmp_path):
    """python -m htd_amd.train on a config file of either baseline, as far as the merged and checked config."""
    from htd_amd.train import load_config, parse_args
    path = tmp_path / f'{name}.py'
    with open(path, 'w') as f:
        for k, v in hand_cfg(name).to_dict().items():
            f.write(f'{k} = {v!r}\n')
    args = parse_args([str(path), '--work-dir', str(tmp_path / 'work'), '--cfg-options', 'optimizer.lr=0.01'])
    cfg = load_config(args)
    assert cfg.model.roi_head.type == dict(faster_rcnn='StandardRoIHead', cascade_rcnn='CascadeRoIHead')[name]
    assert cfg.optimizer.lr == 0.01 and cfg.work_dir == str(tmp_path / 'work')
    assert json.loads(json.dumps(cfg.model.to_dict())) == reference_cfg(name)['model']
