"""IoU-family regression losses on decoded boxes (IoULoss, BoundedIoULoss, GIoULoss, DIoULoss, CIoULoss), bbox_overlaps(mode='giou')
and BBoxHead.loss with reg_decoded_bbox, in fp64 on the CPU against tests/golden/iou_loss.npz -- the reference's own iou_loss.py,
iou2d_calculator.py, delta_xywh_bbox_coder.py and BBoxHead.loss (tests/golden/make_golden_iou_loss.py) -- to 1e-12 relative."""
import types

import numpy as np
import pytest
import torch

from iou_loss_util import KINDS, NUM_CLASSES, STDS, build_loss, close, cls_scores, digest, head_loss_fp64, make_head, rows

AVG = 300.0


def w4_of(w):
    return w[:, None] * torch.tensor([1., 0.5, 0.25, 1.25], dtype=w.dtype)


def decoded(rois, deltas, dt=torch.float64):
    from htd_amd.core.bbox import delta2bbox
    return delta2bbox(rois.to(dt), deltas.to(dt), (0., 0., 0., 0.), STDS)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tag', ['main', 'tie'])
def test_loss_modules_match_the_reference_in_fp64(golden, tag, kind):
    """Per-row loss, every recorded reduction with (n,) and (n, 4) weights and an avg_factor, and the gradient with respect to the
    boxes -- on the tie set entry by entry, which pins what autograd does at max / min ties, clamp bounds and zero areas."""
    g = golden('iou_loss')
    rois, deltas, gts, weight, _ = rows(g, tag)
    n = rois.size(0)
    p = f'{tag}.{kind}.'
    mod = build_loss(dict(type=kind, loss_weight=1.0))
    pred = decoded(rois, deltas).requires_grad_()
    tgt, w = gts.double(), weight.double()
    w4 = w4_of(w)
    if kind == 'BoundedIoULoss':                    # an (n, 4) loss: the plain weight on every component
        w = w[:, None].expand(n, 4)
    close(mod(pred, tgt, reduction_override='none'), g[p + 'row64'])
    red = torch.stack([mod(pred, tgt, w), mod(pred, tgt, w4), mod(pred, tgt, w, avg_factor=AVG), mod(pred, tgt, w4, avg_factor=AVG),
                       mod(pred, tgt, w, reduction_override='sum'), mod(pred, tgt, w4, reduction_override='sum'), mod(pred, tgt)])
    close(red, g[p + 'red64'])
    for key, ww in (('none_w1', w), ('none_w4', w4)):
        sums, sample = digest(mod(pred, tgt, ww, reduction_override='none'))
        close(sums, g[p + key + '_sums'])
        close(sample, g[p + key + '_sample'])
    mod(pred, tgt, w4, avg_factor=AVG).backward()
    assert torch.isfinite(pred.grad).all()
    if tag == 'tie':
        close(pred.grad, g[p + 'gpred64'])
    else:
        sums, sample = digest(pred.grad)
        close(sums, g[p + 'gpred_sums'])
        close(sample, g[p + 'gpred_sample'])
    with pytest.raises(ValueError):
        mod(pred, tgt, w, avg_factor=AVG, reduction_override='sum')


def test_loss_module_defaults_are_the_reference_ones():
    from htd_amd.detector import losses as L
    from htd_amd.registry import LOSSES
    for kind in KINDS:
        m = build_loss(dict(type=kind))
        assert type(m) is LOSSES.get(kind) and m.reduction == 'mean' and m.loss_weight == 1.0
        assert m.eps == (1e-3 if kind == 'BoundedIoULoss' else 1e-6)
    assert build_loss(dict(type='BoundedIoULoss')).beta == 0.2
    assert [c.__name__ for c in L.DECODED_BOX_LOSSES] == list(KINDS) and [c.kind for c in L.DECODED_BOX_LOSSES] == [0, 1, 2, 3, 4]


def test_giou_overlaps_match_the_reference(golden):
    from htd_amd.core.bbox import bbox_overlaps
    g = golden('iou_loss')
    for tag in ('main', 'tie'):
        rois, deltas, gts, _, _ = rows(g, tag)
        for dt, sfx, rel in ((torch.float64, '64', 1e-12), (torch.float32, '32', 1e-6)):
            p = decoded(rois, deltas, dt)
            close(bbox_overlaps(p, gts.to(dt), mode='giou', is_aligned=True), g[f'{tag}.giou_aligned{sfx}'], rel)
            close(bbox_overlaps(p[:24], gts[:16].to(dt), mode='giou'), g[f'{tag}.giou_matrix{sfx}'], rel)
    b1, b2 = torch.from_numpy(g['doc_b1']), torch.from_numpy(g['doc_b2'])
    assert np.array_equal(bbox_overlaps(b1, b2, mode='giou').numpy(), g['doc_giou'])
    assert np.array_equal(bbox_overlaps(b1, b2, mode='giou', is_aligned=True).numpy(), g['doc_giou_aligned'])
    close(bbox_overlaps(b1.double(), b2.double(), mode='giou'), g['doc_giou64'])
    assert tuple(bbox_overlaps(b1[:0], b2, mode='giou').shape) == (0, 3)
    with pytest.raises(AssertionError):
        bbox_overlaps(b1, b2, mode='diou')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tag', ['main', 'tie'])
def test_bbox_head_loss_on_decoded_boxes_matches_the_reference(golden, tag, kind):
    """BBoxHead.loss with reg_decoded_bbox=True on the CPU (tensor formulation) against the reference's BBoxHead.loss: a
    class-agnostic head over all rows and a class-specific head over the first rows, losses, accuracy and both gradients."""
    g = golden('iou_loss')
    rois, deltas, gts, weight, labels = rows(g, tag)
    n = rois.size(0)
    p = f'{tag}.{kind}.'
    for spec in (False, True):
        m = min(n, int(g['spec_rows'])) if spec else n
        k = 'spec' if spec else 'head'
        head = make_head(kind, agnostic=not spec, loss_weight=float(g['loss_weight']))
        d = deltas[:m].double()
        if spec:
            from golden_util import seeded_tensor
            full = seeded_tensor(f'iou_loss.{tag}.spec', (m, NUM_CLASSES, 4), scale=0.5).double()
            col = labels[:m].clamp(max=NUM_CLASSES - 1)
            full[torch.arange(m), col] = d
            d = full.view(m, -1)
        bw = weight[:m, None].expand(m, 4).contiguous()
        out = head_loss_fp64(head, cls_scores(tag, n)[:m], d, rois[:m], labels[:m], torch.ones(m), gts[:m], bw)
        close(torch.stack([out['loss_cls'], out['loss_bbox'], out['acc'].reshape(())]), g[p + k + '_scalars64'])
        gd = out['grad_box']
        if spec:
            gfull = gd.view(m, NUM_CLASSES, 4)
            gd = gfull[torch.arange(m), col]
            close(gfull.abs().sum(), g[p + 'spec_gabs64'])             # nothing outside the label's four columns
        close(gd, g[p + k + '_gdeltas64'])
        sums, sample = digest(out['grad_cls'])
        close(sums, g[p + k + '_gcls_sums'])
        close(sample, g[p + k + '_gcls_sample'])


class _HostRead(AssertionError):
    pass


def _no_host_reads(monkeypatch):
    def boom(*a, **k):
        raise _HostRead('the loss path read a tensor on the host')
    for name in ('item', 'tolist', '__bool__', 'any', 'all', 'nonzero', '__float__', '__int__'):
        monkeypatch.setattr(torch.Tensor, name, boom)
    monkeypatch.setattr(torch, 'any', boom)
    monkeypatch.setattr(torch, 'all', boom)


@pytest.mark.parametrize('kind', KINDS)
def test_all_zero_weights_give_exact_zero_without_a_host_read(golden, kind, monkeypatch):
    """The reference leaves early through `torch.any(weight > 0)` (a device-to-host read); here the weighted sum gives the same
    exact 0 and exactly zero, finite gradients, with no .item() / .any() / bool() on the way -- module and BBoxHead.loss alike."""
    g = golden('iou_loss')
    rois, deltas, gts, _, labels = rows(g, 'tie')
    rois, deltas, gts, labels = (torch.cat([a, b]) for a, b in zip(rows(g, 'main')[:3] + [rows(g, 'main')[4]], (rois, deltas, gts, labels)))
    n = rois.size(0)
    # unused slots of the static path as well: zero roi, zero target
    rois[:5], gts[:5], deltas[:5] = 0., 0., 0.
    mod = build_loss(dict(type=kind, loss_weight=10.0))
    head = make_head(kind)
    cls = cls_scores('zero', n).requires_grad_()
    d = deltas.clone().requires_grad_()
    pred = decoded(rois, deltas, torch.float32).requires_grad_()
    ns = torch.tensor(n - 5)
    _no_host_reads(monkeypatch)
    try:
        outs = [mod(pred, gts, torch.zeros(n, 4)), mod(pred, gts, torch.zeros(n, 4), avg_factor=7.0)]
        if kind != 'BoundedIoULoss':
            outs.append(mod(pred, gts, torch.zeros(n)))
        rois5 = torch.cat([torch.zeros(n, 1), rois], 1)
        losses = head.loss(cls, d, rois5, labels, torch.ones(n), gts, torch.zeros(n, 4), num_samples=ns)
        total = sum(outs) + losses['loss_bbox']
        total.backward()
    finally:
        monkeypatch.undo()
    for o in outs + [losses['loss_bbox']]:
        assert float(o.detach()) == 0.0
    for t in (pred.grad, d.grad):
        assert torch.isfinite(t).all() and float(t.abs().max()) == 0.0
    with pytest.raises(_HostRead):          # the guard does catch the reference's early return
        _no_host_reads(monkeypatch)
        try:
            torch.any(torch.zeros(3) > 0)
        finally:
            monkeypatch.undo()


def _giou_cfg(loss0=None, loss1=None):
    from htd_amd.configs import htd_config
    cfg = htd_config(50)
    for h, loss in zip(cfg.model.roi_head.bbox_head, (loss0, loss1)):
        if loss is not None:
            h.update(reg_decoded_bbox=True, loss_bbox=dict(type=loss, loss_weight=10.0))
    return cfg


def test_detector_with_giou_heads_builds_and_trains_static():
    """The reference zoo's `reg_decoded_bbox=True, loss_bbox=dict(type='GIoULoss', loss_weight=10.0)` on both HTD stages builds,
    and stays on the static-shape training path; each head decides for itself; what the fused kernel does not take leaves it."""
    from htd_amd.configs import build_htd_detector
    from htd_amd.detector.losses import CIoULoss, GIoULoss, SmoothL1Loss
    det = build_htd_detector(cfg=_giou_cfg('GIoULoss', 'GIoULoss'))
    rh = det.roi_head
    assert all(type(h.loss_bbox) is GIoULoss and h.reg_decoded_bbox and h.loss_bbox.loss_weight == 10.0 for h in rh.bbox_head)
    assert rh.can_train_static() is True
    rh2 = build_htd_detector(cfg=_giou_cfg(None, 'CIoULoss')).roi_head
    assert type(rh2.bbox_head[0].loss_bbox) is SmoothL1Loss and type(rh2.bbox_head[1].loss_bbox) is CIoULoss
    assert not rh2.bbox_head[0].reg_decoded_bbox and rh2.bbox_head[1].reg_decoded_bbox and rh2.can_train_static() is True
    # decoded boxes under a loss outside the IoU family, or a 'sum' reduction: the tensor formulation, per-image path
    cfg = _giou_cfg('GIoULoss', 'GIoULoss')
    cfg.model.roi_head.bbox_head[1].loss_bbox = dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)
    assert build_htd_detector(cfg=cfg).roi_head.can_train_static() is False
    cfg = _giou_cfg('GIoULoss', 'GIoULoss')
    cfg.model.roi_head.bbox_head[0].loss_bbox = dict(type='GIoULoss', reduction='sum')
    assert build_htd_detector(cfg=cfg).roi_head.can_train_static() is False
    # the RPN keeps its assertion
    cfg = _giou_cfg()
    cfg.model.rpn_head.update(reg_decoded_bbox=True)
    with pytest.raises(AssertionError):
        build_htd_detector(cfg=cfg)


def test_batched_targets_of_a_decoded_head_are_the_gt_boxes():
    """roi_heads.batched_targets for a head with reg_decoded_bbox: positives carry their gt box, everything else zeros with weight 0 --
    what BBoxHead.get_targets gives image by image."""
    from htd_amd.configs import build_htd_detector
    from htd_amd.detector.roi_heads import batched_targets
    rh = build_htd_detector(cfg=_giou_cfg('GIoULoss', None)).roi_head
    gen = torch.Generator().manual_seed(0)

    def boxes(n):
        xy = torch.rand(n, 2, generator=gen) * 100
        return torch.cat([xy, xy + 1 + torch.rand(n, 2, generator=gen) * 50], 1)
    res = [types.SimpleNamespace(pos_bboxes=boxes(a), neg_bboxes=boxes(b), pos_gt_bboxes=boxes(a),
                                 pos_gt_labels=torch.randint(0, 80, (a, ), generator=gen)) for a, b in ((3, 5), (0, 4), (2, 0))]
    for stage in (0, 1):
        got = batched_targets(rh.bbox_head[stage], res, rh.train_cfg[stage])
        want = rh.bbox_head[stage].get_targets(res, None, None, rh.train_cfg[stage])
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(got[2][:3], rh.bbox_head[1].bbox_coder.encode(res[0].pos_bboxes, res[0].pos_gt_bboxes))
    assert torch.equal(batched_targets(rh.bbox_head[0], res, rh.train_cfg[0])[2][:3], res[0].pos_gt_bboxes)


def test_cfg_options_reach_the_bbox_heads():
    """The INTEGRATION.md recipe: `--cfg-options` keys with a list index select one RoI stage, `_delete_` replaces the smooth-L1
    loss dict (its `beta` is no argument of GIoULoss); untouched entries of the list stay as they are."""
    from htd_amd.configs import build_htd_detector, htd_config
    from htd_amd.registry import Config
    from htd_amd.train import parse_args
    args = parse_args(['cfg.py', '--cfg-options', 'model.roi_head.bbox_head.1.reg_decoded_bbox=True',
                       "model.roi_head.bbox_head.1.loss_bbox={'_delete_': True, 'type': 'GIoULoss', 'loss_weight': 10.0}"])
    base = htd_config(50)
    cfg = Config(dict(model=base.model.to_dict(), train_cfg=base.train_cfg.to_dict(), test_cfg=base.test_cfg.to_dict()))
    before = cfg.model.to_dict()
    cfg.merge_from_dict(args.cfg_options)
    heads = cfg.model.roi_head.bbox_head
    assert isinstance(heads, list) and len(heads) == 2 and heads[0].to_dict() == before['roi_head']['bbox_head'][0]
    assert heads[1].reg_decoded_bbox is True and heads[1].loss_bbox.to_dict() == dict(type='GIoULoss', loss_weight=10.0)
    assert heads[1].type == 'HTDBBoxHead' and cfg.model.backbone.to_dict() == before['backbone']
    rh = build_htd_detector(cfg=cfg).roi_head
    assert type(rh.bbox_head[1].loss_bbox).__name__ == 'GIoULoss' and rh.can_train_static()
    with pytest.raises(KeyError):
        cfg.merge_from_dict({'model.roi_head.bbox_head.2.reg_decoded_bbox': True})
