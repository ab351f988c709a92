"""htd_roi_head_loss_decoded on a real MI355X: decode + IoU-family loss + gradient with respect to the deltas, fused with the
cross-entropy of BBoxHead.loss, against the reference's own fp64 results (tests/golden/iou_loss.npz), the fp64 tensor formulation
on the CPU (pinned by tests/test_iou_losses.py), htd_roi_head_loss for the classification half, and a small detector with
IoU-family losses on its two stages.

The ratios measured on the MI355X are in DESIGN.md section 8 f9."""
import numpy as np
import pytest
import torch

from golden_util import load_seeded_
from iou_loss_util import KINDS, NUM_CLASSES, cls_scores, head_loss_fp64, make_head, rows

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


def _fused_head_loss(head, cls, deltas, rois, labels, lw, targets, bw, num_samples, dev):
    """BBoxHead.loss(..., num_samples=...) on the device -> (dict of fp64 CPU tensors, names of the C-ABI calls it made)."""
    from htd_amd import capi
    c = cls.to(dev).requires_grad_()
    d = deltas.to(dev).requires_grad_()
    rois5 = torch.cat([torch.zeros(rois.size(0), 1), rois], 1).to(dev)
    calls, real = [], capi.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    capi.call = spy
    try:
        losses = head.loss(c, d, rois5, labels.to(dev), lw.to(dev), targets.to(dev), bw.to(dev),
                           num_samples=torch.tensor(num_samples, device=dev))
    finally:
        capi.call = real
    (losses['loss_cls'] + losses['loss_bbox']).backward()
    out = dict(loss_cls=losses['loss_cls'], loss_bbox=losses['loss_bbox'], acc=losses['acc'], grad_cls=c.grad, grad_box=d.grad)
    return {k: v.detach().cpu().double() for k, v in out.items()}, calls


def _err(a, b):
    return float((a.reshape(-1) - torch.as_tensor(b, dtype=torch.float64).reshape(-1)).abs().max())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tag', ['main', 'tie'])
def test_fused_kernel_against_the_reference_fp64(golden, tag, kind):
    """Main row set (512 rows, NC = 81) and tie set through the fused path.  For loss_bbox, grad_box and grad_cls the largest absolute
    error against the reference's fp64 is at most 4 x the largest absolute error of the reference's own fp32 run against that fp64,
    per kind and quantity (the kernel's expf / logf / atanf and its summation order differ from torch's CPU ones by a few ulp; the
    conditioning is the loss's own).  grad_cls (512 x 81, too large for the fixture, which holds its digest) is compared with the fp64
    tensor formulation on the CPU, which tests/test_iou_losses.py pins to that digest.  On the tie set this covers the gradient pattern
    at max / min ties, clamp bounds and zero areas; where the reference's fp32 run is not finite (ciou_loss with pred == target: 0 / 0)
    its error is taken over its finite entries (make_golden_iou_loss.py) and the kernel must give the finite fp64 answer.

    The kernel evaluates the box side in fp64 and the caller rounds the summed loss to fp32 once, so loss_bbox is the fp32 number
    nearest the fp64 value: a bound taken from one fp32 run's luck (the reference's fp32 sum lands 3.0e-9 from fp64 on [main-CIoULoss],
    a fortieth of half an ulp) is met by construction, not by the same luck.  Measured ratios: DESIGN.md section 8 f9."""
    g = golden('iou_loss')
    dev = torch.device('cuda:0')
    rois, deltas, gts, weight, labels = rows(g, tag)
    n = rois.size(0)
    p = f'{tag}.{kind}.'
    head = make_head(kind, loss_weight=float(g['loss_weight']))
    bw = weight[:, None].expand(n, 4).contiguous()
    cls = cls_scores(tag, n)
    out, calls = _fused_head_loss(head, cls, deltas, rois, labels, torch.ones(n), gts, bw, n, dev)
    assert calls == ['htd_roi_head_loss_decoded'], calls
    ref = head_loss_fp64(head, cls, deltas, rois, labels, torch.ones(n), gts, bw)
    err32 = g[p + 'head_err32']                       # [loss_bbox, grad deltas, grad cls_score, loss_cls]
    scalars = g[p + 'head_scalars64']                 # [loss_cls, loss_bbox, acc]
    figures = dict(loss_bbox=(_err(out['loss_bbox'], scalars[1]), err32[0]),
                   grad_box=(_err(out['grad_box'], g[p + 'head_gdeltas64']), err32[1]),
                   grad_cls=(_err(out['grad_cls'], ref['grad_cls']), err32[2]))
    for k, (e, e32) in figures.items():
        print(f'{p}{k}: |kernel - fp64| {e:.3e}  |reference fp32 - fp64| {e32:.3e}  ratio {e / max(e32, 1e-300):.2f}')
    for t in out.values():
        assert torch.isfinite(t).all()
    assert float(out['acc']) == float(scalars[2])
    for k, (e, e32) in figures.items():
        assert e <= 4.0 * e32, (k, e, e32)
    # the rows the box side must not touch: exact zeros
    idle = (labels >= NUM_CLASSES) | (weight == 0)
    assert float(out['grad_box'][idle].abs().max() if idle.any() else 0.0) == 0.0


def _case(golden, name, num_classes):
    """Rows of the main set re-labelled for a head of num_classes classes."""
    g = golden('iou_loss')
    rois, deltas, gts, weight, labels = rows(g, 'main')
    n = dict(n1=1, n3=3, n257=257).get(name, 64)
    rois, deltas, gts, weight, labels = (t[:n].clone() for t in (rois, deltas, gts, weight, labels))
    labels = torch.where(labels < NUM_CLASSES, labels % num_classes, torch.full_like(labels, num_classes))
    lw = torch.ones(n)
    if name in ('n1', 'n3'):
        labels[0], weight[0] = 0, 1.0                                     # a row that does regress
    if name == 'no_positive':
        labels[:] = num_classes
    if name == 'padded_only':                                            # unused slots of the static path
        rois[:], gts[:], weight[:], lw[:] = 0., 0., 0., 0.
        deltas[::2] = 0.
        labels[: n // 2] = num_classes
    return rois, deltas, gts, weight, labels, lw


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name,nc', [('n1', 81), ('n3', 81), ('n257', 81), ('nc2', 2), ('nc128', 128), ('no_positive', 81),
                                     ('padded_only', 81)])
def test_fused_kernel_shapes(golden, name, nc, kind):
    """Sizes at which the indexing can go wrong -- fewer rows than the four waves of a block, one row more than a sweep of the
    64 x 4 grid, the smallest and the largest class count -- and batches without a positive or of unused slots only, against the fp64
    tensor formulation on the CPU.  Bound per quantity: 4 x max(error of the fp32 tensor formulation on the same inputs,
    one fp32 ulp of the quantity's largest entry) -- the rule of the main set, with the floor because on a handful of rows the fp32
    run can be exact by luck while a correctly rounded fp32 result may still be half an ulp off."""
    dev = torch.device('cuda:0')
    num_classes = nc - 1
    rois, deltas, gts, weight, labels, lw = _case(golden, name, num_classes)
    n = rois.size(0)
    head = make_head(kind, num_classes=num_classes)
    bw = weight[:, None].expand(n, 4).contiguous()
    cls = cls_scores('shape.' + name, n, nc)
    ns = max(int(lw.sum()), 0)
    out, calls = _fused_head_loss(head, cls, deltas, rois, labels, lw, gts, bw, ns, dev)
    assert calls == ['htd_roi_head_loss_decoded'], calls
    ref = head_loss_fp64(head, cls, deltas, rois, labels, lw, gts, bw, num_samples=ns)
    # the fp32 tensor formulation on the CPU: what plain fp32 arithmetic costs on these inputs
    c32, d32 = cls.clone().requires_grad_(), deltas.clone().requires_grad_()
    l32 = head.loss(c32, d32, torch.cat([torch.zeros(n, 1), rois], 1), labels, lw, gts, bw, num_samples=torch.tensor(ns))
    (l32['loss_cls'] + l32['loss_bbox']).backward()
    f32 = dict(loss_cls=l32['loss_cls'], loss_bbox=l32['loss_bbox'], acc=l32['acc'], grad_cls=c32.grad, grad_box=d32.grad)
    for k in ('loss_cls', 'loss_bbox', 'acc', 'grad_cls', 'grad_box'):
        assert torch.isfinite(out[k]).all(), k
        e, e32 = _err(out[k], ref[k]), _err(f32[k].detach().double(), ref[k])
        bound = 4.0 * max(e32, EPS32 * float(ref[k].abs().max()))
        print(f'{name}.{kind}.{k}: |kernel - fp64| {e:.3e}  |fp32 tensor formulation - fp64| {e32:.3e}  bound {bound:.3e}')
        assert e <= bound, (k, e, bound)
    if name in ('no_positive', 'padded_only'):
        assert float(out['loss_bbox']) == 0.0 and float(out['grad_box'].abs().max()) == 0.0
    if name == 'padded_only':
        assert float(out['loss_cls']) == 0.0 and float(out['grad_cls'].abs().max()) == 0.0 and float(out['acc']) == 0.0


@pytest.mark.parametrize('kind', range(5))
def test_classification_half_is_bitwise_htd_roi_head_loss_and_reproducible(golden, kind):
    """On identical inputs loss_cls, acc and grad_cls of the new entry point are bitwise those of htd_roi_head_loss (the same device
    function), and two calls of the new entry point agree bitwise in every output."""
    from htd_amd import capi
    from htd_amd.core.bbox import _d4
    g = golden('iou_loss')
    dev = torch.device('cuda:0')
    rois, deltas, gts, weight, labels = (t.to(dev) for t in rows(g, 'main'))
    n = rois.size(0)
    gen = torch.Generator().manual_seed(kind)
    cls = (torch.randn(n, 81, generator=gen) * 3).to(dev)
    cls[5, 7] = cls[5, 3] = cls[5].max() + 1.0                             # an exact tie of the maximum
    lw = (torch.rand(n, generator=gen) < 0.85).float().to(dev)
    bw = weight[:, None].expand(n, 4).contiguous()
    blocks = capi.lib().htd_roi_head_loss_partial_rows()

    def run(decoded):
        partial, box_lo = torch.full((blocks, 4), float('nan'), device=dev), torch.full((blocks, ), float('nan'), device=dev)
        gcls, gbox = torch.full_like(cls, float('nan')), torch.full((n, 4), float('nan'), device=dev)
        if decoded:
            capi.call('htd_roi_head_loss_decoded', capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(rois), capi.ptr(deltas),
                      capi.ptr(gts), capi.ptr(bw), n, 81, 80, _d4((0., 0., 0., 0.)), _d4((0.1, 0.1, 0.2, 0.2)), 16 / 1000, kind,
                      1e-3 if kind == 1 else 1e-6, 0.2, capi.ptr(partial), capi.ptr(box_lo), capi.ptr(gcls), capi.ptr(gbox), capi.current_stream_ptr())
        else:
            capi.call('htd_roi_head_loss', capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(deltas), capi.ptr(gts), capi.ptr(bw),
                      n, 81, 80, 1.0, capi.ptr(partial), capi.ptr(gcls), capi.ptr(gbox), capi.current_stream_ptr())
        torch.cuda.synchronize()
        return partial, gcls, gbox, box_lo
    old, new, again = run(False), run(True), run(True)
    assert torch.equal(new[0][:, [0, 1, 3]], old[0][:, [0, 1, 3]]) and torch.equal(new[1], old[1])
    for a, b in zip(new, again):                                            # partial, grad_cls, grad_box, box_lo
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert float(new[0][:, 2].sum()) > 0


# ---------------------------------------------------------------------------------------------------- small detector
def _cfg(loss0, loss1):
    from test_gpu_detector import small_cfg
    cfg = small_cfg()
    for h, loss in zip(cfg.model.roi_head.bbox_head, (loss0, loss1)):
        if loss is not None:
            h.update(reg_decoded_bbox=True, loss_bbox=dict(type=loss, loss_weight=10.0))
    return cfg


def _detector(loss0, loss1, dev):
    from htd_amd.configs import build_htd_detector
    model = build_htd_detector(cfg=_cfg(loss0, loss1))
    load_seeded_(model, 'det.')
    return model.to(dev).train()


def _step_losses(det, golden, dev):
    """One forward of the 2-image batch of the detector tests with the sampler keys a function of the candidate boxes."""
    from htd_amd.core.bbox import set_sample_keys
    from test_gpu_detector import inputs
    img, metas, gts, labels = inputs(golden('detector'), dev)
    coef = torch.tensor([12.9898, 78.233, 37.719, 93.989], device=dev)
    set_sample_keys(lambda cand: torch.frac(torch.sin((torch.round(cand * 64.0) / 64.0 * coef).sum(-1)) * 43758.5453).abs())
    try:
        if hasattr(det.roi_head, '_last_static'):
            del det.roi_head._last_static
        losses = det(img=img, img_metas=metas, gt_bboxes=gts, gt_labels=labels)
        _, log_vars = det._parse_losses(losses)
    finally:
        set_sample_keys(None)
    return {k: float(v) for k, v in log_vars.items()}


@pytest.mark.parametrize('loss0,loss1', [('GIoULoss', 'GIoULoss'), (None, 'CIoULoss')])
def test_small_detector_trains_static_with_iou_losses(golden, loss0, loss1):
    """GIoU on both stages (and stage 0 on smooth-L1 with stage 1 on CIoU): forward_train takes the static-shape path, every loss is
    finite and both regression losses are positive.  With GIoU on both: the fused kernel against the tensor formulation of the same
    step gives every loss within 1e-5 relative (the bound of the fused RPN loss test for the same kind of comparison)."""
    dev = torch.device('cuda:0')
    det = _detector(loss0, loss1, dev)
    assert det.roi_head.can_train_static()
    fused = _step_losses(det, golden, dev)
    assert hasattr(det.roi_head, '_last_static')
    S0, S1 = det.roi_head._last_static
    assert int(S0.is_pos.sum()) > 0 and int(S1.is_pos.sum()) > 0
    assert all(np.isfinite(v) for v in fused.values()), fused
    assert fused['s0.loss_bbox'] > 0 and fused['s1.loss_bbox'] > 0, fused
    if loss0 is None:
        return
    for h in det.roi_head.bbox_head:
        h.fused_loss = False
    plain = _step_losses(det, golden, dev)
    assert hasattr(det.roi_head, '_last_static') and set(plain) == set(fused)
    for k in plain:
        print(f'{k}: fused {fused[k]:.8f}  tensor formulation {plain[k]:.8f}')
    for k in plain:
        assert abs(fused[k] - plain[k]) <= 1e-5 * max(1.0, abs(plain[k])), (k, fused[k], plain[k])


def test_two_trainers_with_giou_heads_end_bitwise_equal():
    """The reproducibility claim of the repository on this path: two Trainers from the same seed, two steps each, end with bitwise
    equal flat parameters."""
    from htd_amd.configs import build_htd_detector
    from htd_amd.runner import Trainer, synthetic_batch
    dev = torch.device('cuda:0')

    def run():
        torch.manual_seed(0)
        model = build_htd_detector(cfg=_cfg('GIoULoss', 'GIoULoss')).to(dev).train()
        tr = Trainer(model, lr=0.01)
        data = synthetic_batch(2, 256, 320, 311, device=dev, seed=1)
        for _ in range(2):
            out = tr.train_step(data)
        assert hasattr(model.roi_head, '_last_static')
        assert torch.isfinite(out['loss'].detach()).item()
        return tr.flat.flat.detach().clone()
    a, b = run(), run()
    assert torch.isfinite(a).all().item() and torch.equal(a, b)
