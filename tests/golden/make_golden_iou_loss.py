#!/usr/bin/env python3
"""Generate tests/golden/iou_loss.npz by running the REFERENCE's own iou_loss.py, iou2d_calculator.py,
delta_xywh_bbox_coder.py and BBoxHead.loss (authoring container only, like make_golden.py, whose mmcv stand-in and
reference namespace this script imports and leaves as they are).

Recorded, for each of IoULoss / BoundedIoULoss / GIoULoss / DIoULoss / CIoULoss, from an fp64 run and an fp32 run of the
same fp32-representable inputs, on two row sets (`main`: 512 random rows without a discontinuity nearby; `tie`: the
non-smooth cases):
  {set}.{kind}.row64             per-row loss of the decoded boxes, fp64 whole; row32 the fp32 run
  {set}.{kind}.red64 / red32     [mean w1, mean w4, mean w1 avg, mean w4 avg, sum w1, sum w4, mean no weight]; w1 is the (n,)
                                 weight (copied to four columns for the bounded loss), w4 = w1[:, None] * (1, .5, .25, 1.25)
  {set}.{kind}.none_w1 / none_w4 digests of the 'none' reduction with (n,) and (n, 4) weights (fp64)
  {set}.{kind}.gpred64           d(mean w4 avg)/d(decoded boxes), fp64: whole on the tie set, a digest on the main set;
                                 gpred_err32 = max |fp32 - fp64|
  {set}.{kind}.head_*            BBoxHead.loss, reg_decoded_bbox=True, class-agnostic, NC = 81: loss_cls / loss_bbox / acc in
                                 fp64 and fp32, grad wrt the deltas whole (fp64), grad wrt cls_score as a digest (fp64: the
                                 512 x 81 matrix does not fit the size limit of a fixture), and err32 = max |fp32 - fp64| of
                                 [loss_bbox, grad deltas, grad cls_score, loss_cls]
  {set}.{kind}.spec_*            the same through a class-specific head on the first SPEC_ROWS rows
plus bbox_overlaps(mode='giou') aligned and in matrix form, the docstring boxes included.

Usage:  python tests/golden/make_golden_iou_loss.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from golden_util import seeded_tensor  # noqa: E402

KINDS = ('IoULoss', 'BoundedIoULoss', 'GIoULoss', 'DIoULoss', 'CIoULoss')
MEANS = (0., 0., 0., 0.)
STDS = (0.1, 0.1, 0.2, 0.2)
NUM_CLASSES = 80
AVG = 300.0
SPEC_ROWS = 48
LOSS_WEIGHT = 10.0


def main_rows(n=512, seed=7):
    rs = np.random.RandomState(seed)
    c = rs.uniform(20, 300, (n, 2))
    s = np.exp(rs.uniform(np.log(4.), np.log(200.), (n, 2)))
    rois = np.concatenate([c - s / 2, c + s / 2], 1)
    gc = c + rs.uniform(-0.35, 0.35, (n, 2)) * s
    gs = s * np.exp(rs.uniform(-0.5, 0.5, (n, 2)))
    gc[rs.rand(n) < 0.2] += 400.
    gts = np.concatenate([gc - gs / 2, gc + gs / 2], 1)
    deltas = 0.5 * rs.randn(n, 4)
    weight = (rs.rand(n) < 0.7).astype(np.float32)
    labels = rs.randint(0, NUM_CLASSES, n)
    labels[rs.rand(n) < 0.25] = NUM_CLASSES
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (rois, deltas, gts, weight)] + \
        [torch.from_numpy(labels.astype(np.int64))]


def tie_rows():
    z = [0., 0., 0., 0.]
    rows = [  # roi, deltas, gt
        ([10, 10, 30, 30], z, [10, 10, 30, 30]),                 # pred == target (gt-born roi, zero deltas)
        ([64, 32, 192, 96], z, [64, 32, 192, 96]),
        ([10, 10, 30, 30], z, [30, 10, 50, 30]),                 # touching along a vertical edge
        ([10, 10, 30, 30], z, [10, 30, 30, 50]),                 # touching along a horizontal edge
        ([10, 10, 30, 30], z, [100, 100, 120, 130]),             # disjoint
        ([100, 100, 120, 130], z, [10, 10, 30, 30]),
        ([10, 10, 30, 30], z, [20, 20, 20, 20]),                 # zero-area gt inside the prediction
        ([10, 10, 30, 30], z, [50, 60, 50, 60]),                 # zero-area gt outside
        ([40, 40, 56, 72], [0., 0., 30., 30.], [30, 30, 80, 90]),            # dw, dh above the clamp
        ([40, 40, 56, 72], [0., 0., -30., -30.], [30, 30, 80, 90]),          # below it
        ([40, 40, 56, 72], [0.5, -0.25, 30., -30.], [30, 30, 80, 90]),
        ([0, 0, 100, 100], z, [0, 0, 100, 10.125]),              # IoU just above 0.1
        ([0, 0, 100, 100], z, [0, 0, 100, 9.875]),               # just below
        ([0, 0, 64, 64], z, [0, 16, 32, 48]),                    # shared left edge, target inside
        ([0, 0, 64, 64], z, [32, 32, 64, 64]),                   # shared corner
        ([16, 16, 48, 80], [0.25, -0.5, 0.75, 0.5], [20, 24, 60, 70]),
    ]
    rois, deltas, gts = (torch.tensor([r[i] for r in rows], dtype=torch.float32) for i in range(3))
    n = len(rows)
    weight = torch.ones(n)
    labels = torch.arange(n, dtype=torch.int64) % NUM_CLASSES
    return [rois, deltas, gts, weight, labels]


def digest(t, samples=64):
    """(sum, abs-sum) and a strided sample of a tensor, float64 (golden_util.digest with a shorter sample)."""
    t = t.detach().double().reshape(-1)
    step = max(1, t.numel() // samples)
    return np.array([t.sum().item(), t.abs().sum().item()]), t[::step][:samples].numpy().copy()


def w4_of(weight):
    """(n, 4) weights whose row mean differs from a plain copy of the (n,) weight."""
    return weight[:, None] * torch.tensor([1., 0.5, 0.25, 1.25], dtype=weight.dtype)


def run_kind(tag, kind, rows, builder, coder, out, grad_cls_ref):
    rois, deltas, gts, weight, labels = rows
    n = rois.size(0)
    cls32 = seeded_tensor(f'iou_loss.{tag}.cls', (n, NUM_CLASSES + 1))
    res = {}
    for dt in (torch.float64, torch.float32):
        r, d0, g, w = (t.to(dt) for t in (rois, deltas, gts, weight))
        mod = builder.build_loss(dict(type=kind, loss_weight=1.0))
        pred = coder.delta2bbox(r, d0, MEANS, STDS).detach().requires_grad_()
        row = mod(pred, g, reduction_override='none')
        w4 = w4_of(w)
        if kind == 'BoundedIoULoss':          # its loss is (n, 4) and takes no (n,) weight: the plain weight on every component
            w = w[:, None].expand(n, 4)
        red = torch.stack([mod(pred, g, w), mod(pred, g, w4), mod(pred, g, w, avg_factor=AVG), mod(pred, g, w4, avg_factor=AVG),
                           mod(pred, g, w, reduction_override='sum'), mod(pred, g, w4, reduction_override='sum'), mod(pred, g)])
        none_w1 = mod(pred, g, w, reduction_override='none')
        none_w4 = mod(pred, g, w4, reduction_override='none')
        mod(pred, g, w4, avg_factor=AVG).backward()
        cur = dict(row=row.detach(), red=red.detach(), none_w1=none_w1.detach(), none_w4=none_w4.detach(), gpred=pred.grad.clone())
        # BBoxHead.loss on the decoded boxes: class-agnostic over all rows, class-specific over the first SPEC_ROWS
        for spec in (False, True):
            m = min(n, SPEC_ROWS) if spec else n
            head = builder.build_head(dict(type='BBoxHead', with_avg_pool=False, roi_feat_size=1, in_channels=8,
                                           num_classes=NUM_CLASSES, reg_class_agnostic=not spec, reg_decoded_bbox=True,
                                           loss_bbox=dict(type=kind, loss_weight=LOSS_WEIGHT)))
            cls = cls32[:m].to(dt).requires_grad_()
            if spec:
                full = seeded_tensor(f'iou_loss.{tag}.spec', (m, NUM_CLASSES, 4), scale=0.5).to(dt)
                col = labels[:m].clamp(max=NUM_CLASSES - 1)
                full[torch.arange(m), col] = d0[:m]
                dl = full.view(m, -1).clone().requires_grad_()
            else:
                dl = d0.clone().requires_grad_()
            rois5 = torch.cat([r.new_zeros(m, 1), r[:m]], 1)
            bw = weight.to(dt)[:m, None].expand(m, 4).contiguous()
            losses = head.loss(cls, dl, rois5, labels[:m], r.new_ones(m), g[:m], bw)
            (losses['loss_cls'] + losses['loss_bbox']).backward()
            k = 'spec' if spec else 'head'
            gd = dl.grad
            if spec:
                gfull = gd.view(m, NUM_CLASSES, 4)
                gd = gfull[torch.arange(m), col]
                cur[f'{k}_gabs'] = gfull.abs().sum()
            cur.update({f'{k}_loss_cls': losses['loss_cls'].detach(), f'{k}_loss_bbox': losses['loss_bbox'].detach(),
                        f'{k}_acc': losses['acc'].detach(), f'{k}_gdeltas': gd.clone(), f'{k}_gcls': cls.grad.clone()})
        res[dt] = cur
    a, b = res[torch.float64], res[torch.float32]
    for v in a.values():
        assert torch.isfinite(v).all(), f'{tag}.{kind}: non-finite value or gradient in the reference fp64 run'
    # The reference's fp32 run is finite on the main set.  On the tie set it is not always: with pred == target its fp32 ciou_loss
    # divides 0 by 0 (union + eps rounds to the union, so 1 - iou + v == 0).  Such rows are listed in bad32, and the fp32 error
    # of the reference is taken over the entries (for the summed loss: over the rows) where its fp32 run is finite.
    bad = ~torch.isfinite(b['row'].reshape(n, -1)).all(1)
    assert tag != 'main' or not bool(bad.any()), f'{tag}.{kind}: non-finite value in the reference fp32 run'
    if not bool(bad.any()):
        for v in b.values():
            assert torch.isfinite(v).all(), f'{tag}.{kind}: non-finite gradient in the reference fp32 run'

    def err(key):
        x, y = b[key].double(), a[key]
        if x.dim() == 0 and not bool(torch.isfinite(x)):
            assert key.endswith('loss_bbox')
            m = n if key.startswith('head') else min(n, SPEC_ROWS)
            use = ((labels[:m] < NUM_CLASSES) & ~bad[:m]).to(x.dtype) * weight[:m].double()
            rows32 = (b['row'].reshape(n, -1)[:m].nan_to_num(0.) * use.float()[:, None]).sum() * LOSS_WEIGHT / m
            rows64 = (a['row'].reshape(n, -1)[:m] * use[:, None]).sum() * LOSS_WEIGHT / m
            return (rows32.double() - rows64).abs()
        d = (x - y).abs()
        return d[torch.isfinite(d)].max()
    p = f'{tag}.{kind}.'
    out[p + 'row64'], out[p + 'row32'], out[p + 'bad32'] = a['row'], b['row'], bad
    out[p + 'red64'], out[p + 'red32'] = a['red'], b['red']
    for key in ('none_w1', 'none_w4'):
        out[p + key + '_sums'], out[p + key + '_sample'] = digest(a[key])
    if tag == 'main':       # whole on the tie set (the gradient pattern at the ties), a digest on the large set
        out[p + 'gpred_sums'], out[p + 'gpred_sample'] = digest(a['gpred'])
    else:
        out[p + 'gpred64'] = a['gpred']
    out[p + 'gpred_err32'] = err('gpred')
    for k in ('head', 'spec'):
        out[p + k + '_scalars64'] = torch.stack([a[f'{k}_loss_cls'], a[f'{k}_loss_bbox'], a[f'{k}_acc'].reshape(())])
        out[p + k + '_scalars32'] = torch.stack([b[f'{k}_loss_cls'], b[f'{k}_loss_bbox'], b[f'{k}_acc'].reshape(())])
        out[p + k + '_gdeltas64'] = a[f'{k}_gdeltas']
        out[p + k + '_gcls_sums'], out[p + k + '_gcls_sample'] = digest(a[f'{k}_gcls'])
        out[p + k + '_err32'] = torch.stack([err(f'{k}_loss_bbox'), err(f'{k}_gdeltas'), err(f'{k}_gcls'), err(f'{k}_loss_cls')])
    out[p + 'spec_gabs64'] = a['spec_gabs']
    # the classification half does not depend on the regression loss
    if grad_cls_ref:
        assert torch.equal(grad_cls_ref[0], a['head_gcls'])
    else:
        grad_cls_ref.append(a['head_gcls'])
    gmax = a['head_gdeltas'].abs().max()
    print(f'{p:22s} loss_bbox {float(a["head_loss_bbox"]):.6f}  fp32 err / max|grad|: gdeltas '
          f'{float(err("head_gdeltas") / gmax):.2e}  gpred {float(err("gpred") / a["gpred"].abs().max()):.2e}')
    return a


def main():
    torch.set_num_threads(8)
    mg.install_mmcv_standin()
    mg.install_reference_namespace()
    mg.ref('mmdet.models.losses')
    mg.ref('mmdet.models.roi_heads.bbox_heads.bbox_head')
    builder = mg.ref('mmdet.models.builder')
    coder = mg.ref('mmdet.core.bbox.coder.delta_xywh_bbox_coder')
    calc = mg.ref('mmdet.core.bbox.iou_calculators.iou2d_calculator')
    out = {}
    for tag, rows in (('main', main_rows()), ('tie', tie_rows())):
        rois, deltas, gts, weight, labels = rows
        out.update({f'{tag}.rois': rois, f'{tag}.deltas': deltas, f'{tag}.gts': gts, f'{tag}.weight': weight,
                    f'{tag}.labels': labels})
        pred64 = coder.delta2bbox(rois.double(), deltas.double(), MEANS, STDS)
        iou = calc.bbox_overlaps(pred64, gts.double(), is_aligned=True)
        if tag == 'main':
            # the comparison set holds no row next to the 0.1 branch point of the reference's iou_loss
            assert float((iou - 0.1).abs().min()) > 1e-3, float((iou - 0.1).abs().min())
        grad_cls_ref = []
        for kind in KINDS:
            run_kind(tag, kind, rows, builder, coder, out, grad_cls_ref)
        for dt, sfx in ((torch.float64, '64'), (torch.float32, '32')):
            p = coder.delta2bbox(rois.to(dt), deltas.to(dt), MEANS, STDS)
            out[f'{tag}.giou_aligned{sfx}'] = calc.bbox_overlaps(p, gts.to(dt), mode='giou', is_aligned=True)
            out[f'{tag}.giou_matrix{sfx}'] = calc.bbox_overlaps(p[:24], gts[:16].to(dt), mode='giou')
    # the boxes of the reference docstring (iou2d_calculator.py:64-75)
    b1 = torch.FloatTensor([[0, 0, 10, 10], [10, 10, 20, 20], [32, 32, 38, 42]])
    b2 = torch.FloatTensor([[0, 0, 10, 20], [0, 10, 10, 19], [10, 10, 20, 20]])
    out.update(doc_b1=b1, doc_b2=b2, doc_giou=calc.bbox_overlaps(b1, b2, mode='giou'),
               doc_giou_aligned=calc.bbox_overlaps(b1, b2, mode='giou', is_aligned=True),
               doc_giou64=calc.bbox_overlaps(b1.double(), b2.double(), mode='giou'))
    out.update(stds=np.array(STDS), means=np.array(MEANS), avg_factor=np.array(AVG), loss_weight=np.array(LOSS_WEIGHT),
               spec_rows=np.array(SPEC_ROWS), kinds=np.array(KINDS))
    mg.npz('iou_loss', **out)


if __name__ == '__main__':
    main()
