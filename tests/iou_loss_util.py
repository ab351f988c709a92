"""Shared by tests/test_iou_losses.py and tests/test_gpu_iou_losses.py: the row sets of tests/golden/iou_loss.npz (recipe in
tests/golden/make_golden_iou_loss.py) and the fp64 tensor formulation of BBoxHead.loss with reg_decoded_bbox on the CPU."""
import numpy as np
import torch

from golden_util import seeded_tensor

KINDS = ('IoULoss', 'BoundedIoULoss', 'GIoULoss', 'DIoULoss', 'CIoULoss')
NUM_CLASSES = 80
STDS = [0.1, 0.1, 0.2, 0.2]


def digest(t, samples=64):
    """make_golden_iou_loss.digest: (sum, abs-sum), strided sample."""
    t = t.detach().double().reshape(-1)
    step = max(1, t.numel() // samples)
    return np.array([t.sum().item(), t.abs().sum().item()]), t[::step][:samples].numpy().copy()


def close(a, ref, rel=1e-12):
    """|a - ref| <= rel * max(|ref| element, largest |ref|): relative to the entry, with the tensor's scale as the floor."""
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    np.testing.assert_allclose(a, ref, rtol=rel, atol=rel * max(float(np.abs(ref).max()), 1e-300))


def rows(g, tag):
    """-> rois, deltas, gts, weight (n,), labels of row set `tag` as fp32 / int64 CPU tensors."""
    return [torch.from_numpy(g[f'{tag}.{k}']) for k in ('rois', 'deltas', 'gts', 'weight', 'labels')]


def cls_scores(tag, n, nc=NUM_CLASSES + 1):
    """The (n, 81) logits the fixture's BBoxHead.loss ran on (first nc columns), or (n, nc) logits of their own for nc > 81."""
    if nc > NUM_CLASSES + 1:
        return seeded_tensor(f'iou_loss.{tag}.cls{nc}', (n, nc))
    return seeded_tensor(f'iou_loss.{tag}.cls', (n, NUM_CLASSES + 1))[:, :nc].contiguous()


def build_loss(cfg):
    import htd_amd.detector  # noqa: F401  (fills the registries)
    from htd_amd.registry import build_loss as build
    return build(cfg)


def make_head(kind, agnostic=True, loss_weight=10.0, num_classes=NUM_CLASSES, **loss_kw):
    from htd_amd.detector.bbox_heads import BBoxHead
    return BBoxHead(with_avg_pool=False, roi_feat_size=1, in_channels=8, num_classes=num_classes, reg_class_agnostic=agnostic,
                    reg_decoded_bbox=True, loss_bbox=dict(type=kind, loss_weight=loss_weight, **loss_kw),
                    bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True, target_means=[0., 0., 0., 0.], target_stds=STDS))


def head_loss_fp64(head, cls, deltas, rois, labels, label_weights, targets, bbox_weights, num_samples=None):
    """The tensor formulation of BBoxHead.loss in fp64 on the CPU (pinned against the reference's own BBoxHead.loss by
    tests/test_iou_losses.py) -> dict(loss_cls, loss_bbox, acc, grad_cls, grad_box), everything float64."""
    c = cls.detach().cpu().double().requires_grad_()
    d = deltas.detach().cpu().double().requires_grad_()
    rois5 = torch.cat([torch.zeros(rois.size(0), 1, dtype=torch.float64), rois.detach().cpu().double()], 1)
    ns = None if num_samples is None else torch.as_tensor(num_samples).cpu()
    losses = head.loss(c, d, rois5, labels.cpu(), label_weights.cpu().double(), targets.cpu().double(), bbox_weights.cpu().double(),
                       num_samples=ns)
    (losses['loss_cls'] + losses['loss_bbox']).backward()
    return dict(loss_cls=losses['loss_cls'].detach(), loss_bbox=losses['loss_bbox'].detach(), acc=losses['acc'].detach(),
                grad_cls=c.grad, grad_box=d.grad)
