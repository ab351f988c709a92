"""Shared by tests/golden/make_golden_ghm.py, tests/test_ghm.py and tests/test_gpu_ghm.py: the seeded inputs of the GHM fixture
(tests/golden/ghm.npz) and `ghm_ref`, an fp64 restatement of mmdet/models/losses/ghm_loss.py that the GPU tests compare against
(pinned to the reference's own run by test_ghm.py)."""
import numpy as np
import torch

import dense_fixture_util as D
from golden_util import seeded_tensor
import retina_util as RU

CONFIG = 'configs/ghm/retinanet_ghm_r50_fpn_1x_coco.py'
GHM_PARAMS = ((1, 0.0), (10, 0.0), (30, 0.0), (1, 0.75), (10, 0.75), (30, 0.75))         # (bins, momentum)
MU = 0.02
EDGE_MARGIN = 1e-4
ALL_BINS = (1, 10, 30)
HEAD_GHMC = dict(bins=30, momentum=0.75, loss_weight=1.0)
HEAD_GHMR = dict(mu=0.02, bins=10, momentum=0.7, loss_weight=10.0)
STATE_KEYS = ('bbox_head.loss_cls.edges', 'bbox_head.loss_cls.acc_sum', 'bbox_head.loss_bbox.edges', 'bbox_head.loss_bbox.acc_sum')


def near_edge(s, bins=ALL_BINS, margin=EDGE_MARGIN):
    """Mask of the entries of s (float64, in [0, 1]) within `margin` of an interior edge k / bins, k = 1 .. bins - 1.  The edges
    are symmetric (k / bins and 1 - k / bins), so this holds for g = s and for g = 1 - s alike."""
    bad = torch.zeros_like(s, dtype=torch.bool)
    for b in bins:
        k = (s * b).round()
        bad |= ((s - k / b).abs() < margin) & (k >= 1) & (k <= b - 1)
    return bad


def clear_of_edges(x, bins=ALL_BINS, margin=EDGE_MARGIN):
    """fp32 logits with every entry whose sigmoid lies within `margin` of a k / bins moved up, 4e-3 at a time, until none does."""
    x = x.clone()
    for _ in range(64):
        bad = near_edge(x.double().sigmoid(), bins, 1.5 * margin)
        if not bad.any():
            return x
        x[bad] += 4e-3
    raise AssertionError('clear_of_edges did not converge')


def edges_of(bins, kind):
    e = torch.arange(bins + 1).float() / bins
    if kind == 'c':
        e[-1] += 1e-6
    else:
        e[-1] = 1e3
    return e


# the fixture's weights (dense_fixture_util): retina_util's, with the four buffers of the loss modules (STATE_KEYS) as the modules
# make them: their own edges, acc_sum = 0
FIXTURE = dict(RU.FIXTURE, constants={'bbox_head.loss_cls.edges': lambda shape: edges_of(shape[0] - 1, 'c'),
                                      'bbox_head.loss_bbox.edges': lambda shape: edges_of(shape[0] - 1, 'r'),
                                      'bbox_head.loss_cls.acc_sum': torch.zeros, 'bbox_head.loss_bbox.acc_sum': torch.zeros})
assert set(FIXTURE['constants']) == set(STATE_KEYS)


def load_fixture_weights_(det, cls_scale):
    return D.load_fixture_weights(det, **FIXTURE, cls_scale=cls_scale)


def fixture_state(keys, shapes, cls_scale):
    return D.fixture_state(keys, shapes, **FIXTURE, cls_scale=cls_scale)


def ghmc_rows(n=64, C=80, tag='ghm.c'):
    """pred (n, C) fp32 clear of every edge, labels (n,) with C = background, weight (n,) with zeros and values other than 1."""
    pred = clear_of_edges(seeded_tensor(f'{tag}.pred.{n}.{C}', (n, C), scale=2.0) - 1.0)
    u = seeded_tensor(f'{tag}.u.{n}.{C}', (n, 2), kind='rand')
    labels = torch.where(u[:, 0] < 0.6, (u[:, 1] * C).long().clamp(max=C - 1), torch.full((n, ), C, dtype=torch.long))
    if n > 1:
        labels[1] = C
    weight = 0.5 + seeded_tensor(f'{tag}.w.{n}.{C}', (n, ), kind='rand')
    weight[3::5] = 0.
    return pred, labels, weight


def ghmr_rows(n=96, tag='ghm.r', seed=0):
    """pred, target (n, 4) fp32, weight (n, 4) of ones with every third row zero; differences from 1e-3 to a few units."""
    pred = seeded_tensor(f'{tag}.pred.{n}.{seed}', (n, 4), scale=0.5)
    mag = 10.0 ** (seeded_tensor(f'{tag}.mag.{n}.{seed}', (n, 4), kind='rand') * 3.5 - 3.0)
    sign = torch.where(seeded_tensor(f'{tag}.sign.{n}.{seed}', (n, 4), kind='rand') < 0.5, -1.0, 1.0)
    target = pred - mag * sign
    weight = torch.ones(n, 4)
    weight[2::3] = 0.
    return pred, target, weight


def ghmr_g(pred, target, mu=MU):
    d = pred.double() - target.double()
    return (d / torch.sqrt(d * d + mu * mu)).abs()


def head_maps(B=2, seed=0):
    """retina_util.head_maps with tags of its own: logits clear of the edges of 30 bins, deltas seeded by `seed`."""
    cls, _ = RU.head_maps(B, tag='ghm.head')
    _, reg = RU.head_maps(B, tag=f'ghm.head{seed}')
    return [clear_of_edges(c, (30, )) for c in cls], reg


def delta_targets64(anchors, gts, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """bbox2delta (core/bbox/transforms.py) in float64 throughout: the reference and htd_amd.core.bbox.bbox2delta cast their
    inputs to fp32, so their result carries fp32 rounding whatever it is given."""
    a, g = anchors.double(), gts.double()
    pw, ph, gw, gh = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1], g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    dx = ((g[..., 0] + g[..., 2]) * 0.5 - (a[..., 0] + a[..., 2]) * 0.5) / pw
    dy = ((g[..., 1] + g[..., 3]) * 0.5 - (a[..., 1] + a[..., 3]) * 0.5) / ph
    d = torch.stack([dx, dy, torch.log(gw / pw), torch.log(gh / ph)], dim=-1)
    return (d - torch.tensor(means, dtype=torch.float64)) / torch.tensor(stds, dtype=torch.float64)


def spread_box_errors(case, tag):
    """In place: the regression maps of a retina_util.head_case get, at every positive anchor, its target plus a seeded error
    of 1e-3 to a few units and either sign, so the g of GHMR fill every bin (seeded deltas of scale 0.5 are all far from their
    targets: one or two bins)."""
    na = case['na']
    assigned, anchors = case['assigned'], case['anchors'].double()
    B, A = assigned.shape
    pos = assigned > 0
    gi = (assigned - 1).clamp(min=0)
    gt_of = torch.gather(case['gts'].double(), 1, gi[..., None].expand(B, A, 4))
    safe = torch.where(pos[..., None], gt_of, anchors[None].expand(B, A, 4))
    # the targets in fp64 (the sum below is rounded to fp32 once): no fp32 implementation's own rounding of them is favoured
    tgt = delta_targets64(anchors[None].expand(B, A, 4), safe)
    mag = 10.0 ** (seeded_tensor(f'{tag}.mag', (B, A, 4), kind='rand') * 3.5 - 3.0)
    sign = torch.where(seeded_tensor(f'{tag}.sign', (B, A, 4), kind='rand') < 0.5, -1.0, 1.0)
    at = 0
    for r in case['reg']:
        h, w = r.shape[-2:]
        n = h * w * na
        want = (tgt + mag * sign).float()[:, at:at + n].reshape(B, h, w, na * 4).permute(0, 3, 1, 2)
        m = pos[:, at:at + n].reshape(B, h, w, na, 1).expand(B, h, w, na, 4).reshape(B, h, w, na * 4).permute(0, 3, 1, 2)
        r[:, :na * 4] = torch.where(m, want, r[:, :na * 4])
        at += n
    return case


# ---------------------------------------------------------------------------- the fp64 restatement
def _ghm_core(g, loss_el, grad_el, valid, tot, edges, bins, mmt, acc, loss_weight):
    """ghm_loss.py:75-94 / :153-172 on flat float64 arrays.  acc: float32 numpy array (moved in place, in the reference's
    fp32 arithmetic) or None.  -> dict(loss, grad, counts, tot, n)."""
    e = edges.double().numpy()
    g, valid = g.numpy(), valid.numpy()
    w = np.zeros_like(g)
    counts = np.zeros(bins, dtype=np.int64)
    n = 0
    for i in range(bins):
        inds = (g >= e[i]) & (g < e[i + 1]) & valid
        num = int(inds.sum())
        counts[i] = num
        if num > 0:
            if mmt > 0:
                acc[i] = np.float32(np.float32(mmt) * acc[i]) + np.float32((1 - mmt) * num)
                w[inds] = np.float64(np.float32(np.float32(1.0) / acc[i]) * np.float32(tot))
            else:
                w[inds] = tot / num
            n += 1
    if n > 0:
        w = w / n
    w = torch.from_numpy(w)
    return dict(loss=float((loss_el * w).sum() / tot * loss_weight), grad=grad_el * w / tot * loss_weight, counts=counts,
                tot=tot, n=n)


def ghmc_ref(pred, labels, weight, bins, mmt=0.0, acc=None, loss_weight=1.0):
    """GHMC.forward in fp64: pred (N, C), labels (N,) with C = background, weight (N,).  grad has pred's shape."""
    x = pred.detach().cpu().double()
    t = RU.onehot(labels.cpu(), x.size(1)).double()
    valid = (weight.cpu() > 0).view(-1, 1).expand_as(x)
    s = x.sigmoid()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none')
    tot = max(float(valid.sum()), 1.0)
    r = _ghm_core((s - t).abs().reshape(-1), bce.reshape(-1), (s - t).reshape(-1), valid.reshape(-1), tot, edges_of(bins, 'c'),
                  bins, mmt, acc, loss_weight)
    r['grad'] = r['grad'].view_as(x)
    return r


def ghmr_ref(pred, target, weight, bins, mmt=0.0, acc=None, loss_weight=1.0, mu=MU):
    """GHMR.forward in fp64 on tensors of one shape."""
    d = pred.detach().cpu().double() - target.detach().cpu().double()
    s = torch.sqrt(d * d + mu * mu)
    w = weight.cpu().double()
    tot = max(float(w.sum()), 1.0)
    r = _ghm_core((d / s).abs().reshape(-1), (s - mu).reshape(-1), (d / s).reshape(-1), (w > 0).reshape(-1), tot,
                  edges_of(bins, 'r'), bins, mmt, acc, loss_weight, )
    r['grad'] = r['grad'].view_as(d)
    return r


def head_ghm_ref(case, pc, pr, acc_c=None, acc_r=None, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """AnchorHead.loss with GHMC(**pc) + GHMR(**pr) on a retina_util.head_case, level by level in level order with shared acc
    arrays (moved in place) -> list per level of dict(c=ghmc_ref result, r=ghmr_ref result), gradients as maps (B, ch, h, w)
    without padding channels."""
    na, C = case['na'], case['C']
    assigned, anchors = case['assigned'], case['anchors'].double()
    B, A = assigned.shape
    pos = assigned > 0
    gi = (assigned - 1).clamp(min=0)
    labels = torch.where(pos, torch.gather(case['gt_labels'], 1, gi), torch.full_like(assigned, C))
    gt_of = torch.gather(case['gts'].double(), 1, gi[..., None].expand(B, A, 4))
    safe = torch.where(pos[..., None], gt_of, anchors[None].expand(B, A, 4))
    tgt = delta_targets64(anchors[None].expand(B, A, 4), safe, means, stds)
    out, at = [], 0
    for c, r in zip(case['cls'], case['reg']):
        h, w = c.shape[-2:]
        n = h * w * na
        sl = slice(at, at + n)
        x = c.permute(0, 2, 3, 1).reshape(-1, C)
        d = r[:, :na * 4].permute(0, 2, 3, 1).reshape(-1, 4)
        rc = ghmc_ref(x, labels[:, sl].reshape(-1), (assigned[:, sl] >= 0).float().reshape(-1), pc['bins'], pc['momentum'], acc_c,
                      pc['loss_weight'])
        rr = ghmr_ref(d, tgt[:, sl].reshape(-1, 4), pos[:, sl].reshape(-1, 1).expand(-1, 4).float(), pr['bins'], pr['momentum'],
                      acc_r, pr['loss_weight'], pr['mu'])
        rc['grad'] = rc['grad'].view(B, h, w, na * C).permute(0, 3, 1, 2)
        rr['grad'] = rr['grad'].view(B, h, w, na * 4).permute(0, 3, 1, 2)
        rr['g'] = ghmr_g(d, tgt[:, sl].reshape(-1, 4), pr['mu'])[pos[:, sl].reshape(-1)]
        out.append(dict(c=rc, r=rr))
        at += n
    return out
