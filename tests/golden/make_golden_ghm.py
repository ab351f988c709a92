#!/usr/bin/env python3
"""Generate tests/golden/ghm.npz and retinanet_ghm_r50_fpn_1x_coco_cfg.json by running the REFERENCE's own GHMC / GHMR
(mmdet/models/losses/ghm_loss.py), RetinaHead.loss with the pair and the RetinaNet built from configs/ghm/ on the CPU (authoring
container only, like make_golden_retinanet.py, whose additions to make_golden's mmcv stand-in are reused).  Only data is stored;
inputs and weights are re-created from seeds by tests/ghm_util.py (load_fixture_weights_ there).

GHM is discontinuous in its inputs: an element that crosses a bin edge changes two bin counts.  Every seeded input is therefore
kept 1e-4 away from every edge (ghm_util.clear_of_edges for logits, asserted here in fp64; regression rows are re-seeded until
no valid g lies within 1e-4 of an edge), so bin counts are unambiguous.  The detector's logits cannot be moved; there the margin
and the effect of a flip are measured instead (below).

Per setting i of ghm_util.GHM_PARAMS (bins, momentum), three consecutive calls k = 0, 1, 2 of one module on different rows:
  c.{i}.loss64 / .loss32 (3,)    GHMC losses of the calls;  c.{i}.acc64 / .acc32 (3, bins): acc_sum after each call (momentum > 0)
  c.{i}.grad64 (n, C)            d loss / d pred of call 0;  c.{i}.counts (3, bins), .tot (3,), .n (3,): recomputed here from the
                                 fp64 g and the module's fp32 edges
  c.{i}.err32 (2,)               the reference's own |fp32 - fp64|: [max over the calls' losses, max over the gradient of call 0]
  r.{i}.*                        the same of GHMR (mu = ghm_util.MU); r.seed: the seed of ghm_util.ghmr_rows that gave the margin
Head (reference RetinaHead with ghm_util.HEAD_GHMC / HEAD_GHMR on ghm_util.head_maps(seed = head.seed) and
baselines_util.detector_inputs()), two consecutive calls:
  head.loss64 / .loss32 (2, 2, 5)   [call][cls, bbox][level];  head.acc_c64 / .acc_c32 (2, 30), head.acc_r64 / .acc_r32 (2, 10)
Detector (the GHM config, ghm_util.load_fixture_weights_(det, cls_scale)), one training step in fp32 and in fp64 (the loss
modules' buffers stay fp32 in both, and the fp64 run replays the anchor assignment of the fp32 run, so the two differ by rounding
alone; see also upcast_bce_target):
  loss.* / loss64.*, grad.{key}.sums / .sample (fp32 run), cls{l}.* / reg{l}.* digests, assigned (2, A) int16, num_pos,
  state_keys / state_shapes, acc_c / acc_r (fp32 run) and acc_c64 / acc_r64 after the step
  margin.edge (2,)   [GHMC, GHMR] 4 x the largest |g_fp32 - g_fp64| between the two runs: the scale at which an honest fp32
                     implementation may bin an element differently
  flip.loss / flip.grad (2,)   [GHMC, GHMR] in fp64: for every valid element within margin.edge of an edge, |change| of its level's
                     loss (of the L1 norm of its level's gradient) if that element alone sat in the neighbouring bin, summed
                     over elements and levels, relative to the loss (the norm) summed over the levels
cls_scale is the first of SCALES for which all four flip figures are <= 1e-4: asserted here, a condition checked on the CPU.

Usage:  python tests/golden/make_golden_ghm.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_retinanet as mgr  # noqa: E402
import baselines_util as BU  # noqa: E402
import retina_util as RU  # noqa: E402
import ghm_util as U  # noqa: E402

SCALES = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3)
FLIP_BOUND = 1e-4


def merged_config():
    from htd_amd import Config
    cfg = Config.fromfile(os.path.join(mg.REF, U.CONFIG))
    return {k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in RU.CFG_KEYS}


def gen_config():
    path = os.path.join(HERE, os.path.basename(U.CONFIG)[:-3] + '_cfg.json')
    with open(path, 'w') as f:
        json.dump(merged_config(), f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {path}')


def hist(g, valid, edges):
    """counts per bin of the valid entries of g (float64) under the fp32 edges, and how close a valid g comes to an interior edge."""
    e = edges.double()
    g = g[valid]
    counts = torch.stack([((g >= e[i]) & (g < e[i + 1])).sum() for i in range(len(e) - 1)])
    gap = float((g.view(-1, 1) - e[1:-1].view(1, -1)).abs().min()) if len(e) > 2 and g.numel() else 1.0
    return counts, gap


def ghmc_g(pred, labels):
    return (pred.double().sigmoid() - RU.onehot(labels, pred.size(1)).double()).abs()


def gen_modules(out, builder):
    rows_c = [U.ghmc_rows(tag=f'ghm.c{k}') for k in range(3)]
    for seed in range(64):
        rows_r = [U.ghmr_rows(tag=f'ghm.r{k}', seed=seed) for k in range(3)]
        gaps = [hist(U.ghmr_g(p, t), w > 0, U.edges_of(b, 'r'))[1] for p, t, w in rows_r for b in U.ALL_BINS]
        if min(gaps) >= U.EDGE_MARGIN:
            break
    else:
        raise AssertionError('no seed keeps the regression rows clear of the edges')
    out['r.seed'] = np.array(seed)
    for i, (bins, mmt) in enumerate(U.GHM_PARAMS):
        for kind, rows in (('c', rows_c), ('r', rows_r)):
            res = {}
            for dt in (torch.float64, torch.float32):
                spec = dict(type='GHMC', bins=bins, momentum=mmt, use_sigmoid=True, loss_weight=1.0) if kind == 'c' else \
                    dict(type='GHMR', mu=U.MU, bins=bins, momentum=mmt, loss_weight=1.0)
                mod = builder.build_loss(spec)
                losses, accs, grad = [], [], None
                for k, (a, b, w) in enumerate(rows):
                    pred = a.detach().clone().to(dt).requires_grad_()
                    loss = mod(pred, b, w) if kind == 'c' else mod(pred, b.to(dt), w.to(dt))
                    if k == 0:
                        loss.backward()
                        grad = pred.grad.clone()
                    losses.append(loss.detach())
                    accs.append(mod.acc_sum.clone() if mmt > 0 else torch.zeros(bins))
                res[dt] = dict(loss=torch.stack(losses), acc=torch.stack(accs), grad=grad)
            a, b = res[torch.float64], res[torch.float32]
            p = f'{kind}.{i}.'
            out[p + 'loss64'], out[p + 'loss32'], out[p + 'acc64'], out[p + 'acc32'] = a['loss'], b['loss'], a['acc'], b['acc']
            out[p + 'grad64'] = a['grad']
            out[p + 'err32'] = torch.stack([(b['loss'].double() - a['loss']).abs().max(), (b['grad'].double() - a['grad']).abs().max()])
            counts, tots = [], []
            for x, y, w in rows:
                if kind == 'c':
                    g, valid = ghmc_g(x, y), (w > 0).view(-1, 1).expand_as(x)
                    c, gap = hist(g, valid, mod.edges)
                    tots.append(max(float(valid.sum()), 1.0))
                else:
                    c, gap = hist(U.ghmr_g(x, y), w > 0, mod.edges)
                    tots.append(max(float(w.sum()), 1.0))
                assert gap >= U.EDGE_MARGIN * 0.999, (kind, bins, gap)
                counts.append(c)
            out[p + 'counts'], out[p + 'tot'] = torch.stack(counts), np.array(tots)
            out[p + 'n'] = (torch.stack(counts) > 0).sum(1)
            print(f'{kind} bins {bins} momentum {mmt}: losses', a['loss'].tolist(), 'err32', out[p + 'err32'].tolist())


def record_calls(mod, store):
    orig = mod.forward

    def rec(pred, target, weight, *a, **k):
        store.append((pred.detach().clone(), target.detach().clone(), weight.detach().clone()))
        return orig(pred, target, weight, *a, **k)
    mod.forward = rec
    return orig


def build_head(builder, dt):
    cfg = merged_config()
    spec = dict(cfg['model']['bbox_head'])
    head = builder.build_head(dict(spec, train_cfg=mg.Config(cfg['train_cfg']), test_cfg=mg.Config(cfg['test_cfg'])))
    assert type(head.loss_cls).__name__ == 'GHMC' and head.loss_cls.bins == U.HEAD_GHMC['bins'] and \
        head.loss_bbox.mu == U.HEAD_GHMR['mu'] and head.loss_bbox.loss_weight == U.HEAD_GHMR['loss_weight']
    return head


def gen_head(out, builder):
    _, metas, gts, labels = BU.detector_inputs()
    gts_t, labels_t = [torch.from_numpy(g) for g in gts], [torch.from_numpy(l) for l in labels]
    for seed in range(64):
        res, ok = {}, True
        for dt, tag in ((torch.float64, '64'), (torch.float32, '32')):
            head = build_head(builder, dt)
            calls_c, calls_r = [], []
            record_calls(head.loss_cls, calls_c)
            record_calls(head.loss_bbox, calls_r)
            cls, reg = U.head_maps(seed=seed)
            ls, acc_c, acc_r = [], [], []
            for _ in range(2):
                l = head.loss([c.to(dt) for c in cls], [r.to(dt) for r in reg], [g.to(dt) for g in gts_t], labels_t, metas)
                assert len(l['loss_cls']) == 5 and len(l['loss_bbox']) == 5
                ls.append(torch.stack([torch.stack(l['loss_cls']), torch.stack(l['loss_bbox'])]))
                acc_c.append(head.loss_cls.acc_sum.clone())
                acc_r.append(head.loss_bbox.acc_sum.clone())
            res[tag] = (torch.stack(ls), torch.stack(acc_c), torch.stack(acc_r))
            if dt == torch.float64:
                for pred, target, w in calls_c[:5]:
                    gap = hist(ghmc_g(pred, target), (w > 0).view(-1, 1).expand_as(pred), head.loss_cls.edges)[1]
                    assert gap >= U.EDGE_MARGIN * 0.999, gap
                for pred, target, w in calls_r[:5]:
                    ok = ok and hist(U.ghmr_g(pred, target, head.loss_bbox.mu), w > 0, head.loss_bbox.edges)[1] >= U.EDGE_MARGIN
                assert sum(int((w > 0).sum()) for _, _, w in calls_r[:5]) > 0
        if ok:
            break
    else:
        raise AssertionError('no seed keeps the regression maps clear of the edges')
    out['head.seed'] = np.array(seed)
    for tag in ('64', '32'):
        out['head.loss' + tag], out['head.acc_c' + tag], out['head.acc_r' + tag] = res[tag]
    print('head seed', seed, 'losses per call', res['64'][0].sum(-1).tolist())


def level_loss(S, num, prev, mmt, lw):
    """The loss of one call from its per-bin sums S of the element losses, the counts and acc_sum before the call (fp64)."""
    filled = num > 0
    n = int(filled.sum())
    if n == 0:
        return 0.0
    acc = mmt * prev + (1 - mmt) * num if mmt > 0 else num.astype(np.float64)
    return lw / n * float((S[filled] / acc[filled]).sum())


def flip_figures(g, el_loss, el_grad, valid, edges, prev, mmt, lw, margin):
    """-> (sum |change of the loss|, sum |change of the gradient's L1 norm|, loss, norm, elements near an edge) of one call."""
    e = edges.double().numpy()
    bins = len(e) - 1
    g, el_loss, el_grad = g[valid].numpy(), el_loss[valid].numpy(), el_grad[valid].numpy()
    idx = np.clip(np.searchsorted(e, g, side='right') - 1, 0, bins - 1)
    num = np.bincount(idx, minlength=bins).astype(np.float64)
    S, G = np.bincount(idx, el_loss, bins), np.bincount(idx, el_grad, bins)
    loss, norm = level_loss(S, num, prev, mmt, lw), level_loss(G, num, prev, mmt, lw)
    d_loss = d_norm = 0.0
    near = 0
    for k in range(1, bins):
        for j in np.nonzero(np.abs(g - e[k]) <= margin)[0]:
            i, o = idx[j], (k if idx[j] == k - 1 else k - 1)
            num2, S2, G2 = num.copy(), S.copy(), G.copy()
            num2[i] -= 1; num2[o] += 1
            S2[i] -= el_loss[j]; S2[o] += el_loss[j]
            G2[i] -= el_grad[j]; G2[o] += el_grad[j]
            d_loss += abs(level_loss(S2, num2, prev, mmt, lw) - loss)
            d_norm += abs(level_loss(G2, num2, prev, mmt, lw) - norm)
            near += 1
    return d_loss, d_norm, loss, norm, near


def run_detector(builder, cls_scale, dt, replay=None):
    cfg = merged_config()
    model = cfg['model']
    model['pretrained'] = None
    torch.manual_seed(0)
    det = builder.build_detector(model, train_cfg=mg.Config(cfg['train_cfg']), test_cfg=mg.Config(cfg['test_cfg']))
    det.init_weights(None)
    U.load_fixture_weights_(det, cls_scale)
    det = det.to(dt)
    # the loss buffers stay fp32, as in an fp32 run of the reference: Module.to would have cast them
    for m in (det.bbox_head.loss_cls, det.bbox_head.loss_bbox):
        m.edges, m.acc_sum = m.edges.float(), m.acc_sum.float()
    det.train()
    imgs, metas, gts, labels = BU.detector_inputs()
    head = det.bbox_head
    trail = dict(c=[], r=[], assigned=[])
    record_calls(head.loss_cls, trail['c'])
    record_calls(head.loss_bbox, trail['r'])
    orig_forward, orig_assign = head.forward, head.assigner.assign

    def rec_forward(feats):
        trail['outs'] = orig_forward(feats)
        return trail['outs']

    def rec_assign(*a, **k):
        r = orig_assign(*a, **k)
        if replay is not None:              # the discrete decisions of the fp32 run, so the two runs differ by rounding alone
            img = len(trail['assigned'])
            pos = replay[img] > 0
            r.gt_inds = replay[img].clone()
            r.labels = torch.where(pos, a[3][(replay[img] - 1).clamp(min=0)], torch.full_like(r.labels, -1))
        trail['assigned'].append(r.gt_inds.clone())
        return r
    head.forward, head.assigner.assign = rec_forward, rec_assign
    losses = det.forward_train(torch.from_numpy(imgs).to(dt), metas, [torch.from_numpy(g).to(dt) for g in gts],
                               [torch.from_numpy(l) for l in labels])
    loss, log_vars = det._parse_losses(losses)
    det.zero_grad()
    loss.backward()
    return det, trail, log_vars


def gen_detector(out, builder, cls_scale):
    det, t32, lv32 = run_detector(builder, cls_scale, torch.float32)
    det64, t64, lv64 = run_detector(builder, cls_scale, torch.float64, replay=t32['assigned'])
    head = det64.bbox_head
    mu = head.loss_bbox.mu
    assert all(torch.equal(a, b) for a, b in zip(t64['assigned'], t32['assigned']))
    assert all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(t64['c'], t32['c']))

    def g_of(kind, pred, target):
        if kind == 'c':
            return (pred.sigmoid() - RU.onehot(target, pred.size(1)).to(pred.dtype)).abs()
        d = pred - target
        return (d / torch.sqrt(mu * mu + d * d)).abs()
    margin, flips = [], []
    for kind, mod in (('c', head.loss_cls), ('r', head.loss_bbox)):
        valids = [((w > 0).view(-1, 1).expand_as(p) if kind == 'c' else w > 0) for p, _, w in t64[kind]]
        dg = [float((g_of(kind, a[0], a[1]).double() - g_of(kind, b[0], b[1]))[v].abs().max()) if v.any() else 0.0
              for a, b, v in zip(t32[kind], t64[kind], valids)]
        margin.append(4.0 * max(dg))
        prev = np.zeros(mod.bins)
        tot = [0.0, 0.0, 0.0, 0.0, 0]
        for (pred, target, w), v in zip(t64[kind], valids):
            g = g_of(kind, pred, target)
            if kind == 'c':
                t = RU.onehot(target, pred.size(1)).double()
                el = torch.nn.functional.binary_cross_entropy_with_logits(pred, t, reduction='none')
            else:
                d = pred - target
                el = torch.sqrt(d * d + mu * mu) - mu
            f = flip_figures(g.reshape(-1), el.reshape(-1), g.reshape(-1), v.reshape(-1), mod.edges, prev, mod.momentum,
                             mod.loss_weight, margin[-1])
            tot = [a + b for a, b in zip(tot, f)]
            num = hist(g.reshape(-1), v.reshape(-1), mod.edges)[0].double().numpy()
            prev = np.where(num > 0, mod.momentum * prev + (1 - mod.momentum) * num, prev)
        # the restated per-level losses are the reference's
        np.testing.assert_allclose(tot[2], float(lv64['loss_cls' if kind == 'c' else 'loss_bbox']), rtol=1e-6)
        flips.append((tot[0] / tot[2], tot[1] / tot[3], tot[4]))
    print(f'cls scale {cls_scale}: margin.edge {margin}, flips (loss, grad norm, elements near an edge) {flips}')
    if max(max(f[:2]) for f in flips) > FLIP_BOUND:
        return False
    out['margin.edge'] = np.array(margin)
    out['flip.loss'], out['flip.grad'] = np.array([f[0] for f in flips]), np.array([f[1] for f in flips])
    out['flip.near'] = np.array([f[2] for f in flips])
    for k, v in lv32.items():
        out['loss.' + k] = np.float64(v)
    for k, v in lv64.items():
        out['loss64.' + k] = np.float64(v)
    params = dict(det.named_parameters())
    for k in RU.grad_keys(det):
        out[f'grad.{k}.sums'], out[f'grad.{k}.sample'] = BU.digest(params[k].grad)
    cls_scores, bbox_preds = t32['outs']
    assert tuple(tuple(c.shape[-2:]) for c in cls_scores) == RU.LEVEL_SIZES
    for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        out[f'cls{l}.sums'], out[f'cls{l}.sample'] = BU.digest(c)
        out[f'reg{l}.sums'], out[f'reg{l}.sample'] = BU.digest(r)
    assigned = torch.stack(t32['assigned'])
    num_pos = (assigned > 0).sum(1)
    assert int(num_pos.min()) > 0, num_pos
    out['assigned'], out['num_pos'] = assigned.to(torch.int16), num_pos
    out['acc_c'], out['acc_r'] = det.bbox_head.loss_cls.acc_sum.clone(), det.bbox_head.loss_bbox.acc_sum.clone()
    out['acc_c64'], out['acc_r64'] = det64.bbox_head.loss_cls.acc_sum.clone(), det64.bbox_head.loss_bbox.acc_sum.clone()
    sd = det.state_dict()
    assert set(U.STATE_KEYS) <= set(sd.keys())
    out['state_keys'] = np.array(list(sd.keys()))
    out['state_shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    out['cls_scale'] = np.array(cls_scale)
    print('positives per image', num_pos.tolist(), 'losses', {k: round(float(v), 5) for k, v in lv32.items()})
    return True


def upcast_bce_target():
    """GHMC.forward casts its binary target to fp32 (ghm_loss.py:67), and torch evaluates binary_cross_entropy_with_logits in
    the target's precision: the loss of an fp64 run would carry fp32 rounding.  The reference module's F is given a BCE that
    casts the target to the logits' dtype first, so its fp64 runs are fp64 throughout; fp32 runs are untouched."""
    import types
    import torch.nn.functional as F
    gl = mg.ref('mmdet.models.losses.ghm_loss')

    def bce(pred, target, weight=None, **kw):
        return F.binary_cross_entropy_with_logits(pred, target.to(pred.dtype), weight, **kw)
    gl.F = types.SimpleNamespace(binary_cross_entropy_with_logits=bce)


def main():
    torch.set_num_threads(8)
    mg.install_mmcv_standin()
    mg.install_reference_namespace()
    mg.ref('mmdet.models.losses')
    upcast_bce_target()
    mgr.extend_standin()
    for m in ('mmdet.models.backbones.resnet', 'mmdet.models.necks.fpn', 'mmdet.models.dense_heads.anchor_head',
              'mmdet.models.dense_heads.retina_head', 'mmdet.models.detectors.base', 'mmdet.models.detectors.single_stage',
              'mmdet.models.detectors.retinanet'):
        mg.ref(m)
    gen_config()
    builder = mg.ref('mmdet.models.builder')
    out = {}
    gen_modules(out, builder)
    gen_head(out, builder)
    for scale in SCALES:
        if gen_detector(out, builder, scale):
            break
    else:
        raise AssertionError('no scale of the classification layer keeps the flip bounds')
    mg.npz('ghm', **out)


if __name__ == '__main__':
    main()
