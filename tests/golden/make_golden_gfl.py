#!/usr/bin/env python3
"""Generate tests/golden/gfl.npz and the two gfl_*_cfg.json by running the REFERENCE's own GFL (detectors/gfl.py,
dense_heads/gfl_head.py, losses/gfocal_loss.py, core/bbox/transforms.py, the ATSS assigner ...) on the CPU (authoring container
only, like make_golden_atss.py, whose stand-in is used as it is).  Only data is stored; weights, maps and inputs are re-created
from seeds by gfl_util.

The reference's mstrain config names a base file its tree does not hold; gfl_util.MISSING_BASE says which sibling stands in.
The JSON holds gfl_util.CFG_KEYS and 'train_pipeline' (data.train.pipeline).

Head level, variant v of gfl_util.HEAD_VARIANTS on gfl_util.head_maps(v) and atss_util.detector_inputs()'s boxes.  The fp32 run is
the reference's GFLHead.loss.  Its _get_target_single mixes dtypes when the gts are fp64, so the fp64 run takes the targets in
fp32 (the gts are fp32 values; the label weights cast, since the score tensor takes their dtype) and calls the reference's
loss_single per level on fp64 maps, with the final division done as `loss` does it; on fp32 maps that path equals `loss` (asserted).
  head.assigned                 (2, A) int16: 0 background, k + 1 = gt k
  head.tdist                    (2, A, 4) unclamped target distances in stride units (fp32 order), 0 on background
  head.{v}.loss64 / .loss32     [loss_cls, loss_bbox, loss_dfl]
  head.{v}.greg64               (2, A, 4 * (reg_max + 1)) gradient of the distribution logits, level-major
  head.{v}.gcls64.sums / .sample  digest of the (2, A, 80) gradient of the class logits
  head.{v}.err32                |fp32 - fp64| of the reference's own runs: [3 losses, max over gcls, greg, score, weight, gclspos]
  head.pos_index                (77, 3) image, anchor and class of every positive;  head.{v}.gclspos64  the gradient of the class
                                logits at those entries (the derivative of QFL's positive element, which the strided digest misses)
  head.{v}.score64 / .score32 / .weight64 / .weight32   (2, A): the IoU score and max_c sigmoid(cls) of the positives, 0 elsewhere
  head.boxes{b} / .score_rows{b}   get_bboxes(with_nms=False) of image b under gfl_util.HEAD_TEST_CFG on the giou maps
  head.nopos.loss               the three losses of the giou head on a batch without gts: [finite, NaN, NaN]
Loss modules (gfl_util.loss_module_case(), fp64): per mode i of gfl_util.LOSS_MODES  qfl.{i} / qfl.{i}.grad, dfl.{i} /
dfl.{i}.grad; b2d.plain / b2d.max7 = bbox2distance of gfl_util.distance_case() without and with max_dis = 7.
Detector (gfl_util.load_fixture_weights_ on the merged r50 config, atss_util.detector_inputs()):
  loss.*  grad.{key}.sums / .sample  cls{l}.* / reg{l}.*  assigned  num_pos  test_dets{b}  nms_pre  state_keys / state_shapes
  margin.key / .score / .iou  cls_scale / cls_bias_shift, as in make_golden_atss.py.

Asserted here (GAP = 1e-3 relative), the conditions under which the tests are fair demands: the fp32 and fp64 assignments are
equal; every positive's target side is either an exact integer or GAP away from one, and either GAP below reg_max - 0.1 or GAP
above it (so label.long() and the clamp land alike in any correctly ordered fp32); every image has a positive; the reg_max 7
variant clamps some sides; the nms_pre cut bites on two levels with GAP between the keys at the cut; score and IoU gaps of the
test detections as in make_golden_fcos.py.

Usage:  python tests/golden/make_golden_gfl.py
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
import make_golden_retinanet as mr  # noqa: E402
import make_golden_atss as ma  # noqa: E402
import baselines_util as BU  # noqa: E402
import gfl_util as U  # noqa: E402

GAP = 1e-3
SCALES = ma.SCALES
SHIFTS = tuple(4.0 + 0.125 * i for i in range(17))      # (ATSS's half steps from 3 to 7 leave no pair with every margin here)


def file2dict(path):
    from htd_amd.registry import _merge
    ns = {}
    exec(compile(open(path).read(), path, 'exec'), ns)
    cfg = {k: v for k, v in ns.items() if not k.startswith('__') and isinstance(v, (dict, list, tuple, str, int, float))}
    bases = cfg.pop('_base_', [])
    merged = {}
    for b in ([bases] if isinstance(bases, str) else bases):
        if not os.path.isfile(os.path.join(os.path.dirname(path), b)):
            b = U.MISSING_BASE[b]
        merged = _merge(merged, file2dict(os.path.join(os.path.dirname(path), b)))
    return _merge(merged, cfg)


def merged_config(which):
    cfg = file2dict(os.path.join(mg.REF, U.CONFIGS[which]))
    out = {k: cfg[k] for k in U.CFG_KEYS}
    out['train_pipeline'] = cfg['data']['train']['pipeline']
    return json.loads(json.dumps(out))


def gen_configs():
    for which in U.CONFIGS:
        path = os.path.join(HERE, os.path.basename(U.CONFIGS[which])[:-3] + '_cfg.json')
        with open(path, 'w') as f:
            json.dump(merged_config(which), f, indent=1, sort_keys=True)
            f.write('\n')
        print(f'wrote {path}')


def ref_head(builder, v='giou'):
    torch.manual_seed(0)
    return builder.build_head(dict(U.head_cfg(v), train_cfg=mg.Config(U.TRAIN_CFG)))


def ref_loss(head, cls, reg, gts_t, labels_t, metas, dt, record=None):
    """The reference's loss with the targets in fp32 and loss_single on maps of dtype dt -> [loss_cls, loss_bbox, loss_dfl]."""
    sizes = [c.shape[-2:] for c in cls]
    anchor_list, valid_flag_list = head.get_anchors(sizes, metas, device='cpu')
    t = head.get_targets(anchor_list, valid_flag_list, gts_t, metas, gt_labels_list=labels_t, label_channels=head.cls_out_channels)
    anchors, labels, lw, bt, _, num_total_pos, _ = t
    nts = max(float(num_total_pos), 1.0)
    res = [head.loss_single(a, c, r, lab, w.to(dt), b, s, num_total_samples=nts)
           for a, c, r, lab, w, b, s in zip(anchors, cls, reg, labels, lw, bt, head.anchor_generator.strides)]
    avg = float(sum(r[3] for r in res))
    return torch.stack([sum(r[0] for r in res), sum(r[1] / avg for r in res), sum(r[2] / avg for r in res)])


def quality_of(head, cls, reg, assigned, padded, dt):
    """score and weight (B, A) of the positives as loss_single computes them, in dt."""
    core = sys.modules['mmdet.core']
    anchors = U.anchors_of()
    rows_c, rows_r = U.maps_to_rows(cls).to(dt), U.maps_to_rows(reg).to(dt)
    stride = torch.cat([torch.full((n, ), float(s)) for n, s in zip(U.LEVEL_ANCHORS, U.STRIDES)])
    score, weight = torch.zeros(assigned.shape, dtype=dt), torch.zeros(assigned.shape, dtype=dt)
    pos = assigned > 0
    b, i = pos.nonzero(as_tuple=True)
    centres = head.anchor_center(anchors[i]) / stride[i, None]
    pred = core.distance2bbox(centres, head.integral(rows_r[b, i]))
    score[pos] = core.bbox_overlaps(pred, padded[b, assigned[pos] - 1] / stride[i, None], is_aligned=True)
    weight[pos] = rows_c[b, i].sigmoid().max(dim=1)[0]
    return score, weight


def cut_gaps(keys, k):
    """The relative gaps between the k-th and the next ranking key of every (image, level) that a cut to k bites on."""
    gaps, at = [], 0
    for n in U.LEVEL_ANCHORS:
        if n > k:
            s = keys[:, at:at + n].sort(1, descending=True)[0]
            gaps.append(float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min()))
        at += n
    return gaps


def search_head_tag():
    """gfl_util.HEAD_TAG and the nms_pre of HEAD_TEST_CFG: of the seed tags gfl.head, gfl.head.v1, ..., v11 the first whose ranking
    keys max_c sigmoid(cls) leave a gap of GAP at both cuts (levels 0 and 1) for some nms_pre in 30 .. 75, and of those the nearest 50."""
    for t in range(12):
        tag = 'gfl.head' if t == 0 else f'gfl.head.v{t}'
        keys = U.maps_to_rows(U.head_maps(tag=tag)[0]).sigmoid().max(-1)[0].double()
        for k in sorted(range(30, 76), key=lambda k: abs(k - 50)):
            gaps = cut_gaps(keys, k)
            if len(gaps) >= 2 and min(gaps) >= GAP:
                return tag, k
    raise AssertionError('no seed tag leaves a key gap at a cut')


def gen_heads(out, builder):
    _, metas, gts, labels = U.detector_inputs()
    gts_t, labels_t = [torch.from_numpy(g) for g in gts], [torch.from_numpy(l) for l in labels]
    head = ref_head(builder)
    anchors = ma.ref_anchors(head)
    ma.check_margins(anchors, gts_t, 'head case')
    a32, a64 = ma.ref_assign(head, anchors, gts_t, torch.float32), ma.ref_assign(head, anchors, gts_t, torch.float64)
    assert torch.equal(a32, a64) and int((a32 > 0).sum(1).min()) > 0
    padded, _, _ = U.pad_gts(gts_t)
    pos = a32 > 0
    lvl = torch.cat([torch.full((n, ), l) for l, n in enumerate(U.LEVEL_ANCHORS)])
    tdist = U.target_distances(anchors, padded, a32)
    stride = torch.cat([torch.full((n, ), float(s)) for n, s in zip(U.LEVEL_ANCHORS, U.STRIDES)]).double()
    b, i = pos.nonzero(as_tuple=True)
    a, g = anchors[i].double(), padded[b, a32[pos] - 1].double()
    cx, cy = ((a[:, 2] + a[:, 0]) / 2) / stride[i], ((a[:, 3] + a[:, 1]) / 2) / stride[i]
    tg = g / stride[i, None]
    t64 = torch.stack([cx - tg[:, 0], cy - tg[:, 1], tg[:, 2] - cx, tg[:, 3] - cy], -1)
    t32 = tdist[pos].double()
    print('head case: positives', int(pos.sum()), 'per level', [int(pos[:, lvl == l].sum()) for l in range(5)],
          'largest target side', float(t32.max()))
    for R in sorted({U.reg_max_of(v) for v in U.HEAD_VARIANTS}):
        for t in (t32, t64):
            c = t.clamp(min=0, max=R - 0.1)
            frac = (c - c.round()).abs()
            integer = (t32 == t32.round()) & (t64 == t64.round())
            assert bool((integer | (frac >= GAP)).all()), ('a target side within GAP of an integer', R)
            lim = R - 0.1
            assert bool((((t - lim).abs() / lim) >= GAP).all()), ('a target side within GAP of the clamp', R)
        assert torch.equal(t32.clamp(min=0, max=R - 0.1).long(), t64.clamp(min=0, max=R - 0.1).long())
        print(f'reg_max {R}: sides that take the clamp', int((t32 > R - 0.1).sum()), 'negative sides', int((t32 < 0).sum()))
    assert int((t32 > 6.9).sum()) > 0
    out['head.assigned'], out['head.tdist'] = a32.to(torch.int16), tdist
    pb, pa = pos.nonzero(as_tuple=True)
    pc = torch.stack([labels_t[int(x)][int(a32[x, y]) - 1] for x, y in zip(pb, pa)])
    out['head.pos_index'] = torch.stack([pb, pa, pc], 1)
    for v in U.HEAD_VARIANTS:
        head = ref_head(builder, v)
        res = {}
        for dt in (torch.float64, torch.float32):
            cls, reg = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps(v)]
            losses = ref_loss(head, cls, reg, gts_t, labels_t, metas, dt)
            losses.sum().backward()
            res[dt] = dict(loss=losses.detach(), g=[U.maps_to_rows([m.grad for m in ms]) for ms in (cls, reg)],
                           q=quality_of(head, [c.detach() for c in cls], [r.detach() for r in reg], a32, padded, dt))
            assert all(torch.isfinite(x).all() for x in res[dt]['g']) and torch.isfinite(losses).all()
            if dt == torch.float32:
                ls = head.loss([c.detach() for c in cls], [r.detach() for r in reg], gts_t, labels_t, metas)
                whole = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_dfl'])])
                assert torch.equal(whole, losses.detach()), (whole, losses)
        a, b32 = res[torch.float64], res[torch.float32]
        p = f'head.{v}.'
        out[p + 'loss64'], out[p + 'loss32'] = a['loss'], b32['loss']
        out[p + 'gcls64.sums'], out[p + 'gcls64.sample'] = BU.digest(a['g'][0])
        out[p + 'greg64'] = a['g'][1]
        gp64, gp32 = a['g'][0][pb, pa, pc], b32['g'][0][pb, pa, pc]
        assert int((gp64 != 0).sum()) == len(pb)
        out[p + 'gclspos64'] = gp64
        out[p + 'score64'], out[p + 'weight64'] = a['q']
        out[p + 'score32'], out[p + 'weight32'] = b32['q']
        out[p + 'err32'] = torch.cat([(b32['loss'].double() - a['loss']).abs()] +
                                     [(gb.double() - ga).abs().max()[None] for ga, gb in zip(a['g'], b32['g'])] +
                                     [(qb.double() - qa).abs().max()[None] for qa, qb in zip(a['q'], b32['q'])] +
                                     [(gp32.double() - gp64).abs().max()[None]])
        print(f'head {v}: loss64', a['loss'].tolist(), 'err32', out[p + 'err32'].tolist())
    # get_bboxes
    assert search_head_tag() == (U.HEAD_TAG, U.HEAD_TEST_CFG['nms_pre']), search_head_tag()
    head = ref_head(builder)
    cls, reg = U.head_maps()
    keys = U.maps_to_rows(cls).sigmoid().max(-1)[0].double()
    at, cut = 0, 0
    for n in U.LEVEL_ANCHORS:
        if n > U.HEAD_TEST_CFG['nms_pre']:
            s = keys[:, at:at + n].sort(1, descending=True)[0]
            k = U.HEAD_TEST_CFG['nms_pre']
            gap = float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min())
            print('key gap at the cut', gap)
            assert gap >= GAP
            cut += 1
        at += n
    assert cut >= 2
    with torch.no_grad():
        res = head.get_bboxes(cls, reg, metas, cfg=mg.Config(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores) in enumerate(res):
        assert boxes.size(0) == 2 * U.HEAD_TEST_CFG['nms_pre'] + 20 + 6 + 2
        out[f'head.boxes{i}'], out[f'head.score_rows{i}'] = boxes, scores.double().sum(1)
    # no positive
    cls, reg = [[m.requires_grad_() for m in ms] for ms in U.head_maps()]
    ls = head.loss(cls, reg, [g.new_zeros(0, 4) for g in gts_t], [l.new_zeros(0) for l in labels_t], metas)
    nopos = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_dfl'])])
    nopos.sum().backward()
    assert bool(torch.isfinite(nopos[0])) and bool(torch.isnan(nopos[1:]).all())
    assert all(bool(torch.isnan(m.grad).all()) for m in reg) and all(bool(torch.isfinite(m.grad).all()) for m in cls)
    out['head.nopos.loss'] = nopos.detach()
    print('no positive:', nopos.tolist())


def gen_loss_modules(out):
    gf = mg.ref('mmdet.models.losses.gfocal_loss')
    core = sys.modules['mmdet.core']
    c = U.loss_module_case()
    for i, (reduction, avg, weighted) in enumerate(U.LOSS_MODES):
        for name, mod, pred, target, weight in (
                ('qfl', gf.QualityFocalLoss(beta=2.0, loss_weight=1.5), c['pred'], (c['label'], c['score']), c['weight']),
                ('qfl15', gf.QualityFocalLoss(beta=1.5, loss_weight=1.0), c['pred'], (c['label'], c['score']), c['weight']),
                ('dfl', gf.DistributionFocalLoss(loss_weight=0.25), c['dpred'], c['dlabel'], c['dweight'])):
            x = pred.clone().requires_grad_()
            val = mod(x, target, weight=weight if weighted else None, avg_factor=avg, reduction_override=reduction)
            val.sum().backward()
            out[f'{name}.{i}'], out[f'{name}.{i}.grad'] = val.detach(), x.grad
    pts, box = U.distance_case()
    out['b2d.plain'], out['b2d.max7'] = core.bbox2distance(pts, box), core.bbox2distance(pts, box, max_dis=7)
    assert bool((out['b2d.plain'] < 0).any()) and bool((out['b2d.plain'] > 6.9).any())


def gen_model(out, builder, cls_scale, bias_shift):
    cfg = merged_config('r50')
    model = cfg['model']
    model['pretrained'] = None
    train_cfg, test_cfg = mg.Config(cfg['train_cfg']), mg.Config(cfg['test_cfg'])
    torch.manual_seed(0)
    det = builder.build_detector(model, train_cfg=train_cfg, test_cfg=test_cfg)
    det.init_weights(None)
    U.load_fixture_weights_(det, cls_scale, bias_shift)
    det.train()
    imgs, metas, gts, labels = U.detector_inputs()
    img_t = torch.from_numpy(imgs)
    gts_t, labels_t = [torch.from_numpy(g) for g in gts], [torch.from_numpy(l) for l in labels]
    head = det.bbox_head
    trail = {}
    orig_forward = head.forward

    def rec_forward(feats):
        r = orig_forward(feats)
        trail['outs'] = r
        return r
    head.forward = rec_forward
    losses = det.forward_train(img_t, metas, gts_t, labels_t)
    loss, log_vars = det._parse_losses(losses)
    det.zero_grad()
    loss.backward()
    for k, v in log_vars.items():
        out['loss.' + k] = np.float64(v)
    params = dict(det.named_parameters())
    for k in U.grad_keys(det):
        out[f'grad.{k}.sums'], out[f'grad.{k}.sample'] = BU.digest(params[k].grad)
    cls_scores, bbox_preds = trail['outs']
    assert tuple(tuple(c.shape[-2:]) for c in cls_scores) == U.LEVEL_SIZES
    for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        out[f'cls{l}.sums'], out[f'cls{l}.sample'] = BU.digest(c)
        out[f'reg{l}.sums'], out[f'reg{l}.sample'] = BU.digest(r)
    anchors = ma.ref_anchors(head)
    a32, a64 = ma.ref_assign(head, anchors, gts_t, torch.float32), ma.ref_assign(head, anchors, gts_t, torch.float64)
    assert torch.equal(a32, a64)
    num_pos = (a32 > 0).sum(1)
    assert int(num_pos.min()) > 0, num_pos
    out['assigned'], out['num_pos'] = a32.to(torch.int16), num_pos
    print('positives per image', num_pos.tolist(), 'losses', {k: round(float(v), 5) for k, v in log_vars.items()})

    det.eval()
    with torch.no_grad():
        cls_scores, bbox_preds = head(det.extract_feat(img_t))
    C = head.cls_out_channels
    keys = [c.permute(0, 2, 3, 1).reshape(2, -1, C).sigmoid().max(-1)[0].double() for c in cls_scores]

    def key_gap(k):
        gaps = []
        for lv in keys:
            if lv.size(1) > k:
                s = lv.sort(1, descending=True)[0]
                gaps.append(float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min()))
        return gaps
    for nms_pre in range(79, 20, -1):
        gaps = key_gap(nms_pre)
        if len(gaps) >= 2 and min(gaps) >= GAP:
            break
    else:
        print(f'cls scale {cls_scale}: no nms_pre < 80 leaves a key gap of 1e-3 at every cut')
        return False
    test_cfg.nms_pre = nms_pre
    head.test_cfg = test_cfg
    with torch.no_grad():
        res = det.simple_test(img_t, metas, rescale=False)
        bbox_list = head.get_bboxes(cls_scores, bbox_preds, metas, with_nms=False)
    thr, iou_thr = test_cfg.score_thr, test_cfg.nms['iou_threshold']
    score_gap = min(float(((s[:, :-1].double() - thr).abs() / thr).min()) for _, s in bbox_list)
    iou_gap = 1.0
    for b in range(2):
        d = BU.dets_array(res[b])
        out[f'test_dets{b}'] = d
        if not 0 < len(d) <= test_cfg.max_per_img:
            return False
        for c in np.unique(d[:, 5]):
            rows = d[d[:, 5] == c].astype(np.float64)
            if len(rows) > 1:
                iou = mr.pair_iou(rows, rows)[np.triu_indices(len(rows), 1)]
                assert np.isfinite(iou).all()
                iou_gap = min(iou_gap, float((np.abs(iou - iou_thr) / iou_thr).min()))
    print(f'scale {cls_scale} shift {bias_shift} nms_pre {nms_pre}: key gaps {gaps}, score gap {score_gap:.3e}, IoU gap {iou_gap:.3e}, detections',
          [len(out[f'test_dets{b}']) for b in range(2)])
    if not (min(gaps) >= GAP and score_gap >= GAP and iou_gap >= GAP and min(len(out[f'test_dets{b}']) for b in range(2)) >= 10):
        return False
    out['nms_pre'] = np.array(nms_pre)
    out['margin.key'], out['margin.score'], out['margin.iou'] = np.array(min(gaps)), np.array(score_gap), np.array(iou_gap)
    sd = det.state_dict()
    assert 'bbox_head.integral.project' in sd
    out['state_keys'] = np.array(list(sd.keys()))
    out['state_shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    out['cls_scale'], out['cls_bias_shift'] = np.array(cls_scale), np.array(bias_shift)
    return True


def main():
    torch.set_num_threads(8)
    mg.install_mmcv_standin()
    mg.install_reference_namespace()
    for m in ('mmdet.models.losses', ):
        mg.ref(m)
    ma.extend_standin()
    for m in ('mmdet.models.backbones.resnet', 'mmdet.models.necks.fpn', 'mmdet.models.dense_heads.anchor_head',
              'mmdet.models.dense_heads.gfl_head', 'mmdet.models.detectors.base', 'mmdet.models.detectors.single_stage',
              'mmdet.models.detectors.gfl'):
        mg.ref(m)
    gen_configs()
    builder = mg.ref('mmdet.models.builder')
    out = {}
    gen_loss_modules(out)
    gen_heads(out, builder)
    for shift, scale in ((sh, sc) for sh in SHIFTS for sc in SCALES):
        model_out = {}
        if gen_model(model_out, builder, scale, shift):
            break
    else:
        raise AssertionError('no scale and bias shift of the classification layer gives the margins')
    out.update(model_out)
    mg.npz('gfl', **out)


if __name__ == '__main__':
    main()
