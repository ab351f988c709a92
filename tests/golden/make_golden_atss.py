#!/usr/bin/env python3
"""Generate tests/golden/atss.npz and the two atss_r*_fpn_1x_coco_cfg.json by running the REFERENCE's own ATSS (detectors/atss.py,
dense_heads/atss_head.py, anchor_head.py, core/bbox/assigners/atss_assigner.py, losses/iou_loss.py, focal_loss.py, necks/fpn.py ...)
on the CPU (authoring container only, like make_golden_fcos.py; make_golden's mmcv stand-in and reference namespace are imported and
left as they are).  The stand-in gains what FCOS's script adds, a reduce_mean that is the identity (one process) and a Tensor.cuda
that stays on the CPU (ATSSHead.loss moves a count to the device by name).  Only data is stored; weights and inputs are re-created
from seeds by atss_util.

On atss_util.detector_inputs() (2 x 128 x 160, the boxes of baselines_util.detector_inputs() scaled in x; levels (16,20) (8,10) (4,5) (2,3) (1,2): the last two hold fewer than topk = 9):
  loss.*                        the log variables of forward_train
  grad.{key}.sums / .sample     digests (baselines_util.digest) of the gradients atss_util.grad_keys lists
  cls{l}.* / reg{l}.* / ctr{l}.*  digests of the three per-level outputs of the training forward
  assigned                      (2, A) int16: 0 background, k + 1 = gt k;  num_pos (2,)
  test_dets{b}                  detections (x1, y1, x2, y2, score, class) of image b;  nms_pre the cut the test config was given
  state_keys / state_shapes     the state-dict keys and their shapes (padded to 4 dims with 0)
  margin.key / .score / .iou    the relative gaps asserted below;  cls_scale / cls_bias_shift the figures of load_fixture_weights_
Head level, variant v of atss_util.HEAD_VARIANTS on atss_util.head_maps() and the same gts, the reference in fp64 and fp32:
  head.{v}.loss64 / .loss32     [loss_cls, loss_bbox, loss_centerness]
  head.{v}.greg64 / .gctr64     (2, A, 4) / (2, A) gradients of the deltas and centerness logits, level-major
  head.{v}.gcls64.sums / .sample  digest of the (2, A, 80) gradient of the logits
  head.{v}.err32                |fp32 - fp64| of the reference's own runs: [3 losses, max over gcls, greg, gctr]
  head.assigned / .ctr_targets / .ltrb   (2, A) int16, (2, A), (2, A, 4): ATSSAssigner.assign, centerness_target and its
                                l, t, r, b (fp32; targets 0 and l, t, r, b 1 where the anchor is background)
  head.boxes{b} / .score_rows{b} / .ctrs{b}   get_bboxes(with_nms=False) of image b under atss_util.HEAD_TEST_CFG on the same
                                maps: decoded boxes, row sums of the scores (fp64) and centerness after the nms_pre cut
Assignment case (atss_util.assignment_case(), 4 images):  ac.assigned (4, A) int16.
Identical gts (atss_util.twin_case()):  twin.assigned (1, A) int16 and twin.ref_lower: whether the reference gave the shared
positives to the lower index.
Cases on pyramids of their own (atss_util.EXTRA_CASES):  x.equal.assigned (1, 2) (IoU equal to the threshold: positive) and
x.std.assigned (1, 3) (positive under the biased deviation only: none).

Asserted here (GAP = 1e-3 relative), the conditions under which exact equality of `assigned` is a fair demand: the reference's
fp32 and fp64 runs make the same assignment everywhere; on every (gt, level) with more anchors than topk the distances of the
topk-th and the next anchor differ by GAP; every candidate's IoU is GAP away from its gt's threshold and its min(l, t, r, b) GAP
away from 0.01; where an anchor is positive for two distinct gts their IoUs differ by GAP; every image of the detector run has a
positive; every level has one in the assignment case, whose named cases are checked one by one; the logarithms and exponentials of
the delta coding of every positive of the head case are the correctly rounded ones (so a kernel with correctly rounded functions
can reproduce the centerness targets bit for bit); the nms_pre cut bites on two levels; key, score and IoU gaps of the test
detections as in make_golden_fcos.py.

Usage:  python tests/golden/make_golden_atss.py
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
import make_golden_fcos as mf  # noqa: E402
import baselines_util as BU  # noqa: E402
import atss_util as U  # noqa: E402

GAP = 1e-3
SCALES = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2)
SHIFTS = (3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0)


def extend_standin():
    mf.extend_standin()
    sys.modules['mmdet.core'].reduce_mean = lambda t: t           # dist_utils.reduce_mean without a process group
    torch.Tensor.cuda = lambda self, *a, **k: self


def merged_config(which):
    from htd_amd import Config
    cfg = Config.fromfile(os.path.join(mg.REF, U.CONFIGS[which]))
    return {k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in U.CFG_KEYS}


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


def ref_anchors(head):
    lv = head.anchor_generator.grid_anchors(U.LEVEL_SIZES, 'cpu')
    assert [a.size(0) for a in lv] == list(U.LEVEL_ANCHORS)
    flat = torch.cat(lv)
    assert torch.equal(flat, U.anchors_of())
    return flat


def ref_assign(head, anchors, gts_list, dtype, level_anchors=U.LEVEL_ANCHORS):
    """ATSSAssigner.assign of the reference, image by image -> (B, A) int64."""
    out = []
    for g in gts_list:
        r = head.assigner.assign(anchors.to(dtype), list(level_anchors), g.to(dtype), None, None)
        out.append(r.gt_inds.clone())
    return torch.stack(out)


def check_margins(anchors, gts_list, what, skip_kth=(), level_anchors=U.LEVEL_ANCHORS):
    """The gaps of the docstring, in fp64.  skip_kth: (image, gt) pairs whose k-th place may tie."""
    a = anchors.double()
    acx, acy = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2
    worst = dict(kth=np.inf, thr=np.inf, inside=np.inf, pair=np.inf)
    for b, gts in enumerate(gts_list):
        pos_iou = {}
        for k, g in enumerate(gts.double()):
            gcx, gcy = (g[0] + g[2]) / 2, (g[1] + g[3]) / 2
            dist = ((acx - gcx) ** 2 + (acy - gcy) ** 2).sqrt()
            cand, start = [], 0
            for n in level_anchors:
                d, order = dist[start:start + n].sort(stable=True)
                kk = min(U.TOPK, n)
                if n > kk and (b, k) not in skip_kth:
                    worst['kth'] = min(worst['kth'], float((d[kk] - d[kk - 1]) / d[kk]))
                cand.append(order[:kk] + start)
                start += n
            cand = torch.cat(cand)
            ious = mr.pair_iou(a[cand].numpy(), g[None].numpy())[:, 0]
            ious = torch.from_numpy(ious)
            thr = ious.mean() + ious.std()
            worst['thr'] = min(worst['thr'], float(((ious - thr).abs() / thr.clamp(min=1e-12)).min()))
            inside = torch.stack([acx[cand] - g[0], acy[cand] - g[1], g[2] - acx[cand], g[3] - acy[cand]]).min(0)[0]
            worst['inside'] = min(worst['inside'], float(((inside - 0.01).abs() / 0.01).min()))
            for i, iou, ins in zip(cand.tolist(), ious.tolist(), inside.tolist()):
                if iou >= float(thr) and ins > 0.01:
                    pos_iou.setdefault(i, []).append((iou, k))
        for i, lst in pos_iou.items():
            for x in range(len(lst)):
                for y in range(x + 1, len(lst)):
                    if not torch.equal(gts[lst[x][1]], gts[lst[y][1]]):
                        worst['pair'] = min(worst['pair'], abs(lst[x][0] - lst[y][0]) / max(lst[x][0], lst[y][0]))
    print(f'{what}: margins', {k: (round(v, 5) if np.isfinite(v) else v) for k, v in worst.items()})
    assert min(worst.values()) >= GAP, (what, worst)


def gen_assignment_case(out, builder):
    head = ref_head(builder)
    anchors = ref_anchors(head)
    gts, _ = U.assignment_case()
    check_margins(anchors, gts, 'assignment case')
    a32, a64 = ref_assign(head, anchors, gts, torch.float32), ref_assign(head, anchors, gts, torch.float64)
    assert torch.equal(a32, a64)
    out['ac.assigned'] = a32.to(torch.int16)
    lvl = torch.cat([torch.full((n, ), l) for l, n in enumerate(U.LEVEL_ANCHORS)])
    pos = a32 > 0
    per_level = [int(pos[:, lvl == l].sum()) for l in range(5)]
    print('assignment case: positives per level', per_level, 'per image', pos.sum(1).tolist(),
          'per gt of image 0', [int((a32[0] == k + 1).sum()) for k in range(len(gts[0]))])
    assert min(per_level) > 0 and int(pos[2].sum()) == 0
    # the named cases
    acx, acy = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2
    g = gts[0]
    assert float((g[0, 0] + g[0, 2]) / 2) == 0.0 and float((g[0, 1] + g[0, 3]) / 2) == 0.0       # the corner node (0, 0)
    assert float((g[1, 1] + g[1, 3]) / 2) > float(acy[:320].max())                              # beyond the last anchor row
    shared = ((a32[0] == 3) | (a32[0] == 4)).sum()
    assert int((a32[0] == 3).sum()) > 0 and int((a32[0] == 4).sum()) > 0 and int(shared) > 0
    assert int((a32[0] == 5).sum()) == 0                                                       # too small for any centre
    assert float((g[5, 0] + g[5, 2]) / 2) == 64.0 and float((g[5, 1] + g[5, 3]) / 2) == 64.0
    far = gts[1][0]
    for l, (s, n) in enumerate(zip((0, 320, 400), (320, 80, 20))):
        assert float(mr.pair_iou(anchors[s:s + n].double().numpy(), far[None].double().numpy()).max()) == 0.0
    tg, _ = U.twin_case()
    check_margins(anchors, tg, 'twin case')
    t32, t64 = ref_assign(head, anchors, tg, torch.float32), ref_assign(head, anchors, tg, torch.float64)
    assert torch.equal(t32, t64)
    out['twin.assigned'] = t32.to(torch.int16)
    lower = int((t32 == 2).sum()) == 0 and int((t32 == 1).sum()) > 0
    out['twin.ref_lower'] = np.array(lower)
    print('twin case: the reference gave the shared positives to the', 'lower' if lower else 'higher (or both)', 'index:',
          [int((t32 == k).sum()) for k in (1, 2, 3)])


def gen_extra_cases(out, builder):
    head = ref_head(builder)
    for name, (sizes, strides, gts) in U.EXTRA_CASES.items():
        anchors = U.anchors_of(sizes, strides)
        counts = [h * w for h, w in sizes]
        if name != 'equal':                     # (there the equality of IoU and threshold is the point: the same fp32 value)
            check_margins(anchors, [gts], name + ' case', level_anchors=counts)
        a32, a64 = (ref_assign(head, anchors, [gts], dt, counts) for dt in (torch.float32, torch.float64))
        assert torch.equal(a32, a64)
        out[f'x.{name}.assigned'] = a32.to(torch.int16)
        print(f'{name} case: the reference assigns', a32.tolist())
    assert out['x.equal.assigned'].tolist() == [[1, 1]] and out['x.std.assigned'].tolist() == [[0, 0, 0]]
    sizes, strides, gts = U.EXTRA_CASES['std']
    ious = torch.from_numpy(mr.pair_iou(U.anchors_of(sizes, strides).double().numpy(), gts.double().numpy())[:, 0])
    assert float(ious.max()) >= float(ious.mean() + ious.std(unbiased=False)) * (1 + GAP)      # the biased deviation would assign it


def gen_heads(out, builder):
    _, metas, gts, labels = U.detector_inputs()
    gts_t, labels_t = [torch.from_numpy(g) for g in gts], [torch.from_numpy(l) for l in labels]
    head = ref_head(builder)
    anchors = ref_anchors(head)
    check_margins(anchors, gts_t, 'head case')
    a32, a64 = ref_assign(head, anchors, gts_t, torch.float32), ref_assign(head, anchors, gts_t, torch.float64)
    assert torch.equal(a32, a64) and int((a32 > 0).sum(1).min()) > 0
    padded, _, _ = U.pad_gts(gts_t)
    ltrb = U.batch_ltrb(anchors, padded, a32)
    pos = a32 > 0
    b, i = pos.nonzero(as_tuple=True)
    ref_ctr = head.centerness_target(anchors[i], head.bbox_coder.encode(anchors[i], padded[b, a32[pos] - 1]))
    ctr = torch.zeros(a32.shape)
    ctr[pos] = ref_ctr
    assert torch.equal(U.centerness_of(ltrb)[pos], ref_ctr)         # the restatement is the reference's arithmetic
    exact = torch.equal(U.batch_ltrb(anchors, padded, a32, rounded=True), ltrb)
    print('head case: positives', pos.sum(1).tolist(), '; logarithms and exponentials correctly rounded on all of them:', exact)
    assert exact
    out['head.assigned'], out['head.ctr_targets'], out['head.ltrb'] = a32.to(torch.int16), ctr, ltrb
    for v in U.HEAD_VARIANTS:
        head = ref_head(builder, v)
        res = {}
        for dt in (torch.float64, torch.float32):
            maps = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps(v)]
            ls = head.loss(*maps, [g.to(dt) for g in gts_t], labels_t, metas)
            losses = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])])
            losses.sum().backward()
            res[dt] = dict(loss=losses.detach(), g=[U.maps_to_rows([m.grad for m in ms]) for ms in maps])
            assert all(torch.isfinite(g).all() for g in res[dt]['g']) and torch.isfinite(losses).all()
        a, b32 = res[torch.float64], res[torch.float32]
        p = f'head.{v}.'
        out[p + 'loss64'], out[p + 'loss32'] = a['loss'], b32['loss']
        out[p + 'gcls64.sums'], out[p + 'gcls64.sample'] = BU.digest(a['g'][0])
        out[p + 'greg64'], out[p + 'gctr64'] = a['g'][1], a['g'][2][..., 0]
        out[p + 'err32'] = torch.cat([(b32['loss'].double() - a['loss']).abs()] +
                                     [(gb.double() - ga).abs().max()[None] for ga, gb in zip(a['g'], b32['g'])])
        print(f'head {v}: loss64', a['loss'].tolist(), 'err32', out[p + 'err32'].tolist())
    cls, reg, ctrm = U.head_maps()
    keys = (U.maps_to_rows(cls).sigmoid() * U.maps_to_rows(ctrm).sigmoid()).max(-1)[0].double()
    at, cut = 0, 0
    for n in U.LEVEL_ANCHORS:
        if n > U.HEAD_TEST_CFG['nms_pre']:
            s = keys[:, at:at + n].sort(1, descending=True)[0]
            k = U.HEAD_TEST_CFG['nms_pre']
            assert float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min()) >= GAP
            cut += 1
        at += n
    assert cut >= 2
    with torch.no_grad():
        res = head.get_bboxes(cls, reg, ctrm, metas, cfg=mg.Config(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores, ctrs) in enumerate(res):
        assert boxes.size(0) == 2 * U.HEAD_TEST_CFG['nms_pre'] + 20 + 6 + 2
        out[f'head.boxes{i}'], out[f'head.score_rows{i}'], out[f'head.ctrs{i}'] = boxes, scores.double().sum(1), ctrs


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
    cls_scores, bbox_preds, centernesses = trail['outs']
    assert tuple(tuple(c.shape[-2:]) for c in cls_scores) == U.LEVEL_SIZES
    for l, (c, r, t) in enumerate(zip(cls_scores, bbox_preds, centernesses)):
        out[f'cls{l}.sums'], out[f'cls{l}.sample'] = BU.digest(c)
        out[f'reg{l}.sums'], out[f'reg{l}.sample'] = BU.digest(r)
        out[f'ctr{l}.sums'], out[f'ctr{l}.sample'] = BU.digest(t)
    anchors = ref_anchors(head)
    a32, a64 = ref_assign(head, anchors, gts_t, torch.float32), ref_assign(head, anchors, gts_t, torch.float64)
    assert torch.equal(a32, a64)
    num_pos = (a32 > 0).sum(1)
    assert int(num_pos.min()) > 0, num_pos
    out['assigned'], out['num_pos'] = a32.to(torch.int16), num_pos
    print('positives per image', num_pos.tolist(), 'losses', {k: round(float(v), 5) for k, v in log_vars.items()})

    det.eval()
    with torch.no_grad():
        cls_scores, bbox_preds, centernesses = head(det.extract_feat(img_t))
    C = head.cls_out_channels
    keys = [(c.permute(0, 2, 3, 1).reshape(2, -1, C).sigmoid() * t.permute(0, 2, 3, 1).reshape(2, -1, 1).sigmoid()).max(-1)[0].double()
            for c, t in zip(cls_scores, centernesses)]

    def key_gap(k):
        gaps = []
        for lvl in keys:
            if lvl.size(1) > k:
                s = lvl.sort(1, descending=True)[0]
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
        bbox_list = head.get_bboxes(cls_scores, bbox_preds, centernesses, metas, with_nms=False)
    thr, iou_thr = test_cfg.score_thr, test_cfg.nms['iou_threshold']
    score_gap = min(float(((s[:, :-1].double() - thr).abs() / thr).min()) for _, s, _ in bbox_list)
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
    extend_standin()
    for m in ('mmdet.models.backbones.resnet', 'mmdet.models.necks.fpn', 'mmdet.models.dense_heads.anchor_head',
              'mmdet.models.dense_heads.atss_head', 'mmdet.models.detectors.base', 'mmdet.models.detectors.single_stage',
              'mmdet.models.detectors.atss'):
        mg.ref(m)
    gen_configs()
    builder = mg.ref('mmdet.models.builder')
    out = {}
    gen_assignment_case(out, builder)
    gen_extra_cases(out, builder)
    gen_heads(out, builder)
    for shift, scale in ((sh, sc) for sh in SHIFTS for sc in SCALES):
        model_out = {}
        if gen_model(model_out, builder, scale, shift):
            break
    else:
        raise AssertionError('no scale and bias shift of the classification layer gives the margins')
    out.update(model_out)
    mg.npz('atss', **out)


if __name__ == '__main__':
    main()
