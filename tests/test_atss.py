"""ATSS without a GPU: the configs against the reference's merged configs, the state dict, ATSSAssigner.assign and the tensor form of
batched_atss_assign against the reference's own assignment on every case of the fixture (tests/golden/atss.npz, recipe in
tests/golden/make_golden_atss.py), the tensor-path loss and the per-image get_bboxes against the reference's own run, the
inside-flag subset, reduce_mean under gloo, and the new entry points of the C ABI."""
import json
import os
import socket

import numpy as np
import pytest
import torch

import atss_util as U
import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def build_head(variant='giou', **extra):
    from htd_amd.registry import ConfigDict, build_head as build
    import htd_amd.detector  # noqa: F401
    train_cfg = dict(U.TRAIN_CFG)
    train_cfg.update(extra.pop('train_cfg', {}))
    return build(dict(U.head_cfg(variant, **extra), train_cfg=ConfigDict(train_cfg)))


def inputs():
    return D.inputs('cpu', U.detector_inputs)[1:]


@pytest.mark.parametrize('which,depth', [('r50', 50), ('r101', 101)])
def test_atss_config_equals_the_reference_merged_config(which, depth):
    from htd_amd.apis import check_supported
    from htd_amd.configs import atss_config
    ref = json.load(open(os.path.join(GOLDEN, os.path.basename(U.CONFIGS[which])[:-3] + '_cfg.json')))
    cfg = atss_config(depth)
    mine = json.loads(json.dumps({k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in U.CFG_KEYS}))
    assert mine == ref
    check_supported(cfg)                        # no grad_clip, a linear warm-up: the train CLI takes it as it is
    with pytest.raises(ValueError):
        atss_config(34)


def test_state_dict_keys_and_shapes_equal_the_fixture(golden):
    from htd_amd.configs import build_baseline_detector
    from htd_amd.detector.anchor_free_heads import Scale
    from htd_amd.registry import BBOX_ASSIGNERS, DETECTORS, HEADS
    g = golden('atss')
    det = build_baseline_detector('atss')
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_keys']]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == g['state_shapes'].tolist()
    head = det.bbox_head
    assert type(det) is DETECTORS.get('ATSS') and type(head) is HEADS.get('ATSSHead')
    assert type(head.assigner) is BBOX_ASSIGNERS.get('ATSSAssigner') and head.assigner.topk == 9
    assert all(type(s) is Scale and float(s.scale.detach()) == 1.0 for s in head.scales) and len(head.scales) == 5
    assert torch.allclose(head.atss_cls.bias.sigmoid(), torch.full_like(head.atss_cls.bias, 0.01))
    assert head.num_anchors == 1 and not head.sampling and head.cls_convs[0].conv.bias is None
    for k in ('cls_convs.0.conv.weight', 'reg_convs.3.gn.bias', 'atss_cls.bias', 'atss_reg.weight', 'atss_centerness.bias',
              'scales.4.scale'):
        assert 'bbox_head.' + k in sd
    anchors = torch.cat(head.anchor_generator.grid_anchors(U.LEVEL_SIZES, 'cpu'))
    assert torch.equal(anchors, U.anchors_of())


def _cases(g):
    """(name, gts list, the reference's assigned or None) of every assignment case of the fixture."""
    _, gts, _ = inputs()
    ac, _ = U.assignment_case()
    twin, _ = U.twin_case()
    tie, _ = U.tie_case()
    return [('head', gts, T(g['head.assigned']).long()), ('detector', gts, T(g['assigned']).long()),
            ('assignment', ac, T(g['ac.assigned']).long()),
            ('twin', twin, T(g['twin.assigned']).long() if bool(g['twin.ref_lower']) else None), ('tie', tie, None)]


def test_assigner_forms_equal_the_reference_assignment(golden):
    """ATSSAssigner.assign in fp64 and fp32 and the tensor form of batched_atss_assign (fp32, and with K padded) equal the
    reference's assignment on every case; the identical gts go to the lower index; where anchors tie around the ninth place the
    forms agree with each other and take the lower anchor index."""
    from htd_amd.core.bbox import ATSSAssigner, _batched_atss_assign_tensor, batched_atss_assign
    g = golden('atss')
    a = ATSSAssigner(topk=U.TOPK)
    anchors = U.anchors_of()
    sizes = list(U.LEVEL_ANCHORS)
    for name, gts, ref in _cases(g):
        per = {dt: torch.stack([a.assign(anchors.to(dt), sizes, x.to(dt)).gt_inds for x in gts]) for dt in (torch.float64, torch.float32)}
        assert torch.equal(per[torch.float64], per[torch.float32]), name
        padded, valid, _ = U.pad_gts(gts)
        bat = batched_atss_assign(a, anchors, sizes, padded, valid)
        wide, wvalid, _ = U.pad_gts(gts, K=padded.size(1) + 3)
        assert torch.equal(bat, _batched_atss_assign_tensor(a, anchors, sizes, wide, wvalid)), name
        assert torch.equal(bat.long(), per[torch.float64]), name
        if ref is not None:
            assert torch.equal(bat.long(), ref), name
        assert int((bat > 0).sum()) > 0
    twin = torch.stack([a.assign(anchors.double(), sizes, x.double()).gt_inds for x in U.twin_case()[0]])
    assert int((twin == 1).sum()) > 0 and int((twin == 2).sum()) == 0
    # the tie: on level 0 the ninth and tenth nearest anchors of a gt centred at (68, 64) lie at the same distance; the lower
    # anchor index is the candidate
    gt = U.tie_case()[0][0]
    cx, cy = (anchors[:320, 0] + anchors[:320, 2]).double() / 2, (anchors[:320, 1] + anchors[:320, 3]).double() / 2
    d, order = ((cx - 68.) ** 2 + (cy - 64.) ** 2).sqrt().sort(stable=True)
    assert float(d[8]) == float(d[9]) and int(order[8]) < int(order[9])
    res = a.assign(anchors.double(), sizes, gt.double(), gt_labels=torch.tensor([4]))
    assert int((res.labels == 4).sum()) == int((res.gt_inds == 1).sum()) > 0 and int((res.labels == -1).sum()) == int((res.gt_inds == 0).sum())
    # an image without gt, and the ignore branch: anchors mostly inside an ignore box are marked -1 and are no candidates
    none = a.assign(anchors, sizes, torch.zeros(0, 4), gt_labels=torch.zeros(0, dtype=torch.long))
    assert int(none.gt_inds.abs().sum()) == 0 and int((none.labels != -1).sum()) == 0
    ig = ATSSAssigner(topk=U.TOPK, ignore_iof_thr=0.5)
    r = ig.assign(anchors, sizes, gt, gt_bboxes_ignore=torch.tensor([[0., 0., 80., 80.]]))
    iof = (anchors[:, 2].clamp(max=80) - anchors[:, 0].clamp(min=0)).clamp(min=0) * \
        (anchors[:, 3].clamp(max=80) - anchors[:, 1].clamp(min=0)).clamp(min=0) / ((anchors[:, 2] - anchors[:, 0]) ** 2)
    assert int((iof > 0.5).sum()) > 0 and torch.equal(r.gt_inds == -1, iof > 0.5)


def test_threshold_cases_equal_the_reference(golden):
    """An IoU equal to the threshold is positive (`>=`), and the deviation is the unbiased one: the largest IoU of the 'std' case
    lies between mean + biased and mean + unbiased deviation and stays background, as in the reference."""
    from htd_amd.core.bbox import ATSSAssigner, batched_atss_assign
    g = golden('atss')
    a = ATSSAssigner(topk=U.TOPK)
    for name, (sizes, strides, gts) in U.EXTRA_CASES.items():
        anchors, counts = U.anchors_of(sizes, strides), [h * w for h, w in sizes]
        ref = T(g[f'x.{name}.assigned']).long()
        assert ref.tolist() == dict(equal=[[1, 1]], std=[[0, 0, 0]])[name]
        for dt in (torch.float64, torch.float32):
            assert torch.equal(a.assign(anchors.to(dt), counts, gts.to(dt)).gt_inds[None], ref), (name, dt)
        assert torch.equal(batched_atss_assign(a, anchors, counts, gts[None], torch.ones(1, 1, dtype=torch.bool)), ref), name


def test_single_candidate_gives_no_positive():
    """One level of one anchor: the unbiased deviation of a single IoU is NaN, so the gt gets no positive, as in the reference."""
    from htd_amd.core.bbox import ATSSAssigner, batched_atss_assign
    a = ATSSAssigner(topk=9)
    anchors = torch.tensor([[0., 0., 64., 64.]])
    gt = torch.tensor([[8., 8., 60., 60.]])
    assert int(a.assign(anchors, [1], gt).gt_inds.sum()) == 0
    assert int(batched_atss_assign(a, anchors, [1], gt[None], torch.ones(1, 1, dtype=torch.bool)).sum()) == 0


def head_targets(head, gts):
    """The head's own targets -> assigned (B, A) and centerness targets (B, A), fp32."""
    anchors = torch.cat(head.anchor_generator.grid_anchors(U.LEVEL_SIZES, 'cpu'))
    assigned = torch.stack([head.assigner.assign(anchors, list(U.LEVEL_ANCHORS), x).gt_inds for x in gts])
    padded, _, _ = U.pad_gts(gts)
    pos = assigned > 0
    b, i = pos.nonzero(as_tuple=True)
    ctr = torch.zeros(assigned.shape)
    ctr[pos] = head.centerness_target(anchors[i], head.bbox_coder.encode(anchors[i], padded[b, assigned[pos] - 1]))
    return assigned, ctr


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_tensor_path_loss_on_the_cpu_matches_the_reference(golden, v):
    """ATSSHead.loss (tensor path) on the seeded maps against the reference head's own result: the assignment exactly, the
    centerness targets to an fp32 ulp of their l, t, r, b (logarithm and exponential are the machine's), losses and gradients in
    fp64 to 1e-10, fp32 within 4 x the reference's own fp32 error.

    The box targets of the fp64 run are fp32 too (bbox2delta casts), through torch's vectorised fp32 log, whose last bit depends on
    the instruction set torch dispatches to.  The fixture was made on an AVX2 host, where this test passes; on an AVX-512 host
    loss_bbox alone missed the 1e-10 by a factor of 4.9 (giou: 6.4e-10 absolute of 1.328; iou: 4.6e-10 of 0.941), the size of one
    fp32 ulp in one of the box targets (supposed from the figures, not taken apart).  The bound stays."""
    g = golden('atss')
    p = f'head.{v}.'
    metas, gts, labels = inputs()
    head = build_head(v)
    assigned, ctr = head_targets(head, gts)
    assert torch.equal(assigned, T(g['head.assigned']).long())
    np.testing.assert_allclose(ctr.numpy(), g['head.ctr_targets'], rtol=1e-5, atol=0)
    padded, _, _ = U.pad_gts(gts)
    ltrb = U.batch_ltrb(U.anchors_of(), padded, assigned)
    np.testing.assert_allclose(ltrb.numpy(), g['head.ltrb'], rtol=0, atol=2e-5)
    np.testing.assert_allclose(U.centerness_of(ltrb).numpy()[assigned > 0], ctr.numpy()[assigned > 0], rtol=1e-6)
    err = g[p + 'err32']
    for dt in (torch.float64, torch.float32):
        maps = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        assert not head._fused_loss_ok(*maps, labels, None, metas)
        ls = head.loss(*maps, [x.to(dt) for x in gts], labels, metas)
        assert set(ls) == {'loss_cls', 'loss_bbox', 'loss_centerness'} and all(len(x) == 5 for x in ls.values())
        mine = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])])
        mine.sum().backward()
        grads = [U.maps_to_rows([m.grad for m in ms]) for ms in maps]
        if dt == torch.float64:
            np.testing.assert_allclose(mine.detach().numpy(), g[p + 'loss64'], rtol=1e-10)
            np.testing.assert_allclose(grads[1].numpy(), g[p + 'greg64'], rtol=1e-10, atol=1e-15)
            np.testing.assert_allclose(grads[2][..., 0].numpy(), g[p + 'gctr64'], rtol=1e-10, atol=1e-15)
            sums, sample = BU.digest(grads[0])
            np.testing.assert_allclose(sums, g[p + 'gcls64.sums'], rtol=1e-10)
            np.testing.assert_allclose(sample, g[p + 'gcls64.sample'], rtol=1e-10, atol=1e-15)
        else:
            for i in range(3):
                assert abs(float(mine[i].detach()) - float(g[p + 'loss64'][i])) <= 4 * max(float(err[i]), 2.0 ** -23 * float(g[p + 'loss64'][i]))
            for grad, want, e in ((grads[1], g[p + 'greg64'], err[4]), (grads[2][..., 0], g[p + 'gctr64'], err[5])):
                assert float((grad.double() - T(want)).abs().max()) <= 4 * max(float(e), 2.0 ** -23 * float(np.abs(want).max()))


def test_allowed_border_subset_equals_a_direct_restatement():
    """allowed_border = 0 removes the anchors that reach past the image: the assignment runs on the subset with the per-level
    counts of get_num_level_anchors_inside, and the loss equals the same head's loss terms written directly on that subset."""
    from htd_amd.core import anchor_inside_flags
    metas, gts, labels = inputs()
    head = build_head('giou', train_cfg=dict(allowed_border=0))
    anchors = U.anchors_of()
    maps = [[m.double().requires_grad_() for m in ms] for ms in U.head_maps()]
    ls = head.loss_tensor(*maps, [x.double() for x in gts], labels, metas)
    mine = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])])
    rows = [U.maps_to_rows([m.detach() for m in ms]) for ms in maps]
    tot_cls, tot_box, tot_ctr, npos, wsum, kept_levels = 0., 0., 0., 0, 0., None
    per_image = []
    for b in range(2):
        inside = anchor_inside_flags(anchors, torch.ones(anchors.size(0), dtype=torch.bool), metas[b]['img_shape'][:2], 0)
        counts = head.get_num_level_anchors_inside(list(U.LEVEL_ANCHORS), inside)
        assert sum(counts) == int(inside.sum()) < anchors.size(0) and counts[0] < U.LEVEL_ANCHORS[0]
        kept_levels = counts
        r = head.assigner.assign(anchors[inside], counts, gts[b].double(), None, labels[b])
        full = torch.zeros(anchors.size(0), dtype=torch.long)
        full[inside] = r.gt_inds
        per_image.append((inside, full))
        npos += max(int((full > 0).sum()), 1)
    assert kept_levels is not None and sum(int((f > 0).sum()) for _, f in per_image) > 0
    for b, (inside, full) in enumerate(per_image):
        lab = torch.full((anchors.size(0), ), 80, dtype=torch.long)
        pos = full > 0
        lab[pos] = labels[b][full[pos] - 1]
        w = inside.double()
        tot_cls = tot_cls + head.loss_cls(rows[0][b], lab, w, avg_factor=float(npos))
        if bool(pos.any()):
            t = head.bbox_coder.encode(anchors[pos], gts[b][full[pos] - 1])
            c = head.centerness_target(anchors[pos], t)
            tot_box = tot_box + head.loss_bbox(head.bbox_coder.decode(anchors[pos], rows[1][b][pos]), head.bbox_coder.decode(anchors[pos], t),
                                               weight=c, avg_factor=1.0)
            tot_ctr = tot_ctr + head.loss_centerness(rows[2][b][pos, 0], c, avg_factor=float(npos))
            wsum += float(c.sum())
    np.testing.assert_allclose(float(mine[0]), float(tot_cls), rtol=1e-12)
    np.testing.assert_allclose(float(mine[1]), float(tot_box) / wsum, rtol=1e-6)
    np.testing.assert_allclose(float(mine[2]), float(tot_ctr), rtol=1e-6)
    whole = build_head('giou').loss_tensor(*[[m.detach() for m in ms] for ms in maps], [x.double() for x in gts], labels, metas)
    assert abs(float(sum(whole['loss_bbox'])) - float(mine[1])) > 1e-6      # the border does remove positives' competitors


def test_no_positive_batch_gives_zero_box_and_centerness_losses():
    metas, gts, labels = inputs()
    head = build_head('giou')
    maps = [[m.double().requires_grad_() for m in ms] for ms in U.head_maps()]
    ls = head.loss(*maps, [x.new_zeros(0, 4).double() for x in gts], [x.new_zeros(0) for x in labels], metas)
    total = sum(ls['loss_cls']) + sum(ls['loss_bbox']) + sum(ls['loss_centerness'])
    assert float(sum(ls['loss_bbox'])) == 0 and float(sum(ls['loss_centerness'])) == 0 and float(sum(ls['loss_cls'])) > 0
    total.backward()
    assert all(float(m.grad.abs().max()) == 0 for ms in maps[1:] for m in ms)
    assert all(torch.isfinite(m.grad).all() for m in maps[0])


def test_per_image_get_bboxes_on_the_cpu_matches_the_reference(golden):
    """The nms_pre cut (biting on levels 0 and 1) by max_c sigmoid(cls) * sigmoid(centerness), the coder's decode clamped to the
    image, the scores with their background column and the centerness: the reference's own output before the NMS."""
    from htd_amd.registry import ConfigDict
    g = golden('atss')
    metas, _, _ = inputs()
    head = build_head('giou')
    res = head.get_bboxes(*U.head_maps(), metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores, ctrs) in enumerate(res):
        assert scores.shape == (boxes.size(0), 81) and float(scores[:, -1].abs().max()) == 0
        np.testing.assert_allclose(boxes.numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-4)       # (exp is the machine's)
        np.testing.assert_array_equal(ctrs.numpy(), g[f'head.ctrs{i}'])
        np.testing.assert_allclose(scores.double().sum(1).numpy(), g[f'head.score_rows{i}'], rtol=1e-12)
        assert float(boxes[:, [0, 2]].max()) <= metas[i]['img_shape'][1] and float(boxes.min()) >= 0


def test_dispatch_rule_and_shared_get_bboxes_code():
    from htd_amd.detector.anchor_free_heads import FCOSHead
    from htd_amd.detector.anchor_heads import ATSSHead, GFLHead, RetinaHead
    from htd_amd.detector.base_dense_head import BaseDenseHead
    from htd_amd.detector.fovea_head import FoveaHead
    from htd_amd.detector.vfnet_head import VFNetHead
    metas, gts, labels = inputs()
    head = build_head('giou')
    assert not head._fused_loss_ok(*U.head_maps(), labels, None, metas)            # CPU maps
    shared = ('_get_bboxes', '_get_bboxes_single', '_get_bboxes_batched')
    assert all(name in vars(BaseDenseHead) for name in shared)
    for cls in (RetinaHead, FCOSHead, ATSSHead, GFLHead, VFNetHead, FoveaHead):
        # the dispatch, the per-image loop and the batched form are BaseDenseHead's own objects, and no class between the head
        # and BaseDenseHead has a copy of them, or of the former key helpers, beside the shared ones
        assert all(getattr(cls, name) is getattr(BaseDenseHead, name) for name in shared)
        for klass in cls.__mro__[:cls.__mro__.index(BaseDenseHead)]:
            assert not [n for n in vars(klass) if n in shared or n.startswith(('_level_keys', '_ctr_'))], klass
    three = build_head('giou', anchor_generator=dict(type='AnchorGenerator', ratios=[0.5, 1.0, 2.0], octave_base_scale=8,
                                                     scales_per_octave=1, strides=list(U.STRIDES)))
    assert three.num_anchors == 3 and three.atss_centerness.weight.size(0) == 3


def test_towers_anchor_targets_and_fused_gate_are_written_once():
    import inspect
    from htd_amd.detector import anchor_free_heads, anchor_heads, fovea_head, vfnet_head
    from htd_amd.detector.anchor_free_heads import FCOSHead
    from htd_amd.detector.anchor_heads import AnchorHead, AnchorTargets, ATSSHead, ATSSTargets, GFLHead, RetinaHead
    from htd_amd.detector.base_dense_head import BaseDenseHead
    from htd_amd.detector.fovea_head import FoveaHead
    from htd_amd.detector.rpn_head import RPNHead
    from htd_amd.detector.vfnet_head import VFNetHead

    def written_once(owner, names, heads):
        assert all(name in vars(owner) for name in names)
        for cls in heads:
            # the owner's own objects, and no class between the head and the owner has a copy
            assert all(getattr(cls, name) is getattr(owner, name) for name in names), cls
            for klass in cls.__mro__[:cls.__mro__.index(owner)]:
                assert not [n for n in vars(klass) if n in names], klass
    six = (RetinaHead, FCOSHead, ATSSHead, GFLHead, VFNetHead, FoveaHead)
    written_once(BaseDenseHead, ('_build_towers', '_init_towers', '_run_towers', '_fused_maps_ok'), six + (RPNHead, ))
    anchor_based = (AnchorHead, RPNHead, RetinaHead, ATSSHead, GFLHead, VFNetHead)
    written_once(AnchorTargets, ('get_anchors', '_anchors_inside', '_anchor_targets_single', '_anchor_targets', '_loss_targets'),
                 anchor_based)
    written_once(ATSSTargets, ('_atss_consts', '_atss_fused_ok', '_atss_fused_targets', 'get_num_level_anchors_inside', '_assign'),
                 (ATSSHead, GFLHead, VFNetHead))
    assert AnchorHead._assign is AnchorTargets._assign is RPNHead._assign is RetinaHead._assign
    assert GFLHead.__bases__ == (ATSSTargets, AnchorHead) == ATSSHead.__bases__ and VFNetHead.__bases__ == (ATSSTargets, FCOSHead)
    # the map rule is stated once, and nothing is borrowed by assignment
    text = ''.join(inspect.getsource(m) for m in (anchor_heads, anchor_free_heads, vfnet_head, fovea_head)) + \
        inspect.getsource(BaseDenseHead)
    assert text.count('t.is_cuda and t.dtype == torch.float32 and M.nhwc_channel_stride(t)') == 1
    assert not [line for line in text.splitlines() if line.startswith('    ') and ' = ' in line and
                line.split(' = ')[1].startswith(('ATSSHead.', 'AnchorHead.')) and line.split(' = ')[0].strip().isidentifier()]
    # the anchor heads have neither tower kwarg: ConvModule's own default bias, no deformable last layer
    assert RetinaHead.conv_bias == 'auto' and RetinaHead.dcn_on_last_conv is False
    # the public return structures are the reference's: 6 of AnchorHead, 7 (the anchors first) of ATSSHead
    metas, gts, labels = inputs()
    head = build_head('giou')
    anchor_list, valid = head.get_anchors(U.LEVEL_SIZES, metas, device='cpu')
    seven = head.get_targets(anchor_list, valid, gts, metas, gt_labels_list=labels, label_channels=80)
    six_ = AnchorHead.get_targets(head, anchor_list, valid, gts, metas, gt_labels_list=labels, label_channels=80)
    assert len(seven) == 7 and len(six_) == 6 and seven[5:] == six_[4:]
    assert all(torch.equal(a, b) for s, t in zip(seven[1:5], six_[:4]) for a, b in zip(s, t))
    assert all(torch.equal(a, torch.stack([x, x])) for a, x in zip(seven[0], anchor_list[0]))      # every anchor is inside


def test_new_abi_symbols_are_declared_and_exported():
    from htd_amd import capi
    names = {n for n, _, _ in capi.declared_functions()}
    want = {'htd_atss_targets_workspace_bytes', 'htd_atss_targets', 'htd_atss_loss_partial_rows', 'htd_atss_loss'}
    assert want <= names
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in want)
    assert lib.htd_atss_loss_partial_rows() > 0 and lib.htd_atss_loss_partial_rows() % 2 == 0
    assert lib.htd_atss_targets_workspace_bytes(2, 428) >= 2 * 428 * 8
    header = open(capi.HEADER).read()
    assert 'atss_assigner.py:33-178' in header and 'atss_head.py:145-295' in header and 'atss_head.py:297-313' in header
    from htd_amd.csrc import build
    assert 'atss.hip' in build.sources() and build.EXTRA['atss.hip'] == ['-ffp-contract=off']


# ---------------------------------------------------------------------------------------------------- reduce_mean
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from htd_amd.core import reduce_mean
    t = torch.tensor([1.0 + rank, 10.0 * (rank + 1), 0.5])
    kept = t.clone()
    out = reduce_mean(t)
    ok = torch.equal(t, kept) and torch.allclose(out, torch.tensor([1.5, 15.0, 0.5])) and out.data_ptr() != t.data_ptr()
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_reduce_mean_is_the_identity_alone_and_the_mean_under_gloo():
    import torch.multiprocessing as mp
    from htd_amd.core import reduce_mean
    t = torch.tensor([3.0, 4.0])
    assert reduce_mean(t) is t                                  # no process group: no collective, no copy
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok in res), res
