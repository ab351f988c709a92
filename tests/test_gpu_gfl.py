"""GFL on the GPU: htd_gfl_quality / htd_gfl_loss / htd_gfl_decode against the reference's own run (tests/golden/gfl.npz) and against
GFLHead.loss_tensor (pinned against that fixture by tests/test_gfl.py), the dispatch rule, the batched get_bboxes, and the GFL
detector against the reference's.

The bound of every value computed by a kernel is the project's rule (dense_fixture_util.bound): 4 x max(the reference's own fp32
error on that case, one fp32 ulp of the largest entry); the fp32 error comes from the fixture or from the fp32 run of the tensor
path on the CPU, never from the code under test.  Assignments are compared bit for bit.  No detector stays on the device between
tests."""
import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T, bound as _bound, err as _err, leave_the_allocator_as_found, spied as _spied  # noqa: F401
import gfl_util as U
from golden_util import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last
KEYS = ('loss_cls', 'loss_bbox', 'loss_dfl')


def inputs(dev):
    return D.inputs(dev, U.detector_inputs)


def _head_on_device(v='giou', **extra):
    from test_gfl import build_head
    return build_head(v, **extra).to(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_fused_head_loss_against_the_reference_fp64_run(golden, v, monkeypatch):
    """GFLHead.loss (fused) on the seeded maps against the reference head's fp64 run under the rule, for every variant (GIoU, IoU,
    reg_max 7 where 25 target sides take the clamp, beta 1.5); exactly one htd_atss_targets, one htd_gfl_quality and one
    htd_gfl_loss call; the assignment equals the reference's; the class gradient through a strided digest and at the 77 entries
    of the positives' own classes; score and weight within the rule of the reference's fp64 values; two
    runs bitwise equal; after a warm call the fused path and its backward read nothing on the host."""
    from test_iou_losses import _no_host_reads
    g = golden('gfl')
    p = f'head.{v}.'
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device(v)
    err = g[p + 'err32']
    runs = []
    for run in range(2):
        cls, reg = [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        assert head._fused_loss_ok(cls, reg, labels, None, metas)
        if run == 1:
            _no_host_reads(monkeypatch)
            torch.cuda.set_sync_debug_mode('error')

        def step():
            ls = head.loss(cls, reg, gts, labels, metas)
            (ls['loss_cls'] + ls['loss_bbox'] + ls['loss_dfl']).backward()
            return ls
        try:
            ls, calls = _spied(step)
        finally:
            torch.cuda.set_sync_debug_mode('default')
            monkeypatch.undo()
        assert [calls.count(n) for n in ('htd_atss_targets', 'htd_gfl_quality', 'htd_gfl_loss')] == [1, 1, 1], calls
        runs.append(([ls[k].detach().clone() for k in KEYS], [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in (cls, reg)],
                     [t.clone() for t in head._last_quality]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1] + runs[0][2], runs[1][0] + runs[1][1] + runs[1][2]))
    assigned, num_pos, norm = head._last_targets
    ref_assigned = T(g['head.assigned']).long()
    assert torch.equal(assigned.cpu().long(), ref_assigned)
    assert float(norm[0]) == float((ref_assigned > 0).sum(1).clamp(min=1).sum())
    losses, grads, (weight, score, wsum) = runs[0]
    worst = {}
    for i, name in enumerate(KEYS):
        ref = T(g[p + 'loss64'][i]).reshape(1).double()
        worst[name] = _err(losses[i].reshape(1), ref) / _bound(err[i], ref)
    ref = T(g[p + 'greg64'])
    worst['greg'] = _err(grads[1], ref) / _bound(err[4], ref)
    ref = T(g[p + 'gcls64.sample'])
    worst['gcls'] = _err(T(BU.digest(grads[0])[1]), ref) / _bound(err[3], ref)
    pi = T(g['head.pos_index']).long()
    ref = T(g[p + 'gclspos64'])
    worst['gclspos'] = _err(grads[0][pi[:, 0], pi[:, 1], pi[:, 2]], ref) / _bound(err[7], ref)
    s64, w64 = T(g[p + 'score64']), T(g[p + 'weight64'])
    worst['score'] = _err(score, s64) / _bound(err[5], s64)
    worst['weight'] = _err(weight, w64) / _bound(err[6], w64)
    e32 = abs(float(T(g[p + 'weight32']).sum()) - float(w64.sum()))
    worst['wsum'] = _err(wsum, w64.sum().reshape(1)) / _bound(e32, w64.sum().reshape(1))
    assert float(score.cpu()[ref_assigned == 0].abs().max()) == 0 and float(weight.cpu()[ref_assigned == 0].abs().max()) == 0
    print(f'head {v}: ' + ', '.join(f'{k} {x:.3f}' for k, x in worst.items()) + ' of the bound')
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- against the tensor path
PYRAMIDS = dict(five=(U.LEVEL_SIZES, U.STRIDES),
                eight=(U.LEVEL_SIZES + ((1, 1), ) * 3, U.STRIDES + (256, 512, 1024)),
                one_anchor=(((1, 1), ), (128, )))


def _shape_head(pyramid, C, reg_max, v='giou', **extra):
    sizes, strides = PYRAMIDS[pyramid]
    return _head_on_device(v, num_classes=C, reg_max=reg_max,
                           anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                                 strides=list(strides)), **extra), sizes


def _shape_inputs(pyramid, C, dev):
    _, metas, gts, labels = inputs(dev)
    if pyramid == 'one_anchor':                 # a 128 x 128 image under one stride-128 anchor
        metas = [dict(m, img_shape=(128, 128, 3), pad_shape=(128, 128, 3)) for m in metas]
    return metas, gts, [x % C for x in labels]


def _tensor_runs(head, cls, reg, gts, labels, metas):
    """loss_tensor on the CPU with fp64 and fp32 maps (fp32 targets) -> {dtype: (losses (3,), [gcls, greg] rows)}."""
    cpu_head = head
    res = {}
    for dt in (torch.float64, torch.float32):
        maps = [[m.detach().cpu().to(dt).contiguous().requires_grad_() for m in ms] for ms in (cls, reg)]
        ls = cpu_head.loss_tensor(*maps, [x.cpu() for x in gts], [x.cpu() for x in labels], metas)
        ls = torch.stack([sum(ls[k]) for k in KEYS])
        ls.sum().backward()
        res[dt] = (ls.detach().double(), [U.maps_to_rows([m.grad for m in ms]).double() for ms in maps])
    return res


def _fused_run(head, cls, reg, gts, labels, metas, scale=None):
    ls = head.loss(cls, reg, gts, labels, metas)
    ls = torch.stack([ls[k] for k in KEYS])
    (ls if scale is None else ls * torch.tensor(scale, device=ls.device)).sum().backward()
    return ls.detach().cpu().double()


@pytest.mark.parametrize('pyramid,C,reg_max', [('five', 80, 16), ('five', 3, 16), ('five', 80, 7), ('five', 3, 1), ('eight', 80, 7),
                                                ('eight', 3, 16)])
def test_fused_head_loss_against_the_tensor_path(pyramid, C, reg_max):
    """The fused form on maps that are channel slices of wider channels_last maps (class and distribution logits both padded)
    against loss_tensor on the CPU in fp64 on the same values, the bound from loss_tensor's own fp32 run: reg_max 1, 7 and 16, C = 80
    (float4 form) and 3 (scalar form), the five-level pyramid (two levels shorter than topk) and an eight-level one, logits of
    +-90 and a saturated distribution among them; the padding channels of both gradient maps are exact zeros."""
    dev = torch.device(DEV)
    head, sizes = _shape_head(pyramid, C, reg_max)
    metas, gts, lab = _shape_inputs(pyramid, C, dev)
    tag = f'gfl.shape.{pyramid}.{C}.{reg_max}'
    cls, reg = U.head_maps(C=C, sizes=sizes, reg_max=reg_max, tag=tag)
    cls[0][0, 0, 8, 9], cls[1][1, C - 1, 2, 2] = 90., -90.
    reg[0][1, :, 6, 7] = 0.
    reg[0][1, reg_max, 6, 7] = 60.                          # a saturated side: the last bin of `left`
    pads = (4 if C == 80 else 2, 4 if reg_max != 7 else 5)
    wide = [[torch.cat([m, seeded_tensor(f'{tag}.{k}{l}', (2, pad, *m.shape[-2:]))], 1).to(dev).contiguous(memory_format=CL)
             .requires_grad_() for l, m in enumerate(ms)] for k, (ms, pad) in enumerate(zip((cls, reg), pads))]
    widths = (C, 4 * (reg_max + 1))
    dcls, dreg = [[m[:, :c] for m in ms] for ms, c in zip(wide, widths)]
    assert head._fused_loss_ok(dcls, dreg, lab, None, metas)
    mine = _fused_run(head, dcls, dreg, gts, lab, metas)
    ref = _tensor_runs(head.cpu(), cls, reg, gts, lab, metas)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert torch.isfinite(mine).all() and torch.isfinite(r64[0]).all() and int((head._last_targets[0] > 0).sum()) > 0
    for i in range(3):
        e32 = _err(r32[0][i].reshape(1), r64[0][i].reshape(1))
        assert _err(mine[i].reshape(1), r64[0][i].reshape(1)) <= _bound(e32, r64[0][i].reshape(1)), (KEYS[i], mine, r64[0])
    for ms, c, a64, a32 in zip(wide, widths, r64[1], r32[1]):
        gr = U.maps_to_rows([m.grad for m in ms]).cpu()
        assert torch.isfinite(gr).all() and float(gr[..., c:].abs().max()) == 0
        assert _err(gr[..., :c], a64) <= _bound(_err(a32, a64), a64), (c, _err(gr[..., :c], a64), _err(a32, a64))


@pytest.mark.parametrize('pyramid', ['five', 'one_anchor'])
def test_fused_head_loss_without_positives(pyramid):
    """No gt anywhere, and a pyramid of one anchor (a single candidate: no positive): NaN box and DFL losses and a NaN gradient on
    every distribution logit (zeros on the padding), as loss_tensor and the reference give; the class part finite and equal."""
    dev = torch.device(DEV)
    head, sizes = _shape_head(pyramid, 80, 16)
    metas, gts, lab = _shape_inputs(pyramid, 80, dev)
    if pyramid == 'five':
        gts, lab = [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in lab]
    cls, reg = U.head_maps(sizes=sizes, tag=f'gfl.nopos.{pyramid}')
    dcls = [m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in cls]
    wide = [torch.cat([m, m[:, :4]], 1).to(dev).contiguous(memory_format=CL).requires_grad_() for m in reg]
    dreg = [m[:, :68] for m in wide]
    assert head._fused_loss_ok(dcls, dreg, lab, None, metas)
    mine = _fused_run(head, dcls, dreg, gts, lab, metas)
    assert int((head._last_targets[0] > 0).sum()) == 0 and float(head._last_quality[2]) == 0
    ref = _tensor_runs(head.cpu(), cls, reg, gts, lab, metas)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert bool(torch.isnan(mine[1:]).all()) and bool(torch.isnan(r64[0][1:]).all()) and bool(torch.isfinite(mine[0]))
    assert _err(mine[0].reshape(1), r64[0][0].reshape(1)) <= _bound(_err(r32[0][0].reshape(1), r64[0][0].reshape(1)), r64[0][0].reshape(1))
    greg = U.maps_to_rows([m.grad for m in wide]).cpu()
    assert bool(torch.isnan(greg[..., :68]).all()) and bool(torch.isnan(r64[1][1]).all()) and float(greg[..., 68:].abs().max()) == 0
    gcls = U.maps_to_rows([m.grad for m in dcls]).cpu()
    assert _err(gcls, r64[1][0]) <= _bound(_err(r32[1][0], r64[1][0]), r64[1][0])


def test_incoming_gradients_on_each_loss_and_a_second_backward():
    """Incoming gradients (2, 3, 5) on the three losses against loss_tensor's fp64 gradients under the same factors (the box and
    the DFL part of a distribution logit's gradient are scaled separately); factors of 1 leave the maps as the forward wrote them;
    a second backward through the same forward raises."""
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou')
    scale = [2.0, 3.0, 5.0]

    def fresh():
        return [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps()]
    cls, reg = fresh()
    _fused_run(head, cls, reg, gts, labels, metas, scale)
    mine = [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in (cls, reg)]
    head_cpu = _head_on_device('giou').cpu()
    ref = {}
    for dt in (torch.float64, torch.float32):
        maps = [[m.to(dt).requires_grad_() for m in ms] for ms in U.head_maps()]
        ls = head_cpu.loss_tensor(*maps, [x.cpu() for x in gts], [x.cpu() for x in labels], metas)
        sum(sum(ls[k]) * s for k, s in zip(KEYS, scale)).backward()
        ref[dt] = [U.maps_to_rows([m.grad for m in ms]).double() for ms in maps]
    for a, a64, a32 in zip(mine, ref[torch.float64], ref[torch.float32]):
        assert _err(a, a64) <= _bound(_err(a32, a64), a64)
    cls1, reg1 = fresh()
    _fused_run(head, cls1, reg1, gts, labels, metas)
    cls2, reg2 = fresh()
    _fused_run(head, cls2, reg2, gts, labels, metas, [1.0, 1.0, 1.0])
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(cls1 + reg1, cls2 + reg2))
    assert float((mine[1] - U.maps_to_rows([m.grad for m in reg1]).cpu()).abs().max()) > 0
    cls, reg = fresh()
    ls = head.loss(cls, reg, gts, labels, metas)
    total = ls['loss_cls'] + ls['loss_bbox'] + ls['loss_dfl']
    total.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()


# ---------------------------------------------------------------------------------------------------- dispatch
def test_dispatch_rule_and_the_tensor_path_on_the_device(golden):
    """Each condition of _fused_loss_ok turned off takes the tensor path.  Where the condition does not change the arithmetic
    (NCHW maps, ignore boxes that touch no anchor, the switch) the device's tensor path gives the fixture's fp64 losses to 1e-5
    relative (fp32 sums of 34 000 QFL terms in another order); where it does (pos_weight, topk 17, DIoULoss, reg_max 32, fp64
    distribution maps, anchors past the padding of a smaller image, allowed_border 48, nine levels) it gives what its own fp64
    run on the CPU gives; a sum reduction on any of the three losses raises on the tensor path as it does in the reference
    (avg_factor with 'sum'), and a class loss other than QFL cannot take the (label, score) target at all."""
    g = golden('gfl')
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou')
    cl = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps()]
    far = [torch.tensor([[900., 900., 950., 950.]], device=dev) for _ in gts]
    assert head._fused_loss_ok(*cl, labels, None, metas)
    assert not head._fused_loss_ok(*nchw, labels, None, metas) and not head._fused_loss_ok(*cl, labels, far, metas)
    assert not head._fused_loss_ok(cl[0], [m.double() for m in cl[1]], labels, None, metas)
    off = _head_on_device('giou')
    off.fused_loss = False
    assert not off._fused_loss_ok(*cl, labels, None, metas)
    for h, maps, ignore in ((head, nchw, None), (head, cl, far), (off, cl, None)):
        ls, calls = _spied(lambda: h.loss(*maps, gts, labels, metas, gt_bboxes_ignore=ignore))
        assert isinstance(ls['loss_cls'], list) and not any(n.startswith('htd_gfl') for n in calls)
        mine = torch.stack([sum(ls[k]) for k in KEYS]).cpu().double()
        np.testing.assert_allclose(mine.numpy(), g['head.giou.loss64'], rtol=1e-5)
    # Anchors past the padding of a smaller second image (260 + 70 of its 320 + 80 fine anchors stay; 46 positives for 51), and
    # allowed_border 48 (320 + 48 anchors stay on two levels; 6 + 23 positives).  On both subsets every candidate IoU keeps 5e-3 of
    # its threshold and every ninth distance of the next (checked in fp64 when the cases were chosen), so the fp32 assigner of the
    # device and the fp64 one of the CPU agree; allowed_border 0 leaves 96 anchors whose candidate IoUs tie with the threshold.
    small = [dict(metas[0]), dict(metas[1], img_shape=(104, 160, 3), pad_shape=(104, 160, 3))]
    nine_sizes, nine_strides = U.LEVEL_SIZES + ((1, 1), ) * 4, U.STRIDES + (256, 512, 1024, 2048)
    nine = dict(anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                      strides=list(nine_strides)))

    def on_dev(ms):
        return [m.to(dev).contiguous(memory_format=CL) for m in ms]
    qfl_sum = dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, reduction='sum', loss_weight=1.0)
    # name -> (head arguments, maps, metas, what the tensor path does: its losses are compared, or it raises as the reference does)
    changed = dict(pos_weight=(dict(train_cfg=dict(pos_weight=2.0)), cl, metas, 'compare'),
                   topk=(dict(train_cfg=dict(assigner=dict(type='ATSSAssigner', topk=17))), cl, metas, 'compare'),
                   diou=(dict(loss_bbox=dict(type='DIoULoss', loss_weight=2.0)), cl, metas, 'compare'),
                   reg_max=(dict(reg_max=32), [cl[0], on_dev(U.head_maps(reg_max=32)[1])], metas, 'compare'),
                   fp64_reg=(dict(), [cl[0], [m.double() for m in cl[1]]], metas, 'compare'),
                   invalid_anchors=(dict(), cl, small, 'compare'),
                   border=(dict(train_cfg=dict(allowed_border=48)), cl, metas, 'compare'),
                   nine_levels=(nine, [on_dev(ms) for ms in U.head_maps(sizes=nine_sizes, tag='gfl.nine')], metas, 'compare'),
                   # avg_factor with a sum reduction raises ValueError, in the reference's weight_reduce_loss too
                   dfl_sum=(dict(loss_dfl=dict(type='DistributionFocalLoss', reduction='sum', loss_weight=0.25)), cl, metas, ValueError),
                   qfl_sum=(dict(loss_cls=qfl_sum), cl, metas, ValueError),
                   box_sum=(dict(loss_bbox=dict(type='GIoULoss', reduction='sum', loss_weight=2.0)), cl, metas, ValueError),
                   # a class loss that is not QFL cannot take the (label, score) target on any path, as in the reference
                   focal=(dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)), cl, metas,
                          Exception))
    for name, (extra, maps, mt, what) in changed.items():
        h = _head_on_device('giou', **extra)
        assert not h._fused_loss_ok(*maps, labels, None, mt), name
        if what != 'compare':
            with pytest.raises(what):
                _, calls = _spied(lambda: h.loss(*maps, gts, labels, mt))
            continue
        ls, calls = _spied(lambda: h.loss(*maps, gts, labels, mt))
        assert isinstance(ls['loss_cls'], list) and not any(n.startswith('htd_gfl') for n in calls), name
        mine = torch.stack([sum(ls[k]) for k in KEYS]).cpu().double()
        ref = h.cpu().loss_tensor(*[[m.cpu().double() for m in ms] for ms in maps], [x.cpu() for x in gts], [x.cpu() for x in labels], mt)
        ref = torch.stack([sum(ref[k]) for k in KEYS])
        assert bool(torch.isfinite(ref).all()), name
        np.testing.assert_allclose(mine.numpy(), ref.numpy(), rtol=1e-5, err_msg=name)


# ---------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize('C,reg_max', [(80, 16), (3, 1), (80, 31), (5, 7)])
def test_decode_kernel_against_fp64(C, reg_max):
    """keys = max_c sigmoid(cls) and dist = softmax-integral x stride of every anchor of three images against fp64 on the CPU:
    the keys within 4 fp32 ulps (one exp, one sum, one division; a sigmoid below 1e-37 may flush to 0), the distances within 16:
    numerator and denominator are sums of at most 8 positive terms per lane and two more across lanes (10 roundings of half an
    ulp) of exponentials good to 2 ulps, 7 ulps each, and the quotient and the product add two more.  Padded strides on both maps,
    logits of +-90."""
    from htd_amd import mmcv_ops as M
    dev = torch.device(DEV)
    cls, reg = U.head_maps(B=3, C=C, reg_max=reg_max, tag=f'gfl.dec.{C}.{reg_max}')
    cls[0][0, 0, 3, 3], cls[0][1, :, 5, 5], reg[1][2, 1, 2, 2] = 90., -90., 90.
    wide = [[torch.cat([m, m[:, :3]], 1).to(dev).contiguous(memory_format=CL) for m in ms] for ms in (cls, reg)]
    dcls, dreg = [m[:, :C] for m in wide[0]], [m[:, :4 * (reg_max + 1)] for m in wide[1]]
    keys, dist = M.gfl_decode(dcls, dreg, U.STRIDES, reg_max)
    rows_c, rows_r = U.maps_to_rows(cls).double(), U.maps_to_rows(reg).double()
    want_k = rows_c.sigmoid().max(-1)[0]
    stride = torch.cat([torch.full((n, ), float(s)) for n, s in zip(U.LEVEL_ANCHORS, U.STRIDES)]).double()
    p = torch.softmax(rows_r.reshape(3, -1, 4, reg_max + 1), -1)
    want_d = (p * torch.arange(reg_max + 1.).double()).sum(-1) * stride[None, :, None]
    assert keys.shape == want_k.shape and dist.shape == want_d.shape
    assert bool(((keys.cpu().double() - want_k).abs() <= 4 * EPS32 * want_k + 1e-37).all())
    tol = 16 * EPS32 * want_d + 1e-37
    assert bool(((dist.cpu().double() - want_d).abs() <= tol).all()), float(((dist.cpu().double() - want_d).abs() / tol).max())
    again = M.gfl_decode(dcls, dreg, U.STRIDES, reg_max)
    assert torch.equal(again[0], keys) and torch.equal(again[1], dist)


def test_get_bboxes_equals_the_fixture_and_batched_equals_the_per_image_loop(golden):
    """get_bboxes(with_nms=False) on the seeded maps: the fixture's boxes and score rows after the nms_pre cut on levels 0 and 1
    (same rows in the same order: the key gap at the cuts is 1e-3).  With NMS, the batched form -- one decode launch, one segmented
    top-k, one NMS without score factors -- agrees BIT FOR BIT with the per-image loop at B = 2 and B = 5, images of different
    shapes and scale factors, the cuts to nms_pre (and none) and max_per_img active."""
    from htd_amd.registry import ConfigDict
    g = golden('gfl')
    dev = torch.device(DEV)
    _, metas, _, _ = inputs(dev)
    head = _head_on_device('giou')
    maps = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
    res = head.get_bboxes(*maps, metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores) in enumerate(res):
        np.testing.assert_allclose(boxes.cpu().numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-3)
        np.testing.assert_allclose(scores.double().sum(1).cpu().numpy(), g[f'head.score_rows{i}'], rtol=1e-5)
    # NCHW-contiguous maps are not the kernel's layout: the tensor operations serve them, with and without the NMS
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps()]
    res, calls = _spied(lambda: head.get_bboxes(*nchw, metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False))
    assert 'htd_gfl_decode' not in calls
    for i, (boxes, scores) in enumerate(res):
        np.testing.assert_allclose(boxes.cpu().numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-3)
        np.testing.assert_allclose(scores.double().sum(1).cpu().numpy(), g[f'head.score_rows{i}'], rtol=1e-5)
    dets, calls = _spied(lambda: head.get_bboxes(*nchw, metas, cfg=ConfigDict(U.HEAD_TEST_CFG)))
    assert 'htd_gfl_decode' not in calls and all(d.shape[1] == 5 and d.shape[0] == l.shape[0] > 0 for d, l in dets)
    H, W = 128, 160
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas5 = [dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), flip=False,
                   scale_factor=np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32)) for i, (h, w) in enumerate(shapes)]
    maps5 = [[torch.cat([m, m.flip(0) * 0.5, m[:1] * 0.0 - 3.0]).contiguous(memory_format=CL) for m in ms] for ms in maps]
    for nms_pre in (U.HEAD_TEST_CFG['nms_pre'], -1):
        cfg = ConfigDict(dict(U.HEAD_TEST_CFG, nms_pre=nms_pre, max_per_img=9, score_thr=0.02))
        for ms, mt in (([[m[:2] for m in x] for x in maps5], metas5[:2]), (maps5, metas5)):
            out = {}
            for mode in (True, False):
                head.batched_get_bboxes = mode
                out[mode], calls = _spied(lambda: head.get_bboxes(*ms, mt, cfg=cfg, rescale=True))
                assert calls.count('htd_gfl_decode') == (1 if mode else len(mt))
            head.batched_get_bboxes = True
            counts = [int(d.shape[0]) for d, _ in out[False]]
            assert max(counts) == 9, counts
            for (d1, l1), (d2, l2) in zip(out[True], out[False]):
                assert torch.equal(d1, d2) and torch.equal(l1, l2)


def test_surface_refuses_bad_arguments():
    """reg_max > 31, more than 8 levels, wrong dtypes and shapes raise before anything is launched."""
    from htd_amd import mmcv_ops as M
    dev = torch.device(DEV)
    cls, reg = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
    anchors = U.anchors_of().to(dev)
    gts = torch.zeros(2, 1, 4, device=dev)
    assigned = torch.zeros(2, anchors.size(0), dtype=torch.int32, device=dev)
    zeros = torch.zeros(2, anchors.size(0), device=dev)
    one = torch.ones(1, device=dev)
    labels = torch.zeros(2, 1, dtype=torch.int64, device=dev)
    reg32 = [m.to(dev).contiguous(memory_format=CL) for m in U.head_maps(reg_max=32)[1]]

    def refused(fn):
        with pytest.raises(ValueError):
            fn()
    refused(lambda: M.gfl_decode(cls, reg32, U.STRIDES, 32))
    refused(lambda: M.gfl_quality(cls, reg32, U.STRIDES, 32, anchors, gts, assigned))
    refused(lambda: M.gfl_decode(cls, reg, U.STRIDES, 7))                                   # 68 channels are not 4 * 8
    refused(lambda: M.gfl_decode(cls, [m.double() for m in reg], U.STRIDES, 16))
    refused(lambda: M.gfl_quality(cls, reg, U.STRIDES, 16, anchors, gts, assigned.long()))
    refused(lambda: M.gfl_loss(cls, reg, U.STRIDES, 16, anchors, gts, labels.int(), assigned, zeros, zeros, one, one, 2))
    refused(lambda: M.gfl_loss(cls, reg, U.STRIDES, 16, anchors, gts, labels, assigned, zeros, zeros, one, one, 3))      # DIoU
    refused(lambda: M.gfl_decode([cls[4]] * 9, [reg[4]] * 9, (8, ) * 9, 16))
    with pytest.raises(NotImplementedError):
        M.gfl_decode(*U.head_maps(), U.STRIDES, 16)                                         # CPU maps
    keys, dist = M.gfl_decode(cls, reg, U.STRIDES, 16)
    assert bool(torch.isfinite(keys).all()) and bool(torch.isfinite(dist).all())


# ---------------------------------------------------------------------------------------------------- the detector
def small_cfg(g):
    from htd_amd.configs import gfl_config
    cfg = gfl_config()
    cfg.test_cfg.nms_pre = int(g['nms_pre'])
    return cfg


@pytest.fixture
def det(golden):
    """A detector of the test's own: nothing of it stays on the device when the test ends."""
    import gc
    from htd_amd import dense
    from htd_amd.configs import build_baseline_detector
    g = golden('gfl')
    model = build_baseline_detector(cfg=small_cfg(g))
    yield U.load_fixture_weights_(model, float(g['cls_scale']), float(g['cls_bias_shift'])).to(torch.device(DEV))
    model.zero_grad(set_to_none=True)
    model.cpu()
    dense.new_step()
    gc.collect()
    torch.cuda.empty_cache()


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step; `assigned` equals the fixture's and the step reaches the fused path: one
    htd_atss_targets, one htd_gfl_quality, one htd_gfl_loss."""
    g = golden('gfl')
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    losses, calls = _spied(lambda: det.forward_train(img, metas, gts, labels))
    assert [calls.count(n) for n in ('htd_atss_targets', 'htd_gfl_quality', 'htd_gfl_loss')] == [1, 1, 1]
    assigned, num_pos, norm = det.bbox_head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g['assigned']).long())
    assert num_pos.tolist() == g['num_pos'].tolist() and float(norm[0]) == float(g['num_pos'].sum())
    D.check_train_step(det, g, '', 'gfl', losses, KEYS, U.grad_keys(det), 3 + len(U.EXTRA_GRAD_KEYS), zero_grad_ok=('.scales.', ))


def test_outputs_and_detections_match_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_outputs and check_detections."""
    g = golden('gfl')
    img, metas, _, _ = inputs(torch.device(DEV))
    worst = D.check_outputs(det, g, '', ('cls', 'reg'), U.LEVEL_SIZES, img)
    det.eval()
    with torch.no_grad():
        res = det.simple_test(img, metas)
    print(f'gfl: worst output ratio {worst:.3f}, worst detection ratio {D.check_detections(res, g, ""):.3f}')


def test_reference_format_checkpoint_round_trip(golden, tmp_path):
    """dense_fixture_util.check_checkpoint_round_trip on the GFL fixture."""
    from htd_amd.configs import build_baseline_detector
    g = golden('gfl')
    state = U.fixture_state(g['state_keys'], g['state_shapes'], float(g['cls_scale']), float(g['cls_bias_shift']))
    assert 'bbox_head.integral.project' in state
    img, metas, _, _ = inputs(torch.device(DEV))
    D.check_checkpoint_round_trip(lambda: build_baseline_detector(cfg=small_cfg(g)), state, g, '', img, metas, tmp_path, tol=1e-2)
