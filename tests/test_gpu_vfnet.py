"""VFNet on the GPU: htd_vfnet_star_fwd / _bwd, htd_vfnet_quality and htd_vfnet_loss against the reference's own run
(tests/golden/vfnet.npz) and against VFNetHead.loss_tensor / star_dcn_offset (pinned against that fixture by tests/test_vfnet.py),
the deformable convolution on star offsets, the dispatch rule, the batched get_bboxes, and the VFNet detector against the
reference's.

The bound of every value computed by a kernel is the project's rule (dense_fixture_util.bound): 4 x max(the reference's own fp32
error on that case, one fp32 ulp of the largest entry); the fp32 error comes from the fixture or from the fp32 run of the tensor
path on the CPU, never from the code under test.  Assignments are compared bit for bit.  No detector stays on the device between
tests."""
import numpy as np
import pytest
import torch

import baselines_util as BU
import dcn_ref as R
import dense_fixture_util as D
from dense_fixture_util import EPS32, bound as _bound, err as _err, leave_the_allocator_as_found, spied as _spied  # noqa: F401
from golden_util import seeded_tensor
from test_vfnet import E_GCLS, E_GCLSPOS, E_GREF, E_GREG, E_INI, E_RF, E_SUMS, KEYS, T
import vfnet_util as U

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last
ENTRIES = ('htd_atss_targets', 'htd_vfnet_quality', 'htd_vfnet_loss')


def inputs(dev):
    return D.inputs(dev, U.detector_inputs)


def _head_on_device(v='giou', **extra):
    from test_vfnet import build_head
    return build_head(v, **extra).to(torch.device(DEV))


def _on_dev(ms, dev=None):
    return [m.to(torch.device(DEV) if dev is None else dev).contiguous(memory_format=CL) for m in ms]


# ---------------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_fused_head_loss_against_the_reference_fp64_run(golden, v, monkeypatch):
    """VFNetHead.loss (fused) on the seeded maps against the reference head's fp64 run under the rule, for every variant (GIoU,
    IoU, iou_weighted off, gamma 1.5 with alpha 0.5, stride-normalised distances): the three losses, both regression gradient
    maps in full, the class gradient through a strided digest and at the 77 entries of the positives' own classes, both IoU
    tensors (one entry clamped to 1e-6) and the three sums; exactly one htd_atss_targets, one htd_vfnet_quality and one
    htd_vfnet_loss call; the assignment equals the reference's; two runs bitwise equal; after a warm call the fused path and
    its backward read nothing on the host."""
    from test_iou_losses import _no_host_reads
    g = golden('vfnet')
    p = f'head.{v}.'
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device(v)
    err = g[p + 'err32']
    runs = []
    for run in range(2):
        cls, reg, ref = [[m.requires_grad_() for m in _on_dev(ms)] for ms in U.head_maps(v)]
        assert head._fused_loss_ok(cls, reg, ref, labels, None, metas)
        if run == 1:
            _no_host_reads(monkeypatch)
            torch.cuda.set_sync_debug_mode('error')

        def step():
            ls = head.loss(cls, reg, ref, gts, labels, metas)
            (ls['loss_cls'] + ls['loss_bbox'] + ls['loss_bbox_rf']).backward()
            return ls
        try:
            ls, calls = _spied(step)
        finally:
            torch.cuda.set_sync_debug_mode('default')
            monkeypatch.undo()
        assert [calls.count(n) for n in ENTRIES] == [1, 1, 1], calls
        runs.append(([ls[k].detach().clone() for k in KEYS], [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in (cls, reg, ref)],
                     [t.clone() for t in head._last_quality]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1] + runs[0][2], runs[1][0] + runs[1][1] + runs[1][2]))
    assigned, num_pos, norm = head._last_targets
    ref_assigned = T(g['head.assigned']).long()
    assert torch.equal(assigned.cpu().long(), ref_assigned)
    losses, grads, (iou_ini, iou_rf, sums) = runs[0]
    worst = {}
    for i, name in enumerate(KEYS):
        want = T(g[p + 'loss64'][i]).reshape(1).double()
        worst[name] = _err(losses[i].reshape(1), want) / _bound(err[i], want)
    for name, mine, e in (('greg', grads[1], E_GREG), ('gref', grads[2], E_GREF)):
        want = T(g[p + name + '64'])
        worst[name] = _err(mine, want) / _bound(err[e], want)
    want = T(g[p + 'gcls64.sample'])
    worst['gcls'] = _err(T(BU.digest(grads[0])[1]), want) / _bound(err[E_GCLS], want)
    pi = T(g['head.pos_index']).long()
    want = T(g[p + 'gclspos64'])
    worst['gclspos'] = _err(grads[0][pi[:, 0], pi[:, 1], pi[:, 2]], want) / _bound(err[E_GCLSPOS], want)
    for name, mine, e in (('iou_ini', iou_ini, E_INI), ('iou_rf', iou_rf, E_RF)):
        want = T(g[p + name + '64'])
        worst[name] = _err(mine, want) / _bound(err[e], want)
        assert float(mine.cpu()[ref_assigned == 0].abs().max()) == 0
    b, l, y, x = U.NO_OVERLAP
    assert float(iou_ini[b, sum(U.LEVEL_ANCHORS[:l]) + y * U.LEVEL_SIZES[l][1] + x]) == float(np.float32(1e-6))
    want = T(g[p + 'sums64'])
    for k in range(3):
        worst[f'sums{k}'] = _err(sums[k].reshape(1), want[k].reshape(1)) / _bound(err[E_SUMS + k], want[k].reshape(1))
    assert float(sums[0]) == float((ref_assigned > 0).sum())
    print(f'head {v}: ' + ', '.join(f'{k} {x:.3f}' for k, x in worst.items()) + ' of the bound')
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- against the tensor path
PYRAMIDS = dict(five=(U.LEVEL_SIZES, U.STRIDES),
                eight=(U.LEVEL_SIZES + ((1, 1), ) * 3, U.STRIDES + (256, 512, 1024)),
                one_anchor=(((1, 1), ), (128, )))


def _shape_head(pyramid, C, v='giou', **extra):
    sizes, strides = PYRAMIDS[pyramid]
    return _head_on_device(v, num_classes=C, strides=list(strides),
                           anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                                 center_offset=0.0, strides=list(strides)), **extra), sizes, strides


def _shape_inputs(pyramid, C, dev):
    _, metas, gts, labels = inputs(dev)
    if pyramid == 'one_anchor':                 # a 128 x 128 image under one stride-128 anchor
        metas = [dict(m, img_shape=(128, 128, 3), pad_shape=(128, 128, 3)) for m in metas]
    return metas, gts, [x % C for x in labels]


def _tensor_runs(head, maps, gts, labels, metas, scale=None):
    """loss_tensor on the CPU with fp64 and fp32 maps (fp32 targets) -> {dtype: (losses (3,), [gcls, greg, gref] rows)}."""
    res = {}
    for dt in (torch.float64, torch.float32):
        leaves = [[m.detach().cpu().to(dt).contiguous().requires_grad_() for m in ms] for ms in maps]
        ls = head.loss_tensor(*leaves, [x.cpu() for x in gts], [x.cpu() for x in labels], metas)
        ls = torch.stack([ls[k] for k in KEYS])
        (ls if scale is None else ls * torch.tensor(scale, dtype=dt)).sum().backward()
        res[dt] = (ls.detach().double(), [U.maps_to_rows([m.grad for m in ms]).double() for ms in leaves])
    return res


def _fused_run(head, maps, gts, labels, metas, scale=None):
    ls, calls = _spied(lambda: head.loss(*maps, gts, labels, metas))
    assert [calls.count(n) for n in ENTRIES] == [1, 1, 1], calls
    ls = torch.stack([ls[k] for k in KEYS])
    (ls if scale is None else ls * torch.tensor(scale, device=ls.device)).sum().backward()
    return ls.detach().cpu().double()


def _padded(maps, pads, tag, dev):
    """Channels_last maps that are channel slices of wider ones -> (the wide leaves, their slices)."""
    wide = [[torch.cat([m, seeded_tensor(f'{tag}.pad{k}.{l}', (m.size(0), pad, *m.shape[-2:]))], 1).to(dev)
             .contiguous(memory_format=CL).requires_grad_() for l, m in enumerate(ms)] for k, (ms, pad) in enumerate(zip(maps, pads))]
    return wide, [[w[:, :m.size(1)] for w, m in zip(ws, ms)] for ws, ms in zip(wide, maps)]


def _check_against_tensor_path(head, maps, wide, gts, lab, metas, mine):
    ref = _tensor_runs(head.cpu(), maps, gts, lab, metas)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert torch.isfinite(mine).all() and torch.isfinite(r64[0]).all()
    for i in range(3):
        e32 = _err(r32[0][i].reshape(1), r64[0][i].reshape(1))
        assert _err(mine[i].reshape(1), r64[0][i].reshape(1)) <= _bound(e32, r64[0][i].reshape(1)), (KEYS[i], mine, r64[0])
    for ws, ms, a64, a32 in zip(wide, maps, r64[1], r32[1]):
        c = ms[0].size(1)
        gr = U.maps_to_rows([m.grad for m in ws]).cpu()
        assert torch.isfinite(gr).all() and (gr.size(-1) == c or float(gr[..., c:].abs().max()) == 0)
        assert _err(gr[..., :c], a64) <= _bound(_err(a32, a64), a64), (c, _err(gr[..., :c], a64), _err(a32, a64))
    return r64


@pytest.mark.parametrize('pyramid,C', [('five', 80), ('five', 3), ('eight', 80), ('eight', 3)])
def test_fused_head_loss_against_the_tensor_path(pyramid, C):
    """The fused form on maps that are channel slices of wider channels_last maps (all three kinds padded) against loss_tensor on
    the CPU in fp64 on the same values, the bound from loss_tensor's own fp32 run: C = 80 (float4 form) and 3 (scalar form), the
    five-level pyramid (two levels shorter than topk) and an eight-level one with three single-anchor levels, logits of +-90
    among them; the padding channels of the three gradient maps are exact zeros."""
    dev = torch.device(DEV)
    head, sizes, strides = _shape_head(pyramid, C)
    metas, gts, lab = _shape_inputs(pyramid, C, dev)
    tag = f'vfnet.shape.{pyramid}.{C}'
    maps = U.head_maps(C=C, sizes=sizes, strides=strides, tag=tag, no_overlap=False)
    maps[0][0][0, 0, 8, 9], maps[0][1][1, C - 1, 2, 2] = 90., -90.
    wide, sliced = _padded(maps, (4 if C == 80 else 2, 4, 3), tag, dev)
    assert head._fused_loss_ok(*sliced, lab, None, metas)
    mine = _fused_run(head, sliced, gts, lab, metas)
    assert int((head._last_targets[0] > 0).sum()) > 0
    _check_against_tensor_path(head, maps, wide, gts, lab, metas, mine)


def test_a_batch_with_one_empty_image_counts_its_positives_once():
    """One image without a gt: htd_atss_targets' norm[0] counts it as one sample (AnchorHead's rule), the varifocal loss must
    not -- sums[0] is the number of positives, and loss_cls agrees with loss_tensor."""
    dev = torch.device(DEV)
    head, sizes, strides = _shape_head('five', 80)
    metas, gts, lab = _shape_inputs('five', 80, dev)
    gts, lab = [gts[0], gts[1].new_zeros(0, 4)], [lab[0], lab[1].new_zeros(0)]
    maps = U.head_maps(tag='vfnet.empty_image', no_overlap=False)
    leaves = [[m.requires_grad_() for m in _on_dev(ms)] for ms in maps]
    mine = _fused_run(head, leaves, gts, lab, metas)
    assigned, num_pos, norm = head._last_targets
    n = int((assigned > 0).sum())
    assert num_pos.tolist() == [n, 0] and n > 0 and float(norm[0]) == n + 1 and float(head._last_quality[2][0]) == n
    _check_against_tensor_path(head, maps, leaves, gts, lab, metas, mine)


@pytest.mark.parametrize('pyramid', ['five', 'one_anchor'])
def test_fused_head_loss_without_positives(pyramid):
    """No gt anywhere, and a pyramid of one anchor (a single candidate: no positive): both box losses exactly 0 with exactly zero
    gradients on every distance (padding included), the varifocal loss finite over factor 1 and equal to loss_tensor's."""
    dev = torch.device(DEV)
    head, sizes, strides = _shape_head(pyramid, 80)
    metas, gts, lab = _shape_inputs(pyramid, 80, dev)
    if pyramid == 'five':
        gts, lab = [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in lab]
    maps = U.head_maps(sizes=sizes, strides=strides, tag=f'vfnet.nopos.{pyramid}', no_overlap=False)
    wide, sliced = _padded(maps, (0, 4, 2), f'vfnet.nopos.{pyramid}', dev)
    assert head._fused_loss_ok(*sliced, lab, None, metas)
    mine = _fused_run(head, sliced, gts, lab, metas)
    assert int((head._last_targets[0] > 0).sum()) == 0 and head._last_quality[2].tolist() == [0.0, 0.0, 0.0]
    assert float(mine[1]) == 0 and float(mine[2]) == 0 and bool(torch.isfinite(mine[0])) and float(mine[0]) > 0
    for ws in wide[1:]:
        assert all(float(m.grad.abs().max()) == 0 for m in ws)
    _check_against_tensor_path(head, maps, wide, gts, lab, metas, mine)


def test_incoming_gradients_on_each_loss_and_a_second_backward():
    """Incoming gradients (2, 3, 5) on the three losses against loss_tensor's fp64 gradients under the same factors; factors of 1
    leave the maps as the forward wrote them; a second backward through the same forward raises."""
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou')
    scale = [2.0, 3.0, 5.0]

    def fresh():
        return [[m.requires_grad_() for m in _on_dev(ms)] for ms in U.head_maps()]
    maps = fresh()
    _fused_run(head, maps, gts, labels, metas, scale)
    mine = [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in maps]
    ref = _tensor_runs(_head_on_device('giou').cpu(), U.head_maps(), gts, labels, metas, scale)
    for a, a64, a32 in zip(mine, ref[torch.float64][1], ref[torch.float32][1]):
        assert _err(a, a64) <= _bound(_err(a32, a64), a64)
    maps1, maps2 = fresh(), fresh()
    _fused_run(head, maps1, gts, labels, metas)
    _fused_run(head, maps2, gts, labels, metas, [1.0, 1.0, 1.0])
    assert all(torch.equal(a.grad, b.grad) for x, y in zip(maps1, maps2) for a, b in zip(x, y))
    for k in range(3):
        assert float((mine[k] - U.maps_to_rows([m.grad for m in maps1[k]]).cpu()).abs().max()) > 0
    cls, reg, ref_maps = fresh()
    ls = head.loss(cls, reg, ref_maps, gts, labels, metas)
    total = ls['loss_cls'] + ls['loss_bbox'] + ls['loss_bbox_rf']
    total.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()


# ---------------------------------------------------------------------------------------------------- star offsets
@pytest.mark.parametrize('gm', [0.1, 1.0])
@pytest.mark.parametrize('norm', ['reg_denom', 'stride'])
@pytest.mark.parametrize('shape,pad', [((2, 4, 1, 2), 0), ((2, 4, 3, 5), 0), ((2, 4, 16, 20), 0), ((2, 4, 3, 5), 2), ((2, 4, 16, 20), 4)])
def test_star_kernel_against_the_tensor_form_in_fp64(shape, pad, norm, gm):
    """htd_vfnet_star_fwd: bbox_pred and the 18 offset channels within one fp32 ulp of the largest entry of star_dcn_offset in fp64
    on the CPU.  htd_vfnet_star_bwd under both incoming gradients, and with either absent, within 4 x max(the fp32 tensor form's
    own error, an ulp of the largest entry).  Plain maps and channel slices of wider ones (whose padding gets a zero gradient)."""
    from htd_amd import mmcv_ops as M
    from test_vfnet import build_head
    dev = torch.device(DEV)
    head = build_head(bbox_norm_type=norm, gradient_mul=gm)
    stride, denom = 16, (128 if norm == 'reg_denom' else 16)
    x = U.star_case(shape, tag=f'vfnet.star.{norm}')
    gp, go = seeded_tensor('vfnet.star.gp', shape), seeded_tensor('vfnet.star.go', (shape[0], 18, *shape[2:]))

    def tensor_form(dt, use):
        leaf = x.detach().clone().to(dt).requires_grad_()
        pred = leaf.exp() * denom
        off = head.star_dcn_offset(pred, gm, stride)
        total = sum(t for t, u in (((pred * gp.to(dt)).sum(), use[0]), ((off * go.to(dt)).sum(), use[1])) if u)
        total.backward()
        return pred.detach(), off.detach(), leaf.grad
    for use in ((True, True), (True, False), (False, True)):
        wide = torch.cat([x, seeded_tensor('vfnet.star.padding', (shape[0], pad, *shape[2:]))], 1) if pad else x
        wide = wide.to(dev).contiguous(memory_format=CL).requires_grad_()
        (pred, off), calls = _spied(lambda: M.vfnet_star(wide[:, :4], denom, stride, gm))
        assert calls == ['htd_vfnet_star_fwd'] and pred.shape == shape and off.shape == (shape[0], 18, *shape[2:])
        total = sum(t for t, u in (((pred * gp.to(dev)).sum(), use[0]), ((off * go.to(dev)).sum(), use[1])) if u)
        _, calls = _spied(total.backward)
        assert calls == ['htd_vfnet_star_bwd']
        p64, o64, g64 = tensor_form(torch.float64, use)
        _, _, g32 = tensor_form(torch.float32, use)
        assert _err(pred, p64) <= EPS32 * float(p64.abs().max()), _err(pred, p64) / (EPS32 * float(p64.abs().max()))
        assert _err(off, o64) <= EPS32 * float(o64.abs().max()), _err(off, o64) / (EPS32 * float(o64.abs().max()))
        assert _err(wide.grad[:, :4], g64) <= _bound(_err(g32, g64), g64), (use, _err(wide.grad[:, :4], g64), _err(g32, g64))
        assert pad == 0 or float(wide.grad[:, 4:].abs().max()) == 0
    base = head.dcn_base_offset.float().flatten()           # the six untouched channels are exactly 0 - base
    untouched = [3, 6, 8, 9, 10, 15]
    assert torch.equal(off[:, untouched].cpu(), (0 - base[untouched]).view(1, 6, 1, 1).expand(shape[0], 6, *shape[2:]))


def test_deform_conv_on_star_offsets_that_reach_beyond_the_map():
    """deform_conv2d (htd_deform_im2col and the GEMM with its ReLU epilogue, as VFNetHead calls it) on star offsets of boxes far
    larger than a 5 x 7 map, so that most taps sample outside (-1, H) x (-1, W), against dcn_ref.im2col and an einsum in fp64, C =
    32; forward and the gradients of input, offsets and weight under the tolerances of test_gpu_dcn.py::test_deform_conv_fwd_bwd."""
    from htd_amd import mmcv_ops as M
    from htd_amd.dcn import deform_conv2d
    dev = torch.device(DEV)
    B, C, H, W, Co = 2, 32, 5, 7, 16
    x = seeded_tensor('vfnet.dcn.x', (B, C, H, W))
    w = seeded_tensor('vfnet.dcn.w', (Co, C, 3, 3)) / (C * 9) ** 0.5
    go = seeded_tensor('vfnet.dcn.go', (B, Co, H, W))
    logits = seeded_tensor('vfnet.dcn.logits', (B, 4, H, W), scale=0.8)
    with torch.no_grad():
        _, off = M.vfnet_star(logits.to(dev).contiguous(memory_format=CL), 64, 8, 0.1)
    off = off.cpu().contiguous()
    s = R.sample_points(off.permute(0, 2, 3, 1).reshape(B * H * W, -1).double(), B, H, W, 3, 3, 1, 1, 1, 1)
    outside = (s.h <= -1) | (s.h >= H) | (s.w <= -1) | (s.w >= W)
    assert 0.3 < float(outside.double().mean()) < 0.95 and float(off.abs().max()) > 2 * max(H, W)
    leaves = [t.double().requires_grad_() for t in (x, off, w)]
    cols = R.im2col(leaves[0].permute(0, 2, 3, 1), leaves[1].permute(0, 2, 3, 1).reshape(B * H * W, -1), None, 3, 3, 1, 1, 1, 1)
    ref = torch.einsum('mkc,ock->mo', cols, leaves[2].reshape(Co, C, 9)).relu().reshape(B, H, W, Co).permute(0, 3, 1, 2)
    grads = torch.autograd.grad((ref * go.double()).sum(), leaves)
    xd, od, wd = (t.to(dev).contiguous(memory_format=CL).requires_grad_() for t in (x, off, w))
    y = deform_conv2d(xd, od, wd, 1, 1, 1, relu=True)
    torch.testing.assert_close(y.detach().cpu(), ref.detach().float(), rtol=1e-4, atol=1e-4)
    y.backward(go.to(dev))
    torch.testing.assert_close(xd.grad.cpu(), grads[0].float(), rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(od.grad.cpu(), grads[1].float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(wd.grad.cpu(), grads[2].float(), rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------------------------------------------- dispatch
def test_dispatch_rule_and_the_tensor_path_on_the_device(golden):
    """Each condition of _fused_loss_ok turned off takes the tensor path.  Where the condition does not change the arithmetic
    (NCHW maps, ignore boxes that touch no anchor, the switch) the device's tensor path gives the fixture's fp64 losses to 1e-5
    relative (fp32 sums of 34 000 terms in another order); where it does, it gives what its own fp64 run on the CPU gives."""
    g = golden('vfnet')
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou')
    cl = [_on_dev(ms) for ms in U.head_maps()]
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps()]
    far = [torch.tensor([[900., 900., 950., 950.]], device=dev) for _ in gts]
    assert head._fused_loss_ok(*cl, labels, None, metas)
    assert not head._fused_loss_ok(*nchw, labels, None, metas) and not head._fused_loss_ok(*cl, labels, far, metas)
    off = _head_on_device('giou')
    off.fused_loss = False
    assert not off._fused_loss_ok(*cl, labels, None, metas)
    for h, maps, ignore in ((head, nchw, None), (head, cl, far), (off, cl, None)):
        ls, calls = _spied(lambda: h.loss(*maps, gts, labels, metas, gt_bboxes_ignore=ignore))
        assert not any(n.startswith('htd_vfnet') for n in calls)
        mine = torch.stack([ls[k] for k in KEYS]).cpu().double()
        np.testing.assert_allclose(mine.numpy(), g['head.giou.loss64'], rtol=1e-5)
    small = [dict(metas[0]), dict(metas[1], img_shape=(104, 160, 3), pad_shape=(104, 160, 3))]
    nine_sizes, nine_strides = U.LEVEL_SIZES + ((1, 1), ) * 4, U.STRIDES + (256, 512, 1024, 2048)
    nine = dict(strides=list(nine_strides),
                anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                      center_offset=0.0, strides=list(nine_strides)))
    changed = dict(use_atss=(dict(use_atss=False), cl, metas),
                   use_vfl=(dict(use_vfl=False), cl, metas),
                   sync_num_pos=(dict(sync_num_pos=False), cl, metas),
                   pos_weight=(dict(train_cfg=dict(pos_weight=2.0), use_vfl=False), cl, metas),
                   pos_weight_vfl=(dict(train_cfg=dict(pos_weight=2.0)), cl, metas),
                   topk=(dict(train_cfg=dict(assigner=dict(type='ATSSAssigner', topk=17))), cl, metas),
                   diou=(dict(loss_bbox=dict(type='DIoULoss', loss_weight=1.5)), cl, metas),
                   diou_rf=(dict(loss_bbox_refine=dict(type='DIoULoss', loss_weight=2.0)), cl, metas),
                   fp64=(dict(), [[m.double() for m in ms] for ms in cl], metas),
                   invalid_anchors=(dict(), cl, small),
                   nine_levels=(nine, [_on_dev(ms) for ms in U.head_maps(sizes=nine_sizes, strides=nine_strides, tag='vfnet.nine',
                                                                         no_overlap=False)], metas))
    for name, (extra, maps, mt) in changed.items():
        h = _head_on_device('giou', **extra)
        assert not h._fused_loss_ok(*maps, labels, None, mt), name
        ls, calls = _spied(lambda: h.loss(*maps, gts, labels, mt))
        assert not any(n.startswith('htd_vfnet') for n in calls), name
        mine = torch.stack([ls[k] for k in KEYS]).cpu().double()
        ref = h.cpu().loss_tensor(*[[m.cpu().double() for m in ms] for ms in maps], [x.cpu() for x in gts], [x.cpu() for x in labels], mt)
        ref = torch.stack([ref[k] for k in KEYS])
        assert bool(torch.isfinite(ref).all()), name
        np.testing.assert_allclose(mine.numpy(), ref.numpy(), rtol=1e-5, err_msg=name)
    for extra in (dict(loss_cls=U._vfl(reduction='sum')), dict(loss_bbox=dict(type='GIoULoss', reduction='sum', loss_weight=1.5))):
        h = _head_on_device('giou', **extra)
        assert not h._fused_loss_ok(*cl, labels, None, metas)
        with pytest.raises(ValueError):                  # avg_factor with a sum reduction, in the reference too
            h.loss(*cl, gts, labels, metas)


# ---------------------------------------------------------------------------------------------------- inference
def test_get_bboxes_equals_the_fixture_and_batched_equals_the_per_image_loop(golden):
    """get_bboxes(with_nms=False) on the seeded maps: the fixture's boxes and score rows after the nms_pre cut on levels 0 and 1
    (same rows in the same order: the key gap at the cuts is 1e-3), from channels_last and from NCHW maps.  With NMS, the batched
    form -- one key launch, one segmented top-k, one NMS without score factors -- agrees BIT FOR BIT with the per-image loop at
    B = 2 and B = 5, images of different shapes and scale factors, the cuts to nms_pre (and none) and max_per_img active."""
    from htd_amd.registry import ConfigDict
    g = golden('vfnet')
    dev = torch.device(DEV)
    _, metas, _, _ = inputs(dev)
    head = _head_on_device('giou')
    maps = [_on_dev(ms) for ms in U.head_maps()]
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps()]
    for ms in (maps, nchw):
        res = head.get_bboxes(*ms, metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
        for i, (boxes, scores) in enumerate(res):
            np.testing.assert_allclose(boxes.cpu().numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-3)
            np.testing.assert_allclose(scores.double().sum(1).cpu().numpy(), g[f'head.score_rows{i}'], rtol=1e-5)
    H, W = 128, 160
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas5 = [dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), flip=False,
                   scale_factor=np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32)) for i, (h, w) in enumerate(shapes)]
    maps5 = [[torch.cat([m, m.flip(0) * 0.5, m[:1] * 0.0 + (-3.0 if k == 0 else 9.0)]).contiguous(memory_format=CL) for m in ms]
             for k, ms in enumerate(maps)]
    for nms_pre in (U.HEAD_TEST_CFG['nms_pre'], -1):
        cfg = ConfigDict(dict(U.HEAD_TEST_CFG, nms_pre=nms_pre, max_per_img=9, score_thr=0.02))
        for ms, mt in (([[m[:2] for m in x] for x in maps5], metas5[:2]), (maps5, metas5)):
            out = {}
            for mode in (True, False):
                head.batched_get_bboxes = mode
                out[mode], calls = _spied(lambda: head.get_bboxes(*ms, mt, cfg=cfg, rescale=True))
                assert calls.count('htd_retina_keys') == (0 if nms_pre < 0 else 1 if mode else len(mt))
            head.batched_get_bboxes = True
            counts = [int(d.shape[0]) for d, _ in out[False]]
            assert max(counts) == 9, counts
            for (d1, l1), (d2, l2) in zip(out[True], out[False]):
                assert torch.equal(d1, d2) and torch.equal(l1, l2)


def test_surface_refuses_bad_arguments():
    """Wrong shapes, dtypes, box kinds, more than 8 levels and CPU tensors raise before anything is launched."""
    from htd_amd import mmcv_ops as M
    dev = torch.device(DEV)
    cls, reg, ref = [_on_dev(ms) for ms in U.head_maps()]
    anchors = U.anchors_of().to(dev)
    gts = torch.zeros(2, 1, 4, device=dev)
    assigned = torch.zeros(2, anchors.size(0), dtype=torch.int32, device=dev)
    zeros = torch.zeros(2, anchors.size(0), device=dev)
    sums = torch.ones(3, device=dev)
    labels = torch.zeros(2, 1, dtype=torch.int64, device=dev)

    def refused(fn):
        with pytest.raises(ValueError):
            fn()
    refused(lambda: M.vfnet_star(cls[0], 64, 8, 0.1))                                       # 80 channels
    refused(lambda: M.vfnet_star(reg[0].double(), 64, 8, 0.1))
    refused(lambda: M.vfnet_star(reg[0], 64, 0, 0.1))                                       # stride 0
    refused(lambda: M.vfnet_quality(reg, ref, anchors, gts, assigned.long()))
    refused(lambda: M.vfnet_quality(reg, cls, anchors, gts, assigned))
    refused(lambda: M.vfnet_quality(reg, [m.double() for m in ref], anchors, gts, assigned))
    refused(lambda: M.vfnet_loss(cls, reg, ref, anchors, gts, labels.int(), assigned, zeros, zeros, sums, 2, 2))
    refused(lambda: M.vfnet_loss(cls, reg, ref, anchors, gts, labels, assigned, zeros, zeros, sums, 3, 2))       # DIoU
    refused(lambda: M.vfnet_loss(cls, reg, ref, anchors, gts, labels, assigned, zeros, zeros, sums, 2, 1))       # bounded IoU
    refused(lambda: M.vfnet_loss(cls, reg, ref, anchors, gts, labels, assigned, zeros, zeros, sums[:2], 2, 2))
    nine = [reg[4]] * 9
    refused(lambda: M.vfnet_quality(nine, nine, torch.zeros(18, 4, device=dev), gts, torch.zeros(2, 18, dtype=torch.int32, device=dev)))
    with pytest.raises(NotImplementedError):
        M.vfnet_star(U.head_maps()[1][0], 64, 8, 0.1)                                       # a CPU map
    iou_ini, iou_rf, s = M.vfnet_quality(reg, ref, anchors, gts, assigned)
    assert s.tolist() == [0.0, 0.0, 0.0] and float(iou_ini.abs().max()) == 0 and float(iou_rf.abs().max()) == 0


# ---------------------------------------------------------------------------------------------------- the detector
def small_cfg(g):
    from htd_amd.configs import vfnet_config
    cfg = vfnet_config()
    cfg.test_cfg.nms_pre = int(g['nms_pre'])
    return cfg


@pytest.fixture
def det(golden):
    """A detector of the test's own: nothing of it stays on the device when the test ends."""
    import gc
    from htd_amd import dense
    from htd_amd.configs import build_baseline_detector
    g = golden('vfnet')
    model = build_baseline_detector(cfg=small_cfg(g))
    yield U.load_fixture_weights_(model, float(g['cls_scale']), float(g['cls_bias_shift'])).to(torch.device(DEV))
    model.zero_grad(set_to_none=True)
    model.cpu()
    dense.new_step()
    gc.collect()
    torch.cuda.empty_cache()


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step; `assigned` equals the fixture's and the step reaches the kernels: five
    htd_vfnet_star_fwd and _bwd, one htd_atss_targets, htd_vfnet_quality, htd_vfnet_loss."""
    g = golden('vfnet')
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    losses, calls = _spied(lambda: det.forward_train(img, metas, gts, labels))
    assert [calls.count(n) for n in ENTRIES] == [1, 1, 1] and calls.count('htd_vfnet_star_fwd') == 5
    assigned, num_pos, norm = det.bbox_head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g['assigned']).long())
    assert num_pos.tolist() == g['num_pos'].tolist() and float(det.bbox_head._last_quality[2][0]) == float(g['num_pos'].sum())
    back = []
    D.check_train_step(det, g, '', 'vfnet', losses, ('loss_cls', 'loss_bbox', 'loss_bbox_rf'), U.grad_keys(det),
                       3 + len(U.EXTRA_GRAD_KEYS), zero_grad_ok=('.scales.', ), backward=lambda loss: back.extend(_spied(loss.backward)[1]))
    assert back.count('htd_vfnet_star_bwd') == 5


def test_outputs_and_detections_match_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_outputs and check_detections."""
    g = golden('vfnet')
    img, metas, _, _ = inputs(torch.device(DEV))
    worst = D.check_outputs(det, g, '', ('cls', 'reg', 'ref'), U.LEVEL_SIZES, img)
    det.eval()
    with torch.no_grad():
        res = det.simple_test(img, metas)
    print(f'vfnet: worst output ratio {worst:.3f}, worst detection ratio {D.check_detections(res, g, ""):.3f}')


def test_fused_and_tensor_path_train_steps_agree(det, golden):
    """The same step with the kernels switched off (tensor-form star offsets and loss): the same losses to 1e-4 relative -- both
    are fp32 evaluations of one function whose offsets differ by an ulp and whose 34 000-term sums run in another order."""
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    fused = det._parse_losses(det.forward_train(img, metas, gts, labels))[1]
    det.bbox_head.fused_loss = False
    losses, calls = _spied(lambda: det.forward_train(img, metas, gts, labels))
    assert not any(n.startswith('htd_vfnet') for n in calls)
    plain = det._parse_losses(losses)[1]
    for k in fused:
        np.testing.assert_allclose(fused[k], plain[k], rtol=1e-4, err_msg=k)


def test_reference_format_checkpoint_round_trip(golden, tmp_path):
    """dense_fixture_util.check_checkpoint_round_trip on the VFNet fixture."""
    from htd_amd.configs import build_baseline_detector
    g = golden('vfnet')
    state = U.fixture_state(g['state_keys'], g['state_shapes'], float(g['cls_scale']), float(g['cls_bias_shift']))
    img, metas, _, _ = inputs(torch.device(DEV))
    D.check_checkpoint_round_trip(lambda: build_baseline_detector(cfg=small_cfg(g)), state, g, '', img, metas, tmp_path, tol=1e-2)
