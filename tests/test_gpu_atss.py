"""ATSS on the GPU: htd_atss_targets and htd_atss_loss against the reference's own run (tests/golden/atss.npz) and against
ATSSAssigner / ATSSHead.loss_tensor (pinned against that fixture by tests/test_atss.py), the fused ATSSHead.loss against the
reference's fp64 run, the shared batched get_bboxes, and the ATSS detector against the reference's.

The bound of every value computed by a kernel is the project's rule (dense_fixture_util.bound): 4 x max(the reference's own fp32
error on that case, one fp32 ulp of the largest entry); the fp32 error comes from the fixture or from the fp32 run of the tensor
path, never from the code under test.  Assignments are compared bit for bit, the centerness targets under the rule of _check_ctr."""
import numpy as np
import pytest
import torch

import atss_util as U
import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T, bound as _bound, err as _err, leave_the_allocator_as_found  # noqa: F401
from golden_util import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last


def inputs(dev):
    return D.inputs(dev, U.detector_inputs)


# ---------------------------------------------------------------------------------------------------- the targets kernel
def _targets_raw(anchors, sizes, gts, valid, topk=U.TOPK):
    """htd_atss_targets on outputs pre-filled with -7 / NaN -> CPU tensors (assigned, ctr_targets, num_pos, norm)."""
    from htd_amd import capi, mmcv_ops as M
    from htd_amd.core.bbox import _d4
    dev = torch.device(DEV)
    anchors, gts, valid = anchors.to(dev).contiguous(), gts.to(dev).contiguous(), valid.to(dev).contiguous()
    B, K = valid.shape
    A = anchors.size(0)
    assigned = torch.full((B, A), -7, dtype=torch.int32, device=dev)
    ctr = torch.full((B, A), float('nan'), device=dev)
    num_pos = torch.full((B, ), -7, dtype=torch.int32, device=dev)
    norm = torch.full((3, ), float('nan'), device=dev)
    ws = torch.full((capi.lib().htd_atss_targets_workspace_bytes(B, A) // 8, ), float('nan'), dtype=torch.float64, device=dev)
    capi.call('htd_atss_targets', M._P(anchors), M._i64s(sizes), len(sizes), M._P(gts), M._P(valid), B, K, int(topk), _d4(U.MEANS),
              _d4(U.STDS), 16 / 1000, M._P(assigned), M._P(ctr), M._P(ws), M._P(num_pos), M._P(norm), M._S())
    torch.cuda.synchronize()
    return assigned.cpu(), ctr.cpu(), num_pos.cpu(), norm.cpu()


def _check_ctr(ctr, ltrb_ref, ctr_ref, pos):
    """The rule of test_gpu_fcos.py:_check_ctr on the reference's l, t, r, b: the kernel's divisions and square root are correctly
    rounded, the vectorised fp32 torch.sqrt of the reference's CPU run is not always, so the kernel equals the correctly rounded
    root of the reference's own fp32 product bit for bit and the reference's value within 2 fp32 ulps."""
    lr, tb = ltrb_ref[..., [0, 2]], ltrb_ref[..., [1, 3]]
    prod = (lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0])           # IEEE fp32 on the CPU
    rounded = torch.where(pos, prod.double().sqrt().float(), torch.zeros_like(prod))
    assert torch.equal(ctr, rounded)
    if ctr_ref is not None:
        assert bool(((ctr - ctr_ref).abs() <= 2 * EPS32 * ctr_ref).all())
    return rounded


def _check_counts(out, a_ref, rounded, B):
    assigned, ctr, num_pos, norm = out
    n = (a_ref > 0).sum(1)
    assert num_pos.tolist() == n.tolist()
    total = int(n.clamp(min=1).sum())
    assert float(norm[0]) == total and float(norm[1]) == total
    s64 = rounded.double().sum()
    e32 = abs(float(rounded.sum()) - float(s64))                # the fp32 sum of the same targets
    assert abs(float(norm[2]) - float(s64)) <= _bound(e32, s64.reshape(1)), (float(norm[2]), float(s64))


def _case(g, name):
    if name == 'head':
        _, _, gts, _ = U.detector_inputs()
        return [T(x) for x in gts], T(g['head.assigned']).long()
    if name == 'assignment':
        return U.assignment_case()[0], T(g['ac.assigned']).long()
    twin = U.twin_case()[0]
    return twin, (T(g['twin.assigned']).long() if bool(g['twin.ref_lower']) else None)


@pytest.mark.parametrize('name', ['head', 'assignment', 'twin'])
def test_targets_kernel_equals_the_reference(golden, name):
    """The head case (the reference's centerness targets too), the assignment case -- a gt centred on the map corner, one below the
    last anchor row, overlapping gts, a gt too small for any centre, levels of all-zero IoU, an image without gt, padded slots,
    ties inside the selected nine, the two levels shorter than topk -- and the identical gts: the reference's assignment bit for
    bit, every output element written, num_pos and norm right, two runs bitwise equal."""
    from htd_amd.core.bbox import ATSSAssigner
    g = golden('atss')
    gts, ref = _case(g, name)
    anchors = U.anchors_of()
    padded, valid, _ = U.pad_gts(gts)
    if ref is None:                             # (the reference did not take the lower index: the host class is the reference)
        a = ATSSAssigner(topk=U.TOPK)
        ref = torch.stack([a.assign(anchors.double(), list(U.LEVEL_ANCHORS), x.double()).gt_inds for x in gts])
    out = _targets_raw(anchors, U.LEVEL_ANCHORS, padded, valid)
    assert torch.equal(out[0].long(), ref)
    pos = ref > 0
    if name == 'head':
        rounded = _check_ctr(out[1], T(g['head.ltrb']), T(g['head.ctr_targets']), pos)
    else:
        rounded = _check_ctr(out[1], U.batch_ltrb(anchors, padded, ref, rounded=True), None, pos)
    _check_counts(out, ref, rounded, len(gts))
    if name == 'twin':
        assert int((out[0] == 1).sum()) > 0 and int((out[0] == 2).sum()) == 0
    again = _targets_raw(anchors, U.LEVEL_ANCHORS, padded, valid)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


@pytest.mark.parametrize('name', list(U.EXTRA_CASES))
def test_targets_kernel_threshold_cases(golden, name):
    """An IoU equal to the threshold is positive; the deviation is the unbiased one (the 'std' case has a positive under the biased
    deviation only): the reference's assignment."""
    g = golden('atss')
    sizes, strides, gts = U.EXTRA_CASES[name]
    ref = T(g[f'x.{name}.assigned']).long()
    out = _targets_raw(U.anchors_of(sizes, strides), [h * w for h, w in sizes], gts[None], torch.ones(1, 1, dtype=torch.bool))
    assert torch.equal(out[0].long(), ref) and ref.tolist() == dict(equal=[[1, 1]], std=[[0, 0, 0]])[name]
    assert out[2].tolist() == [int((ref > 0).sum())]


def _host_assign(anchors, sizes, gts_list, topk):
    from htd_amd.core.bbox import ATSSAssigner
    a = ATSSAssigner(topk=topk)
    return torch.stack([a.assign(anchors, list(sizes), x).gt_inds for x in gts_list])


def test_targets_kernel_ties_go_to_the_lower_index():
    """Four anchors at the same distance around the ninth place (and two on levels 1 and 2): ATSSAssigner's rule, (fp32 distance,
    anchor index), in fp32 on the CPU."""
    gts, _ = U.tie_case()
    anchors = U.anchors_of()
    padded, valid, _ = U.pad_gts(gts)
    out = _targets_raw(anchors, U.LEVEL_ANCHORS, padded, valid)
    ref = _host_assign(anchors, U.LEVEL_ANCHORS, gts, U.TOPK)
    assert torch.equal(out[0].long(), ref) and int((ref > 0).sum()) > 0


def _random_gts(B, K, tag, W=160., H=128.):
    c = seeded_tensor(f'{tag}.c', (B, K, 2), kind='rand') * torch.tensor([W, H])
    wh = seeded_tensor(f'{tag}.wh', (B, K, 2), kind='rand') * torch.tensor([W, H]) * 0.8 + 6.
    return torch.cat([c - wh / 2, c + wh / 2], -1)


@pytest.mark.parametrize('topk', [1, 9, 16])
@pytest.mark.parametrize('pyramid', ['five', 'one_anchor', 'short', 'eight', 'wide'])
def test_targets_kernel_shapes(pyramid, topk):
    """Seeded gts (fractional coordinates: no exact ties) on the five-level pyramid, on a single anchor (one candidate: a NaN
    threshold, no positive), on one level shorter than topk, on eight levels, and on a 40 x 50 first level (eight blocks of the
    second launch, 32 anchors per lane of the first): ATSSAssigner in fp32 on the CPU bit for bit -- its distances and IoUs are the
    same IEEE operations --, K = 7 with invalid slots."""
    sizes, strides = dict(five=(U.LEVEL_SIZES, U.STRIDES), one_anchor=(((1, 1), ), (8, )), short=(((2, 3), ), (32, )),
                          eight=(((8, 10), ) * 2 + ((4, 5), ) * 2 + ((2, 3), ) * 2 + ((1, 2), ) * 2, (16, 16, 32, 32, 64, 64, 128, 128)),
                          wide=(((40, 50), (20, 25), (10, 13)), (8, 16, 32)))[pyramid]
    anchors = U.anchors_of(sizes, strides)
    if pyramid == 'eight':                      # the twin levels differ: the second of each pair is shifted by a third of a stride
        at = 0
        for l, (h, w) in enumerate(sizes):
            if l % 2:
                anchors[at:at + h * w] += strides[l] / 3.
            at += h * w
    counts = [h * w for h, w in sizes]
    B, K = 3, 7
    gts = _random_gts(B, K, f'atss.tk.{pyramid}', *((400., 320.) if pyramid == 'wide' else (160., 128.)))
    valid = torch.ones(B, K, dtype=torch.bool)
    valid[0, 2] = valid[1, 5:] = False
    valid[2] = False
    out = _targets_raw(anchors, counts, gts, valid, topk)
    ref = torch.zeros(B, anchors.size(0), dtype=torch.long)
    for b in range(B):
        keep = valid[b].nonzero()[:, 0]
        if len(keep):
            r = _host_assign(anchors, counts, [gts[b, keep]], topk)[0]
            ref[b] = torch.where(r > 0, keep[(r - 1).clamp(min=0)] + 1, torch.zeros_like(r))
    assert torch.equal(out[0].long(), ref)
    rounded = _check_ctr(out[1], U.batch_ltrb(anchors, gts, ref, rounded=True), None, ref > 0)
    _check_counts(out, ref, rounded, B)
    if pyramid == 'one_anchor' or (pyramid == 'short' and topk == 1):
        assert int((ref > 0).sum()) == 0        # a single candidate per gt
    elif pyramid in ('five', 'eight', 'wide') and topk > 1:
        assert int((ref > 0).sum()) > 0


def test_targets_kernel_padded_and_permuted_gts(golden):
    """The assignment case with K padded from 6 to 11, the valid slots scattered and the gts permuted: the permuted result."""
    g = golden('atss')
    gts, _ = U.assignment_case()
    anchors = U.anchors_of()
    ref = T(g['ac.assigned']).long()
    K = 11
    padded, valid = torch.zeros(4, K, 4), torch.zeros(4, K, dtype=torch.bool)
    want = torch.zeros_like(ref)
    for b, x in enumerate(gts):
        slots = torch.from_numpy(np.random.RandomState(b).permutation(K)[:len(x)].copy())
        padded[b, slots], valid[b, slots] = x, True
        padded[b, ~valid[b]] = torch.tensor([40., 40., 90., 90.])               # what an invalid slot holds is not read as a gt
        if len(x):
            want[b] = torch.where(ref[b] > 0, slots[(ref[b] - 1).clamp(min=0)] + 1, torch.zeros_like(ref[b]))
    out = _targets_raw(anchors, U.LEVEL_ANCHORS, padded, valid)
    assert torch.equal(out[0].long(), want)
    assert out[2].tolist() == (ref > 0).sum(1).tolist()


def test_targets_surface_refuses_bad_arguments():
    from htd_amd import mmcv_ops as M
    dev = torch.device(DEV)
    anchors = U.anchors_of().to(dev)
    gts, valid = torch.zeros(1, 1, 4, device=dev), torch.zeros(1, 1, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError):
        M.atss_targets(anchors, U.LEVEL_ANCHORS, gts, valid, 17)
    with pytest.raises(ValueError):
        M.atss_targets(anchors, (1, ) * 9, gts, valid, 9)
    with pytest.raises(ValueError):
        M.atss_targets(anchors, U.LEVEL_ANCHORS[:-1], gts, valid, 9)
    a, c, n, norm = M.atss_targets(anchors, U.LEVEL_ANCHORS, gts, valid, 9)     # no valid gt
    assert int(a.abs().sum()) == 0 and float(c.abs().sum()) == 0 and norm.tolist() == [1.0, 1.0, 0.0]


# ---------------------------------------------------------------------------------------------------- the head loss
def _head_on_device(v, **extra):
    from test_atss import build_head
    return build_head(v, **extra).to(torch.device(DEV))


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_fused_head_loss_against_the_reference_fp64_run(golden, v, monkeypatch):
    """ATSSHead.loss (fused) on the seeded maps against the reference head's fp64 run under the rule, for both box losses; exactly one
    htd_atss_targets and one htd_atss_loss call; the assignment equals the reference's; two runs bitwise equal; after a warm call
    the fused path and its backward read nothing on the host (tensor reads made to raise, and the sync debug mode of torch set to
    'error')."""
    from htd_amd import capi
    from test_iou_losses import _no_host_reads
    g = golden('atss')
    p = f'head.{v}.'
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device(v)
    err = g[p + 'err32']
    runs = []
    for run in range(2):
        maps = [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        assert head._fused_loss_ok(*maps, labels, None, metas)
        calls, real = [], capi.call

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        capi.call = spy
        if run == 1:
            _no_host_reads(monkeypatch)
            torch.cuda.set_sync_debug_mode('error')
        try:
            ls = head.loss(*maps, gts, labels, metas)
            (ls['loss_cls'] + ls['loss_bbox'] + ls['loss_centerness']).backward()
        finally:
            torch.cuda.set_sync_debug_mode('default')
            monkeypatch.undo()
            capi.call = real
        assert calls.count('htd_atss_loss') == 1 and calls.count('htd_atss_targets') == 1
        runs.append(([ls[k].detach().clone() for k in ('loss_cls', 'loss_bbox', 'loss_centerness')],
                     [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in maps]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]))
    assigned, ctr_t, num_pos, norm = head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g['head.assigned']).long())
    _check_ctr(ctr_t.cpu(), T(g['head.ltrb']), T(g['head.ctr_targets']), T(g['head.assigned']) > 0)
    losses, grads = runs[0]
    worst = {}
    for i, name in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness')):
        ref = T(g[p + 'loss64'][i]).reshape(1).double()
        worst[name] = _err(losses[i].reshape(1), ref) / _bound(err[i], ref)
    for name, mine, ref, e32 in (('greg', grads[1], T(g[p + 'greg64']), err[4]), ('gctr', grads[2][..., 0], T(g[p + 'gctr64']), err[5])):
        worst[name] = _err(mine, ref) / _bound(e32, ref)
    ref = T(g[p + 'gcls64.sample'])
    worst['gcls'] = _err(T(BU.digest(grads[0])[1]), ref) / _bound(err[3], ref)
    print(f'head {v}: ' + ', '.join(f'{k} {x:.3f}' for k, x in worst.items()) + ' of the bound')
    assert max(worst.values()) <= 1.0, worst


def _tensor_runs(head, cls_maps, reg_maps, ctr_maps, gts, labels, metas):
    """loss_tensor on the CPU in fp64 and fp32 -> {dtype: (losses (3,), [gcls, greg, gctr] rows)}."""
    res = {}
    for dt in (torch.float64, torch.float32):
        maps = [[m.detach().cpu().to(dt).contiguous().requires_grad_() for m in ms] for ms in (cls_maps, reg_maps, ctr_maps)]
        ls = head.loss_tensor(*maps, [x.cpu().to(dt) for x in gts], [x.cpu() for x in labels], metas)
        ls = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])])
        ls.sum().backward()
        res[dt] = (ls.detach().double(), [U.maps_to_rows([m.grad for m in ms]).double() for ms in maps])
    return res


def _fused_run(head, maps, gts, labels, metas, scale=1.0):
    ls = head.loss(*maps, gts, labels, metas)
    ls = torch.stack([ls['loss_cls'], ls['loss_bbox'], ls['loss_centerness']])
    (ls * ls.new_tensor(scale)).sum().backward()            # scale: one factor, or one per loss
    return ls.detach().cpu().double()


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_fused_head_loss_against_the_tensor_path_with_padded_channels(v):
    """The fused form on maps that are channel slices of wider channels_last maps (84, 8 and 4 channels; C = 80 and, in the scalar
    form of the kernel, C = 3) against loss_tensor in fp64 on the same values, the bound from loss_tensor's own fp32 run; the slices
    are read in place (the gradients of the padding channels are exact zeros) and the hand-made rows -- a prediction equal to its
    target, deltas beyond the ratio clip, logits of +-90 -- stay finite."""
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    for C in (80, 3):
        head = _head_on_device(v, num_classes=C)
        lab = [x % C for x in labels]
        cls, reg, ctr = U.head_maps(C=C, tag=f'atss.pad.{C}')
        reg[0][0, :, 3, 4] = torch.tensor([0.5, -0.5, 30., -30.])              # beyond the clip of |log(16 / 1000)| / 0.2
        cls[1][1, 0, 2, 2], ctr[1][1, 0, 2, 2], ctr[0][0, 0, 8, 9] = 90., -90., 90.
        wide = [[torch.cat([m, seeded_tensor(f'atss.pad.{C}.{k}{l}', (2, pad, *m.shape[-2:]))], 1).to(dev).contiguous(memory_format=CL)
                 .requires_grad_() for l, m in enumerate(ms)] for k, (ms, pad) in enumerate(((cls, 4 if C == 80 else 2), (reg, 4), (ctr, 3)))]
        maps = [[m[:, :c] for m in ms] for ms, c in zip(wide, (C, 4, 1))]
        assert head._fused_loss_ok(*maps, lab, None, metas)
        mine = _fused_run(head, maps, gts, lab, metas)
        ref = _tensor_runs(head, cls, reg, ctr, gts, lab, metas)
        r64, r32 = ref[torch.float64], ref[torch.float32]
        assert torch.isfinite(mine).all() and torch.isfinite(r64[0]).all()
        for i in range(3):
            assert _err(mine[i].reshape(1), r64[0][i].reshape(1)) <= _bound(_err(r32[0][i].reshape(1), r64[0][i].reshape(1)), r64[0][i].reshape(1)), (C, i)
        for ms, c, a64, a32 in zip(wide, (C, 4, 1), r64[1], r32[1]):
            g = U.maps_to_rows([m.grad for m in ms]).cpu()
            assert torch.isfinite(g).all() and float(g[..., c:].abs().max()) == 0
            assert _err(g[..., :c], a64) <= _bound(_err(a32, a64), a64), (C, c)
        at = 3 * 20 + 4                         # the anchor of the deltas beyond the clip: they pass no gradient
        if int(head._last_targets[0][0, at]) > 0:
            assert float(U.maps_to_rows([m.grad for m in wide[1]])[0, at, 2:4].abs().max()) == 0


def test_fused_head_loss_without_positives_and_with_incoming_gradients():
    """No gt anywhere: the box and centerness losses and their gradients are exactly 0, the focal loss is averaged over the number
    of images.  Incoming gradients of 2, 3 and 5 on the three losses scale each kind of gradient map by its own factor exactly; a
    second backward through the same forward raises."""
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou')

    def fresh():
        return [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps()]
    maps = fresh()
    ls = _fused_run(head, maps, [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in labels], metas)
    assert float(ls[1]) == 0 and float(ls[2]) == 0 and float(ls[0]) > 0
    assert all(float(m.grad.abs().max()) == 0 for ms in maps[1:] for m in ms) and all(torch.isfinite(m.grad).all() for m in maps[0])
    ref = _tensor_runs(head, *U.head_maps(), [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in labels], metas)
    r64, r32 = ref[torch.float64][0][0].reshape(1), ref[torch.float32][0][0].reshape(1)
    assert _err(ls[0].reshape(1), r64) <= _bound(_err(r32, r64), r64)
    out = {}
    for scale in (1.0, (2.0, 3.0, 5.0)):
        maps = fresh()
        _fused_run(head, maps, gts, labels, metas, scale)
        out[scale] = [[m.grad.clone() for m in ms] for ms in maps]
    ones, scaled = out.values()
    assert all(any(float(x.abs().max()) > 0 for x in xs) for xs in ones)
    for xs, ys, f in zip(ones, scaled, (2.0, 3.0, 5.0)):     # each kind of map with its own factor
        for a, b in zip(xs, ys):
            assert torch.equal(a * f, b)
    maps = fresh()
    ls = head.loss(*maps, gts, labels, metas)
    total = ls['loss_cls'] + ls['loss_bbox'] + ls['loss_centerness']
    total.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()


def test_dispatch_rule_and_the_tensor_path_on_the_device(golden):
    """Three anchors per location, ignore boxes and NCHW-contiguous maps take the tensor path, which is still right on the device:
    against the fixture's fp64 losses (ignore boxes that touch no anchor, NCHW) and against its own fp64 run on the CPU (three
    anchors) to 1e-5 relative (fp32 sums of 34 000 focal terms in another order than the CPU's)."""
    g = golden('atss')
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou')
    cl = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps()]
    far = [torch.tensor([[900., 900., 950., 950.]], device=dev) for _ in gts]
    assert head._fused_loss_ok(*cl, labels, None, metas)
    assert not head._fused_loss_ok(*nchw, labels, None, metas) and not head._fused_loss_ok(*cl, labels, far, metas)
    for maps, ignore in ((nchw, None), (cl, far)):
        ls = head.loss(*maps, gts, labels, metas, gt_bboxes_ignore=ignore)
        assert isinstance(ls['loss_cls'], list)                                 # the tensor path's per-level lists
        mine = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])]).cpu().double()
        np.testing.assert_allclose(mine.numpy(), g['head.giou.loss64'], rtol=1e-5)
    three = _head_on_device('giou', anchor_generator=dict(type='AnchorGenerator', ratios=[0.5, 1.0, 2.0], octave_base_scale=8,
                                                          scales_per_octave=1, strides=list(U.STRIDES)))
    maps3 = [[seeded_tensor(f'atss.three.{k}{l}', (2, 3 * c, h, w), scale=s) for l, (h, w) in enumerate(U.LEVEL_SIZES)]
             for k, (c, s) in enumerate(((80, 2.0), (4, 1.5), (1, 1.5)))]
    dev3 = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in maps3]
    assert not three._fused_loss_ok(*dev3, labels, None, metas)
    ls = three.loss(*dev3, gts, labels, metas)
    mine = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])]).cpu().double()
    ref = three.loss_tensor(*[[m.double() for m in ms] for ms in maps3], [x.cpu().double() for x in gts], [x.cpu() for x in labels], metas)
    ref = torch.stack([sum(ref['loss_cls']), sum(ref['loss_bbox']), sum(ref['loss_centerness'])])
    np.testing.assert_allclose(mine.numpy(), ref.numpy(), rtol=1e-5)


def test_a_positive_label_weight_takes_the_tensor_path(golden):
    """train_cfg.pos_weight = 2 weighs the positives' focal rows by 2 on the tensor path; the kernel has label weight 1 only, so the
    rule refuses it.  The tensor path on the device against its own fp64 run on the CPU to 1e-5 relative (as above); loss_cls differs
    from the fixture's (pos_weight -1), the other two losses do not."""
    g = golden('atss')
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device('giou', train_cfg=dict(pos_weight=2.0))
    cl = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
    assert not head._fused_loss_ok(*cl, labels, None, metas)
    assert _head_on_device('giou', train_cfg=dict(pos_weight=-1))._fused_loss_ok(*cl, labels, None, metas)
    ls = head.loss(*cl, gts, labels, metas)
    assert isinstance(ls['loss_cls'], list)
    mine = torch.stack([sum(ls['loss_cls']), sum(ls['loss_bbox']), sum(ls['loss_centerness'])]).cpu().double()
    ref = head.loss_tensor(*[[m.double() for m in ms] for ms in U.head_maps()], [x.cpu().double() for x in gts],
                           [x.cpu() for x in labels], metas)
    ref = torch.stack([sum(ref['loss_cls']), sum(ref['loss_bbox']), sum(ref['loss_centerness'])])
    np.testing.assert_allclose(mine.numpy(), ref.numpy(), rtol=1e-5)
    want = g['head.giou.loss64']
    np.testing.assert_allclose(mine.numpy()[1:], want[1:], rtol=1e-5)
    assert float(mine[0]) > float(want[0]) * (1 + 1e-3)


# ---------------------------------------------------------------------------------------------------- boxes
def test_get_bboxes_equals_the_fixture_and_batched_equals_the_per_image_loop(golden):
    """get_bboxes(with_nms=False) on the seeded maps: the fixture's boxes, score rows and centerness after the nms_pre cut on
    levels 0 and 1 (same rows in the same order: the key gap at the cuts is 1e-3; values to fp32 rounding of exp and sigmoid on
    another machine: 1e-3 of a pixel, 1e-5 relative).  With NMS, the batched form -- one key launch, one segmented top-k, one NMS
    with the centerness as score factor -- agrees BIT FOR BIT with the per-image loop at B = 2 and B = 5, images of different
    shapes and scale factors, the cuts to nms_pre (and none) and max_per_img active."""
    from htd_amd import capi
    from htd_amd.registry import ConfigDict
    g = golden('atss')
    dev = torch.device(DEV)
    _, metas, _, _ = inputs(dev)
    head = _head_on_device('giou')
    maps = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
    res = head.get_bboxes(*maps, metas, cfg=ConfigDict(U.HEAD_TEST_CFG), with_nms=False)
    for i, (boxes, scores, ctrs) in enumerate(res):
        np.testing.assert_allclose(boxes.cpu().numpy(), g[f'head.boxes{i}'], rtol=0, atol=1e-3)
        np.testing.assert_allclose(ctrs.cpu().numpy(), g[f'head.ctrs{i}'], rtol=1e-5)
        np.testing.assert_allclose(scores.double().sum(1).cpu().numpy(), g[f'head.score_rows{i}'], rtol=1e-5)
    H, W = 128, 160
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas5 = [dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), flip=False,
                   scale_factor=np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32)) for i, (h, w) in enumerate(shapes)]
    maps5 = [[torch.cat([m, m.flip(0) * 0.5, m[:1] * 0.0 - 3.0]) .contiguous(memory_format=CL) for m in ms] for ms in maps]
    for nms_pre in (U.HEAD_TEST_CFG['nms_pre'], -1):
        cfg = ConfigDict(dict(U.HEAD_TEST_CFG, nms_pre=nms_pre, max_per_img=9, score_thr=0.02))
        for ms, mt in (([[m[:2] for m in x] for x in maps5], metas5[:2]), (maps5, metas5)):
            out = {}
            for mode in (True, False):
                head.batched_get_bboxes = mode
                calls, real = [], capi.call

                def spy(name, *a, **k):
                    calls.append(name)
                    return real(name, *a, **k)
                capi.call = spy
                try:
                    out[mode] = head.get_bboxes(*ms, mt, cfg=cfg, rescale=True)
                finally:
                    capi.call = real
                if nms_pre > 0:
                    assert calls.count('htd_fcos_keys') == (1 if mode else len(mt))
            head.batched_get_bboxes = True
            counts = [int(d.shape[0]) for d, _ in out[False]]
            assert max(counts) == 9, counts
            for (d1, l1), (d2, l2) in zip(out[True], out[False]):
                assert torch.equal(d1, d2) and torch.equal(l1, l2)


# ---------------------------------------------------------------------------------------------------- the detector
def small_cfg(g):
    from htd_amd.configs import atss_config
    cfg = atss_config()
    cfg.test_cfg.nms_pre = int(g['nms_pre'])
    return cfg


@pytest.fixture
def det(golden):
    """A detector of the test's own: nothing of it stays on the device when the test ends (the step registries of `dense` hold
    the weights of the last step until new_step())."""
    import gc
    from htd_amd import dense
    from htd_amd.configs import build_baseline_detector
    g = golden('atss')
    model = build_baseline_detector(cfg=small_cfg(g))
    yield U.load_fixture_weights_(model, float(g['cls_scale']), float(g['cls_bias_shift'])).to(torch.device(DEV))
    model.zero_grad(set_to_none=True)
    model.cpu()                                 # (pytest keeps the fixture's value until after this finaliser)
    dense.new_step()
    gc.collect()
    torch.cuda.empty_cache()


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step; `assigned` equals the fixture's and the step takes one htd_atss_targets
    and one htd_atss_loss."""
    g = golden('atss')
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    losses, calls = D.spied(lambda: det.forward_train(img, metas, gts, labels))
    assert calls.count('htd_atss_loss') == 1 and calls.count('htd_atss_targets') == 1
    assigned, _, num_pos, norm = det.bbox_head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g['assigned']).long())
    assert num_pos.tolist() == g['num_pos'].tolist() and float(norm[0]) == float(g['num_pos'].sum())
    D.check_train_step(det, g, '', 'atss', losses, ('loss_cls', 'loss_bbox', 'loss_centerness'), U.grad_keys(det),
                       3 + len(U.EXTRA_GRAD_KEYS), zero_grad_ok=('.scales.', ))


def test_outputs_and_detections_match_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_outputs and check_detections."""
    g = golden('atss')
    img, metas, _, _ = inputs(torch.device(DEV))
    worst = D.check_outputs(det, g, '', ('cls', 'reg', 'ctr'), U.LEVEL_SIZES, img)
    det.eval()
    with torch.no_grad():
        res = det.simple_test(img, metas)
    print(f'atss: worst output ratio {worst:.3f}, worst detection ratio {D.check_detections(res, g, ""):.3f}')


def test_reference_format_checkpoint_round_trip(golden, tmp_path):
    """dense_fixture_util.check_checkpoint_round_trip on the ATSS fixture."""
    from htd_amd.configs import build_baseline_detector
    g = golden('atss')
    state = U.fixture_state(g['state_keys'], g['state_shapes'], float(g['cls_scale']), float(g['cls_bias_shift']))
    img, metas, _, _ = inputs(torch.device(DEV))
    D.check_checkpoint_round_trip(lambda: build_baseline_detector(cfg=small_cfg(g)), state, g, '', img, metas, tmp_path, tol=1e-2)
