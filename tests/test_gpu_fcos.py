"""FCOS on the GPU: htd_fcos_targets / htd_fcos_loss / htd_fcos_keys at every form and edge against the reference's own run
(tests/golden/fcos.npz) and the restatements of fcos_util (pinned against that fixture by tests/test_fcos.py), the fused
FCOSHead.loss against the reference's fp64 run, and the FCOS detector against the reference's.

The bound of every value computed by a kernel is the project's rule (dense_fixture_util.bound):
4 x max(the reference's own fp32 error on that case, one fp32 ulp of the largest entry); the fp32 error comes from the fixture or
from the fp32 run of the formula, never from the code under test.  Assignments and distances are compared bit for bit, the
centerness targets under the rule of _check_ctr."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T, bound as _bound, err as _err
import fcos_util as U
from golden_util import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last
PYRAMIDS = dict(five=(U.LEVEL_SIZES, U.STRIDES, U.SMALL_RANGES, 2), one=(((1, 1), ), (8, ), ((-1, U.INF), ), 1))


# ---------------------------------------------------------------------------------------------------- the targets kernel
def _targets_raw(sizes, strides, ranges, gts, valid, cs, radius, norm):
    """htd_fcos_targets on outputs pre-filled with -7 / NaN -> CPU tensors (assigned, bbox_targets, ctr_targets, num_pos, norm)."""
    from htd_amd import capi, mmcv_ops as M
    dev = torch.device(DEV)
    gts, valid = gts.to(dev).contiguous(), valid.to(dev).contiguous()
    B, K = valid.shape
    hw, st, P = M._fcos_levels(sizes, strides)
    rg = (ctypes.c_float * (2 * len(ranges)))(*[float(v) for r in ranges for v in r])
    assigned = torch.full((B, P), -7, dtype=torch.int32, device=dev)
    bt = torch.full((B, P, 4), float('nan'), device=dev)
    ctr = torch.full((B, P), float('nan'), device=dev)
    num_pos = torch.full((B, ), -7, dtype=torch.int32, device=dev)
    norm_t = torch.full((3, ), float('nan'), device=dev)
    ws = torch.full((capi.lib().htd_fcos_targets_workspace_bytes(B, P) // 8, ), float('nan'), dtype=torch.float64, device=dev)
    capi.call('htd_fcos_targets', hw, st, rg, len(sizes), M._P(gts), M._P(valid), B, K, int(cs), float(radius), int(norm),
              M._P(assigned), M._P(bt), M._P(ctr), M._P(ws), M._P(num_pos), M._P(norm_t), M._S())
    torch.cuda.synchronize()
    return assigned.cpu(), bt.cpu(), ctr.cpu(), num_pos.cpu(), norm_t.cpu()


def _check_ctr(ctr, bt_ref, ctr_ref, pos):
    """The centerness targets: the kernel's divisions and square root are correctly rounded, the vectorised fp32 torch.sqrt of the
    reference's CPU run is not (one ulp off the rounded fp64 root on about 0.6 % of its inputs), so the kernel equals the
    correctly rounded root of the reference's own fp32 product bit for bit and the reference's value within 2 fp32 ulps."""
    lr, tb = bt_ref[..., [0, 2]], bt_ref[..., [1, 3]]
    prod = (lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0])           # IEEE fp32 on the CPU
    rounded = torch.where(pos, prod.double().sqrt().float(), torch.zeros_like(prod))
    assert torch.equal(ctr, rounded)
    assert float((ctr.double() - ctr_ref.double()).abs().max()) <= 2 * EPS32 * max(float(ctr_ref.max()), 1e-30)
    assert bool(((ctr - ctr_ref).abs() <= 2 * EPS32 * ctr_ref).all())
    return rounded


def _check_targets(out, ref, B):
    assigned, bt, ctr, num_pos, norm = out
    a_ref, bt_ref, ctr_ref = ref
    assert torch.equal(assigned.long(), a_ref.long())
    assert torch.equal(bt, bt_ref)                              # every element written: no NaN of the pre-fill is left
    rounded = _check_ctr(ctr, bt_ref, ctr_ref, a_ref > 0)
    n = (a_ref > 0).sum(1)
    assert num_pos.tolist() == n.tolist()
    total = int(n.sum())
    assert float(norm[0]) == total + B and float(norm[1]) == max(total, 1)
    s64 = rounded.double().sum()
    e32 = abs(float(rounded.sum()) - float(s64))                # the fp32 sum of the same targets
    assert abs(float(norm[2]) - float(s64)) <= _bound(e32, s64.reshape(1)), (float(norm[2]), float(s64))


@pytest.mark.parametrize('B', [4, 2])
@pytest.mark.parametrize('c', range(len(U.TARGET_COMBOS)))
def test_targets_kernel_equals_the_reference_on_the_targets_case(golden, c, B):
    """An empty image beside full ones, nested boxes, equal areas, a point on an edge, boxes past the image and a largest distance
    on every range bound: the reference's fp32 run bit for bit, twice."""
    g = golden('fcos')
    cs, norm = U.TARGET_COMBOS[c]
    gts, _ = U.targets_case()
    padded, valid, _ = U.pad_gts(gts[:B])
    ref = tuple(T(g[f'tc.{c}.{k}'])[:B] for k in ('assigned', 'bbox_targets', 'ctr_targets'))
    out = _targets_raw(U.LEVEL_SIZES, U.STRIDES, U.SMALL_RANGES, padded, valid, cs, U.CASE_RADIUS, norm)
    _check_targets(out, ref, B)
    again = _targets_raw(U.LEVEL_SIZES, U.STRIDES, U.SMALL_RANGES, padded, valid, cs, U.CASE_RADIUS, norm)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def _random_gts(B, K, tag):
    """K seeded boxes per image around a 128 x 160 image, some past it; slot 2 repeats slot 0 (equal areas: the lower index wins)
    and slot 1 is cut to an edge through points of the finest level."""
    if K == 0:
        return torch.zeros(B, 1, 4), torch.zeros(B, 1, dtype=torch.bool)
    c = seeded_tensor(f'{tag}.c', (B, K, 2), kind='rand') * torch.tensor([180., 150.]) - 10.
    wh = seeded_tensor(f'{tag}.wh', (B, K, 2), kind='rand') * 90. + 3.
    gts = torch.cat([c - wh / 2, c + wh / 2], -1).round()
    if K >= 3:
        gts[:, 2] = gts[:, 0]
        gts[:, 1, 0] = 20.
    return gts, torch.ones(B, K, dtype=torch.bool)


@pytest.mark.parametrize('pyramid', list(PYRAMIDS))
@pytest.mark.parametrize('c', range(len(U.TARGET_COMBOS)))
@pytest.mark.parametrize('K', [0, 1, 3, 257])
def test_targets_kernel_shapes(K, c, pyramid):
    """No gt anywhere, one, three and 257 (more than one LDS chunk) on the five-level pyramid at B = 2 and on a single 1 x 1 level
    at B = 1, with the default ranges scaled / open and both radii: the fp32 restatement of the reference bit for bit."""
    sizes, strides, ranges, B = PYRAMIDS[pyramid]
    cs, norm = U.TARGET_COMBOS[c]
    gts, valid = _random_gts(B, K, f'fcos.tk.{K}.{pyramid}')
    if pyramid == 'one' and K:
        gts[0, 0] = torch.tensor([-3., -2., 9., 11.])           # holds the level's only point (4, 4)
    if K == 257:
        valid[-1, 200:] = False                                 # images of different lengths
    radius = 1.5 if K == 257 else U.CASE_RADIUS
    ref = U.targets_ref(sizes, strides, ranges, gts, valid, cs, radius, norm)
    out = _targets_raw(sizes, strides, ranges, gts, valid, cs, radius, norm)
    _check_targets(out, ref, B)
    if K:
        assert int(out[3].sum()) > 0


# ---------------------------------------------------------------------------------------------------- the loss kernel
def _loss_case(pyramid, C, kind, tag):
    """Seeded maps with padding channels on the five-level pyramid, the assignment of seeded gts, and hand-made positives: one
    whose prediction equals its target, one whose prediction misses its target (IoU 0: the clamp and the lift), one with
    distances of 1e4; logits of +-90 in the classification and centerness maps."""
    sizes, strides, ranges, B = PYRAMIDS[pyramid]
    pad = (0, 0, 0) if pyramid == 'one' else ((4 if C % 4 == 0 else 3), 4, 3)
    norm = kind == 'giou'
    gts, valid = _random_gts(B, 5, tag + '.gts')
    if pyramid == 'one':
        gts[0, 0] = torch.tensor([-3., -2., 9., 11.])
    labels = (seeded_tensor(tag + '.lab', (B, 5), kind='rand') * C).long().clamp(max=C - 1)
    assigned, bt, ctr_t = U.targets_ref(sizes, strides, ranges, gts, valid, norm, U.CASE_RADIUS, norm)
    full = dict(cls=[seeded_tensor(f'{tag}.cls{l}', (B, C + pad[0], h, w), scale=2.0) - 1.0 for l, (h, w) in enumerate(sizes)],
                reg=[seeded_tensor(f'{tag}.reg{l}', (B, 4 + pad[1], h, w), scale=0.5).exp() * (1.5 if norm else 1.5 * strides[l])
                     for l, (h, w) in enumerate(sizes)],
                ctr=[seeded_tensor(f'{tag}.ctr{l}', (B, 1 + pad[2], h, w), scale=1.5) for l, (h, w) in enumerate(sizes)])
    # hand-made rows, written through the (B, P, c) view of the maps
    rows = {k: U.maps_to_rows(v) for k, v in full.items()}
    pos = (assigned > 0).nonzero()
    assert len(pos) >= (1 if pyramid == 'one' else 4)
    b0, p0 = pos[0]
    rows['reg'][b0, p0, :4] = bt[b0, p0]                        # prediction == target
    rows['ctr'][b0, p0, 0] = 90.
    rows['cls'][b0, p0, 0] = -90.
    if len(pos) >= 4:
        b1, p1 = pos[1]
        rows['reg'][b1, p1, :4] = torch.tensor([-1e3, -1e3, 1.2e3, 1.2e3])          # a box far from its point and its target
        rows['ctr'][b1, p1, 0] = -90.
        b2, p2 = pos[2]
        rows['reg'][b2, p2, :4] = torch.tensor([1e4, 9e3, 1e4, 8e3])
        b3, p3 = pos[3]
        rows['cls'][b3, p3, int(labels[b3, int(assigned[b3, p3]) - 1])] = 90.
    rows['cls'][0, -1, C - 1] = 90.
    maps = {}
    at = 0
    for l, (h, w) in enumerate(sizes):
        for k in full:
            m = rows[k][:, at:at + h * w].reshape(B, h, w, -1).permute(0, 3, 1, 2)
            maps.setdefault(k, []).append(m.contiguous(memory_format=CL))
        at += h * w
    return dict(sizes=sizes, strides=strides, B=B, C=C, maps=maps, labels=labels, assigned=assigned, bt=bt, ctr_t=ctr_t)


def _loss_raw(case, kind, gamma, alpha, weights, assigned=None):
    """htd_fcos_loss on the (possibly sliced) device maps with gradient buffers pre-filled with NaN -> losses (3,) fp64 and the
    three lists of full-width gradient maps, on the CPU."""
    from htd_amd import capi, mmcv_ops as M
    dev = torch.device(DEV)
    C, B = case['C'], case['B']
    wide = {k: [m.to(dev).contiguous(memory_format=CL) for m in v] for k, v in case['maps'].items()}
    view = dict(cls=[m[:, :C] for m in wide['cls']], reg=[m[:, :4] for m in wide['reg']], ctr=[m[:, :1] for m in wide['ctr']])
    grads = {k: [torch.full_like(m, float('nan')) for m in v] for k, v in wide.items()}
    gview = dict(cls=[m[:, :C] for m in grads['cls']], reg=[m[:, :4] for m in grads['reg']], ctr=[m[:, :1] for m in grads['ctr']])
    assert all(M.nhwc_channel_stride(a) == b.size(1) for k in view for a, b in zip(view[k], wide[k]))
    hw, st, P = M._fcos_levels(case['sizes'], case['strides'])
    tabs = [M._level_tables(view[k]) for k in ('cls', 'reg', 'ctr')]
    gtabs = [M._level_tables(gview[k])[0] for k in ('cls', 'reg', 'ctr')]
    assigned = (case['assigned'] if assigned is None else assigned).to(dev).to(torch.int32).contiguous()
    bt, ctr_t, labels = case['bt'].to(dev).contiguous(), case['ctr_t'].to(dev).contiguous(), case['labels'].to(dev).contiguous()
    n = int((assigned > 0).sum())
    norm = torch.tensor([n + B, max(n, 1), float(ctr_t[assigned > 0].double().sum())], dtype=torch.float32, device=dev)
    rows = capi.lib().htd_fcos_loss_partial_rows()
    partial = torch.full((rows, 2), float('nan'), device=dev)
    capi.call('htd_fcos_loss', tabs[0][0], tabs[0][1], tabs[1][0], tabs[1][1], tabs[2][0], tabs[2][1], hw, st, len(case['sizes']), B,
              C, M._P(labels), labels.size(1), M._P(assigned), M._P(bt), M._P(ctr_t), M._P(norm), M.FCOS_BOX_KINDS[kind], 1e-6,
              float(gamma), float(alpha), float(weights[0]), float(weights[1]), float(weights[2]), M._P(partial), gtabs[0],
              gtabs[1], gtabs[2], M._S())
    torch.cuda.synchronize()
    s = partial.double().view(2, rows // 2, 2).sum(1).cpu()
    nm = norm.double().cpu()
    losses = torch.stack([weights[0] * s[0, 0] / nm[0], weights[1] * s[0, 1] / nm[2] if n else s[0, 1],
                          weights[2] * s[1, 0] / nm[1]])
    assert float(s[1, 1]) == 0
    return losses, {k: [m.cpu() for m in v] for k, v in grads.items()}


@pytest.mark.parametrize('pyramid', list(PYRAMIDS))
@pytest.mark.parametrize('kind', ['IoULoss', 'GIoULoss'])
@pytest.mark.parametrize('C', [1, 3, 80, 81])
def test_loss_kernel_against_the_fp64_formula(C, kind, pyramid):
    """The VEC = 4 and scalar forms, both box losses, gamma 2 and 1.5, loss weights != 1, maps that are channel slices of wider
    ones: the three losses and every element of the three gradient maps within the bound of the fp64 formula; padding channels
    and non-positive points hold exact zeros; everything finite; two runs bitwise equal."""
    short = 'iou' if kind == 'IoULoss' else 'giou'
    case = _loss_case(pyramid, C, short, f'fcos.lk.{C}.{pyramid}')
    gamma = 2.0 if C in (1, 80) else 1.5
    weights = (1.0, 1.0, 1.0) if C in (1, 81) else (0.5, 2.0, 1.5)
    sl = dict(cls=C, reg=4, ctr=1)
    args = ([m[:, :C] for m in case['maps']['cls']], [m[:, :4] for m in case['maps']['reg']], [m[:, :1] for m in case['maps']['ctr']],
            case['strides'], case['labels'], case['assigned'], case['bt'], case['ctr_t'])
    r64 = U.loss_ref(*args, kind=short, gamma=gamma, alpha=0.25, weights=weights)
    r32 = U.loss_ref(*args, kind=short, gamma=gamma, alpha=0.25, weights=weights, dtype=torch.float32)
    losses, grads = _loss_raw(case, kind, gamma, 0.25, weights)
    again = _loss_raw(case, kind, gamma, 0.25, weights)
    assert torch.equal(losses, again[0]) and all(torch.equal(a, b) for k in grads for a, b in zip(grads[k], again[1][k]))
    assert torch.isfinite(losses).all() and torch.isfinite(r64['losses']).all()
    worst = {}
    for i, name in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness')):
        ref = r64['losses'][i].reshape(1)
        e, e32 = _err(losses[i].reshape(1), ref), _err(r32['losses'][i].reshape(1), ref)
        worst[name] = e / max(_bound(e32, ref), 1e-300)
        assert e <= _bound(e32, ref), (name, e, e32, float(ref))
    for k, rk in (('cls', 'gcls'), ('reg', 'greg'), ('ctr', 'gctr')):
        ref = torch.cat([m.reshape(-1) for m in r64[rk]])
        e32 = _err(torch.cat([m.reshape(-1) for m in r32[rk]]), ref)
        mine = torch.cat([m[:, :sl[k]].reshape(-1) for m in grads[k]])
        assert torch.isfinite(mine).all()
        assert all(float(m[:, sl[k]:].abs().max()) == 0 for m in grads[k] if m.size(1) > sl[k]), k      # padding: exact zeros
        worst['g' + k] = _err(mine, ref) / max(_bound(e32, ref), 1e-300)
        assert _err(mine, ref) <= _bound(e32, ref), (k, _err(mine, ref), e32)
    neg = case['assigned'] <= 0
    if bool(neg.any()):
        assert float(U.maps_to_rows(grads['reg'])[neg].abs().max()) == 0 and float(U.maps_to_rows(grads['ctr'])[neg].abs().max()) == 0
    print(f'C {C} {kind} {pyramid}: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + ' of the bound')


@pytest.mark.parametrize('kind', ['IoULoss', 'GIoULoss'])
def test_loss_kernel_without_positives(kind):
    """No positive point: the box and centerness losses are exactly 0 with exactly zero gradients (the reference's
    `pos_bbox_preds.sum()` branch); the focal loss is averaged over the number of images."""
    case = _loss_case('five', 80, 'iou', 'fcos.lk.zero')
    none = torch.zeros_like(case['assigned'])
    losses, grads = _loss_raw(case, kind, 2.0, 0.25, (1.0, 1.0, 1.0), assigned=none)
    assert float(losses[1]) == 0 and float(losses[2]) == 0 and float(losses[0]) > 0
    assert all(float(m.abs().max()) == 0 for k in ('reg', 'ctr') for m in grads[k])
    args = ([m[:, :80] for m in case['maps']['cls']], [m[:, :4] for m in case['maps']['reg']], [m[:, :1] for m in case['maps']['ctr']],
            case['strides'], case['labels'], none, case['bt'], case['ctr_t'])
    r64, r32 = U.loss_ref(*args), U.loss_ref(*args, dtype=torch.float32)
    ref = r64['losses'][0].reshape(1)
    assert _err(losses[0].reshape(1), ref) <= _bound(_err(r32['losses'][0].reshape(1), ref), ref)


def test_loss_surface_scales_incoming_gradients_and_refuses_a_second_backward():
    from htd_amd import mmcv_ops as M
    case = _loss_case('five', 80, 'iou', 'fcos.lk.auto')
    dev = torch.device(DEV)
    tg = [case[k].to(dev) for k in ('labels', 'assigned', 'bt', 'ctr_t')]
    tg[1] = tg[1].to(torch.int32)
    n = int((tg[1] > 0).sum())
    norm = torch.tensor([n + 2, max(n, 1), float(tg[3][tg[1] > 0].double().sum())], dtype=torch.float32, device=dev)
    out = {}
    for scale in ((1.0, 1.0, 1.0), (2.0, 3.0, 5.0)):        # one factor per loss: a swap of two factors or widths would show
        maps = [[m[:, :c].to(dev).contiguous(memory_format=CL).requires_grad_() for m in case['maps'][k]]
                for k, c in (('cls', 80), ('reg', 4), ('ctr', 1))]
        ls = M.fcos_loss(*maps, case['strides'], tg[0], tg[1], tg[2], tg[3], norm, M.FCOS_BOX_KINDS['IoULoss'])
        total = scale[0] * ls[0] + scale[1] * ls[1] + scale[2] * ls[2]
        total.backward(retain_graph=True)
        out[scale] = [[m.grad.clone() for m in ms] for ms in maps]
        assert all(torch.isfinite(x).all() for xs in out[scale] for x in xs)
    ones, scaled = out.values()
    assert all(any(float(x.abs().max()) > 0 for x in xs) for xs in ones)
    for xs, ys, f in zip(ones, scaled, (2.0, 3.0, 5.0)):     # each kind of map with its own factor
        for a, b in zip(xs, ys):
            assert torch.equal(a * f, b)
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()


def test_keys_kernel_against_the_tensor_formula():
    """max_c sigmoid(cls) * sigmoid(centerness) of every point of every level, on sliced maps and at C = 3 / 80: within 5 fp32
    epsilons of the tensor formula in fp64 (each fp32 sigmoid 1 / (1 + exp(-x)): exp to an ulp, a sum and a quotient rounded, 2
    epsilons; two of them and the rounded product: 4.5), identical between whole-batch and per-image calls."""
    from htd_amd import mmcv_ops as M
    dev = torch.device(DEV)
    for C in (3, 80):
        case = _loss_case('five', C, 'iou', f'fcos.keys.{C}')
        cls = [m.to(dev).contiguous(memory_format=CL)[:, :C] for m in case['maps']['cls']]
        ctr = [m.to(dev).contiguous(memory_format=CL)[:, :1] for m in case['maps']['ctr']]
        keys = M.fcos_keys(cls, ctr, case['strides'])
        ref = (U.maps_to_rows([c.double() for c in cls]).sigmoid() * U.maps_to_rows([c.double() for c in ctr]).sigmoid()).max(-1)[0]
        assert keys.shape == ref.shape == (2, 428)
        assert bool(((keys.double() - ref).abs() <= 5 * EPS32 * ref + 1.2e-38).all())      # (+ the smallest normal: sigmoid(-90))
        for b in range(2):
            one = M.fcos_keys([c[b][None] for c in cls], [c[b][None] for c in ctr], case['strides'])
            assert torch.equal(one[0], keys[b])


# ---------------------------------------------------------------------------------------------------- the head
def _head_on_device(v):
    from htd_amd.registry import build_head
    import htd_amd.detector  # noqa: F401
    return build_head(U.head_cfg(v)).to(torch.device(DEV))


def inputs(dev):
    return D.inputs(dev, BU.detector_inputs)


@pytest.mark.parametrize('v', list(U.HEAD_VARIANTS))
def test_fused_head_loss_against_the_reference_fp64_run(golden, v, monkeypatch):
    """FCOSHead.loss (fused) on the seeded maps against the reference head's fp64 run under the rule, for both variants; the
    assignment equals the reference's; two runs bitwise equal; after a warm call the fused path and its backward read nothing on
    the host (tensor reads made to raise, and the sync debug mode of torch set to 'error')."""
    from htd_amd import capi
    from test_iou_losses import _no_host_reads
    g = golden('fcos')
    p = f'head.{v}.'
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device(v)
    err = g[p + 'err32']
    runs = []
    for run in range(2):
        maps = [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps(v)]
        assert head._fused_loss_ok(*maps)
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
        assert calls.count('htd_fcos_loss') == 1 and calls.count('htd_fcos_targets') == 1
        runs.append(([ls[k].detach().clone() for k in ('loss_cls', 'loss_bbox', 'loss_centerness')],
                     [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in maps]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]))
    assigned, bt, ctr_t, num_pos, norm = head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g[p + 'assigned']).long())
    assert torch.equal(bt.cpu(), T(g[p + 'bbox_targets']))
    _check_ctr(ctr_t.cpu(), T(g[p + 'bbox_targets']), T(g[p + 'ctr_targets']), T(g[p + 'assigned']) > 0)
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


def test_fused_head_loss_against_the_tensor_path_on_the_same_device_maps():
    """The fused form against loss_tensor run in fp64 on the same maps, the bound from loss_tensor's own fp32 run; maps that are not
    channels_last take the tensor form."""
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    for v in U.HEAD_VARIANTS:
        head = _head_on_device(v)
        res = {}
        for mode, dt, where in (('fused', torch.float32, dev), ('t64', torch.float64, 'cpu'), ('t32', torch.float32, 'cpu')):
            maps = [[m.to(where).to(dt) for m in ms] for ms in U.head_maps(v)]
            if mode == 'fused':
                maps = [[m.contiguous(memory_format=CL) for m in ms] for ms in maps]
            maps = [[m.requires_grad_() for m in ms] for ms in maps]
            fn = head.loss if mode == 'fused' else head.loss_tensor
            ls = fn(*maps, [x.to(where).to(dt) for x in gts], [x.to(where) for x in labels], metas)
            ls = torch.stack([ls['loss_cls'], ls['loss_bbox'], ls['loss_centerness']])
            ls.sum().backward()
            res[mode] = (ls.detach().cpu().double(), [U.maps_to_rows([m.grad for m in ms]).cpu().double() for ms in maps])
        for i in range(3):
            ref = res['t64'][0][i].reshape(1)
            assert _err(res['fused'][0][i].reshape(1), ref) <= _bound(_err(res['t32'][0][i].reshape(1), ref), ref), (v, i)
        for a, r64, r32 in zip(res['fused'][1], res['t64'][1], res['t32'][1]):
            assert _err(a, r64) <= _bound(_err(r32, r64), r64), v
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps('iou')]
    assert not head._fused_loss_ok(*nchw)


# ---------------------------------------------------------------------------------------------------- the detector
def small_cfg(g):
    from htd_amd.configs import fcos_config
    cfg = fcos_config()
    cfg.test_cfg.nms_pre = int(g['nms_pre'])
    return cfg


@pytest.fixture(scope='module')
def det(golden):
    from htd_amd.configs import build_baseline_detector
    g = golden('fcos')
    model = build_baseline_detector(cfg=small_cfg(g))
    return U.load_fixture_weights_(model, float(g['cls_scale']), float(g['cls_bias_shift'])).to(torch.device(DEV))


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step; `assigned` equals the fixture's and the step takes one htd_fcos_targets
    and one htd_fcos_loss."""
    g = golden('fcos')
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    losses, calls = D.spied(lambda: det.forward_train(img, metas, gts, labels))
    assert calls.count('htd_fcos_loss') == 1 and calls.count('htd_fcos_targets') == 1
    assigned, _, _, num_pos, norm = det.bbox_head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g['assigned']).long())
    assert num_pos.tolist() == g['num_pos'].tolist() and float(norm[0]) == float(g['num_pos'].sum()) + 2
    keys = U.grad_keys(det)
    assert len(keys) == 3 + len(U.EXTRA_GRAD_KEYS), keys        # (the backbone's BatchNorm parameters are frozen in this config)
    D.check_train_step(det, g, '', 'fcos', losses, ('loss_cls', 'loss_bbox', 'loss_centerness'), keys, len(keys),
                       zero_grad_ok=('.scales.', ))


def test_outputs_and_detections_match_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_outputs (the distances are exponentials) and check_detections.  The pyramid crosses
    the GroupNorm dispatch boundary (only 16 x 20 has more than 196 pixels), so both GroupNorm kernels are in it."""
    g = golden('fcos')
    img, metas, _, _ = inputs(torch.device(DEV))
    worst = D.check_outputs(det, g, '', ('cls', 'reg', 'ctr'), U.LEVEL_SIZES, img)
    det.eval()
    with torch.no_grad():
        res = det.simple_test(img, metas)
    print(f'fcos: worst output ratio {worst:.3f}, worst detection ratio {D.check_detections(res, g, ""):.3f}')


def test_towers_on_the_smallest_levels_equal_torch_group_norm(det):
    """ConvModule's GroupNorm branch on the 2 x 3 and 1 x 2 levels (under the whole-map dispatch boundary) and on 16 x 20 (over it)
    against torch's conv2d + group_norm + relu in fp64."""
    import torch.nn.functional as F
    dev = torch.device(DEV)
    m = det.bbox_head.cls_convs[0]
    for h, w in ((16, 20), (2, 3), (1, 2)):
        x = seeded_tensor(f'fcos.tower.{h}', (2, 256, h, w)).to(dev).contiguous(memory_format=CL)
        with torch.no_grad():
            y = m(x)
        ref = F.relu(F.group_norm(F.conv2d(x.cpu().double(), m.conv.weight.detach().cpu().double(), None, 1, 1), 32,
                                  m.gn.weight.detach().cpu().double(), m.gn.bias.detach().cpu().double(), m.gn.eps))
        assert y.shape == ref.shape
        assert _err(y, ref) <= 2e-4 * max(1.0, float(ref.abs().max())), (h, w)


@pytest.mark.parametrize('nms_pre', ['fixture', -1])
@pytest.mark.parametrize('scale', ['array', None])
def test_batched_get_bboxes_equals_the_per_image_loop(det, golden, scale, nms_pre):
    """get_bboxes of the whole batch -- one key launch, one segmented top-k, one NMS with the centerness as score factor -- agrees
    BIT FOR BIT with the per-image loop: B = 2 and B = 5, images of different shapes and scale factors, a blank image, the cuts to
    nms_pre (and none: nms_pre <= 0) and max_per_img active.  NCHW-contiguous copies of the maps give, in both forms, exactly
    what the head's own channels_last maps give."""
    img, _, _, _ = inputs(torch.device(DEV))
    H, W = img.shape[-2:]
    img5 = torch.cat([img, img.flip(0) * 0.5, img[:1] * 0.0])
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas = []
    for i, (h, w) in enumerate(shapes):
        sf = np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32) if scale == 'array' else np.ones(4, dtype=np.float32)
        metas.append(dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), scale_factor=sf, flip=False))
    det.eval()
    head = det.bbox_head
    old_cfg = copy.deepcopy(head.test_cfg)
    try:
        head.test_cfg.max_per_img = 9
        if nms_pre == -1:
            head.test_cfg.nms_pre = -1
        for im, ms in ((img, metas[:2]), (img5, metas)):
            with torch.no_grad():
                outs = head(det.extract_feat(im))
                nchw = [[t.contiguous() for t in maps] for maps in outs]
                assert not any(maps[0].is_contiguous(memory_format=torch.channels_last) for maps in nchw[:2])
                res, res_nchw = {}, {}
                for mode in (True, False):
                    head.batched_get_bboxes = mode
                    res[mode] = head.get_bboxes(*outs, ms, rescale=scale is not None)
                    res_nchw[mode] = head.get_bboxes(*nchw, ms, rescale=scale is not None)
            counts = [int(d.shape[0]) for d, _ in res[False]]
            assert max(counts) == 9 and sum(counts) >= 18, counts
            for (d1, l1), (d2, l2) in zip(res[True], res[False]):
                assert torch.equal(d1, d2) and torch.equal(l1, l2)
            for mode in (True, False):          # NCHW-contiguous copies of the maps: the same detections in both forms
                for (d1, l1), (d2, l2) in zip(res_nchw[mode], res[mode]):
                    assert torch.equal(d1, d2) and torch.equal(l1, l2)
    finally:
        head.batched_get_bboxes = True
        head.test_cfg = old_cfg


def test_reference_format_checkpoint_round_trip(golden, tmp_path):
    """dense_fixture_util.check_checkpoint_round_trip on the FCOS fixture."""
    from htd_amd.configs import build_baseline_detector
    g = golden('fcos')
    state = U.fixture_state(g['state_keys'], g['state_shapes'], float(g['cls_scale']), float(g['cls_bias_shift']))
    img, metas, _, _ = inputs(torch.device(DEV))
    ckpt = D.check_checkpoint_round_trip(lambda: build_baseline_detector(cfg=small_cfg(g)), state, g, '', img, metas, tmp_path, tol=1e-2)
    assert ckpt['meta']['epoch'] == 3


def test_transposed_batch_after_a_batch_gives_the_result_of_a_fresh_head(det):
    """An H x W batch and then a W x H batch in one process: losses, gradients and detections of the second equal those of a head
    that has seen nothing before (caches key on the feature-map shapes, not on their products)."""
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    img_t = img.transpose(2, 3).contiguous()
    H, W = img_t.shape[-2:]
    metas_t = [dict(m, img_shape=(H - 3, W, 3), pad_shape=(H, W, 3), ori_shape=(H - 3, W, 3)) for m in metas]
    gts_t = [x[:, [1, 0, 3, 2]].contiguous() for x in gts]

    def run(model, first):
        out = []
        for im, ms, gs in ([(img, metas, gts)] if first else []) + [(img_t, metas_t, gts_t)]:
            model.train()
            model.zero_grad()
            losses = model.forward_train(im, ms, gs, labels)
            loss, _ = model._parse_losses(losses)
            loss.backward()
            model.eval()
            with torch.no_grad():
                res = model.simple_test(im, ms)
            out = [loss.detach().clone(), model.bbox_head.conv_cls.weight.grad.clone(), model.bbox_head.conv_reg.bias.grad.clone(),
                   model.bbox_head.conv_centerness.weight.grad.clone(), [BU.dets_array(r) for r in res]]
        return out
    fresh = copy.deepcopy(det)
    for m in (det, fresh):
        m.bbox_head.__dict__.pop('_prior_cache', None)
    a, b = run(det, True), run(fresh, False)
    assert torch.isfinite(a[0]).item() and all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    assert all(np.array_equal(x, y) for x, y in zip(a[4], b[4])) and sum(len(x) for x in a[4]) > 0


def test_center_variant_trains_and_tests_through_the_fused_path():
    """The second reference config (centre sampling, stride-normalised distances, centerness on the regression tower, conv biases,
    GIoULoss): forward_train through the fused kernels with finite losses and gradients, simple_test with detections inside the
    images; its head-level arithmetic is held against the reference by test_fused_head_loss_against_the_reference_fp64_run."""
    from htd_amd.configs import build_baseline_detector, fcos_config
    cfg = fcos_config(50, U.VARIANT_OF['center'])
    cfg.test_cfg.score_thr = 1e-4
    model = build_baseline_detector(cfg=cfg)
    model = U.load_fixture_weights_(model, 1.0, 5.0).to(torch.device(DEV))
    img, metas, gts, labels = inputs(torch.device(DEV))
    model.train()
    (loss, log_vars), calls = D.spied(lambda: model._parse_losses(model.forward_train(img, metas, gts, labels)))
    assert calls.count('htd_fcos_loss') == 1
    loss.backward()
    assert np.isfinite(list(log_vars.values())).all() and log_vars['loss_bbox'] > 0 and log_vars['loss_centerness'] > 0
    assert all(torch.isfinite(p.grad).all() for p in model.bbox_head.parameters())
    assert int(model.bbox_head._last_targets[3].sum()) > 0
    model.eval()
    with torch.no_grad():
        res = model.simple_test(img, metas)
    d = BU.dets_array(res[0])
    assert len(d) > 0 and d[:, :4].min() >= 0 and d[:, 2].max() <= metas[0]['img_shape'][1]
