"""FoveaBox on the GPU: htd_fovea_targets / htd_fovea_loss / htd_fovea_align_fwd / _bwd at every form and edge against the
reference's own run (tests/golden/fovea.npz), the head's tensor path (pinned against that fixture by tests/test_fovea.py) and
the fp64 formulas of fovea_util, the fused FoveaHead.loss against the reference's fp64 run, and both FOVEA detectors against the
reference's.

The bound of every value computed by a kernel is the project's rule (dense_fixture_util.bound): 4 x max(the reference's own fp32
error on that case, one fp32 ulp of the largest entry); the fp32 error comes from the fixture or from the fp32 run of the formula
on the CPU, never from the code under test.  Assignments are compared bit for bit.  The log targets are compared within
LOG_TOL = 1.5 ulp of log 16: torch's CPU logarithm is good to one ulp (not correctly rounded), the kernel's is the rounding of
the fp64 logarithm (half an ulp), and no target exceeds log 16 in magnitude."""
import copy

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T, bound as _bound, err as _err, leave_the_allocator_as_found, spied as _spied  # noqa: F401
import fovea_util as U
from golden_util import seeded_tensor

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CL = torch.channels_last
LOG_TOL = 1.5 * 2.0 ** -22              # 1.5 ulp of a value in [2, 4): log 16 = 2.77
PYRAMIDS = dict(five=(U.LEVEL_SIZES, U.STRIDES, U.BASE_EDGES, U.DEFAULT_RANGES),
                odd=(((5, 7), (3, 4), (2, 2), (1, 1), (1, 1)), U.STRIDES, U.BASE_EDGES, U.DEFAULT_RANGES),
                one=(((1, 1), ), (8, ), (16, ), ((1, 2048), )))


def inputs(dev):
    return D.inputs(dev, BU.detector_inputs)


def _cpu_head(**extra):
    from test_fovea import build_head
    return build_head(**extra)


# ---------------------------------------------------------------------------------------------------- the targets kernel
def _targets_raw(sizes, strides, bases, ranges, sigma, gts, valid):
    """htd_fovea_targets on outputs pre-filled with -7 / NaN -> CPU tensors (assigned, bbox_targets, num_pos, norm)."""
    import ctypes
    from htd_amd import capi, mmcv_ops as M
    dev = torch.device(DEV)
    B, K = valid.shape
    hw, st, P = M._fcos_levels(sizes, strides)
    g = gts.to(dev).float().contiguous()
    v = valid.to(dev).contiguous()
    assigned = torch.full((B, P), -7, dtype=torch.int32, device=dev)
    bt = torch.full((B, P, 4), float('nan'), device=dev)
    num_pos = torch.full((B, ), -7, dtype=torch.int32, device=dev)
    norm = torch.full((2, ), float('nan'), device=dev)
    ws = torch.empty(capi.lib().htd_fovea_targets_workspace_bytes(B, P) // 4, dtype=torch.int32, device=dev)
    capi.call('htd_fovea_targets', hw, st, (ctypes.c_float * len(st))(*[float(b) for b in bases]),
              (ctypes.c_float * (2 * len(st)))(*[float(x) for r in ranges for x in r]), len(st), float(sigma),
              M._P(g) if K else None, M._P(v) if K else None, B, K, M._P(assigned), M._P(bt), M._P(ws), M._P(num_pos), M._P(norm),
              M._S())
    return assigned.cpu(), bt.cpu(), num_pos.cpu(), norm.cpu()


def _check_targets(out, want_assigned, want_bt, B):
    assigned, bt, num_pos, norm = out
    assert torch.equal(assigned.long(), want_assigned.long())
    assert bool(torch.isfinite(bt).all()) and float(bt[assigned == 0].abs().max() if bool((assigned == 0).any()) else 0) == 0
    assert float((bt - want_bt).abs().max()) <= LOG_TOL
    assert num_pos.tolist() == (want_assigned > 0).sum(1).tolist()
    total = int((want_assigned > 0).sum())
    assert norm.tolist() == [float(total + B), float(max(total, 1))]


@pytest.mark.parametrize('B', [4, 2])
def test_targets_kernel_equals_the_reference_on_the_targets_case(golden, B):
    """The fixture's case (gts outside the map, an empty rectangle, sizes on the bounds, nested gts, both clamps, an empty image):
    `assigned` bit for bit, the log targets within LOG_TOL, zeros under the background; every element written."""
    g = golden('fovea')
    gts, _ = U.targets_case()
    padded, valid, _ = U.pad_gts(gts[:B])
    sizes, strides, bases, ranges = PYRAMIDS['five']
    out = _targets_raw(sizes, strides, bases, ranges, U.SIGMA, padded, valid)
    _check_targets(out, T(g['tc.assigned'])[:B], T(g['tc.bbox_targets'])[:B], B)
    assert int((out[0] > 0).sum()) == (31 if B == 4 else 19)


def _random_gts(tag, B, K, W, H):
    """B x K boxes around a W x H image: centres up to a fifth outside it, sides log-uniform from 4 to 2.5 x the image, one in
    five slots invalid."""
    c = seeded_tensor(tag + '.c', (B, K, 2), kind='rand') * 1.4 - 0.2
    s = 4.0 * (2.5 * max(W, H) / 4.0) ** seeded_tensor(tag + '.s', (B, K, 2), kind='rand')
    cx, cy = c[..., 0] * W, c[..., 1] * H
    gts = torch.stack([cx - s[..., 0] / 2, cy - s[..., 1] / 2, cx + s[..., 0] / 2, cy + s[..., 1] / 2], -1)
    valid = seeded_tensor(tag + '.v', (B, K), kind='rand') > 0.2
    return gts, valid


@pytest.mark.parametrize('sigma', [0.4, 1.0])
@pytest.mark.parametrize('K', [0, 1, 3, 257])
@pytest.mark.parametrize('pyr', ['odd', 'one'])
def test_targets_kernel_equals_the_tensor_path(pyr, K, sigma):
    """Pyramids whose levels share a block (5 x 7, 3 x 4, 2 x 2, 1 x 1, 1 x 1) and a single 1 x 1 level; no gt, one, three and
    more than one chunk of them, some slots invalid; sigma 0.4 and 1: the kernel's assignment equals the tensor path's
    (FoveaHead.get_targets on the valid gts of each image) exactly."""
    sizes, strides, bases, ranges = PYRAMIDS[pyr]
    B = 3
    W, H = sizes[0][1] * strides[0], sizes[0][0] * strides[0]
    gts, valid = _random_gts(f'fovea.tg.{pyr}.{K}', B, K, W, H)
    out = _targets_raw(sizes, strides, bases, ranges, sigma, gts, valid)
    head = _cpu_head(strides=list(strides), base_edge_list=list(bases), scale_ranges=ranges, sigma=sigma, num_classes=300)
    lists = [gts[b][valid[b]] for b in range(B)]
    want_a, want_bt = U.head_targets(head, lists, sizes=sizes)
    # head_targets counts within the valid gts of an image: back to the padded index
    index = [valid[b].nonzero().flatten() for b in range(B)]
    want_pad = torch.stack([torch.where(want_a[b] > 0, index[b][(want_a[b] - 1).clamp(min=0)] + 1 if len(index[b]) else want_a[b],
                                        torch.zeros_like(want_a[b])) for b in range(B)])
    _check_targets(out, want_pad, want_bt, B)
    if K == 257 and pyr == 'odd':
        assert int((want_pad > 256).sum()) > 0 and int((want_pad > 0).sum()) > 20      # the second chunk wins somewhere


def test_targets_kernel_gives_equal_sizes_to_the_higher_index():
    """The tie rule on 20 nested gts of equal gt_areas: the kernel and the tensor path agree exactly, and the point all hold goes
    to the last gt."""
    gts, _ = U.tie_case(20)
    sizes, strides, bases, ranges = PYRAMIDS['five']
    out = _targets_raw(sizes, strides, bases, ranges, U.SIGMA, gts[None], torch.ones(1, 20, dtype=torch.bool))
    want_a, want_bt = U.head_targets(_cpu_head(scale_ranges=ranges), [gts])
    _check_targets(out, want_a, want_bt, 1)
    assert int(out[0][0, U.LEVEL_POINTS[0] + 33]) == 20


def test_targets_kernel_compares_rounded_square_roots():
    """Two areas that round to the same fp32 root tie in the kernel as in the tensor path: the higher index wins every painted
    point, although its area is the larger one."""
    gts, _ = U.sqrt_tie_case()
    sizes, strides, bases, ranges = PYRAMIDS['five']
    out = _targets_raw(sizes, strides, bases, ranges, U.SIGMA, gts[None], torch.ones(1, 2, dtype=torch.bool))
    want_a, want_bt = U.head_targets(_cpu_head(scale_ranges=ranges), [gts])
    _check_targets(out, want_a, want_bt, 1)
    assert set(out[0].flatten().tolist()) == {0, 2}


# ---------------------------------------------------------------------------------------------------- the loss kernel
def _loss_case(pyr, C, tag, positives=True, B=2, pad=0):
    """Seeded maps on a pyramid (channels_last on the device, `pad` extra channels behind those of both kinds of map), an
    assignment of a fifth of the points to K = 5 gts and seeded targets in [-log 16, log 16]."""
    sizes = PYRAMIDS[pyr][0]
    dev = torch.device(DEV)
    P = sum(h * w for h, w in sizes)

    def maps(name, ch, scale, shift=0.0):
        out = []
        for l, (h, w) in enumerate(sizes):
            full = (seeded_tensor(f'{tag}.{name}{l}', (B, ch + pad, h, w), scale=scale) - shift).to(dev).contiguous(memory_format=CL)
            out.append(full[:, :ch] if pad else full)
        return out
    cls, reg = maps('cls', C, 2.0, 2.0), maps('reg', 4, 1.5)
    K = 5
    u = seeded_tensor(tag + '.a', (B, P), kind='rand')
    assigned = torch.where(u < 0.2, (u * 5 * K).floor().int() + 1, torch.zeros(B, P, dtype=torch.int32)).to(torch.int32)
    if not positives:
        assigned.zero_()
    labels = (seeded_tensor(tag + '.l', (B, K), kind='rand') * C).floor().long().clamp(max=C - 1)
    bt = (seeded_tensor(tag + '.t', (B, P, 4), kind='rand') * 2 - 1) * float(np.log(16))
    bt = torch.where((assigned > 0)[..., None], bt, torch.zeros_like(bt))
    n = int((assigned > 0).sum())
    norm = torch.tensor([float(n + B), float(max(n, 1))])
    return dict(cls=cls, reg=reg, assigned=assigned, labels=labels, bt=bt, norm=norm, B=B, P=P)


def _run_loss(case, gamma=1.5, alpha=0.4, beta=0.11, weights=(1.0, 1.0), incoming=(1.0, 1.0)):
    from htd_amd import mmcv_ops as M
    dev = torch.device(DEV)
    cls = [m.detach().requires_grad_() for m in case['cls']]
    reg = [m.detach().requires_grad_() for m in case['reg']]
    lc, lb = M.fovea_loss(cls, reg, case['labels'].to(dev), case['assigned'].to(dev), case['bt'].to(dev), case['norm'].to(dev), beta,
                          gamma, alpha, weights[0], weights[1])
    total = lc * incoming[0] + lb * incoming[1]
    return lc, lb, total, cls, reg


def _loss_raw(case, C, gamma, alpha, beta, weights):
    """htd_fovea_loss on the (possibly sliced) device maps with full-width gradient buffers pre-filled with NaN -> losses (2,)
    fp64 and the two lists of full-width gradient maps, on the CPU."""
    from htd_amd import capi, mmcv_ops as M
    dev = torch.device(DEV)
    B = case['B']
    wide = [[m._base if m._base is not None else m for m in ms] for ms in (case['cls'], case['reg'])]
    grads = [[torch.full_like(m, float('nan')) for m in ms] for ms in wide]
    gview = [[m[:, :c] for m in ms] for ms, c in zip(grads, (C, 4))]
    tabs = [M._level_tables(ms) for ms in (case['cls'], case['reg'])]
    gtabs = [M._level_tables(ms)[0] for ms in gview]
    assert all(M.nhwc_channel_stride(a) == b.size(1) for ms, ws in zip((case['cls'], case['reg']), wide) for a, b in zip(ms, ws))
    sizes = M._i64s([int(m.shape[-2] * m.shape[-1]) for m in case['cls']])
    labels, assigned, bt, norm = (case[k].to(dev).contiguous() for k in ('labels', 'assigned', 'bt', 'norm'))
    rows = capi.lib().htd_fovea_loss_partial_rows()
    partial = torch.full((rows, 2), float('nan'), device=dev)
    capi.call('htd_fovea_loss', tabs[0][0], tabs[0][1], tabs[1][0], tabs[1][1], sizes, len(case['cls']), B, C, M._P(labels),
              labels.size(1), M._P(assigned), M._P(bt), M._P(norm), float(beta), float(gamma), float(alpha), float(weights[0]),
              float(weights[1]), M._P(partial), gtabs[0], gtabs[1], M._S())
    torch.cuda.synchronize()
    s = partial.double().sum(0).cpu()
    nm = case['norm'].double()
    return torch.stack([weights[0] * s[0] / nm[0], weights[1] * s[1] / nm[1]]), [[m.cpu() for m in ms] for ms in grads]


@pytest.mark.parametrize('positives', [True, False])
@pytest.mark.parametrize('C', [1, 3, 80, 81])
def test_loss_kernel_against_the_fp64_formula(C, positives):
    """htd_fovea_loss against fovea_util.loss_ref in fp64, the bound from the formula's own fp32 run: C = 80 takes the float4
    sweep, C = 1 / 3 / 81 the scalar one; maps that are channel slices of wider ones (padded channel strides); gamma 1.5 (the
    general power) and gamma 2 (the fast form); loss weights != 1; with and without positives, where the box loss is exactly 0.
    Every element of both gradient maps is written: zeros on padding channels and on non-positive regression rows; two runs
    bitwise equal."""
    pad = 4 if C == 80 else 3
    case = _loss_case('odd', C, f'fovea.loss.{C}.{positives}', positives, pad=pad)
    weights = (1.0, 1.0) if C in (1, 81) else (0.5, 0.75)
    for gamma in (1.5, 2.0):
        losses, grads = _loss_raw(case, C, gamma, 0.4, 0.11, weights)
        again = _loss_raw(case, C, gamma, 0.4, 0.11, weights)
        assert torch.equal(losses, again[0]) and all(torch.equal(a, b) for x, y in zip(grads, again[1]) for a, b in zip(x, y))
        args = (case['cls'], case['reg'], case['labels'], case['assigned'], case['bt'])
        r64 = U.loss_ref(*args, gamma=gamma, alpha=0.4, beta=0.11, weights=weights)
        r32 = U.loss_ref(*args, gamma=gamma, alpha=0.4, beta=0.11, weights=weights, dtype=torch.float32)
        for i in range(2):
            ref = r64['losses'][i].reshape(1)
            assert _err(losses[i].reshape(1), ref) <= _bound(_err(r32['losses'][i].reshape(1), ref), ref), (C, gamma, i)
        for mine, a64, a32, c in ((grads[0], r64['gcls'], r32['gcls'], C), (grads[1], r64['greg'], r32['greg'], 4)):
            assert all(bool(torch.isfinite(m).all()) and float(m[:, c:].abs().max()) == 0 for m in mine)       # padding: exact zeros
            g, g64, g32 = U.maps_to_rows([m[:, :c] for m in mine]), U.maps_to_rows(a64), U.maps_to_rows(a32)
            assert _err(g, g64) <= _bound(_err(g32, g64), g64), (C, gamma, c)
        neg = case['assigned'] <= 0
        assert float(U.maps_to_rows(grads[1])[neg].abs().max()) == 0
        if not positives:
            assert float(losses[1]) == 0 and float(losses[0]) > 0


def test_loss_kernel_scales_by_incoming_gradients_and_refuses_a_second_backward():
    """Incoming gradients other than 1 scale the finished maps on the device (htd_fovea_grad_scale: the classification map by one
    factor, the regression map by the other, padding left alone); a second backward through the same forward raises."""
    case = _loss_case('odd', 80, 'fovea.loss.scale')
    lc, lb, total, cls, reg = _run_loss(case)
    total.backward()
    base = [m.grad.clone() for m in cls + reg]
    lc, lb, total, cls, reg = _run_loss(case, incoming=(0.5, -3.0))
    (_, calls) = _spied(lambda: total.backward(retain_graph=True))
    assert calls.count('htd_fovea_grad_scale') == 1
    for m, b, f in zip(cls + reg, base, [0.5] * len(cls) + [-3.0] * len(reg)):
        assert torch.equal(m.grad, b * f)
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()


# ---------------------------------------------------------------------------------------------------- the align kernels
@pytest.mark.parametrize('dg', [1, 4])
@pytest.mark.parametrize('shape', [(1, 1, 1, 0), (2, 3, 5, 0), (2, 9, 11, 0), (2, 3, 5, 4)])
def test_align_kernels_against_the_fp64_formula(shape, dg):
    """htd_fovea_align_fwd / _bwd against conv_offset(exp(x)) and its autograd in fp64, the bound from the fp32 tensor form on the
    CPU: 1 x 1, 3 x 5 and 2 x 9 x 11 maps (198 pixels: four blocks, the last one partly filled), a channel stride of 8 behind the
    four logits, 1 and 4 deformable groups; two runs bitwise equal."""
    from htd_amd import mmcv_ops as M
    B, H, W, pad = shape
    dev = torch.device(DEV)
    tag = f'fovea.align.{B}.{H}.{W}.{pad}.{dg}'
    full = seeded_tensor(tag + '.x', (B, 4 + pad, H, W), scale=0.7).to(dev).contiguous(memory_format=CL)
    x0 = full[:, :4] if pad else full
    w0 = seeded_tensor(tag + '.w', (dg * 18, 4, 1, 1), scale=0.1).to(dev)
    go = seeded_tensor(tag + '.g', (B, dg * 18, H, W)).to(dev).contiguous(memory_format=CL)
    runs = []
    for _ in range(2):
        x, w = x0.detach().requires_grad_(), w0.detach().requires_grad_()
        (off, calls) = _spied(lambda: M.fovea_align(x, w))
        assert calls == ['htd_fovea_align_fwd'] and off.shape == (B, dg * 18, H, W) and M.nhwc_channel_stride(off) == dg * 18
        (_, calls) = _spied(lambda: off.backward(go))
        assert calls == ['htd_fovea_align_bwd']
        runs.append((off.detach().clone(), x.grad.clone(), w.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    r64, r32 = U.align_ref(x0, w0, go), U.align_ref(x0, w0, go, dtype=torch.float32)
    for mine, a64, a32 in zip(runs[0], r64, r32):
        assert mine.shape == a64.shape
        assert _err(mine, a64) <= _bound(_err(a32, a64), a64), (shape, dg)
    if pad:     # raw calls on sentinel-filled buffers with padded strides: every element written, zeros on the padding
        from htd_amd import capi
        O = dg * 18
        wide = torch.full((B, O + 2, H, W), float('nan'), device=dev).contiguous(memory_format=CL)
        capi.call('htd_fovea_align_fwd', M._P(x0), 4 + pad, M._P(w0.reshape(O, 4).contiguous()), B, H, W, dg, M._P(wide), O + 2, M._S())
        assert torch.equal(wide[:, :O], runs[0][0]) and float(wide[:, O:].abs().max()) == 0
        gfull = torch.full((B, 4 + pad, H, W), float('nan'), device=dev).contiguous(memory_format=CL)
        gw = torch.full((O, 4), float('nan'), device=dev)
        ws = torch.empty(capi.lib().htd_fovea_align_bwd_workspace_bytes(B, H, W, dg) // 4, device=dev)
        capi.call('htd_fovea_align_bwd', M._P(x0), 4 + pad, M._P(w0.reshape(O, 4).contiguous()), M._P(go), O, B, H, W, dg, M._P(gfull),
                  4 + pad, M._P(gw), M._P(ws), M._S())
        assert torch.equal(gfull[:, :4], runs[0][1]) and float(gfull[:, 4:].abs().max()) == 0
        assert torch.equal(gw.view(O, 4, 1, 1), runs[0][2])


def test_feature_align_takes_the_kernels_on_device_maps():
    """FeatureAlign.forward on fp32 channels_last GPU logits goes through htd_fovea_align_fwd and equals the tensor form
    (conv_offset(shape)) under the rule; other layouts take the tensor form."""
    from htd_amd.detector import FeatureAlign
    dev = torch.device(DEV)
    fa = FeatureAlign(32, 32, kernel_size=3, deform_groups=4).to(dev)
    fa.init_weights()
    x = seeded_tensor('fovea.fa.x', (2, 32, 6, 7)).to(dev).contiguous(memory_format=CL)
    logits = seeded_tensor('fovea.fa.l', (2, 4, 6, 7), scale=0.5).to(dev).contiguous(memory_format=CL)
    (y, calls) = _spied(lambda: fa(x, logits=logits))
    assert calls.count('htd_fovea_align_fwd') == 1
    fa.fused = False
    (y2, calls) = _spied(lambda: fa(x, logits.exp()))
    assert calls.count('htd_fovea_align_fwd') == 0 and y.shape == y2.shape == (2, 32, 6, 7)
    assert float(y.detach().min()) >= 0 and _err(y, y2.detach().cpu().double()) <= 1e-4 * max(1.0, float(y2.detach().abs().max()))
    fa.fused = True
    assert fa._kernel_ok(logits) and not fa._kernel_ok(logits.double()) and not fa._kernel_ok(logits.cpu())


# ---------------------------------------------------------------------------------------------------- the head
def _head_on_device(**extra):
    return _cpu_head(**extra).to(torch.device(DEV))


def test_fused_head_loss_against_the_reference_fp64_run(golden, monkeypatch):
    """FoveaHead.loss (fused) on the seeded maps against the reference head's fp64 run under the rule; the assignment equals the
    reference's; one htd_fovea_targets and one htd_fovea_loss call; two runs bitwise equal; after a warm call the fused path and
    its backward read nothing on the host (tensor reads made to raise, and the sync debug mode of torch set to 'error')."""
    from htd_amd import capi
    from test_iou_losses import _no_host_reads
    g = golden('fovea')
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device()
    err = g['head.err32']
    runs = []
    for run in range(2):
        maps = [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps()]
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
            (ls['loss_cls'] + ls['loss_bbox']).backward()
        finally:
            torch.cuda.set_sync_debug_mode('default')
            monkeypatch.undo()
            capi.call = real
        assert calls.count('htd_fovea_loss') == 1 and calls.count('htd_fovea_targets') == 1
        runs.append(([ls[k].detach().clone() for k in ('loss_cls', 'loss_bbox')],
                     [U.maps_to_rows([m.grad for m in ms]).cpu() for ms in maps]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]))
    assigned, bt, num_pos, norm = head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g['head.assigned']).long())
    assert float((bt.cpu() - T(g['head.bbox_targets'])).abs().max()) <= LOG_TOL
    assert num_pos.tolist() == (T(g['head.assigned']) > 0).sum(1).tolist()
    losses, grads = runs[0]
    for i in range(2):
        ref = T(g['head.loss64'][i]).reshape(1)
        assert _err(losses[i].reshape(1), ref) <= _bound(err[i], ref), i
    assert _err(grads[1], T(g['head.greg64'])) <= _bound(err[3], T(g['head.greg64']))
    sums, sample = BU.digest(grads[0])
    ref = T(g['head.gcls64.sample'])
    assert float((T(sample) - ref).abs().max()) <= _bound(err[2], ref)


def test_fused_head_loss_against_the_tensor_path_on_the_same_maps():
    """Fused against the tensor path (fp64 and fp32 on the CPU copies of the same device maps), under the rule; NCHW maps and
    HTD_FOVEA_FUSED=0 (the head's `fused_loss` attribute) take the tensor path."""
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device()
    res = {}
    for mode in ('fused', 't64', 't32'):
        dt = torch.float64 if mode == 't64' else torch.float32
        where = dev if mode == 'fused' else torch.device('cpu')
        maps = [[(m.to(dev).contiguous(memory_format=CL) if mode == 'fused' else m.to(dt)).requires_grad_() for m in ms]
                for ms in U.head_maps()]
        h = head if mode == 'fused' else _cpu_head()
        (ls, calls) = _spied(lambda: h.loss(*maps, [x.to(where).to(dt) for x in gts], [x.to(where) for x in labels], metas))
        assert ('htd_fovea_loss' in calls) == (mode == 'fused')
        ls = torch.stack([ls['loss_cls'], ls['loss_bbox']])
        ls.sum().backward()
        res[mode] = (ls.detach().cpu().double(), [U.maps_to_rows([m.grad for m in ms]).cpu().double() for ms in maps])
    for i in range(2):
        ref = res['t64'][0][i].reshape(1)
        assert _err(res['fused'][0][i].reshape(1), ref) <= _bound(_err(res['t32'][0][i].reshape(1), ref), ref), i
    for a, r64, r32 in zip(res['fused'][1], res['t64'][1], res['t32'][1]):
        assert _err(a, r64) <= _bound(_err(r32, r64), r64)
    nchw = [[m.to(dev) for m in ms] for ms in U.head_maps()]
    assert not head._fused_loss_ok(*nchw)
    head.fused_loss = False
    try:
        maps = [[m.to(dev).contiguous(memory_format=CL) for m in ms] for ms in U.head_maps()]
        (ls, calls) = _spied(lambda: head.loss(*maps, gts, labels, metas))
        assert 'htd_fovea_loss' not in calls and 'htd_fovea_targets' not in calls
        np.testing.assert_allclose(float(ls['loss_bbox']), float(res['t64'][0][1]), rtol=1e-5)
    finally:
        del head.fused_loss


def test_fused_head_loss_without_positives():
    dev = torch.device(DEV)
    _, metas, gts, labels = inputs(dev)
    head = _head_on_device()
    maps = [[m.to(dev).contiguous(memory_format=CL).requires_grad_() for m in ms] for ms in U.head_maps()]
    (ls, calls) = _spied(lambda: head.loss(*maps, [x.new_zeros(0, 4) for x in gts], [x.new_zeros(0) for x in labels], metas))
    assert calls.count('htd_fovea_loss') == 1
    (ls['loss_cls'] + ls['loss_bbox']).backward()
    assert float(ls['loss_bbox'].detach()) == 0 and float(ls['loss_cls'].detach()) > 0
    assert all(float(m.grad.abs().max()) == 0 for m in maps[1]) and all(bool(torch.isfinite(m.grad).all()) for m in maps[0])
    assert head._last_targets[3].tolist() == [2.0, 1.0]


# ---------------------------------------------------------------------------------------------------- the detectors
def small_cfg(g, which):
    from htd_amd.configs import fovea_config
    cfg = fovea_config(**U.CONFIG_ARGS[which])
    cfg.test_cfg.nms_pre = int(g[which + '.nms_pre'])
    return cfg


@pytest.fixture(scope='module', params=U.DETECTOR_CONFIGS)
def det(golden, request):
    from htd_amd.configs import build_fovea_detector
    g = golden('fovea')
    which = request.param
    model = build_fovea_detector(cfg=small_cfg(g, which))
    model = U.load_fixture_weights_(model, float(g[which + '.cls_scale']), float(g[which + '.cls_bias_shift']))
    return which, model.to(torch.device(DEV))


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step; `assigned` equals the fixture's.  The align config goes through the
    FeatureAlign kernels, once per level and direction."""
    which, det = det
    g = golden('fovea')
    p = which + '.'
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    (losses, calls) = _spied(lambda: det.forward_train(img, metas, gts, labels))
    assert calls.count('htd_fovea_loss') == 1 and calls.count('htd_fovea_targets') == 1
    assert calls.count('htd_fovea_align_fwd') == (5 if which == 'align' else 0)
    assigned, _, num_pos, norm = det.bbox_head._last_targets
    assert torch.equal(assigned.cpu().long(), T(g[p + 'assigned']).long())
    assert num_pos.tolist() == g[p + 'num_pos'].tolist() and float(norm[0]) == float(g[p + 'num_pos'].sum()) + 2
    back = []
    D.check_train_step(det, g, p, f'fovea {which}', losses, ('loss_cls', 'loss_bbox'), U.grad_keys(det), 11,
                       backward=lambda loss: back.extend(_spied(loss.backward)[1]))
    assert back.count('htd_fovea_align_bwd') == (5 if which == 'align' else 0)


def test_outputs_and_detections_match_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_outputs and check_detections."""
    which, det = det
    g = golden('fovea')
    img, metas, _, _ = inputs(torch.device(DEV))
    worst = D.check_outputs(det, g, which + '.', ('cls', 'reg'), U.LEVEL_SIZES, img)
    det.eval()
    with torch.no_grad():
        res = det.simple_test(img, metas)
    print(f'fovea {which}: worst output ratio {worst:.3f}, worst detection ratio {D.check_detections(res, g, which + "."):.3f}')


@pytest.mark.parametrize('nms_pre', ['fixture', -1])
def test_batched_get_bboxes_equals_the_per_image_loop(det, golden, nms_pre):
    """get_bboxes of the whole batch -- one key launch, one segmented top-k, one NMS without score factor -- agrees BIT FOR BIT with
    the per-image loop: B = 2 and B = 5, images of different shapes and scale factors, a blank image, the cuts to nms_pre (and
    none: nms_pre <= 0) and max_per_img active."""
    which, det = det
    img, _, _, _ = inputs(torch.device(DEV))
    H, W = img.shape[-2:]
    img5 = torch.cat([img, img.flip(0) * 0.5, img[:1] * 0.0])
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas = []
    for i, (h, w) in enumerate(shapes):
        sf = np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32)
        metas.append(dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), scale_factor=sf, flip=False))
    det.eval()
    head = det.bbox_head
    old_cfg = copy.deepcopy(head.test_cfg)
    try:
        head.test_cfg.max_per_img = 9
        head.test_cfg.score_thr = 1e-3
        if nms_pre == -1:
            head.test_cfg.nms_pre = -1
        for im, ms in ((img, metas[:2]), (img5, metas)):
            with torch.no_grad():
                outs = head(det.extract_feat(im))
                res = {}
                for mode in (True, False):
                    head.batched_get_bboxes = mode
                    (res[mode], calls) = _spied(lambda: head.get_bboxes(*outs, ms, rescale=True))
                    if nms_pre != -1:
                        assert calls.count('htd_retina_keys') == (1 if mode else len(ms))
            counts = [int(d.shape[0]) for d, _ in res[False]]
            assert max(counts) == 9 and sum(counts) >= 18, counts
            for (d1, l1), (d2, l2) in zip(res[True], res[False]):
                assert torch.equal(d1, d2) and torch.equal(l1, l2)
    finally:
        head.batched_get_bboxes = True
        head.test_cfg = old_cfg


def test_reference_format_checkpoint_round_trip(det, golden, tmp_path):
    """dense_fixture_util.check_checkpoint_round_trip on both FoveaBox fixtures."""
    from htd_amd.configs import build_fovea_detector
    which, _ = det
    g = golden('fovea')
    p = which + '.'
    state = U.fixture_state(g[p + 'state_keys'], g[p + 'state_shapes'], float(g[p + 'cls_scale']), float(g[p + 'cls_bias_shift']))
    img, metas, _, _ = inputs(torch.device(DEV))
    ckpt = D.check_checkpoint_round_trip(lambda: build_fovea_detector(cfg=small_cfg(g, which)), state, g, p, img, metas, tmp_path, tol=1e-3)
    assert ckpt['meta']['epoch'] == 3
