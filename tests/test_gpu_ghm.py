"""GHM on a real MI355X: htd_ghmc_loss and htd_ghm_head_loss against the fp64 restatement of the reference (ghm_util.ghmc_ref /
ghmr_ref / head_ghm_ref, pinned to the reference's own run by tests/test_ghm.py) and the reference's own fp32 error
(tests/golden/ghm.npz), the fused head loss against its tensor path, the detector against the reference run, the CLI.

GHM is discontinuous in its inputs: an element that crosses a bin edge changes two bin counts and, in a thinly filled bin, its
neighbours' weights by a large factor.  No tolerance here hides that.  Seeded logits pass through ghm_util.clear_of_edges (1e-4
clear of every edge, three orders above the fp32 error of g) and seeded regression maps are chosen so that no positive's g lies
within 1e-4 of an edge, so bin counts, tot and n must EQUAL the fp64 reference's.  Where the logits come from a network, the
elements within the fixture's margin.edge of an edge are counted (under 0.1 % is asserted) and left out of the gradient
comparison, and the fixture's flip bound (asserted by its generator) says what such an element can change.

Values against fp64 follow the project's rule: |kernel - fp64| <= 4 x max(the reference's own
|fp32 - fp64|, one fp32 ulp of the largest entry).  The ratios measured on the MI355X are in DESIGN.md section 8 f14."""
import ctypes

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T, bound as _bound, err as _err  # noqa: F401
import ghm_util as U
import retina_util as RU

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _module(kind, bins, mmt, loss_weight=1.0):
    import htd_amd.detector  # noqa: F401
    from htd_amd.registry import build_loss
    if kind == 'c':
        return build_loss(dict(type='GHMC', bins=bins, momentum=mmt, use_sigmoid=True, loss_weight=loss_weight))
    return build_loss(dict(type='GHMR', mu=U.MU, bins=bins, momentum=mmt, loss_weight=loss_weight))


# ---------------------------------------------------------------------------------------------------- the matrix kernel
def _matrix(pred, labels, weight, bins, mmt, acc, loss_weight=1.0):
    """One raw call of htd_ghmc_loss -> dict(loss (float64 sum of the partial sums), partial, grad, counts, tot, n); acc (bins,)
    float32 on the device moves in place; outputs pre-filled with NaN."""
    from htd_amd import capi, mmcv_ops as M
    N, C = pred.shape
    grad = torch.full_like(pred, float('nan'))
    partial = torch.full((capi.lib().htd_focal_loss_partial_rows(), 2), float('nan'), device=pred.device)
    ws = M.ghm_workspace(1, pred.device)
    ws.fill_(-7)
    edges = U.edges_of(bins, 'c').to(pred.device)
    capi.call('htd_ghmc_loss', capi.ptr(pred), capi.ptr(labels), capi.ptr(weight), N, C, capi.ptr(edges), bins, float(mmt),
              capi.ptr(acc) if mmt > 0 else None, float(loss_weight), capi.ptr(ws), capi.ptr(partial), capi.ptr(grad),
              capi.current_stream_ptr())
    torch.cuda.synchronize()
    counts, tot, n, _ = M.ghm_workspace_views(ws)
    assert float(partial[:, 1].abs().max()) == 0.0
    return dict(loss=float(partial[:, 0].double().sum()), partial=partial, grad=grad, counts=counts[0, 0, :bins].tolist(),
                tot=max(int(tot[0, 0]), 1), n=int(n[0, 0]))


@pytest.mark.parametrize('i', range(len(U.GHM_PARAMS)))
def test_matrix_kernel_against_reference_fixture(golden, i):
    """Three consecutive calls on the fixture's rows: loss and gradient within the rule's bound of the reference's fp64 run, bin
    counts, tot and n equal to it, the acc_sum trail within rtol 1e-6; a repeated call from the same acc_sum is bitwise equal;
    the GHMC module on the GPU takes this path and gives the same bits."""
    g = golden('ghm')
    bins, mmt = U.GHM_PARAMS[i]
    p = f'c.{i}.'
    acc = torch.zeros(bins, device=DEV)
    mod = _module('c', bins, mmt).to(DEV)
    worst = {}
    for k in range(3):
        pred, labels, weight = (t.to(DEV) for t in U.ghmc_rows(tag=f'ghm.c{k}'))
        before = acc.clone()
        r = _matrix(pred, labels, weight, bins, mmt, acc)
        assert torch.isfinite(r['grad']).all() and np.isfinite(r['loss'])
        assert r['counts'] == g[p + 'counts'][k].tolist() and r['tot'] == g[p + 'tot'][k] and r['n'] == g[p + 'n'][k]
        ref = T(g[p + 'loss64'][k]).reshape(1)
        e = _err([r['loss']], ref)
        worst['loss'] = max(worst.get('loss', 0.0), e / _bound(g[p + 'err32'][0], ref))
        assert e <= _bound(g[p + 'err32'][0], ref), (k, e)
        if k == 0:
            ref = T(g[p + 'grad64'])
            e = _err(r['grad'], ref)
            worst['grad'] = e / _bound(g[p + 'err32'][1], ref)
            assert e <= _bound(g[p + 'err32'][1], ref), e
        if mmt > 0:
            np.testing.assert_allclose(acc.cpu().numpy(), g[p + 'acc64'][k], rtol=1e-6)
        again_acc = before.clone()
        again = _matrix(pred, labels, weight, bins, mmt, again_acc)
        assert torch.equal(again['partial'], r['partial']) and torch.equal(again['grad'], r['grad']) and torch.equal(again_acc, acc)
        x = pred.clone().requires_grad_()
        out = mod(x, labels, weight)
        (out * 2.0).backward()
        assert torch.equal(out.detach(), r['partial'][:, 0].sum()) and torch.equal(x.grad, r['grad'] * 2.0)
        if mmt > 0:
            assert torch.equal(mod.acc_sum, acc)
    print(f'bins {bins} momentum {mmt}: ' + ', '.join(f'{k} {v:.3f} of the bound' for k, v in worst.items()))


def _cpu_module_run(pred, labels, weight, bins, mmt, acc0, dtype):
    """The tensor form of GHMC on the CPU (the reference's arithmetic, tests/test_ghm.py) from the acc_sum state acc0 -> (loss,
    gradient)."""
    mod = _module('c', bins, mmt)
    if mmt > 0:
        mod.acc_sum.copy_(T(acc0))
    x = pred.detach().cpu().to(dtype).requires_grad_()
    loss = mod(x, labels.cpu(), weight.cpu())
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g


def _check_matrix(pred, labels, weight, bins, mmt):
    acc0 = np.linspace(3.0, 40.0, bins).astype(np.float32)
    acc = acc0.copy()
    ref = U.ghmc_ref(pred, labels, weight, bins, mmt, acc)
    l32, g32 = _cpu_module_run(pred, labels, weight, bins, mmt, acc0, torch.float32)     # the reference's fp32 run on the case
    dev_acc = T(acc0).to(DEV)
    r = _matrix(pred.to(DEV), labels.to(DEV), weight.to(DEV), bins, mmt, dev_acc)
    assert r['counts'] == ref['counts'].tolist() and r['tot'] == ref['tot'] and r['n'] == ref['n']
    assert torch.isfinite(r['grad']).all()
    rl = torch.tensor([ref['loss']], dtype=torch.float64)
    assert _err([r['loss']], rl) <= _bound(_err(l32.reshape(1), rl), rl), (r['loss'], ref['loss'])
    assert _err(r['grad'], ref['grad']) <= _bound(_err(g32, ref['grad']), ref['grad'])
    if mmt > 0:
        np.testing.assert_allclose(dev_acc.cpu().numpy(), acc, rtol=1e-6)
    return r, ref


@pytest.mark.parametrize('variant', ['mixed', 'allbg', 'w0'])
@pytest.mark.parametrize('C', [1, 3, 80, 81])
@pytest.mark.parametrize('N', [1, 3, 257])
def test_matrix_kernel_shapes(N, C, variant):
    """Fewer rows than a wave, rows x classes that fill no whole float4 / block, the scalar path (C = 81, C = 3, C = 1) and the
    vector path, every row background, every weight 0 (tot = 1, n = 0, loss 0, zero gradient, acc_sum untouched): against
    ghm_ref, with and without momentum."""
    pred, labels, weight = U.ghmc_rows(N, C, tag='ghm.shape')
    if variant == 'allbg':
        labels[:] = C
    if variant == 'w0':
        weight[:] = 0.
    for bins, mmt in ((30, 0.75), (10, 0.0)):
        r, ref = _check_matrix(pred, labels, weight, bins, mmt)
        if variant == 'w0':
            assert r['loss'] == 0.0 and float(r['grad'].abs().max()) == 0.0 and r['n'] == 0 and r['tot'] == 1


def test_matrix_kernel_wraps_its_grid():
    """30 000 x 80: 600 000 float4 units against the 524 288 threads of the fixed grid, in both passes."""
    pred, labels, weight = U.ghmc_rows(30000, 80, tag='ghm.wrap')
    assert 30000 * 20 > 2048 * 256
    _check_matrix(pred, labels, weight, 30, 0.75)


# ---------------------------------------------------------------------------------------------------- the head kernel
def _ghm_case(**kw):
    """retina_util.head_case with logits clear of the edges and regression maps whose positives are 1e-3 to a few units from
    their targets (ghm_util.spread_box_errors), seeded until no positive's g lies within 1e-4 of an edge of 10 bins."""
    for seed in range(32):
        case = U.spread_box_errors(RU.head_case(tag=f'ghm.case{seed}', **kw), f'ghm.case{seed}')
        case['cls'] = [U.clear_of_edges(c, (30, )) for c in case['cls']]
        ref = U.head_ghm_ref(case, U.HEAD_GHMC, U.HEAD_GHMR, np.zeros(30, np.float32), np.zeros(10, np.float32))
        g = torch.cat([lv['r']['g'].reshape(-1) for lv in ref])
        if not U.near_edge(g, (10, )).any():
            return case
    raise AssertionError('no seed keeps the regression maps clear of the edges')


def _head_raw(case, pc, pr, acc_c, acc_r):
    """One raw call of htd_ghm_head_loss on the case (regression maps channel-padded, read in place) -> dict; gradient buffers
    and the workspace pre-filled with a sentinel."""
    from htd_amd import capi, mmcv_ops as M
    na, C = case['na'], case['C']
    cl = [c.to(DEV).contiguous(memory_format=torch.channels_last) for c in case['cls']]
    rg_full = [r.to(DEV).contiguous(memory_format=torch.channels_last) for r in case['reg']]
    rg = [r[:, :na * 4] for r in rg_full]
    gcls = [torch.full_like(c, float('nan')) for c in cl]
    greg_full = [torch.full_like(r, float('nan')) for r in rg_full]
    anchors, gts = case['anchors'].to(DEV).contiguous(), case['gts'].to(DEV).contiguous()
    labels, assigned = case['gt_labels'].to(DEV).contiguous(), case['assigned'].to(DEV).contiguous()
    B, A = assigned.shape
    L = len(cl)
    ct, cs, pix = M._level_tables(cl)
    rt, rs, _ = M._level_tables(rg)
    gct, _, _ = M._level_tables(gcls)
    grt, grs, _ = M._level_tables([g_[:, :na * 4] for g_ in greg_full])
    assert list(rs) == [na * 4 + case['reg_pad']] * L == list(grs)
    partial = torch.full((capi.lib().htd_focal_loss_partial_rows(), 2), float('nan'), device=DEV)
    ws = M.ghm_workspace(L, DEV)
    ws.fill_(-7)
    ec, er = U.edges_of(pc['bins'], 'c').to(DEV), U.edges_of(pr['bins'], 'r').to(DEV)
    f4 = (ctypes.c_float * 4)
    capi.call('htd_ghm_head_loss', ct, cs, rt, rs, pix, L, B, na, C, capi.ptr(anchors), capi.ptr(gts), capi.ptr(labels),
              capi.ptr(assigned), A, gts.size(1), f4(0, 0, 0, 0), f4(1, 1, 1, 1), capi.ptr(ec), pc['bins'], float(pc['momentum']),
              capi.ptr(acc_c) if pc['momentum'] > 0 else None, capi.ptr(er), pr['bins'], float(pr['momentum']),
              capi.ptr(acc_r) if pr['momentum'] > 0 else None, float(pr['mu']), float(pc['loss_weight']), float(pr['loss_weight']),
              capi.ptr(ws), capi.ptr(partial), gct, grt, capi.current_stream_ptr())
    torch.cuda.synchronize()
    counts, tot, n, _ = M.ghm_workspace_views(ws)
    return dict(partial=partial, gcls=gcls, greg_full=greg_full, counts=counts.cpu(), tot=tot.cpu(), n=n.cpu())


def _tensor_head_fp32(case, pc, pr, acc_c, acc_r):
    """The per-level tensor form of the two modules on the CPU in fp32 (the reference's arithmetic): what its fp32 run gives on
    the case -> (sum of the GHMC losses, sum of the GHMR losses, gcls list, greg list)."""
    from htd_amd.core.bbox import bbox2delta
    na, C = case['na'], case['C']
    mc, mr = _module('c', pc['bins'], pc['momentum'], pc['loss_weight']), _module('r', pr['bins'], pr['momentum'], pr['loss_weight'])
    if pc['momentum'] > 0:
        mc.acc_sum.copy_(T(acc_c))
    if pr['momentum'] > 0:
        mr.acc_sum.copy_(T(acc_r))
    assigned, anchors = case['assigned'], case['anchors']
    B, A = assigned.shape
    pos = assigned > 0
    gi = (assigned - 1).clamp(min=0)
    labels = torch.where(pos, torch.gather(case['gt_labels'], 1, gi), torch.full_like(assigned, C))
    gt_of = torch.gather(case['gts'], 1, gi[..., None].expand(B, A, 4))
    safe = torch.where(pos[..., None], gt_of, anchors[None].expand(B, A, 4))
    tgt = bbox2delta(anchors[None].expand(B, A, 4).reshape(-1, 4), safe.reshape(-1, 4), (0., ) * 4, (1., ) * 4).view(B, A, 4)
    cls = [c.clone().requires_grad_() for c in case['cls']]
    reg = [r[:, :na * 4].clone().requires_grad_() for r in case['reg']]
    lc = lr = 0.0
    at = 0
    for c, r in zip(cls, reg):
        n = c.shape[2] * c.shape[3] * na
        sl = slice(at, at + n)
        lc = lc + mc(c.permute(0, 2, 3, 1).reshape(-1, C), labels[:, sl].reshape(-1), (assigned[:, sl] >= 0).float().reshape(-1))
        lr = lr + mr(r.permute(0, 2, 3, 1).reshape(-1, 4), tgt[:, sl].reshape(-1, 4),
                     pos[:, sl].reshape(-1, 1).expand(-1, 4).float())
        at += n
    (lc + lr).backward()
    return lc.detach(), lr.detach(), [c.grad for c in cls], [r.grad if r.grad is not None else torch.zeros_like(r) for r in reg]


def _check_head(case, pc, pr, acc_c0, acc_r0):
    """One call from the given acc_sum state against head_ghm_ref -> (kernel result, acc_c, acc_r after, worst ratios)."""
    na, C = case['na'], case['C']
    L = len(case['cls'])
    acc_c, acc_r = acc_c0.copy(), acc_r0.copy()
    ref = U.head_ghm_ref(case, pc, pr, acc_c, acc_r)
    l32c, l32r, g32c, g32r = _tensor_head_fp32(case, pc, pr, acc_c0, acc_r0)
    dc, dr = T(acc_c0).to(DEV), T(acc_r0).to(DEV)
    r = _head_raw(case, pc, pr, dc, dr)
    for l in range(L):
        for which, key, bins in ((0, 'c', pc['bins']), (1, 'r', pr['bins'])):
            assert r['counts'][which, l, :bins].tolist() == ref[l][key]['counts'].tolist(), (l, key)
            assert max(int(r['tot'][which, l]), 1) == ref[l][key]['tot'] and int(r['n'][which, l]) == ref[l][key]['n'], (l, key)
    assert torch.isfinite(r['partial']).all() and all(torch.isfinite(t).all() for t in r['gcls'] + r['greg_full'])
    sums = r['partial'].double().sum(0).cpu()
    worst = {}
    for j, key, l32 in ((0, 'c', l32c), (1, 'r', l32r)):
        want = torch.tensor([sum(lv[key]['loss'] for lv in ref)], dtype=torch.float64)
        e, b = _err(sums[j].reshape(1), want), _bound(_err(l32.reshape(1), want), want)
        worst['loss ' + key] = e / b
        assert e <= b, (key, e, b, float(sums[j]), float(want))
    for key, mine, g32 in (('c', r['gcls'], g32c), ('r', [t[:, :na * 4] for t in r['greg_full']], g32r)):
        ref_g = [lv[key]['grad'] for lv in ref]
        big = max(float(t.abs().max()) for t in ref_g)
        e32 = max(_err(a, b) for a, b in zip(g32, ref_g))
        e = max(_err(a, b) for a, b in zip(mine, ref_g))
        worst['grad ' + key] = e / (4.0 * max(e32, EPS32 * big))
        assert e <= 4.0 * max(e32, EPS32 * big), (key, e, e32)
    if pc['momentum'] > 0:
        np.testing.assert_allclose(dc.cpu().numpy(), acc_c, rtol=1e-6)
    if pr['momentum'] > 0:
        np.testing.assert_allclose(dr.cpu().numpy(), acc_r, rtol=1e-6)
    # exact zeros where the buffers went in as NaN: padding channels, anchors with assigned < 0, non-positive anchors (boxes)
    B = case['assigned'].size(0)
    assert all(float(t[:, na * 4:].abs().max()) == 0.0 for t in r['greg_full'])
    gc = torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, C) for t in r['gcls']], 1).cpu()
    gr = torch.cat([t[:, :na * 4].permute(0, 2, 3, 1).reshape(B, -1, 4) for t in r['greg_full']], 1).cpu()
    assert float(gc[case['assigned'] < 0].abs().max()) == 0.0 and float(gr[case['assigned'] <= 0].abs().max()) == 0.0
    assert float(gc[case['assigned'] >= 0].abs().min()) > 0.0
    return r, dc, dr, ref, worst


@pytest.mark.parametrize('mmt_c,mmt_r', [(0.75, 0.7), (0.0, 0.0)])
def test_head_kernel_against_ghm_ref_per_level(mmt_c, mmt_r):
    """htd_ghm_head_loss on five levels of 4x5 .. 1x1 pixels, B = 3, channel-padded regression maps, an image without ground
    truth, an image without a positive, invalid anchors that cover all of image 0's anchors of levels 3 and 4, levels without any
    positive (GHMR: tot = 1, n = 0, loss 0, zero gradient): per-level counts, tot and n equal ghm_ref run level by level in level
    order, losses and gradients within the rule's bound, a second call continues the first's acc_sum, a repeated call from the
    same state is bitwise equal, and running the levels in another order would not pass."""
    case = _ghm_case()
    pc, pr = dict(U.HEAD_GHMC, momentum=mmt_c), dict(U.HEAD_GHMR, momentum=mmt_r)
    na = case['na']
    A3 = sum(h * w for h, w in RU.HEAD_CASE_SIZES[:3]) * na
    assert bool((case['assigned'][0, A3:] < 0).all()) and bool((case['assigned'][1:, A3:] >= 0).all())
    z_c, z_r = np.zeros(pc['bins'], np.float32), np.zeros(pr['bins'], np.float32)
    r1, dc, dr, ref1, worst = _check_head(case, pc, pr, z_c, z_r)
    no_pos = [l for l in range(5) if ref1[l]['r']['n'] == 0]
    assert no_pos and all(int(r1['tot'][1, l]) == 0 and float(r1['greg_full'][l].abs().max()) == 0.0 for l in no_pos)
    assert any(lv['r']['n'] > 0 for lv in ref1)
    print(f'momentum {mmt_c} / {mmt_r}: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    # the second call starts from what the first left
    _, dc2, dr2, _, worst2 = _check_head(case, pc, pr, dc.cpu().numpy().copy(), dr.cpu().numpy().copy())
    print('second call: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst2.items()))
    again = _head_raw(case, pc, pr, T(z_c).to(DEV), T(z_r).to(DEV))
    assert torch.equal(again['partial'], r1['partial'])
    assert all(torch.equal(a, b) for a, b in zip(again['gcls'] + again['greg_full'], r1['gcls'] + r1['greg_full']))
    if mmt_c > 0:
        assert not torch.equal(dc2, dc)
        # level order matters: the same levels in reverse order leave another acc_sum and give other losses
        rev = dict(case, cls=case['cls'][::-1], reg=case['reg'][::-1])
        sizes = [c.shape[2] * c.shape[3] * na for c in case['cls']]
        offs = np.cumsum([0] + sizes)
        order = torch.cat([torch.arange(offs[l], offs[l + 1]) for l in range(4, -1, -1)])
        rev['assigned'], rev['anchors'] = case['assigned'][:, order], case['anchors'][order]
        acc_rev = z_c.copy()
        ref_rev = U.head_ghm_ref(rev, pc, pr, acc_rev, z_r.copy())
        total, total_rev = sum(lv['c']['loss'] for lv in ref1), sum(lv['c']['loss'] for lv in ref_rev)
        assert abs(total - total_rev) > 1e-3 * abs(total) and float(np.abs(acc_rev - dc.cpu().numpy()).max()) > 1e-3 * float(acc_rev.max())


def test_head_kernel_scalar_path_and_autograd_scaling():
    """C = 3 (27 classification channels per pixel: the scalar path) through the autograd surface with incoming gradients other
    than 1, against ghm_ref."""
    from htd_amd import mmcv_ops as M
    case = RU.head_case(C=3, reg_pad=0, tag='ghm.scalar')
    case['gt_labels'] = case['gt_labels'] % 3
    case['cls'] = [U.clear_of_edges(c, (30, )) for c in case['cls']]
    ref = U.head_ghm_ref(case, U.HEAD_GHMC, U.HEAD_GHMR, np.zeros(30, np.float32), np.zeros(10, np.float32))
    assert not U.near_edge(torch.cat([lv['r']['g'].reshape(-1) for lv in ref]), (10, )).any()
    want = [sum(lv[k]['loss'] for lv in ref) for k in ('c', 'r')]
    for scale in (1.0, 3.0):
        mc, mr = _module('c', 30, 0.75).to(DEV), _module('r', 10, 0.7, 10.0).to(DEV)
        cl = [c.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_() for c in case['cls']]
        rg = [r.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_() for r in case['reg']]
        lc, lb, ws = M.ghm_head_loss(cl, rg, case['na'], 3, case['anchors'].to(DEV), case['gts'].to(DEV), case['gt_labels'].to(DEV),
                                     case['assigned'].to(DEV), (0., 0., 0., 0.), (1., 1., 1., 1.), mc, mr, return_workspace=True)
        ((lc + lb) * scale).backward()
        counts = M.ghm_workspace_views(ws)[0].cpu()
        assert all(counts[0, l, :30].tolist() == ref[l]['c']['counts'].tolist() for l in range(5))
        np.testing.assert_allclose([float(lc.detach()), float(lb.detach())], want, rtol=1e-5)
        for a, b in zip([t.grad for t in cl + rg], [lv['c']['grad'] for lv in ref] + [lv['r']['grad'] for lv in ref]):
            torch.testing.assert_close(a.cpu().double(), b * scale, rtol=1e-4, atol=1e-6 * max(1.0, float(b.abs().max())))


def test_head_kernel_wraps_its_grid():
    """B = 2 on levels of 64 x 72 and 2 x 3 pixels: 9 228 pixel rows against 8 192 wavefronts and 590 592 regression float4s
    against 524 288 threads (the maps padded to 256 channels), in the histogram pass and in the loss pass."""
    case = _ghm_case(B=2, reg_pad=220, sizes=((64, 72), (2, 3)), strides=(8, 256), scale=14.0)
    B = case['assigned'].size(0)
    rows = B * (64 * 72 + 6)
    assert rows > 2048 * 4 and rows * 64 > 2048 * 256
    _check_head(case, U.HEAD_GHMC, U.HEAD_GHMR, np.linspace(5.0, 900.0, 30).astype(np.float32), np.linspace(1.0, 9.0, 10).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the detector
def inputs(dev):
    return D.inputs(dev, BU.detector_inputs)


@pytest.fixture(scope='module')
def det(golden):
    from htd_amd.configs import build_retinanet_ghm_detector
    g = golden('ghm')
    model = build_retinanet_ghm_detector()
    return U.load_fixture_weights_(model, float(g['cls_scale'])).to(torch.device(DEV))


def _reset(det):
    with torch.no_grad():
        det.bbox_head.loss_cls.acc_sum.zero_()
        det.bbox_head.loss_bbox.acc_sum.zero_()


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step (the fixture's flip bound of 1e-4, asserted by its generator, fits inside
    the bound of the losses); `assigned` equals the fixture's; acc_sum of both losses within rtol 1e-5; one htd_ghm_head_loss call."""
    g = golden('ghm')
    assert float(g['flip.loss'].max()) <= 1e-4 and float(g['flip.grad'].max()) <= 1e-4
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    _reset(det)
    losses, calls = D.spied(lambda: det.forward_train(img, metas, gts, labels))
    assert calls.count('htd_ghm_head_loss') == 1 and 'htd_retina_loss' not in calls
    assert torch.equal(det.bbox_head._last_assigned[0].cpu(), T(g['assigned']).long())
    keys = RU.grad_keys(det)
    assert len(keys) == 5 + len(RU.EXTRA_GRAD_KEYS), keys
    D.check_train_step(det, g, '', 'retinanet-ghm', losses, ('loss_cls', 'loss_bbox'), keys, len(keys))
    acc_c, acc_r = det.bbox_head.loss_cls.acc_sum.cpu().numpy(), det.bbox_head.loss_bbox.acc_sum.cpu().numpy()
    rel = max(float(np.abs(a[r > 0] / r[r > 0] - 1).max()) for a, r in ((acc_c, g['acc_c']), (acc_r, g['acc_r'])))
    print(f'retinanet-ghm: acc_sum worst relative {rel:.2e}')
    np.testing.assert_allclose(acc_c, g['acc_c'], rtol=1e-5)
    np.testing.assert_allclose(acc_r, g['acc_r'], rtol=1e-5)


def _record(mod, store):
    orig = mod.forward

    def rec(pred, target, weight, *a, **k):
        store.append((pred.detach(), target.detach(), weight.detach()))
        return orig(pred, target, weight, *a, **k)
    mod.forward = rec
    return orig


def test_fused_head_loss_matches_tensor_path_bitwise_repeatable_and_reads_nothing(det, golden, monkeypatch):
    """The fused RetinaHead.loss with GHMC + GHMR against its tensor path on the small detector: values to 1e-5, gradients of
    every level's maps to rtol 1e-4 / atol 1e-6 of the largest entry, leaving out the elements whose g (read from the tensor path)
    lies within the fixture's margin.edge of an edge -- fewer than 0.1 % of the valid elements, asserted; two fused runs from
    equal acc_sum are bitwise equal, acc_sum included; the fused path and its backward run with .item() / .tolist() / bool() /
    any() / all() / nonzero() of tensors made to raise; htd_ghm_head_loss is called iff fused."""
    from htd_amd import capi
    from test_iou_losses import _no_host_reads
    g = golden('ghm')
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    head = det.bbox_head
    with torch.no_grad():
        cls0, reg0 = head(det.extract_feat(img))
    out, seen_c, seen_r = {}, [], []
    for mode in ('fused', 'fused2', 'tensor'):
        _reset(det)
        head.fused_loss = mode != 'tensor'
        cls = [c.clone().requires_grad_() for c in cls0]
        reg = [r.clone().requires_grad_() for r in reg0]
        calls, real = [], capi.call

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        capi.call = spy
        if mode == 'fused2':
            head.loss(cls, reg, gts, labels, metas)            # caches (anchors, gt padding) are warm: a production step
            _reset(det)
            _no_host_reads(monkeypatch)
        if mode == 'tensor':
            orig = (_record(head.loss_cls, seen_c), _record(head.loss_bbox, seen_r))
        try:
            losses = head.loss(cls, reg, gts, labels, metas)
            total = sum(losses['loss_cls']) + 2.0 * sum(losses['loss_bbox'])
            total.backward()
        finally:
            monkeypatch.undo()
            capi.call = real
            head.fused_loss = True
            if mode == 'tensor':
                head.loss_cls.forward, head.loss_bbox.forward = orig
        assert ('htd_ghm_head_loss' in calls) == (mode != 'tensor')
        assert len(losses['loss_cls']) == (5 if mode == 'tensor' else 1)
        out[mode] = ([sum(losses[k]).detach() for k in ('loss_cls', 'loss_bbox')], [t.grad.clone() for t in cls + reg],
                     [head.loss_cls.acc_sum.clone(), head.loss_bbox.acc_sum.clone()])
    (lf, gf, af), (l2, g2, a2), (lt, gt_, at) = out['fused'], out['fused2'], out['tensor']
    assert all(torch.equal(a, b) for a, b in zip(lf + gf + af, l2 + g2 + a2))
    for a, b in zip(lf, lt):
        assert abs(float(a) - float(b)) <= 1e-5 * max(1.0, abs(float(b))), (lf, lt)
    assert float(lt[0]) > 0 and float(lt[1]) > 0
    for a, b in zip(af, at):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=0)
    # elements near an edge, from the tensor path's own inputs
    mu, B = head.loss_bbox.mu, cls0[0].size(0)
    skip, near, valid = [], 0, 0
    for (pred, target, w), c in zip(seen_c, cls0):
        gg = (pred.double().sigmoid() - (target.view(-1, 1) == torch.arange(pred.size(1), device=pred.device)).double()).abs()
        m = U.near_edge(gg, (head.loss_cls.bins, ), float(g['margin.edge'][0])) & (w > 0).view(-1, 1)
        near, valid = near + int(m.sum()), valid + int((w > 0).sum()) * pred.size(1)
        skip.append(m.view(B, c.size(2), c.size(3), -1).permute(0, 3, 1, 2))
    for (pred, target, w), r in zip(seen_r, reg0):
        d = pred.double() - target.double()
        gg = (d / torch.sqrt(d * d + mu * mu)).abs()
        m = U.near_edge(gg, (head.loss_bbox.bins, ), float(g['margin.edge'][1])) & (w > 0)
        near, valid = near + int(m.sum()), valid + int((w > 0).sum())
        skip.append(m.view(B, r.size(2), r.size(3), -1).permute(0, 3, 1, 2))
    print(f'{near} of {valid} valid elements within margin.edge of an edge')
    assert near < 1e-3 * valid
    for a, b, m in zip(gf, gt_, skip):
        a, b = torch.where(m, torch.zeros_like(a), a), torch.where(m, torch.zeros_like(b), b)
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * max(1.0, float(b.abs().max())))


def test_nchw_maps_and_mixed_pairs_take_the_tensor_path_and_second_backward_raises(det):
    from htd_amd import capi
    from htd_amd.registry import build_loss
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    head = det.bbox_head
    with torch.no_grad():
        cls0, reg0 = head(det.extract_feat(img))
    calls, real = [], capi.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    out = {}
    for layout in ('nhwc', 'nchw', 'mixed'):
        _reset(det)
        fmt = torch.contiguous_format if layout == 'nchw' else torch.channels_last
        cls = [c.clone(memory_format=fmt).requires_grad_() for c in cls0]
        reg = [r.clone(memory_format=fmt).requires_grad_() for r in reg0]
        calls.clear()
        capi.call = spy
        keep = head.loss_bbox
        if layout == 'mixed':
            head.loss_bbox = build_loss(dict(type='L1Loss', loss_weight=1.0))
        try:
            losses = head.loss(cls, reg, gts, labels, metas)
        finally:
            capi.call = real
            head.loss_bbox = keep
        assert ('htd_ghm_head_loss' in calls) == (layout == 'nhwc') and 'htd_retina_loss' not in calls
        out[layout] = (losses, cls)
    for k in ('loss_cls', 'loss_bbox'):
        a, b = float(sum(out['nhwc'][0][k]).detach()), float(sum(out['nchw'][0][k]).detach())
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b))
    losses, cls = out['nhwc']
    total = sum(losses['loss_cls']) + 2.0 * sum(losses['loss_bbox'])
    total.backward(retain_graph=True)
    first = cls[0].grad.clone()
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()
    assert torch.equal(cls[0].grad, first)


def test_cli_runs_the_ghm_config_and_a_resumed_run_continues_acc_sum(golden, tmp_path):
    """`python -m htd_amd.train` for one epoch (optimizer_config.grad_clip = None written into the config: the CLI refuses
    clipping) and `python -m htd_amd.test` on its checkpoint, from a config file that holds retinanet_ghm_config(); the
    checkpoint carries the four buffers with acc_sum moved; a run resumed to a second epoch starts from the saved acc_sum."""
    import json
    import os
    import re
    import subprocess
    import sys
    from test_datasets import write_png_set
    from test_gpu_test_loop import SHAPES
    from htd_amd.configs import retinanet_ghm_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data_root = str(tmp_path / 'data')
    os.makedirs(data_root)
    ann = write_png_set(data_root, SHAPES, seed=4)
    cfg = retinanet_ghm_config()
    cfg.test_cfg.score_thr = 0.0
    cfg.test_cfg.nms_pre = 50
    for split in (cfg.data.train, cfg.data.val, cfg.data.test):
        split.ann_file, split.img_prefix = ann, os.path.join(data_root, 'imgs')
    cfg.data.test.pipeline[1]['img_scale'] = (128, 128)
    cfg.data.val.pipeline[1]['img_scale'] = (128, 128)
    cfg.data.train.pipeline[2]['img_scale'] = (128, 128)
    cfg.model.pretrained = None
    cfg.data.workers_per_gpu = 0
    cfg.total_epochs = 1
    cfg.optimizer_config.grad_clip = None
    cfg.log_config = dict(interval=2, hooks=[dict(type='TextLoggerHook')])
    work = tmp_path / 'work'

    def write(total_epochs):
        cfg.total_epochs = total_epochs
        path = tmp_path / f'ghm_tiny_{total_epochs}.py'
        path.write_text(''.join(f'{k} = {v!r}\n' for k, v in cfg.to_dict().items()))
        return str(path)

    def cli(args):
        return subprocess.run([sys.executable] + args, cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True,
                              text=True, timeout=600)
    cfg_file = write(1)
    p = cli(['-m', 'htd_amd.train', cfg_file, '--work-dir', str(work), '--seed', '1'])
    assert p.returncode == 0, p.stderr[-4000:]
    (name, ) = [f for f in os.listdir(work) if f.endswith('.log.json')]
    lines = [json.loads(l) for l in open(os.path.join(work, name))]
    train = [l for l in lines if l.get('mode') == 'train']
    assert train and all({'loss_cls', 'loss_bbox', 'loss'} <= set(l) and np.isfinite(l['loss']) for l in train)
    assert any(l.get('mode') == 'val' and 'bbox_mAP' in l for l in lines)
    ck1 = torch.load(os.path.join(str(work), 'epoch_1.pth'), map_location='cpu')
    sd1 = ck1['state_dict']
    assert set(U.STATE_KEYS) <= set(sd1)
    assert torch.equal(sd1['bbox_head.loss_cls.edges'], U.edges_of(30, 'c')) and torch.equal(sd1['bbox_head.loss_bbox.edges'], U.edges_of(10, 'r'))
    assert float(sd1['bbox_head.loss_cls.acc_sum'].sum()) > 0 and float(sd1['bbox_head.loss_bbox.acc_sum'].sum()) > 0
    p = cli(['-m', 'htd_amd.test', cfg_file, os.path.join(str(work), 'epoch_1.pth'), '--eval', 'bbox'])
    assert p.returncode == 0, p.stderr[-3000:]
    assert re.search(r"'bbox_mAP'(?::|,) ([^,)}]+)", p.stdout) is not None, (p.stdout[-3000:], p.stderr[-3000:])
    # a resumed run starts from the checkpoint's acc_sum, not from 0: resumed from a copy whose bin 0 of GHMC holds 1e12, the
    # 15 to 20 updates of the second epoch (momentum 0.75; bin 0 is filled in every call) leave it above 1e9, while the counts
    # of a 128 x 128 batch stay below 1e6
    sd1['bbox_head.loss_cls.acc_sum'][0] = 1e12
    torch.save(ck1, os.path.join(str(work), 'epoch_1_marked.pth'))
    p = cli(['-m', 'htd_amd.train', write(2), '--work-dir', str(work), '--seed', '1', '--no-validate', '--resume-from',
             os.path.join(str(work), 'epoch_1_marked.pth')])
    assert p.returncode == 0, p.stderr[-4000:]
    sd2 = torch.load(os.path.join(str(work), 'epoch_2.pth'), map_location='cpu')['state_dict']
    a2 = sd2['bbox_head.loss_cls.acc_sum']
    assert 1e8 < float(a2[0]) < 1e12 and float(a2[1:].max()) < 1e6 and float(sd2['bbox_head.loss_bbox.acc_sum'].max()) < 1e6
