"""Every kernel form of htd_amd/csrc/roi_align.hip, called through the C ABI, against the fp64 reference of roi_align_ref.py.

The case table lives in roi_align_ref.py (test_roi_align_ref.py shows on the CPU which launcher branch each case takes and that the
table reaches all of them).  'exact' and 'edge' cases have dyadic geometry and small integer values: every weight, product and
partial sum is exact in fp32 in any order, atomics included, so the kernels must EQUAL the reference.  'random' cases are bounded
element by element by  |got - ref| <= C_BOUND * 2^-24 * A,  A = the operator applied to |input| (the sum of the absolute terms),
C_BOUND = 4 * C_ORACLE and C_ORACLE the fp32 C oracle's own distance from the reference as measured in test_roi_align_ref.py.
RoIs with a sample within 1e-3 px of the drop rule's discontinuity are left out of value comparisons (their gradient rows are zero)
and must still give finite numbers.  test_report_observed_ratios prints the kernels' worst ratio per form."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import roi_align_ref as R
from roi_align_ref import C_BOUND, EPS32, LEVEL_CASES, SINGLE_CASES

pytestmark = pytest.mark.gpu
NAN = float('nan')
OBSERVED = {}           # form -> worst |got - ref| / (2^-24 A) seen on the random cases (a record, not a tolerance)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    from htd_amd import capi
    return capi.current_stream_ptr()


def call(name, *args):
    from htd_amd import capi
    capi.call(name, *args)


def check(form, kind, got, ref, A, rows=None):
    """got (device) against (ref, A) on `rows` (bool over dim 0; default all): finite everywhere; exact cases equal the reference,
    random cases stay within C_BOUND * 2^-24 * A"""
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), form
    if rows is not None:
        got, ref, A = got[rows], ref[rows], A[rows]
    if kind != 'random':
        assert torch.equal(got, ref.float()), (form, float((got.double() - ref).abs().max()))
        return
    err = (got.double() - ref).abs()
    zero = A == 0
    assert float(err[zero].max() if zero.any() else 0.0) == 0.0, form          # no term at all: exactly zero
    ratio = float((err[~zero] / (EPS32 * A[~zero])).max()) if (~zero).any() else 0.0
    OBSERVED[form] = max(OBSERVED.get(form, 0.0), ratio)
    assert ratio <= C_BOUND, (form, ratio)


def level_tables(maps):
    L = len(maps)
    return ((ctypes.c_int * L)(*[m[0] for m in maps]), (ctypes.c_int * L)(*[m[1] for m in maps]),
            (ctypes.c_float * L)(*[m[2] for m in maps]))


def ptr_table(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def gather_workspace(n, L, dev):
    from htd_amd import capi
    return torch.empty(L * capi.lib().htd_roi_align_bwd_gather_workspace_bytes(n), dtype=torch.uint8, device=dev)


def fold_workspace(n, Hs, L, pw, C, dev):
    from htd_amd import capi
    return torch.empty(capi.lib().htd_roi_align_fold_workspace_bytes(n, Hs, L, pw, C), dtype=torch.uint8, device=dev)


def single_fwd(c, feat, rois, lv=None, level=0, fill=NAN):
    out = torch.full((c.n, c.ph, c.pw, c.C), fill, device=feat.device)
    call('htd_roi_align_fwd', P(feat), P(rois), P(lv), level, P(out), c.n, c.B, c.C, c.H, c.W, c.ph, c.pw, c.scale, c.sr, c.aligned, S())
    return out


def single_bwd(c, grad, rois, lv=None, level=0):
    gf = torch.zeros((c.B, c.H, c.W, c.C), device=grad.device)
    call('htd_roi_align_bwd', P(grad), P(rois), P(lv), level, P(gf), c.n, c.B, c.C, c.H, c.W, c.ph, c.pw, c.scale, c.sr, c.aligned, S())
    return gf


def single_gather(c, grad, rois, into, accumulate, lv=None, level=0, shape=None, scale=None):
    B, H, W, C = shape or (c.B, c.H, c.W, c.C)
    ws = gather_workspace(c.n, 1, grad.device)
    call('htd_roi_align_bwd_gather', P(grad), P(rois), P(lv), level, P(into), c.n, B, C, H, W, c.ph, c.pw,
         c.scale if scale is None else scale, c.sr, c.aligned, accumulate, P(ws), S())
    return into


def masked_grad(grad, near):
    g = grad.clone()
    g[near] = 0.0           # RoIs near the drop boundary carry no gradient: the reference leaves them out
    return g


ALL_SINGLE = [c.name for c in SINGLE_CASES]
GATHER_SINGLE = [c.name for c in SINGLE_CASES if R.gather_ok(c.ph, c.pw)]


@pytest.mark.parametrize('name', ALL_SINGLE)
def test_forward_single_map(dev, name):
    """htd_roi_align_fwd: the workgroup-per-bin and the wavefront-per-bin kernel (R.fwd_form), all rows and with a level list"""
    d = R.make_single(name)
    c = d.case
    ref, A, _, _, near = R.ref_single(name)
    feat, rois = d.feat.to(dev), d.rois.to(dev)
    out = single_fwd(c, feat, rois)
    check(c.fwd, c.kind, out, ref, A, ~near)
    if c.kind == 'random' and (c.ph, c.pw) == (7, 7):           # the suite's customary fp32 tolerance as an outer ceiling
        torch.testing.assert_close(out.cpu()[~near].double(), ref[~near], rtol=1e-5, atol=2e-5)
    bad = (d.rois[:, 0] < 0) | (d.rois[:, 0] >= c.B)
    assert float(out.cpu()[bad].abs().max() if bad.any() else 0.0) == 0.0       # a batch index out of range: zeros
    # a level list: the rows of level 1 are written with the same bits, the others are left alone
    lv = (torch.arange(c.n) % 2).to(dev)
    part = single_fwd(c, feat, rois, lv, 1, fill=-7.0)
    assert torch.equal(part[1::2], out[1::2]) and bool((part[0::2] == -7.0).all())


@pytest.mark.parametrize('name', ALL_SINGLE)
def test_backward_scatter(dev, name):
    """htd_roi_align_bwd: the bin-wise kernel, the row-wise kernel with a slot per map row and with 8 slots striding a taller map
    (R.bwd_form), all rows and with a level list"""
    d = R.make_single(name)
    c = d.case
    _, _, gref, gA, near = R.ref_single(name)
    grad, rois = masked_grad(d.grad, near).to(dev), d.rois.to(dev)
    check(c.bwd, c.kind, single_bwd(c, grad, rois), gref, gA)
    oref, oA = R.ref_single_odd(name)
    lv = (torch.arange(c.n) % 2).to(dev)
    check(c.bwd, c.kind, single_bwd(c, grad, rois, lv, 1), oref, oA)


@pytest.mark.parametrize('name', GATHER_SINGLE)
def test_backward_gather_single_map(dev, name):
    """htd_roi_align_bwd_gather: two wavefronts per tile without a level list, one with; a NaN-filled map comes back clean, two runs
    give the same bits, accumulate = 1 adds onto the map and leaves the pixels no RoI reaches bit for bit"""
    d = R.make_single(name)
    c = d.case
    _, _, gref, gA, near = R.ref_single(name)
    grad, rois = masked_grad(d.grad, near).to(dev), d.rois.to(dev)
    shape = (c.B, c.H, c.W, c.C)
    a = single_gather(c, grad, rois, torch.full(shape, NAN, device=dev), 0)
    check('gather_rs2', c.kind, a, gref, gA)
    assert torch.equal(a, single_gather(c, grad, rois, torch.full(shape, NAN, device=dev), 0))
    gen = torch.Generator().manual_seed(c.n)
    base = R._values(gen, shape, c.kind)
    b = single_gather(c, grad, rois, base.to(dev), 1).cpu()
    assert torch.equal(b[gA == 0], base[gA == 0])
    if c.kind == 'random':
        err = (b.double() - (base.double() + gref)).abs()
        assert bool((err <= C_BOUND * EPS32 * gA + 2 * EPS32 * (base.double() + gref).abs()).all())
    else:
        assert torch.equal(b, (base.double() + gref).float())
    oref, oA = R.ref_single_odd(name)
    lv = (torch.arange(c.n) % 2).to(dev)
    o = single_gather(c, grad, rois, torch.full(shape, NAN, device=dev), 0, lv, 1)
    check('gather_rs1', c.kind, o, oref, oA)
    assert torch.equal(o, single_gather(c, grad, rois, torch.full(shape, NAN, device=dev), 0, lv, 1))


def test_twenty_identical_rois_sum_in_roi_order(dev):
    """the 'fixed' case holds twenty copies of one RoI with twenty different gradients: the gather adds them in RoI order"""
    d = R.make_single('fixed')
    c = d.case
    same = (d.rois[:, 1:] == d.rois[R.N_FIXED, 1:]).all(1) & (d.rois[:, 0] == d.rois[R.N_FIXED, 0])
    assert int(same.sum()) == 20 and not bool(R.ref_single('fixed')[4][same].any())
    rois, grad = d.rois[same], d.grad[same]
    gref, gA = R.roi_align_ref_bwd(grad, rois, d.feat.shape, c.ph, c.pw, c.scale, c.sr, c.aligned)
    c20 = c._replace(n=20)
    got = single_gather(c20, grad.to(dev), rois.to(dev), torch.full(d.feat.shape, NAN, device=dev), 0)
    check('gather_rs2', 'random', got, gref, gA)
    one = single_gather(c20._replace(n=1), grad[:1].to(dev), rois[:1].to(dev), torch.full(d.feat.shape, NAN, device=dev), 0)
    assert float(got.abs().max()) > 0 and torch.equal(got == 0, one == 0)        # the same strip, nothing beside it


def test_gather_rejects_what_it_has_no_kernel_for(dev):
    """more than 8 x 8 bins, more than GL_MAX = 6 levels: a ValueError, nothing launched"""
    d = R.make_single('p9')
    c = d.case
    with pytest.raises(ValueError):
        single_gather(c, d.grad.to(dev), d.rois.to(dev), torch.zeros((c.B, c.H, c.W, c.C), device=dev), 0)
    maps = R._PYR8[:7]
    for ph, L in ((9, 3), (7, 7)):
        Hs, Ws, sc = level_tables(maps[:L])
        n, C = 4, 4
        ms = [torch.zeros((2, h, w, C), device=dev) for h, w, _ in maps[:L]]
        rois = torch.tensor([[0, 0., 0., 8., 8.]] * n, device=dev)
        lv = torch.zeros(n, dtype=torch.int64, device=dev)
        g = torch.zeros((n, ph, ph, C), device=dev)
        ac = (ctypes.c_int * L)(*([0] * L))
        ws, fold = gather_workspace(n, L, dev), fold_workspace(n, Hs, L, min(ph, 8), C, dev)
        with pytest.raises(ValueError):
            call('htd_roi_align_levels_bwd_gather', P(g), P(rois), P(lv), ptr_table(ms), Hs, Ws, sc, ac, L, n, 2, C, ph, ph, 0, 1, P(ws), S())
        with pytest.raises(ValueError):
            call('htd_roi_align_levels_bwd_gather_folded', P(g), P(rois), P(lv), ptr_table(ms), Hs, Ws, sc, ac, L, n, 2, C, ph, ph, 0, 1,
                 P(ws), P(fold), S())
        with pytest.raises(ValueError):
            call('htd_roi_align_all_levels_bwd_gather', ptr_table([g] * L), P(rois), ptr_table(ms), Hs, Ws, sc, ac, L, n, 2, C, ph, ph, 0, 1,
                 P(ws), S())
        with pytest.raises(ValueError):
            call('htd_roi_align_all_levels_bwd_gather_folded', ptr_table([g] * L), P(rois), ptr_table(ms), Hs, Ws, sc, ac, L, n, 2, C, ph,
                 ph, 0, 1, P(ws), P(fold), S())


ALL_LEVELS = [c.name for c in LEVEL_CASES]
GATHER_LEVELS = [c.name for c in LEVEL_CASES if R.gather_ok(c.ph, c.pw, len(c.maps))]


@pytest.mark.parametrize('name', ALL_LEVELS)
def test_forward_levels(dev, name):
    """htd_roi_align_levels_fwd and _amax (the same bits, and max |out| bit for bit; levels -1 and L give zero rows), and
    htd_roi_align_all_levels_fwd with a workgroup or a wavefront per bin (R.all_fwd_form): the bits of L single-map calls"""
    d = R.make_levels(name)
    c = d.case
    L = len(c.maps)
    ref, A, _, near = R.ref_levels(name)
    feats, rois, lv = [f.to(dev) for f in d.feats], d.rois.to(dev), d.levels.to(dev)
    Hs, Ws, sc = level_tables(c.maps)
    out = torch.full((c.n, c.ph, c.pw, c.C), NAN, device=dev)
    call('htd_roi_align_levels_fwd', ptr_table(feats), Hs, Ws, sc, L, P(rois), P(lv), P(out), c.n, c.B, c.C, c.ph, c.pw, c.sr,
         c.aligned, S())
    check('levels_fwd', c.kind, out, ref, A, ~near)
    bad = (d.levels < 0) | (d.levels >= L) | (d.rois[:, 0] < 0) | (d.rois[:, 0] >= c.B)
    assert float(out.cpu()[bad].abs().max() if bad.any() else 0.0) == 0.0
    out2 = torch.full((c.n, c.ph, c.pw, c.C), NAN, device=dev)
    amax = torch.zeros(1, device=dev)
    call('htd_roi_align_levels_fwd_amax', ptr_table(feats), Hs, Ws, sc, L, P(rois), P(lv), P(out2), c.n, c.B, c.C, c.ph, c.pw, c.sr,
         c.aligned, P(amax), S())
    check('levels_fwd_amax', c.kind, out2, ref, A, ~near)
    assert torch.equal(out, out2) and torch.equal(amax[0], out.abs().max())
    # every RoI on every level
    fw, _, nl = R.ref_all(name)
    outs = [torch.full((c.n, c.ph, c.pw, c.C), NAN, device=dev) for _ in range(L)]
    call('htd_roi_align_all_levels_fwd', ptr_table(feats), Hs, Ws, sc, L, P(rois), ptr_table(outs), c.n, c.B, c.C, c.ph, c.pw, c.sr,
         c.aligned, S())
    for l, (h, w, s) in enumerate(c.maps):
        check(c.all_fwd, c.kind, outs[l], fw[l][0], fw[l][1], ~nl[l])
        one = single_fwd(R.Single(name, c.kind, c.B, c.C, h, w, s, c.ph, c.pw, c.sr, c.aligned, c.n, '', '', ''), feats[l], rois)
        assert torch.equal(outs[l], one), l


def levels_gather(c, d, dev, grad, present, acc, bases, folded):
    """htd_roi_align_levels_bwd_gather(_folded) into maps that start as `bases` (None: NaN-filled); present[l] False -> NULL"""
    L = len(c.maps)
    Hs, Ws, sc = level_tables(c.maps)
    ms = [None if not present[l] else (bases[l].to(dev) if acc[l] else torch.full(d.shapes[l], NAN, device=dev)) for l in range(L)]
    ac = (ctypes.c_int * L)(*acc)
    ws = gather_workspace(c.n, L, dev)
    rois, lv = d.rois.to(dev), d.levels.to(dev)
    if folded:
        fold = fold_workspace(c.n, Hs, L, c.pw, c.C, dev)
        call('htd_roi_align_levels_bwd_gather_folded', P(grad), P(rois), P(lv), ptr_table(ms), Hs, Ws, sc, ac, L, c.n, c.B, c.C, c.ph,
             c.pw, c.sr, c.aligned, P(ws), P(fold), S())
    else:
        call('htd_roi_align_levels_bwd_gather', P(grad), P(rois), P(lv), ptr_table(ms), Hs, Ws, sc, ac, L, c.n, c.B, c.C, c.ph, c.pw,
             c.sr, c.aligned, P(ws), S())
    return ms


def all_gather(c, d, dev, grads, acc, bases, folded):
    L = len(c.maps)
    Hs, Ws, sc = level_tables(c.maps)
    ms = [bases[l].to(dev) if acc[l] else torch.full(d.shapes[l], NAN, device=dev) for l in range(L)]
    ac = (ctypes.c_int * L)(*acc)
    ws = gather_workspace(c.n, L, dev)
    rois = d.rois.to(dev)
    if folded:
        fold = fold_workspace(c.n, Hs, L, c.pw, c.C, dev)
        call('htd_roi_align_all_levels_bwd_gather_folded', ptr_table(grads), P(rois), ptr_table(ms), Hs, Ws, sc, ac, L, c.n, c.B, c.C,
             c.ph, c.pw, c.sr, c.aligned, P(ws), P(fold), S())
    else:
        call('htd_roi_align_all_levels_bwd_gather', ptr_table(grads), P(rois), ptr_table(ms), Hs, Ws, sc, ac, L, c.n, c.B, c.C, c.ph,
             c.pw, c.sr, c.aligned, P(ws), S())
    return ms


def check_onto(form, kind, got, base, acc, gref, gA):
    """a gathered map: accumulate = 0 -> the reference; accumulate = 1 -> base + reference, unreached pixels bit for bit"""
    if not acc:
        return check(form, kind, got, gref, gA)
    got = got.cpu()
    assert torch.equal(got[gA == 0], base[gA == 0]), form
    want = base.double() + gref
    if kind != 'random':
        assert torch.equal(got, want.float()), form
    else:
        assert bool(((got.double() - want).abs() <= C_BOUND * EPS32 * gA + 2 * EPS32 * want.abs()).all()), form


@pytest.mark.parametrize('name', GATHER_LEVELS)
def test_backward_gather_levels(dev, name):
    """htd_roi_align_levels_bwd_gather and _folded (one wavefront per tile): a level without RoIs, a level without a map, fresh and
    accumulated maps in one launch; folded == unfolded == one htd_roi_align_bwd_gather per level == a second run, bit for bit"""
    d = R.make_levels(name)
    c = d.case
    L = len(c.maps)
    _, _, bw, near = R.ref_levels(name)
    grad = masked_grad(d.grad, near).to(dev)
    gen = torch.Generator().manual_seed(c.n + 1)
    bases = [R._values(gen, shp, c.kind) for shp in d.shapes]
    for present, acc in (((True, True, False), (0, 1, 0)), ((False, True, True), (1, 0, 1))):
        got = levels_gather(c, d, dev, grad, present, acc, bases, False)
        fol = levels_gather(c, d, dev, grad, present, acc, bases, True)
        again = levels_gather(c, d, dev, grad, present, acc, bases, False)
        for l in range(L):
            if not present[l]:
                assert got[l] is None
                continue
            check_onto('levels_gather_rs1', c.kind, got[l], bases[l], acc[l], *bw[l])
            check_onto('levels_gather_rs1_folded', c.kind, fol[l], bases[l], acc[l], *bw[l])
            assert torch.equal(got[l], fol[l]) and torch.equal(got[l], again[l]), l
            h, w, s = c.maps[l]
            per = bases[l].to(dev) if acc[l] else torch.full(d.shapes[l], NAN, device=dev)
            single_gather(c, grad, d.rois.to(dev), per, acc[l], d.levels.to(dev), l, d.shapes[l], s)
            assert torch.equal(got[l], per), l


@pytest.mark.parametrize('name', GATHER_LEVELS)
def test_backward_gather_all_levels(dev, name):
    """htd_roi_align_all_levels_bwd_gather and _folded (two wavefronts per tile), a gradient tensor per level: folded == unfolded ==
    one htd_roi_align_bwd_gather per level == a second run, bit for bit"""
    d = R.make_levels(name)
    c = d.case
    L = len(c.maps)
    _, bw, nl = R.ref_all(name)
    grads = [masked_grad(g, nl[l]).to(dev) for l, g in enumerate(d.grads)]
    gen = torch.Generator().manual_seed(c.n + 2)
    bases = [R._values(gen, shp, c.kind) for shp in d.shapes]
    acc = (0, 1, 0)
    got = all_gather(c, d, dev, grads, acc, bases, False)
    fol = all_gather(c, d, dev, grads, acc, bases, True)
    again = all_gather(c, d, dev, grads, acc, bases, False)
    for l in range(L):
        check_onto('all_gather_rs2', c.kind, got[l], bases[l], acc[l], *bw[l])
        check_onto('all_gather_rs2_folded', c.kind, fol[l], bases[l], acc[l], *bw[l])
        assert torch.equal(got[l], fol[l]) and torch.equal(got[l], again[l]), l
        per = bases[l].to(dev) if acc[l] else torch.full(d.shapes[l], NAN, device=dev)
        single_gather(c, grads[l], d.rois.to(dev), per, acc[l], None, 0, d.shapes[l], c.maps[l][2])
        assert torch.equal(got[l], per), l


def test_forced_roi_split_in_a_fresh_process(dev, tmp_path):
    """HTD_ROI_BWD_SPLIT = 4 (compiled, never chosen) and = 1 (instead of the 2 the forms without a level list choose) is read once
    per process: tools/roi_gather_driver.py runs the gather entry points in a child, once per value; the maps it leaves are held
    against the reference here.  A child that fails ends the test before the next one starts."""
    assert 'HTD_ROI_BWD_SPLIT' not in os.environ
    names = ('L3_sr', 'xL3')
    for name in names:
        d = R.make_levels(name)
        c = d.case
        near, nl = R.ref_levels(name)[3], R.ref_all(name)[2]
        grads = [masked_grad(g, nl[l] | near) for l, g in enumerate(d.grads)]
        np.savez(str(tmp_path / f'{name}_in.npz'), rois=d.rois.numpy(), levels=d.levels.numpy(), shapes=np.array(d.shapes),
                 scales=np.array(d.scales, np.float32), params=np.array([c.ph, c.pw, c.sr, c.aligned]),
                 **{f'grad{l}': g.numpy() for l, g in enumerate(grads)})
    for split in ('4', '1'):
        files = [str(tmp_path / f'{name}_{kind}.npz') for name in names for kind in ('in', f'out{split}')]
        run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'roi_gather_driver.py')] + files,
                             env=dict(os.environ, HTD_ROI_BWD_SPLIT=split), timeout=120, capture_output=True, text=True)
        assert run.returncode == 0, (split, run.stderr[-2000:])
        for name in names:
            d = R.make_levels(name)
            c = d.case
            L = len(c.maps)
            near, nl = R.ref_levels(name)[3], R.ref_all(name)[2]
            got = {k: torch.from_numpy(v) for k, v in np.load(str(tmp_path / f'{name}_out{split}.npz')).items()}
            keep = ~(nl[0] | near)
            gref, gA = R.roi_align_ref_bwd(d.grads[0][keep], d.rois[keep], d.shapes[0], c.ph, c.pw, d.scales[0], c.sr, c.aligned)
            check(f'gather_forced_rs{split}', c.kind, got['single'], gref, gA)
            for l in range(L):
                keep = ~(nl[l] | near)
                sel = ~(nl[0] | near) & (d.levels == l)                    # grad0's rows that were not zeroed
                lref, lA = R.roi_align_ref_bwd(d.grad[sel], d.rois[sel], d.shapes[l], c.ph, c.pw, d.scales[l], c.sr, c.aligned)
                check(f'levels_gather_forced_rs{split}', c.kind, got[f'levels{l}'], lref, lA)
                assert torch.equal(got[f'levels{l}'], got[f'levels_folded{l}'])
                aref, aA = R.roi_align_ref_bwd(d.grads[l][keep], d.rois[keep], d.shapes[l], c.ph, c.pw, d.scales[l], c.sr, c.aligned)
                check(f'all_gather_forced_rs{split}', c.kind, got[f'all{l}'], aref, aA)
                assert torch.equal(got[f'all{l}'], got[f'all_folded{l}'])


def test_report_observed_ratios():
    """not a check: the worst |got - ref| / (2^-24 A) of every form on the random cases of this run, for whoever changes the kernels"""
    for form in sorted(OBSERVED):
        print(f'observed {form:28s} {OBSERVED[form]:10.2f}   (bound {C_BOUND:.0f})')
