"""The fp64 RoIAlign reference of roi_align_ref.py and the case table of test_gpu_roi_align_ops.py, checked on the CPU: the einsum
form against the per-sample definition, both against the fp32 C oracle, the transpose by the adjoint identity, the exact cases'
exactness, how many RoIs the drop-boundary filter leaves out, and that the table reaches every kernel form of roi_align.hip."""
import pytest
import torch

import roi_align_ref as R
from roi_align_ref import D64, EPS32, LEVEL_CASES, LEVELS, SINGLE, SINGLE_CASES

SLOW_CASES = ['n5', 'n1', 'fixed', 'fixed_a', 'wide', 'tall', 'p1', 'p83', 'p25', 'p9', 'w1', 'h1', 'm1', 'odd', 'x_small', 'x_odd', 'x_edge']
SLOW_ROWS = 16          # the fixed rows come first


@pytest.mark.parametrize('name', SLOW_CASES)
def test_einsum_reference_equals_the_per_sample_definition(name):
    d = R.make_single(name)
    c = d.case
    rois = d.rois[:SLOW_ROWS]
    feat = d.feat[..., :4]
    slow = R.roi_align_ref_slow(feat, rois, c.ph, c.pw, c.scale, c.sr, c.aligned)
    fast, A = R.roi_align_ref(feat, rois, c.ph, c.pw, c.scale, c.sr, c.aligned)
    assert float((fast - slow).abs().max()) <= 1e-12
    assert bool((A >= fast.abs() - 1e-12).all())
    bad = (rois[:, 0] < 0) | (rois[:, 0] >= c.B)
    assert float(slow[bad].abs().max() if bad.any() else 0.0) == 0.0 and float(fast[bad].abs().max() if bad.any() else 0.0) == 0.0


def _oracle_single(d, sel):
    """the C oracle (NCHW fp32) on the rows `sel`, in the kernels' layouts"""
    from oracle import ops as O
    c = d.case
    f = d.feat.permute(0, 3, 1, 2).contiguous()
    out = O.roi_align_fwd(f, d.rois[sel], (c.ph, c.pw), c.scale, c.sr, bool(c.aligned)).permute(0, 2, 3, 1)
    g = d.grad[sel].permute(0, 3, 1, 2).contiguous()
    gf = O.roi_align_bwd(g, d.rois[sel], f.shape, c.scale, c.sr, bool(c.aligned)).permute(0, 2, 3, 1)
    return out, gf


def _ratio(got, ref, A):
    """max |got - ref| / (2^-24 A); where A == 0 every term is zero and got must be exactly zero"""
    err = (got.to(D64) - ref).abs()
    assert float(err[A == 0].max() if (A == 0).any() else 0.0) == 0.0
    return float((err[A > 0] / (EPS32 * A[A > 0])).max()) if (A > 0).any() else 0.0


def _single_oracle_ratios(name):
    d = R.make_single(name)
    c = d.case
    out, A, gf, gA, near = R.ref_single(name)
    ok = (d.rois[:, 0] >= 0) & (d.rois[:, 0] < c.B)          # the oracle indexes the batch unguarded
    assert float(out[~ok].abs().max() if (~ok).any() else 0.0) == 0.0
    sel = ok & ~near
    o_out, o_gf = _oracle_single(d, sel)
    return o_out, out[sel], A[sel], o_gf, gf, gA


@pytest.fixture(scope='module')
def oracle_ratios():
    """{case: (forward ratio, backward ratio)} of the C oracle against the fp64 reference, over the whole case table"""
    res = {}
    for c in SINGLE_CASES:
        o_out, out, A, o_gf, gf, gA = _single_oracle_ratios(c.name)
        res[c.name] = (_ratio(o_out, out, A), _ratio(o_gf, gf, gA))
    from oracle import ops as O
    for c in LEVEL_CASES:
        d = R.make_levels(c.name)
        fw, bw, nl = R.ref_all(c.name)
        ok = (d.rois[:, 0] >= 0) & (d.rois[:, 0] < c.B)
        rf = rb = 0.0
        for l, (h, w, s) in enumerate(c.maps):
            sel = ok & ~nl[l]
            f = d.feats[l].permute(0, 3, 1, 2).contiguous()
            o = O.roi_align_fwd(f, d.rois[sel], (c.ph, c.pw), s, c.sr, bool(c.aligned)).permute(0, 2, 3, 1)
            rf = max(rf, _ratio(o, fw[l][0][sel], fw[l][1][sel]))
            g = d.grads[l][sel].permute(0, 3, 1, 2).contiguous()
            og = O.roi_align_bwd(g, d.rois[sel], f.shape, s, c.sr, bool(c.aligned)).permute(0, 2, 3, 1)
            rb = max(rb, _ratio(og, bw[l][0], bw[l][1]))
        res[c.name] = (rf, rb)
    return res


def test_c_oracle_agrees_at_fp32_accuracy_and_c_oracle_is_what_the_module_records(oracle_ratios):
    """c_oracle = max |oracle - ref| / (2^-24 A) over the whole table, forward and backward: the fp32 per-sample oracle's distance
    from the fp64 reference (most of it the float32 sample coordinates: a coordinate near 100 px carries 4e-6 px of rounding).
    The GPU tests allow the kernels R.C_BOUND = 4 * R.C_ORACLE; the recorded constant may not be below the measured one."""
    for name, (rf, rb) in oracle_ratios.items():
        print(f'c_oracle {name:10s} forward {rf:9.2f} backward {rb:9.2f}')
    worst = max(max(v) for v in oracle_ratios.values())
    print(f'c_oracle = {worst:.2f} (recorded {R.C_ORACLE}), c = {R.C_BOUND}')
    assert worst <= R.C_ORACLE and R.C_ORACLE <= 1.25 * worst + 1, (worst, R.C_ORACLE)
    assert R.C_BOUND == 4 * R.C_ORACLE
    # fp32 accuracy in the suite's customary terms on the unit-normal 7 x 7 cases
    for name in ('n5', 'wave4', 'wave260', 'rows'):
        o_out, out, A, o_gf, gf, gA = _single_oracle_ratios(name)
        torch.testing.assert_close(o_out.to(D64), out, rtol=1e-5, atol=2e-5)
        torch.testing.assert_close(o_gf.to(D64), gf, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('name', [c.name for c in SINGLE_CASES if c.kind != 'random'])
def test_exact_cases_are_exact_for_the_c_oracle(name, oracle_ratios):
    """Dyadic geometry and small integers: the fp32 oracle, whose order of operations is not the kernels', equals the fp64
    reference, and the reference has room in 24 bits (terms are multiples of the weights' quantum, partial sums bounded by A)."""
    assert oracle_ratios[name] == (0.0, 0.0)
    d = R.make_single(name)
    c = d.case
    out, A, gf, gA, near = R.ref_single(name)
    assert torch.equal(out.float().double(), out) and torch.equal(gf.float().double(), gf)
    wy, wx, _ = R._operator(d.rois, c.B, c.H, c.W, c.ph, c.pw, c.scale, c.sr, c.aligned)
    quantum = _quantum(wy) * _quantum(wx)
    assert max(float(A.max()), float(gA.max())) / quantum < 2 ** 24, (float(gA.max()), quantum)


def _quantum(w):
    q = 1.0
    while not bool(((w / q) == (w / q).round()).all()):
        q /= 2
        assert q > 2.0 ** -20
    return q


@pytest.mark.parametrize('name', [c.name for c in LEVEL_CASES if c.kind != 'random'])
def test_exact_level_cases_are_exact_for_the_c_oracle(name, oracle_ratios):
    assert oracle_ratios[name] == (0.0, 0.0)
    d = R.make_levels(name)
    c = d.case
    fw, bw, nl = R.ref_all(name)
    for l, (h, w, s) in enumerate(c.maps):
        wy, wx, _ = R._operator(d.rois, c.B, h, w, c.ph, c.pw, s, c.sr, c.aligned)
        quantum = _quantum(wy) * _quantum(wx)
        assert max(float(fw[l][1].max()), float(bw[l][1].max())) / quantum < 2 ** 24, (name, l)


@pytest.mark.parametrize('name', ['n5', 'fixed', 'wide', 'tall', 'p25', 'p9', 'rows', 'm1', 'x_rows'])
def test_backward_reference_is_the_transpose(name):
    """<ref(x), g> == <x, ref_bwd(g)> to 1e-12 relative (of the sum of the absolute terms)"""
    d = R.make_single(name)
    c = d.case
    x, g = d.feat.double(), d.grad.double()
    out, A = R.roi_align_ref(x, d.rois, c.ph, c.pw, c.scale, c.sr, c.aligned)
    gf, gA = R.roi_align_ref_bwd(g, d.rois, x.shape, c.ph, c.pw, c.scale, c.sr, c.aligned)
    lhs, rhs = float((out * g).sum()), float((x * gf).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((A * g.abs()).sum())
    assert abs(float((A * g.abs()).sum()) - float((x.abs() * gA).sum())) <= 1e-12 * float((A * g.abs()).sum())


def test_level_wrappers_pick_the_map_and_zero_unknown_levels():
    d = R.make_levels('L3')
    c = d.case
    out, A, bw, near = R.ref_levels('L3')
    bad = (d.levels < 0) | (d.levels >= len(c.maps))
    assert int(bad.sum()) == 2 and float(out[bad].abs().max()) == 0.0
    for l in c.use:
        sel = d.levels == l
        one, _ = R.roi_align_ref(d.feats[l], d.rois[sel], c.ph, c.pw, d.scales[l], c.sr, c.aligned)
        assert torch.equal(out[sel], one)
    assert float(bw[1][0].abs().max()) == 0.0                       # the empty level


def test_drop_boundary_filter_leaves_out_at_most_five_percent_and_nothing_exact():
    for c in SINGLE_CASES:
        near = R.ref_single(c.name)[4]
        share = float(near.double().mean())
        print(f'{c.name:10s} near the drop boundary: {int(near.sum())} of {c.n}')
        assert share <= 0.05 if c.kind == 'random' else int(near.sum()) == 0, (c.name, share)
    for c in LEVEL_CASES:
        nl = R.near_levels(c.name)
        for l in range(len(c.maps)):
            share = float(nl[l].double().mean())
            print(f'{c.name:10s} level {l} near the drop boundary: {int(nl[l].sum())} of {c.n}')
            assert share <= 0.05 if c.kind == 'random' else int(nl[l].sum()) == 0, (c.name, l, share)


def test_near_drop_boundary_flags_near_misses_only():
    f = torch.float32
    # aligned = 0, one bin, one sample: the sample is the RoI's centre
    rois = torch.tensor([[0, -2.0, 1.0, 0.0, 3.0],            # x = -1 exactly: kept by both, not flagged
                         [0, -2.0005, 1.0, 0.0, 3.0],         # x = -1.00025: flagged
                         [0, 4.0, 1.0, 6.0, 3.0],             # x = W exactly
                         [0, 4.0, 1.0, 6.001, 3.0],           # x = W + 0.0005: flagged
                         [0, 1.0, 5.0, 3.0, 7.0],             # y = H exactly
                         [0, 1.0, 5.0, 3.0, 7.001],           # flagged
                         [0, 1.0, 1.0, 3.0, 3.0]], dtype=f)   # inside
    got = R.near_drop_boundary(rois, 6, 5, 1, 1, 1.0, 1, 0)
    assert got.tolist() == [False, True, False, True, False, True, False]


FORMS = {'fwd_split8', 'fwd_wave', 'levels_fwd', 'levels_fwd_amax', 'all_fwd_w8', 'all_fwd_w1', 'bwd_bins', 'bwd_rows_full',
         'bwd_rows_strided', 'gather_rs2', 'gather_rs1', 'levels_gather_rs1', 'levels_gather_rs1_folded', 'all_gather_rs2',
         'all_gather_rs2_folded'}


def forms_of_single(c):
    forms = {R.fwd_form(c.n, c.ph, c.pw, c.C), R.bwd_form(c.n, c.ph, c.pw, c.C, c.H)}
    if R.gather_ok(c.ph, c.pw):
        forms |= {'gather_rs2', 'gather_rs1'}           # without / with a level list
    return forms


def forms_of_levels(c):
    L = len(c.maps)
    forms = {'levels_fwd', 'levels_fwd_amax', R.all_fwd_form(L, c.n, c.ph, c.pw, c.C)}
    if R.gather_ok(c.ph, c.pw, L):
        forms |= {'levels_gather_rs1', 'levels_gather_rs1_folded', 'all_gather_rs2', 'all_gather_rs2_folded'}
    return forms


def test_cases_select_every_kernel_form():
    """The case table put through the launchers' arithmetic (roi_align.hip: launch(), htd_roi_align_all_levels_fwd, gather_split):
    each case takes the form it is labelled with, and every form is taken by at least one exact and one random case."""
    reached = {'random': set(), 'exact': set()}
    for c in SINGLE_CASES:
        assert R.fwd_form(c.n, c.ph, c.pw, c.C) == c.fwd and R.bwd_form(c.n, c.ph, c.pw, c.C, c.H) == c.bwd, c.name
        if 'T' in c.flags:                           # 8 slots striding a 20-row map under RoIs taller than 8 rows
            assert c.bwd == 'bwd_rows_strided' and c.n * R.chunks_of(c.C) >= 2048 and c.H > 8
        forms = forms_of_single(c)
        reached['random' if c.kind == 'random' else 'exact'] |= forms
        print(f'{c.name:10s} {c.kind:6s} n={c.n:<5d} C={c.C:<4d} {c.H}x{c.W} out {c.ph}x{c.pw}: {", ".join(sorted(forms))}')
    for c in LEVEL_CASES:
        assert R.all_fwd_form(len(c.maps), c.n, c.ph, c.pw, c.C) == c.all_fwd, c.name
        forms = forms_of_levels(c)
        reached['random' if c.kind == 'random' else 'exact'] |= forms
        print(f'{c.name:10s} {c.kind:6s} n={c.n:<5d} C={c.C:<4d} L={len(c.maps)} out {c.ph}x{c.pw}: {", ".join(sorted(forms))}')
    assert reached['random'] == FORMS and reached['exact'] == FORMS, (FORMS - reached['random'], FORMS - reached['exact'])
    # the thresholds themselves, from either side
    assert R.fwd_form(167, 7, 7, 4) == 'fwd_split8' and R.fwd_form(168, 7, 7, 4) == 'fwd_wave' and R.fwd_form(84, 7, 7, 260) == 'fwd_wave'
    assert R.all_fwd_form(3, 222, 7, 7, 4) == 'all_fwd_w8' and R.all_fwd_form(3, 223, 7, 7, 4) == 'all_fwd_w1'
    assert R.bwd_form(255, 7, 7, 4, 9) == 'bwd_bins' and R.bwd_form(256, 7, 7, 4, 9) == 'bwd_rows_full'
    assert R.bwd_form(300, 9, 9, 4, 14) == 'bwd_bins' and R.bwd_form(128, 8, 8, 260, 9) == 'bwd_rows_full'
    assert R.bwd_form(2047, 7, 7, 4, 20) == 'bwd_rows_strided' and R.bwd_form(1820, 7, 7, 4, 10) == 'bwd_rows_full'
    assert R.bwd_form(2048, 7, 7, 4, 20) == 'bwd_rows_strided' and R.bwd_form(2048, 7, 7, 4, 8) == 'bwd_rows_full'
    assert not R.gather_ok(9, 9) and not R.gather_ok(7, 7, 7) and R.gather_ok(8, 8, 6)


def test_case_table_covers_the_geometry_the_kernels_branch_on():
    S, Lv = SINGLE_CASES, LEVEL_CASES
    assert {(c.ph, c.pw) for c in S} >= {(1, 1), (7, 7), (8, 8), (8, 3), (2, 5), (9, 9)}
    for kind in ('random', ):
        assert {c.sr for c in S if c.kind == kind} == {0, 1, 2, 4} and {c.aligned for c in S if c.kind == kind} == {0, 1}
    assert {c.C for c in S} >= {4, 256, 260} and {c.W for c in S} >= {1, 5, 8, 13} and {c.n for c in S} >= {1, 63, 65, 130}
    assert any(c.H == 1 for c in S) and any(c.H == 1 and c.W == 1 for c in S)
    assert any(c.B * c.H * ((c.W + 7) // 8) * R.chunks_of(c.C) % 2 == 1 for c in S)          # an odd tile count: RS = 2's idle group
    assert {len(c.maps) for c in Lv} >= {3, 8}
    # footprints past 64 pixels: a bin 75 columns wide, a bin 70 rows tall, a RoI more than 64 columns wide on the row-wise form
    assert SINGLE['wide'].W / SINGLE['wide'].pw > 64 and SINGLE['tall'].H / SINGLE['tall'].ph > 64
    # ... and in every other kernel that walks a footprint in blocks of 64: the wavefront-per-bin forward (fwd_wave), both forms of
    # the all-levels forward, the levels forward.  sampling_ratio = 4 over one bin: samples at 1/8, 3/8, 5/8, 7/8 of the extent
    assert SINGLE['wide_wave'].fwd == SINGLE['tall_wave'].fwd == 'fwd_wave'
    assert SINGLE['wide_wave'].W * 6 / 8 > 64 and SINGLE['tall_wave'].H * 6 / 8 > 64
    c = LEVELS['L3_wide']
    assert c.all_fwd == 'all_fwd_w8' and c.maps[0][0] / c.ph > 64 and c.maps[0][1] / c.pw > 64
    c = LEVELS['L3_big']
    assert c.all_fwd == 'all_fwd_w1' and (c.ph, c.pw, c.sr) == (1, 1, 4) and c.maps[0][0] * 6 / 8 > 64 and c.maps[0][1] * 6 / 8 > 64
    for name in ('L3_wide', 'L3_big'):
        d = R.make_levels(name)
        assert int(d.levels[1]) == 0 and d.rois[1].tolist()[1:] == [0.0, 0.0, float(d.case.maps[0][1]), float(d.case.maps[0][0])]
    for name in ('rows', 'x_rows'):
        d = R.make_single(name)
        assert float(((d.rois[:, 3] - d.rois[:, 1]) * d.case.scale).max()) > 64 and d.case.bwd == 'bwd_rows_full'
    for name in ('strided', 'x_strided'):
        d = R.make_single(name)
        rows = ((d.rois[:, 4] - d.rois[:, 2]) * d.case.scale)[R.N_FIXED if 'F' in d.case.flags else 0:]     # past the fixed geometry
        assert float(rows.min()) > 8.5, name
    d = R.make_single('x_edge')
    assert d.case.aligned == 0 and d.case.sr == 1 and (d.case.ph, d.case.pw) == (1, 1)
    cx = (d.rois[:, 1] + d.rois[:, 3]) / 2 * d.case.scale
    cy = (d.rois[:, 2] + d.rois[:, 4]) / 2 * d.case.scale
    assert {-1.0, float(d.case.W)} <= set(cx.tolist()) and {-1.0, float(d.case.H)} <= set(cy.tolist())
