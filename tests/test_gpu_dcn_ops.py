"""The deformable sampling kernels of csrc/dcn.hip, called through the C entry points (so the launcher's choice of kernel
is part of what is tested), against the float64 reference tests/dcn_ref.py.

Inputs.  x and the gradient columns are bf16-representable, so the float and the bf16 entry points see the same numbers and
share one reference.  Offsets lie on a 2^-10 grid: sampling position = integer + offset is then exact in fp32 (|position| <
128 needs 7 + 10 bits), as are the bilinear fractions lh, lw, 1 - lh, 1 - lw and their pairwise products (10 + 10 bits).  The
kernels therefore sample at exactly the reference's point with exactly its weights, and what is left is the rounding of the
products and sums, which the bounds below count.  (Without the grid an fp32 position carries an error of half an ulp of the
POSITION, 2^-20 at h = 16, which no count of roundings of the VALUE covers.)

Border kinds.  `build_offsets` places, in chosen (pixel, group, tap) slots, one sample of each kind of the border rule (zero
outside the open interval (-1, H) x (-1, W), per-corner zero padding) and fills the rest with randn * sigma; `check_kinds`
asserts from the reference's own validity masks that each kind is present.

Bounds, u = 2^-24, A = the reference sum with every term replaced by its absolute value, n = its number of terms:
  columns         (4 + 8) u A: 4 products and 3 additions, one mask product.
  goffset, gmask  (n + 8) u A, n = channels of the deformable group: at most 7 roundings inside a term, n - 1 additions
                  (lane-serial, then the wave tree).
  gx              (n + 8) u A with n = the corners landing on the element (+ 1 for the value gx held before: the entry point
                  accumulates) and A including that value: 3 roundings inside a term, n additions in any order.
  bf16 columns    2^-8 |ref| on top: half an ulp of the final rounding to bf16.
No figure here was chosen by running the kernels."""
import functools

import pytest
import torch

import dcn_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BF = torch.bfloat16
GUARD = 256                      # sentinel elements before and after every output buffer (keeps 16-byte alignment)
SENTINEL = -12288.0              # bf16-representable

GEOM = {'3x3s1': (3, 1, 1, 1), '3x3s2': (3, 2, 1, 1), '3x3d2': (3, 1, 2, 2), '3x3s2d2': (3, 2, 2, 2), '1x1': (1, 1, 0, 1)}


# --------------------------------------------------------------------------------------------------------------- inputs
def build_offsets(B, H, W, k, stride, pad, dil, dg, sigma, gen):
    """[M, dg*taps*2] float64 on the 2^-10 grid: one slot per border kind, the rest randn * sigma."""
    Ho, Wo = R.out_size(H, W, k, k, stride, pad, dil)
    taps, M = k * k, B * Ho * Wo
    off = (torch.round(torch.randn(M, dg, taps, 2, generator=gen, dtype=torch.float64) * sigma * 1024) / 1024)
    targets = [(0.375, 1.6875),                    # fractional, all four corners in the map
               (1.0, 2.0),                         # exactly on a pixel
               (-1.0, 1.25), (float(H), 1.25), (1.25, -1.0), (1.25, float(W)),              # exactly on the open border
               (-0.25, 1.5), (H - 0.75, 1.5), (1.5, -0.25), (1.5, W - 0.75),                # two corners live
               (50.0 + 0.5, 1.0), (1.0, -50.0 - 0.5)]                                       # far outside
    total = M * dg * taps
    assert total >= len(targets)
    step = total // len(targets)
    for i, (th, tw) in enumerate(targets):
        slot = i * step + i % step                 # distinct slots, spread over pixels, groups and taps
        m, rest = divmod(slot, dg * taps)
        g, t = divmod(rest, taps)
        oy, ox = (m // Wo) % Ho, m % Wo
        off[m, g, t, 0] = th - (oy * stride - pad + (t // k) * dil)
        off[m, g, t, 1] = tw - (ox * stride - pad + (t % k) * dil)
    return off.reshape(M, dg * taps * 2)


def check_kinds(s, H, W):
    """Every kind of the border rule occurs (a condition on the inputs; build_offsets satisfies it by construction)."""
    h, w, ok = s.h, s.w, s.ok
    frac = lambda t: t != torch.floor(t)
    all4 = ok[0] & ok[1] & ok[2] & ok[3]
    n_ok = sum(o.long() for o in ok)
    kinds = {
        'fractional inside': all4 & frac(h) & frac(w),
        'integer': s.inside & ~frac(h) & ~frac(w) & (h >= 0) & (w >= 0),
        'h == -1': (h == -1) & (w > 0) & (w < W - 1), 'h == H': (h == H) & (w > 0) & (w < W - 1),
        'w == -1': (w == -1) & (h > 0) & (h < H - 1), 'w == W': (w == W) & (h > 0) & (h < H - 1),
        'h in (-1, 0)': (h > -1) & (h < 0) & (n_ok == 2), 'h in (H-1, H)': (h > H - 1) & (h < H) & (n_ok == 2),
        'w in (-1, 0)': (w > -1) & (w < 0) & (n_ok == 2), 'w in (W-1, W)': (w > W - 1) & (w < W) & (n_ok == 2),
        'far outside': ((h.abs() > 40) | (w.abs() > 40)) & ~s.inside}
    for name, m in kinds.items():
        assert bool(m.any()), 'no sample of kind: ' + name
    for name in ('h == -1', 'h == H', 'w == -1', 'w == W', 'far outside'):
        assert not bool((kinds[name] & s.inside).any())


class Case:
    pass


@functools.lru_cache(maxsize=4)
def make_case(B, H, W, C, geom, dg, with_mask, sigma):
    """Inputs (float64, CPU) and the reference results of one geometry; shared by the float and bf16 tests of it."""
    k, stride, pad, dil = GEOM[geom]
    gen = torch.Generator().manual_seed(1000 * C + 10 * H + dg + (7 if with_mask else 0))
    c = Case()
    c.args = (B, H, W, C, k, k, stride, pad, dil, dg)
    c.geo = (k, k, stride, pad, dil, dg)
    c.Ho, c.Wo = R.out_size(H, W, k, k, stride, pad, dil)
    c.taps, c.M = k * k, B * c.Ho * c.Wo
    q = lambda t: t.to(BF).double()
    c.x = q(torch.randn(B, H, W, C, generator=gen))
    c.off = build_offsets(B, H, W, k, stride, pad, dil, dg, sigma, gen)
    c.mask = torch.rand(c.M, dg * c.taps, generator=gen).double() if with_mask else None      # fp32-representable
    c.gcol = q(torch.randn(c.M, c.taps, C, generator=gen))
    c.gx0 = torch.randn(B, H, W, C, generator=gen).double()                                  # what gx holds before the call
    c.s = R.sample_points(c.off, B, H, W, k, k, stride, pad, dil, dg)
    check_kinds(c.s, H, W)
    c.cols = R.im2col(c.x, c.off, c.mask, *c.geo)
    c.A_cols, c.n_cols = R.im2col_terms(c.x, c.off, c.mask, *c.geo)
    c.gx, c.goff, c.gmask = R.col2im(c.x, c.off, c.mask, c.gcol, *c.geo)
    c.t = R.col2im_terms(c.x, c.off, c.mask, c.gcol, *c.geo)
    return c


def guarded(body):
    """A device copy of `body` as a slice of a larger allocation with sentinel rows around it -> (slice, whole)."""
    whole = torch.full((body.numel() + 2 * GUARD,), SENTINEL, dtype=body.dtype, device='cuda:0')
    view = whole[GUARD:GUARD + body.numel()].view(body.shape)
    view.copy_(body)
    return view, whole


def nan_out(shape, dtype=torch.float32):
    return guarded(torch.full(shape, float('nan'), dtype=dtype))


def guards_intact(whole):
    torch.cuda.synchronize()
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def within(got, ref, bound, what):
    got = got.detach().double().cpu()
    assert not bool(torch.isnan(got).any()), what + ': NaN left in the output'
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('%s: max err %.3g, max err / bound %.3g' % (what, float(err.max()), ratio))
    bad = err > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError('%s: %d elements beyond the bound, first at %s: got %r, want %r, bound %.3g' % (
            what, int(bad.sum()), i, float(got[i]), float(ref[i]), float(bound[i])))


def dev_inputs(c, dt):
    d = 'cuda:0'
    return (c.x.to(dt).to(d), c.off.float().to(d), None if c.mask is None else c.mask.float().to(d), c.gcol.to(dt).to(d))


def run_im2col(c, dt):
    from htd_amd import capi
    P = capi.ptr
    x, off, mask, _ = dev_inputs(c, dt)
    cols, whole = nan_out((c.M, c.taps, c.args[3]), dt)
    capi.call('htd_deform_im2col' + ('_bf16' if dt == BF else ''), P(x), P(off), P(mask), P(cols), *c.args,
              capi.current_stream_ptr())
    assert guards_intact(whole), 'im2col wrote outside its columns'
    return cols


def check_im2col(c, dt):
    cols = run_im2col(c, dt)
    bound = (c.n_cols + 8) * U * c.A_cols
    if dt == BF:
        bound = bound + 2.0 ** -8 * c.cols.abs()
    within(cols, c.cols, bound, 'columns')
    dead = ~(c.s.ok[0] | c.s.ok[1] | c.s.ok[2] | c.s.ok[3])                     # [M, dg, taps]: nothing to sample
    assert bool(dead.any())
    rows = R.per_channel(dead, c.args[3] // c.args[9])
    assert bool((cols.float().cpu()[rows] == 0).all()), 'columns of an outside tap are not exactly zero'


def run_col2im(c, dt, want=(True, True, True)):
    """-> gx, goffset, gmask (None where not requested or no mask); gx starts from c.gx0."""
    from htd_amd import capi
    P = capi.ptr
    x, off, mask, gcol = dev_inputs(c, dt)
    dg, taps = c.args[9], c.taps
    gx, w_gx = guarded(c.gx0.float()) if want[0] else (None, None)
    goff, w_go = nan_out((c.M, dg * taps * 2)) if want[1] else (None, None)
    gmask, w_gm = nan_out((c.M, dg * taps)) if want[2] and mask is not None else (None, None)
    capi.call('htd_deform_col2im' + ('_bf16' if dt == BF else ''), P(x), P(off), P(mask), P(gcol), P(gx), P(goff),
              P(gmask), *c.args, capi.current_stream_ptr())
    for w in (w_gx, w_go, w_gm):
        assert w is None or guards_intact(w), 'col2im wrote outside an output buffer'
    return gx, goff, gmask


def check_col2im(c, dt, want=(True, True, True)):
    gx, goff, gmask = run_col2im(c, dt, want)
    t = c.t
    if gx is not None:
        gx0 = c.gx0.float().double()
        within(gx, gx0 + c.gx, (t['n_gx'] + 1 + 8) * U * (t['A_gx'] + gx0.abs()), 'gx')
    if goff is not None:
        within(goff, c.goff, (t['n_c'] + 8) * U * t['A_goffset'], 'goffset')
    if gmask is not None:
        within(gmask, c.gmask, (t['n_c'] + 8) * U * t['A_gmask'], 'gmask')
    return gx, goff, gmask


# --------------------------------------------------------------------------------------------------------------- im2col
IM2COL_CH = [(4, 1, False), (4, 1, True),             # one lane
             (64, 1, False), (64, 1, True),
             (260, 1, False), (260, 1, True),         # second pass of the lane loop, not a multiple of 64
             (8, 2, False), (8, 2, True),             # a float4 exactly fills a deformable group
             (64, 4, True)]


@pytest.mark.parametrize('dt', [torch.float32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('C,dg,with_mask', IM2COL_CH)
@pytest.mark.parametrize('geom', ['3x3s1', '3x3s2', '3x3d2', '1x1'])
def test_im2col(geom, C, dg, with_mask, dt):
    """deform_im2col_kernel<float>, <bf16>: every column within its bound, outside taps exactly zero, nothing written
    outside the columns, no element left unwritten."""
    check_im2col(make_case(2, 9, 11, C, geom, dg, with_mask, 1.5), dt)


# -------------------------------------------------------------------------------------------------------- col2im, direct
@pytest.mark.parametrize('C,dg,with_mask', [(16, 1, False), (16, 1, True), (260, 1, False), (8, 2, False), (8, 2, True),
                                            (128, 4, True)])       # 128: C % 64 == 0, but the groups force the direct kernel
@pytest.mark.parametrize('geom', ['3x3s1', '3x3s2', '3x3d2', '1x1'])
def test_col2im_direct(geom, C, dg, with_mask):
    """deform_col2im_kernel<float>: gx (accumulated onto a non-zero tensor), goffset and gmask within their bounds."""
    check_col2im(make_case(2, 9, 11, C, geom, dg, with_mask, 1.5), torch.float32)


@pytest.mark.parametrize('C,dg', [(16, 1), (8, 2)])
@pytest.mark.parametrize('absent', [0, 1, 2], ids=['no_gx', 'no_goffset', 'no_gmask'])
def test_col2im_direct_null_outputs(absent, C, dg):
    """Each output of the direct kernel in turn passed as NULL: the other two are unchanged."""
    want = tuple(i != absent for i in range(3))
    check_col2im(make_case(2, 9, 11, C, '3x3s1', dg, True, 1.5), torch.float32, want)


# ----------------------------------------------------------------------------------------------------- col2im, row-owned
@pytest.mark.parametrize('with_mask', [False, True], ids=['v1', 'mask'])
@pytest.mark.parametrize('sigma', [0.4, 4.0])          # all halves inside the LDS window / most in the common bucket
@pytest.mark.parametrize('H,W', [(19, 21), (3, 3)])    # not a multiple of the 8 (4) pixel tile / smaller than a tile
@pytest.mark.parametrize('C', [64, 192])               # one slice / three slices, one per workgroup
@pytest.mark.parametrize('geom', ['3x3s1', '3x3s2', '3x3d2', '3x3s2d2', '1x1'])
def test_col2im_rows(geom, C, H, W, sigma, with_mask):
    """deform_col2im_rows_kernel<float> and deform_goffset_kernel<float> (C % 64 == 0, one deformable group, stride <= 2;
    the dilated 3x3 window is 15 x 15 x 64 floats = 76 KB, just under the launcher's limit)."""
    check_col2im(make_case(2, H, W, C, geom, 1, with_mask, sigma), torch.float32)


def test_col2im_rows_null_goffset_and_gmask():
    """The row-owned path with only gx, and with only one of goffset / gmask, requested."""
    c = make_case(2, 19, 21, 64, '3x3s1', 1, True, 0.4)
    for want in ((True, False, False), (True, True, False), (True, False, True)):
        check_col2im(c, torch.float32, want)


def test_col2im_rows_several_slices_per_workgroup():
    """slices_per_block = 2.  Launch arithmetic of launch_col2im: stride 2 -> 4 x 4 pixel tiles; a 64 x 64 map gives
    32 x 32 outputs = 64 tiles per image, B = 16 -> nt = 1024 tiles; C = 192 -> 3 slices; groups_y = min(3, ceil(2048 / nt))
    = 2, slices_per_block = ceil(3 / 2) = 2: workgroup row 0 walks slices 0 and 1 through one LDS window (zeroed in
    between), row 1 the single slice 2.  A float64 reference of 28 M gradient columns is too slow for the suite, so this
    one case compares with the DIRECT kernel run on 32-channel slices (as test_col2im_row_owned_kernel_matches_direct_kernel
    does), both sides fp32: bound 2 (n + 8) u A, A from the same direct run on |gcol|, n = corners landing on the element
    (tests/dcn_ref.py, evaluated on the device)."""
    from htd_amd import capi
    P, S = capi.ptr, capi.current_stream_ptr
    dev = torch.device('cuda:0')
    B, H, W, C, stride = 16, 64, 64, 192, 2
    Ho, Wo = R.out_size(H, W, 3, 3, stride, 1, 1)
    M = B * Ho * Wo
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(B, H, W, C, generator=g, device=dev)
    off = torch.round(torch.randn(M, 18, generator=g, device=dev) * 1.5 * 1024) / 1024
    gcol = torch.randn(M, 9, C, generator=g, device=dev)
    gx, whole = guarded(torch.zeros(B, H, W, C))
    capi.call('htd_deform_col2im', P(x), P(off), None, P(gcol), P(gx), None, None, B, H, W, C, 3, 3, stride, 1, 1, 1, S())
    assert guards_intact(whole)
    ref, A = torch.zeros_like(x), torch.zeros_like(x)
    for c0 in range(0, C, 32):
        xs, gs = x[..., c0:c0 + 32].contiguous(), gcol[..., c0:c0 + 32].contiguous()
        for dst, src in ((ref, gs), (A, gs.abs())):
            part = torch.zeros_like(xs)
            capi.call('htd_deform_col2im', P(xs), P(off), None, P(src), P(part), None, None, B, H, W, 32, 3, 3, stride, 1, 1,
                      1, S())
            dst[..., c0:c0 + 32] = part
    s = R.sample_points(off.double(), B, H, W, 3, 3, stride, 1, 1, 1)
    n = torch.zeros(B * H * W, dtype=torch.float64, device=dev)
    for ok, idx in zip(s.ok, s.idx):
        n.index_add_(0, idx.reshape(-1), ok.reshape(-1).double())
    bound = 2 * (n.view(B, H, W, 1) + 8) * U * A.double()
    err = (gx.double() - ref.double()).abs()
    print('gx: max err %.3g, max err / bound %.3g' % (float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert float(ref.abs().max()) > 1 and bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize('C,dg,H,W,geom', [(128, 1, 19, 21, '3x3s1'),          # row-owned + goffset kernel
                                           (192, 1, 3, 3, '3x3s2d2'),
                                           (16, 1, 9, 11, '3x3s1'),            # direct
                                           (128, 4, 9, 11, '3x3d2')])
def test_col2im_bf16(C, dg, H, W, geom):
    """deform_col2im_rows_kernel<bf16>, deform_goffset_kernel<bf16>, deform_col2im_kernel<bf16>, with a mask: the inputs are
    bf16-representable and everything after the loads is fp32, so the float bounds hold unchanged."""
    check_col2im(make_case(2, H, W, C, geom, dg, True, 1.5), BF)


# --------------------------------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize('C,dg,H,W', [(8, 2, 9, 11), (192, 1, 19, 21)], ids=['direct', 'rows'])
def test_outputs_without_atomics_repeat_bit_for_bit(C, dg, H, W):
    """Columns, goffset and gmask of two consecutive calls are identical.  Not asserted of gx: both col2im kernels add into
    it with global float atomics in an order that is not fixed (and the row-owned kernel fills its buckets in atomic
    order), so gx may differ in the last bits from call to call."""
    c = make_case(2, H, W, C, '3x3s1', dg, True, 1.5)
    a, b = run_im2col(c, torch.float32), run_im2col(c, torch.float32)
    assert torch.equal(a, b)
    (_, go1, gm1), (_, go2, gm2) = run_col2im(c, torch.float32), run_col2im(c, torch.float32)
    assert torch.equal(go1, go2) and torch.equal(gm1, gm2)


# ---------------------------------------------------------------------------------------------- through the Python layer
CL = torch.channels_last


def _nchw(t, B, Ho, Wo):
    return t.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('C,with_mask', [(16, False), (16, True), (64, False), (64, True)])
def test_deform_conv2d_two_deformable_groups(C, with_mask):
    """deform_conv2d(deform_groups=2), v1 and v2: forward against the C oracle, gradients against float64 autograd of
    dcn_ref.im2col followed by an einsum; tolerances of tests/test_gpu_dcn.py::test_deform_conv_fwd_bwd."""
    from htd_amd.dcn import deform_conv2d
    from oracle import ops as O
    dev = torch.device('cuda:0')
    B, H, W, Co, dg = 2, 11, 13, 24, 2
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
    off = torch.randn(B, dg * 18, H, W, generator=g) * 1.5
    mask = torch.rand(B, dg * 9, H, W, generator=g) if with_mask else None
    go = torch.randn(B, Co, H, W, generator=g)
    ref_c = O.deform_conv2d(x, off, w, 1, 1, 1, deform_groups=dg, mask=mask)
    leaves = [t.double().requires_grad_() for t in (x, off, w) + ((mask,) if with_mask else ())]
    xr, offr, wr = leaves[:3]
    mr = leaves[3] if with_mask else None
    k2 = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    cols = R.im2col(xr.permute(0, 2, 3, 1), k2(offr), k2(mr) if with_mask else None, 3, 3, 1, 1, 1, dg)
    ref = _nchw(torch.einsum('mkc,ock->mo', cols, wr.reshape(Co, C, 9)), B, H, W)
    torch.testing.assert_close(ref.detach().float(), ref_c, rtol=1e-4, atol=1e-4)          # the two references agree
    grads = torch.autograd.grad((ref * go.double()).sum(), leaves)
    xd = x.to(dev).contiguous(memory_format=CL).requires_grad_()
    od = off.to(dev).contiguous(memory_format=CL).requires_grad_()
    wd = w.to(dev).contiguous(memory_format=CL).requires_grad_()
    md = mask.to(dev).contiguous(memory_format=CL).requires_grad_() if with_mask else None
    y = deform_conv2d(xd, od, wd, 1, 1, 1, deform_groups=dg, mask=md)
    torch.testing.assert_close(y.detach().cpu(), ref_c, rtol=1e-4, atol=1e-4)
    y.backward(go.to(dev))
    torch.testing.assert_close(xd.grad.cpu(), grads[0].float(), rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(od.grad.cpu(), grads[1].float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(wd.grad.cpu(), grads[2].float(), rtol=1e-3, atol=1e-3)
    if with_mask:
        torch.testing.assert_close(md.grad.cpu(), grads[3].float(), rtol=1e-3, atol=1e-3)


def test_pack_layer_two_deformable_groups():
    """DeformConv2dPack(deform_groups=2): conv_offset predicts 2 * 2 * 9 = 36 channels, and with its zero initialisation
    the layer is the plain convolution."""
    import torch.nn.functional as F
    from htd_amd.dcn import DeformConv2dPack
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    layer = DeformConv2dPack(32, 32, 3, padding=1, deform_groups=2).to(dev)
    assert layer.conv_offset.weight.shape == (36, 32, 3, 3) and layer.conv_offset.bias.shape == (36,)
    assert layer.conv_offset.weight.abs().sum().item() == 0.0 and layer.conv_offset.bias.abs().sum().item() == 0.0
    x = torch.randn(2, 32, 10, 12, device=dev).contiguous(memory_format=CL)
    y = layer(x)
    ref = F.conv2d(x.cpu().double(), layer.weight.detach().cpu().double(), None, 1, 1)
    torch.testing.assert_close(y.detach().cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_deform_conv_bf16_two_deformable_groups():
    """deform_groups = 2 through DeformConv2dBf16Function against the fp32 kernels on the same bf16-rounded operands, with
    the bounds of tests/test_gpu_dcn.py::test_deform_conv_bf16_tracks_fp32 (relative L2 error)."""
    from htd_amd.dcn import DeformConv2dBf16Function, DeformConv2dFunction
    dev = torch.device('cuda:0')
    B, C, H, W, Co, dg = 2, 64, 13, 15, 64, 2
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g).to(BF).float()
    w = (torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5).to(BF).float()
    bias = torch.randn(Co, generator=g) * 0.1
    off = torch.randn(B, dg * 18, H, W, generator=g) * 1.2
    go = torch.randn(B, Co, H, W, generator=g).to(BF).float()
    outs = []
    for dt in (torch.float32, BF):
        xd = x.to(dev).to(dt).contiguous(memory_format=CL).requires_grad_()
        od = off.to(dev).contiguous(memory_format=CL).requires_grad_()
        wd = w.to(dev).contiguous(memory_format=CL).requires_grad_()
        bd = bias.to(dev).requires_grad_()
        if dt == BF:
            y = DeformConv2dBf16Function.apply(xd, od, None, wd, 1, 1, 1, dg, bd, False)
        else:
            y = DeformConv2dFunction.apply(xd, od, None, wd, 1, 1, 1, dg, bd, False, 1)
        assert y.dtype == dt
        y.backward(go.to(dev).to(dt))
        outs.append([t.detach().float() for t in (y, xd.grad, od.grad, wd.grad, bd.grad)])
    for n, a, b in zip(['y', 'gx', 'goffset', 'gw', 'gbias'], *outs):
        err = float((a - b).norm() / a.norm())
        tol = {'y': 5e-3, 'gx': 1.5e-2, 'goffset': 2e-2, 'gw': 1e-2, 'gbias': 5e-3}[n]
        assert err <= tol, (n, err)
