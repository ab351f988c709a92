"""tests/dcn_ref.py (the float64 reference of the deformable sampling kernels) against three independent statements of the
same operator: the C oracle's forward, the oracle's torch restatement (deform_groups = 1, gradients) and finite differences.
CPU only."""
import pytest
import torch

import dcn_ref as R

U = 2.0 ** -24          # unit roundoff of fp32


def _case(B, C, H, W, kh, stride, pad, dil, dg, with_mask, seed, sigma=1.5):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = R.out_size(H, W, kh, kh, stride, pad, dil)
    taps, M = kh * kh, B * Ho * Wo
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    # offsets on a 2^-10 grid: position = integer + offset is then exact in fp32 too, so an fp32 implementation samples
    # at the very point the float64 reference does and differs from it by the rounding of its sums alone
    off = torch.round(torch.randn(M, dg * taps * 2, generator=g, dtype=torch.float64) * sigma * 1024) / 1024
    mask = torch.rand(M, dg * taps, generator=g, dtype=torch.float64) if with_mask else None
    return x, off, mask, (Ho, Wo, taps, M)


def _nchw(t, B, Ho, Wo):
    """[M, ch] kernel layout -> (B, ch, Ho, Wo) of the Python interfaces."""
    return t.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('B,C,H,W,kh,stride,pad,dil,dg,with_mask', [
    (2, 8, 9, 11, 3, 1, 1, 1, 2, False),
    (1, 12, 7, 8, 3, 1, 1, 1, 3, False),
    (2, 16, 9, 11, 3, 1, 2, 2, 4, True),
    (2, 8, 9, 11, 3, 2, 1, 1, 2, True),
    (2, 8, 6, 7, 1, 1, 0, 1, 2, False),
    (1, 16, 10, 9, 3, 2, 2, 2, 1, True)])
def test_forward_matches_c_oracle(B, C, H, W, kh, stride, pad, dil, dg, with_mask):
    """columns @ W^T against oracle.ops.deform_conv2d.  The oracle sums K = taps * C products in fp32, so it may differ
    from the float64 value by (K + 8) * 2^-24 * sum |terms| (K additions, and a few roundings inside each term)."""
    from oracle import ops as O
    x, off, mask, (Ho, Wo, taps, M) = _case(B, C, H, W, kh, stride, pad, dil, dg, with_mask, seed=C + H)
    x, off = x.float().double(), off.float().double()               # what the fp32 oracle is given, exactly
    mask = mask.float().double() if with_mask else None
    Co = 5
    w = torch.randn(Co, C, kh, kh, generator=torch.Generator().manual_seed(1)).double()
    cols = R.im2col(x, off, mask, kh, kh, stride, pad, dil, dg)
    A, n = R.im2col_terms(x, off, mask, kh, kh, stride, pad, dil, dg)
    assert n == 4 and bool((A >= cols.abs() - 1e-12).all())
    wk = w.permute(0, 2, 3, 1).reshape(Co, taps * C)                # [Co][tap][c], the order of the columns
    y = _nchw(cols.reshape(M, -1) @ wk.t(), B, Ho, Wo)
    bound = _nchw(A.reshape(M, -1) @ wk.abs().t(), B, Ho, Wo) * (taps * C + 8) * U
    ref = O.deform_conv2d(x.permute(0, 3, 1, 2), _nchw(off, B, Ho, Wo), w, stride, pad, dil, deform_groups=dg,
                          mask=None if mask is None else _nchw(mask, B, Ho, Wo)).double()
    err = (y - ref).abs()
    print('max err %.3g, max err / bound %.3g, max |y| %.3g' % (err.max(), (err / bound.clamp_min(1e-300)).max(), ref.abs().max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('kh,stride,pad,dil,with_mask', [(3, 1, 1, 1, False), (3, 2, 1, 1, True), (3, 1, 2, 2, True),
                                                         (1, 1, 0, 1, False)])
def test_gradients_match_oracle_autograd(kh, stride, pad, dil, with_mask):
    """gx, goffset, gmask of col2im against autograd through oracle.ops.deform_conv2d_autograd, both in float64."""
    from oracle import ops as O
    B, C, H, W, Co = 2, 8, 7, 9, 6
    x, off, mask, (Ho, Wo, taps, M) = _case(B, C, H, W, kh, stride, pad, dil, 1, with_mask, seed=kh + stride + dil)
    g = torch.Generator().manual_seed(2)
    w = torch.randn(Co, C, kh, kh, generator=g, dtype=torch.float64)
    gy = torch.randn(B, Co, Ho, Wo, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_()
    offr = _nchw(off, B, Ho, Wo).requires_grad_()
    mr = _nchw(mask, B, Ho, Wo).requires_grad_() if with_mask else None
    y = O.deform_conv2d_autograd(xr, offr, w, stride, pad, dil, mask=mr)
    grads = torch.autograd.grad((y * gy).sum(), [xr, offr] + ([mr] if with_mask else []))
    wk = w.permute(0, 2, 3, 1).reshape(Co, taps * C)
    cols = R.im2col(x, off, mask, kh, kh, stride, pad, dil)
    torch.testing.assert_close(_nchw(cols.reshape(M, -1) @ wk.t(), B, Ho, Wo), y.detach(), rtol=1e-12, atol=1e-12)
    gcol = (gy.permute(0, 2, 3, 1).reshape(M, Co) @ wk).reshape(M, taps, C)
    gx, goff, gmask = R.col2im(x, off, mask, gcol, kh, kh, stride, pad, dil)
    torch.testing.assert_close(gx.permute(0, 3, 1, 2), grads[0], rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(_nchw(goff, B, Ho, Wo), grads[1], rtol=1e-11, atol=1e-11)
    if with_mask:
        torch.testing.assert_close(_nchw(gmask, B, Ho, Wo), grads[2], rtol=1e-11, atol=1e-11)
    else:
        assert gmask is None
    # the bound terms dominate the values they bound, and n_gx counts the corners that count
    t = R.col2im_terms(x, off, mask, gcol, kh, kh, stride, pad, dil)
    assert bool((t['A_gx'] >= gx.abs() - 1e-10).all()) and bool((t['A_goffset'] >= goff.abs() - 1e-10).all())
    if with_mask:
        assert bool((t['A_gmask'] >= gmask.abs() - 1e-10).all())
    s = R.sample_points(off, B, H, W, kh, kh, stride, pad, dil, 1)
    assert t['n_c'] == C and float(t['n_gx'].sum()) == C * sum(int(ok.sum()) for ok in s.ok)
    assert bool((t['A_gx'][t['n_gx'] == 0] == 0).all())


def test_gradcheck_two_deformable_groups():
    """Finite differences in float64, deform_groups = 2 with a mask; sampling points kept 0.15 away from integers (the
    kinks of bilinear interpolation) and from the border rule's jumps."""
    B, C, H, W, dg = 1, 4, 5, 6, 2
    x, off, mask, (Ho, Wo, taps, M) = _case(B, C, H, W, 3, 1, 1, 1, dg, True, seed=5)
    frac = off - torch.floor(off)
    off = torch.floor(off) + frac.clamp(0.15, 0.85)                 # base positions are integers
    x.requires_grad_(), off.requires_grad_(), mask.requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b, c: R.im2col(a, b, c, 3, 3, 1, 1, 1, dg), (x, off, mask), eps=1e-6,
                                    atol=1e-7, rtol=1e-6)


def test_border_rule_by_hand():
    """One pixel, 1x1 kernel, a 2x2 map [[1, 2], [3, 4]]: the rule at -1, in (-1, 0), on integers, in (H-1, H) and at H."""
    x = torch.tensor([[1., 2.], [3., 4.]], dtype=torch.float64).view(1, 2, 2, 1).expand(1, 2, 2, 4).contiguous()
    # the single output pixel of a stride-2 1x1 conv sits at (0, 0), so the offset is the sampling position
    for (h, w), want in {(-1., 0.): 0., (0., -1.): 0., (2., 0.): 0., (0., 2.): 0., (-0.25, 0.): 0.75, (0., -0.5): 0.5,
                         (1.5, 0.): 1.5, (0., 1.25): 1.5, (1., 1.): 4., (0.5, 0.5): 2.5, (1.5, 1.5): 1., (50., -50.): 0.,
                         (-0.5, -0.5): 0.25}.items():
        off = torch.tensor([[h, w]], dtype=torch.float64)
        col = R.im2col(x, off, None, 1, 1, 2, 0, 1)
        assert col.shape == (1, 1, 4) and float(col[0, 0, 0]) == want, ((h, w), float(col[0, 0, 0]), want)
