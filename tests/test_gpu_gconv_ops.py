"""The grouped convolution kernels of csrc/gconv.hip through their C entry points, exact on integers.

Inputs are integers in [-3, 3] stored as fp32.  A product is at most 9 and the longest sum here has under 10^4 terms, so every
partial sum is an integer far below 2^24: fp32 arithmetic (the kernels use fp32-input MFMAs) is exact in any order, and each
result must be torch.equal to the float64 evaluation cast to fp32.  Every output buffer is a NaN-filled slice of a larger
allocation with sentinel rows around it: the sentinels must survive and no NaN may be left.

Layouts: x [B, H, W, C]; w grouped KRSC [C][taps][cg]; y [B, Ho, Wo, C]; the column buffer of the `cols` forms [M][taps][C]."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
GUARD = 256
SENTINEL = -12288.0


def guarded_nan(*shape):
    whole = torch.full((int(np.prod(shape)) + 2 * GUARD,), SENTINEL, device='cuda:0')
    view = whole[GUARD:-GUARD].view(shape)
    view.fill_(float('nan'))
    return view, whole


def guards_intact(whole):
    torch.cuda.synchronize()
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).double()


def out_size(H, W, kh, kw, stride, pad, dil):
    return (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1


def exact(got, want, what):
    got, want = got.cpu(), want.float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, want %r' % (
            what, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))


# ------------------------------------------------------------------------------------------------------- weight packing
def pack_ref(w, C, groups, taps, transpose):
    """The layout comment of gconv.hip restated: wp[((os*islabs + is)*taps + tap)*64 + l][s], l = n + 16 j, holds
    forward  : W[out = 16 os + n][tap][in = 16 in_slab + 4 j + s]
    transpose: W[out = 16 in_slab + 4 j + s][tap][in = 16 os + n]
    with W the dense [C][taps][C] tensor that is w [C][taps][cg] inside a group and zero across groups, and
    in_slab = os (cg <= 16) or (os // islabs) * islabs + is."""
    cg = C // groups
    islabs = 1 if cg <= 16 else cg // 16
    dense = torch.zeros(C, taps, C, dtype=w.dtype)
    for o in range(C):
        g = o // cg
        dense[o, :, g * cg:(g + 1) * cg] = w[o]
    wp = torch.zeros(C // 16, islabs, taps, 64, 4, dtype=w.dtype)
    for os in range(C // 16):
        for i in range(islabs):
            in_slab = os if islabs == 1 else (os // islabs) * islabs + i
            for l in range(64):
                n, j = l % 16, l // 16
                for s in range(4):
                    a, c = 16 * os + n, 16 * in_slab + 4 * j + s
                    wp[os, i, :, l, s] = dense[c, :, a] if transpose else dense[a, :, c]
    return wp.reshape(-1), dense


def pack(w, C, groups, kh, kw, transpose):
    """w [C, taps, cg] float64 (CPU) -> packed device tensor, through the C entry points."""
    from htd_amd import capi
    n = capi.lib().htd_gconv2d_packed_floats(C, groups, kh, kw)
    assert n > 0
    wp, whole = guarded_nan(n)
    capi.call('htd_gconv2d_pack_weights', capi.ptr(w.float().cuda()), capi.ptr(wp), C, groups, kh, kw, int(transpose),
              capi.current_stream_ptr())
    assert guards_intact(whole)
    return wp


@pytest.mark.parametrize('transpose', [0, 1])
@pytest.mark.parametrize('C,groups,kh,kw', [(16, 4, 3, 3), (48, 6, 1, 1), (64, 4, 2, 2), (64, 2, 3, 3), (96, 2, 1, 3),
                                            (128, 2, 3, 1)])        # cg = 4, 8, 16, 32, 48, 64
def test_pack_weights(C, groups, kh, kw, transpose):
    cg, taps = C // groups, kh * kw
    w = ints(torch.Generator().manual_seed(C + groups), C, taps, cg)
    w[w == 0] = 1                                   # no zero weights: every zero in the packed tensor is a cross-group one
    want, dense = pack_ref(w, C, groups, taps, transpose)
    islabs = 1 if cg <= 16 else cg // 16
    assert want.numel() == (C // 16) * islabs * taps * 256
    got = pack(w, C, groups, kh, kw, transpose)
    assert got.numel() == want.numel()              # = htd_gconv2d_packed_floats
    exact(got, want, 'packed weights')
    assert int((got == 0).sum()) == int((want == 0).sum())          # cross-group entries are exactly zero


# ----------------------------------------------------------------------------------- forward, data and weight gradients
def run_gconv(B, H, W, C, groups, kh, kw, stride, pad, dil, use_bias, relu, gen):
    """All three cols = 0 entry points on one integer problem against F.conv2d(groups=) in float64 and its autograd."""
    from htd_amd import capi
    P, S = capi.ptr, capi.current_stream_ptr
    cg, taps = C // groups, kh * kw
    Ho, Wo = out_size(H, W, kh, kw, stride, pad, dil)
    geo = (B, H, W, C, groups, kh, kw, stride, pad, dil)
    x = ints(gen, B, H, W, C)
    w = ints(gen, C, taps, cg)
    bias = ints(gen, C) if use_bias else None
    gy = ints(gen, B, Ho, Wo, C)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_()
    wr = w.reshape(C, kh, kw, cg).permute(0, 3, 1, 2).clone().requires_grad_()
    conv = F.conv2d(xr, wr, None, stride, pad, dil, groups)
    gxr, gwr = torch.autograd.grad((conv * gy.permute(0, 3, 1, 2)).sum(), [xr, wr])
    yr = conv.detach() + (bias.view(1, C, 1, 1) if use_bias else 0)
    yr = torch.relu(yr) if relu else yr
    xd, gyd = x.float().cuda(), gy.float().cuda()
    y, whole = guarded_nan(B, Ho, Wo, C)
    capi.call('htd_gconv2d_fwd', P(xd), P(pack(w, C, groups, kh, kw, 0)), P(bias.float().cuda() if use_bias else None), P(y),
              *geo, int(relu), 0, S())
    assert guards_intact(whole), 'forward wrote outside y'
    exact(y, yr.permute(0, 2, 3, 1), 'y')
    gx, whole = guarded_nan(B, H, W, C)
    capi.call('htd_gconv2d_bwd_data', P(gyd), P(pack(w, C, groups, kh, kw, 1)), P(gx), *geo, 0, S())
    assert guards_intact(whole), 'data gradient wrote outside gx'
    exact(gx, gxr.permute(0, 2, 3, 1), 'gx')
    nbytes = capi.lib().htd_gconv2d_wgrad_workspace_bytes(*geo)
    assert nbytes > 0 and nbytes % 4 == 0
    ws, whole_ws = guarded_nan(nbytes // 4)
    gw, whole = guarded_nan(C, taps, cg)
    capi.call('htd_gconv2d_bwd_weight', P(xd), P(gyd), P(gw), *geo, 0, P(ws), S())
    assert guards_intact(whole) and guards_intact(whole_ws), 'weight gradient wrote outside gw or its workspace'
    exact(gw, gwr.permute(0, 2, 3, 1).reshape(C, taps, cg), 'gw')


# B, H, W, C, groups, kh, kw, stride, pad, dil.  M = B * Ho * Wo output pixels; the data gradient runs over B * H * W.
TABLE = [
    (1, 5, 7, 16, 4, 3, 3, 1, 1, 1),        # cg 4; C = 16: one slab, three idle waves; M = 35 < 64, not a multiple of 4
    (3, 6, 5, 48, 1, 3, 3, 1, 1, 1),        # cg 48: three input slabs per output slab; M = 90
    (1, 9, 11, 64, 8, 3, 3, 2, 1, 1),       # cg 8, stride 2; M = 30
    (3, 7, 9, 96, 6, 3, 3, 1, 2, 2),        # cg 16, dilation 2, pad 2; M = 189
    (1, 13, 16, 128, 4, 3, 3, 3, 1, 1),     # cg 32, stride 3: the generic-stride branch of the data gradient; M = 30
    (1, 6, 6, 128, 2, 3, 3, 1, 0, 1),       # cg 64, pad 0; M = 16
    (1, 1, 257, 64, 4, 3, 3, 1, 1, 1),      # M = 257: two weight-gradient chunks, of 132 and 125 rows (chunk_rows =
                                            # ceil(ceil(M / chunks) / 4) * 4 keeps the last one nearly full) (KW3)
    (1, 1, 257, 64, 16, 1, 1, 1, 0, 1),     # M = 257, 1x1: the non-KW3 instantiations
    (3, 14, 13, 16, 1, 3, 3, 1, 1, 1),      # M = 546 > 512: three chunks; one slab of cg 16
    (3, 13, 14, 128, 32, 3, 3, 1, 1, 1),    # M = 546, cg 4 at C = 128
    (1, 8, 9, 64, 4, 2, 2, 1, 0, 1),        # 2x2; M = 56
    (3, 9, 8, 48, 3, 2, 2, 2, 1, 2),        # 2x2, stride 2, dilation 2; M = 60
    (3, 6, 7, 64, 2, 1, 3, 1, 1, 1),        # 1x3 (KW3 with 3 taps), cg 32; M = 168
    (1, 7, 6, 96, 12, 3, 1, 1, 1, 1),       # 3x1 (not KW3: dy = tap, dx = 0), cg 8; M = 56
    (3, 9, 9, 128, 8, 1, 1, 2, 0, 1),       # 1x1 stride 2; M = 75
    (1, 10, 11, 48, 12, 1, 1, 3, 0, 1),     # 1x1 stride 3, cg 4; M = 16
    (3, 11, 10, 64, 1, 3, 3, 2, 2, 2),      # cg 64, stride 2 with dilation 2; M = 90
    (1, 12, 12, 96, 2, 3, 3, 3, 0, 2),      # cg 48, stride 3, dilation 2; M = 9
    (1, 7, 8, 16, 2, 2, 2, 3, 2, 1),        # 2x2 stride 3 pad 2, cg 8; M = 16
    (1, 10, 10, 64, 2, 3, 3, 1, 0, 1),      # M = 64 exactly: one full block
    (3, 10, 9, 96, 3, 3, 3, 2, 1, 1)]       # cg 32 at C = 96: the last block of slabs half idle; M = 75


@pytest.mark.parametrize('row', range(len(TABLE)))
def test_gconv_fwd_dgrad_wgrad_exact(row):
    """gconv_kernel<G_CONV>, <G_DGRAD> and gconv_wgrad_kernel<G_CONV>, each with KW3 on (kw = 3) and off; bias and ReLU
    epilogue on and off in turn."""
    run_gconv(*TABLE[row], use_bias=row % 2 == 0, relu=row % 4 < 2, gen=torch.Generator().manual_seed(100 + row))


def test_table_covers_every_listed_value():
    """The table above holds each channel count, group width, kernel, stride, dilation, pad, batch and pixel count that the
    kernels branch on (a condition on the table, not on the kernels)."""
    col = lambda i: {r[i] for r in TABLE}
    assert {r[3] // r[4] for r in TABLE} >= {4, 8, 16, 32, 48, 64} and col(3) >= {16, 48, 64, 96, 128}
    assert {(r[5], r[6]) for r in TABLE} >= {(3, 3), (1, 1), (2, 2), (1, 3), (3, 1)}
    assert col(7) >= {1, 2, 3} and col(9) >= {1, 2} and col(8) >= {0, 1, 2} and col(0) >= {1, 3}
    M = {r[0] * int(np.prod(out_size(r[1], r[2], *r[5:10]))) for r in TABLE}
    assert 257 in M and min(M) < 64 and max(M) > 512 and any(m % 4 for m in M)
    assert {r[6] == 3 for r in TABLE} == {True, False}


# ---------------------------------------------------------------------------------------------------- the `cols` forms
@pytest.mark.parametrize('B,H,W,kh,pad', [(2, 5, 5, 3, 1), (3, 10, 10, 3, 1), (2, 6, 6, 2, 0)],
                         ids=['M50', 'M300', 'M50_2x2'])
@pytest.mark.parametrize('C,groups', [(64, 16), (64, 4), (128, 4)], ids=['cg4', 'cg16', 'cg32'])
def test_gconv_cols_forms_exact(C, groups, B, H, W, kh, pad):
    """cols = 1: the grouped GEMM over gathered columns [M][taps][C] (gconv_kernel<G_COLS>, <G_DGRAD_COLS>,
    gconv_wgrad_kernel<G_COLS>; the 2x2 case takes their non-KW3 instantiations) against a float64 einsum per group.  The
    data gradient must write all `taps` rows of every pixel."""
    from htd_amd import capi
    P, S = capi.ptr, capi.current_stream_ptr
    kw = kh
    cg, taps = C // groups, kh * kw
    Ho, Wo = out_size(H, W, kh, kw, 1, pad, 1)
    M = B * Ho * Wo
    assert M in (50, 300)
    geo = (B, H, W, C, groups, kh, kw, 1, pad, 1)
    gen = torch.Generator().manual_seed(C + groups + M)
    cols, w, bias, gy = ints(gen, M, taps, C), ints(gen, C, taps, cg), ints(gen, C), ints(gen, M, C)
    cg_ = cols.reshape(M, taps, groups, cg)
    wg, gyg = w.reshape(groups, cg, taps, cg), gy.reshape(M, groups, cg)          # [g][o][tap][ci], [m][g][o]
    y_ref = torch.relu(torch.einsum('mtgc,gotc->mgo', cg_, wg).reshape(M, C) + bias)
    gcol_ref = torch.einsum('mgo,gotc->mtgc', gyg, wg).reshape(M, taps, C)
    gw_ref = torch.einsum('mgo,mtgc->gotc', gyg, cg_).reshape(C, taps, cg)
    cd, gyd = cols.float().cuda(), gy.float().cuda()
    y, whole = guarded_nan(M, C)
    capi.call('htd_gconv2d_fwd', P(cd), P(pack(w, C, groups, kh, kw, 0)), P(bias.float().cuda()), P(y), *geo, 1, 1, S())
    assert guards_intact(whole)
    exact(y, y_ref, 'y (cols)')
    gcol, whole = guarded_nan(M, taps, C)
    capi.call('htd_gconv2d_bwd_data', P(gyd), P(pack(w, C, groups, kh, kw, 1)), P(gcol), *geo, 1, S())
    assert guards_intact(whole)
    assert not bool(torch.isnan(gcol).any()), 'the data gradient left rows of the gradient columns unwritten'
    exact(gcol, gcol_ref, 'gradient columns')
    nbytes = capi.lib().htd_gconv2d_wgrad_workspace_bytes(*geo)
    ws, whole_ws = guarded_nan(nbytes // 4)
    gw, whole = guarded_nan(C, taps, cg)
    capi.call('htd_gconv2d_bwd_weight', P(cd), P(gyd), P(gw), *geo, 1, P(ws), S())
    assert guards_intact(whole) and guards_intact(whole_ws)
    exact(gw, gw_ref, 'gw (cols)')


# ----------------------------------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize('C,groups,kh,kw', [(48, 4, 3, 3), (64, 4, 2, 5), (24, 6, 3, 3)],
                         ids=['12_per_group', '10_taps', 'C_not_16n'])
def test_gconv_rejects(C, groups, kh, kw):
    """Unsupported shapes come back as an error from every entry point, and nothing is launched: the outputs keep their NaN."""
    from htd_amd import capi
    P, S = capi.ptr, capi.current_stream_ptr
    B, H, W = 1, 8, 8
    geo = (B, H, W, C, groups, kh, kw, 1, 1, 1)
    Ho, Wo = out_size(H, W, kh, kw, 1, 1, 1)
    x = torch.ones(B, H, W, C, device='cuda:0')
    gy = torch.ones(B, Ho, Wo, C, device='cuda:0')
    wp = torch.ones(C * C * kh * kw * 4, device='cuda:0')
    outs = [guarded_nan(max(B * Ho * Wo, B * H * W) * C * kh * kw) for _ in range(4)]
    err = (ValueError, capi.HtdError)
    with pytest.raises(err):
        capi.call('htd_gconv2d_pack_weights', P(x), P(outs[0][0]), C, groups, kh, kw, 0, S())
    with pytest.raises(err):
        capi.call('htd_gconv2d_fwd', P(x), P(wp), None, P(outs[1][0]), *geo, 0, 0, S())
    with pytest.raises(err):
        capi.call('htd_gconv2d_bwd_data', P(gy), P(wp), P(outs[2][0]), *geo, 0, S())
    with pytest.raises(err):
        capi.call('htd_gconv2d_bwd_weight', P(x), P(gy), P(outs[3][0]), *geo, 0, P(wp), S())
    assert capi.lib().htd_gconv2d_wgrad_workspace_bytes(*geo) == -1
    for view, whole in outs:
        assert guards_intact(whole) and bool(torch.isnan(view).all())


# ----------------------------------------------------------------------------------------------------------------- fuzz
def test_gconv_fuzz_exact():
    """30 random valid geometries from one seed through the three cols = 0 entry points, integer-exact, in-process."""
    rs = np.random.RandomState(20240)
    gen = torch.Generator().manual_seed(20240)
    done = 0
    while done < 30:
        cg = int(rs.choice([4, 8, 16, 32, 48, 64]))
        C = int(rs.choice([c for c in (16, 32, 48, 64, 96, 128) if c % cg == 0]))
        kh, kw = int(rs.randint(1, 4)), int(rs.randint(1, 4))
        stride, dil, pad = int(rs.randint(1, 4)), int(rs.randint(1, 3)), int(rs.randint(0, 3))
        B, H, W = int(rs.randint(1, 4)), int(rs.randint(3, 15)), int(rs.randint(3, 15))
        Ho, Wo = out_size(H, W, kh, kw, stride, pad, dil)
        if Ho <= 0 or Wo <= 0:
            continue
        geo = (B, H, W, C, C // cg, kh, kw, stride, pad, dil)
        try:
            run_gconv(*geo, use_bias=bool(rs.randint(2)), relu=bool(rs.randint(2)), gen=gen)
        except AssertionError as e:
            raise AssertionError('geometry (B, H, W, C, groups, kh, kw, stride, pad, dil) = %r: %s' % (geo, e))
        done += 1
