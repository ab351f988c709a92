"""Plain tensor formulation of the two sampling halves of the deformable convolution (csrc/dcn.hip): the reference
tests/test_gpu_dcn_ops.py holds the kernels to.  No HIP and no C ABI in here; the adjoint (col2im) is autograd of the forward
(im2col), which is written with `gather`.  tests/test_dcn_ref.py pins it to the C oracle, to the oracle's own autograd
restatement and to torch.autograd.gradcheck, so the reference cannot drift with the code under test.

Every function computes in the dtype of its inputs (the tests pass float64) and on their device.  Layouts are the kernels' own:

    x        [B, H, W, C]
    offset   [M, dg * taps * 2]     M = B * Ho * Wo, (dy, dx) pairs, deformable group major, then tap
    mask     [M, dg * taps]         or None (DCN v1)
    columns  [M, taps, C]

Sampling rule (mmcv's deformable_im2col): a sample at (h, w) is zero outside the open interval (-1, H) x (-1, W); inside it,
each of the four bilinear corners that lies outside the map contributes zero.

Besides the values, the *_terms functions return what a rounding-error bound needs: A, the same sum with every term replaced
by its absolute value, and n, the number of terms of the sum."""
import torch


def out_size(H, W, kh, kw, stride, pad, dil):
    return (H + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1, (W + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1


class Samples:
    """Sampling points of every (output pixel, deformable group, tap), each field [M, dg, taps]:
    h, w      position; inside   the (-1, H) x (-1, W) test
    ok[i], idx[i], wt[i]         of corner i in (top-left, top-right, bottom-left, bottom-right): lies in the map (and the
                                 sample is inside), row of x.reshape(B*H*W, C) it reads (clamped where not ok), bilinear weight"""


def sample_points(offset, B, H, W, kh, kw, stride, pad, dil, dg):
    Ho, Wo = out_size(H, W, kh, kw, stride, pad, dil)
    taps, M = kh * kw, B * Ho * Wo
    dt, dev = offset.dtype, offset.device
    off = offset.reshape(M, dg, taps, 2)
    ar = lambda n: torch.arange(n, dtype=dt, device=dev)
    oy = (ar(Ho) * stride - pad).view(1, Ho, 1).expand(B, Ho, Wo).reshape(M, 1, 1)
    ox = (ar(Wo) * stride - pad).view(1, 1, Wo).expand(B, Ho, Wo).reshape(M, 1, 1)
    ky = (ar(kh) * dil).repeat_interleave(kw).view(1, 1, taps)
    kx = (ar(kw) * dil).repeat(kh).view(1, 1, taps)
    img = torch.arange(B, device=dev).view(B, 1).expand(B, Ho * Wo).reshape(M, 1, 1) * (H * W)
    s = Samples()
    s.h, s.w = oy + ky + off[..., 0], ox + kx + off[..., 1]
    s.inside = (s.h > -1) & (s.w > -1) & (s.h < H) & (s.w < W)
    h0, w0 = torch.floor(s.h), torch.floor(s.w)
    lh, lw = s.h - h0, s.w - w0
    s.ok, s.idx, s.wt = [], [], []
    for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        yy, xx = h0.detach() + dy, w0.detach() + dx
        s.ok.append(s.inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1))
        s.idx.append((yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long() + img)
        s.wt.append(wt)
    return s


def per_channel(t, cpg):
    """[M, dg, taps] -> [M, taps, C]: every channel gets the value of its deformable group."""
    return t.permute(0, 2, 1).repeat_interleave(cpg, dim=2)


def group_sum(t, dg):
    """[M, taps, C] -> [M, dg, taps]: sum over the channels of each deformable group."""
    M, taps, C = t.shape
    return t.reshape(M, taps, dg, C // dg).sum(3).permute(0, 2, 1)


def corners(x, s, dg):
    """The four corner values [M, taps, C] (zero where the corner does not count) and their weights [M, taps, C]."""
    C = x.shape[-1]
    flat = x.reshape(-1, C)
    vals, wts = [], []
    for ok, idx, wt in zip(s.ok, s.idx, s.wt):
        gi = per_channel(idx, C // dg)
        v = torch.gather(flat, 0, gi.reshape(-1, C)).reshape(gi.shape)
        vals.append(v * per_channel(ok, C // dg).to(x.dtype))
        wts.append(per_channel(wt, C // dg))
    return vals, wts


def im2col(x, offset, mask, kh, kw, stride, pad, dil, deform_groups=1):
    """-> columns [M, taps, C]."""
    B, H, W, C = x.shape
    s = sample_points(offset, B, H, W, kh, kw, stride, pad, dil, deform_groups)
    vals, wts = corners(x, s, deform_groups)
    col = sum(w * v for w, v in zip(wts, vals))
    if mask is not None:
        col = col * per_channel(mask.reshape(-1, deform_groups, kh * kw), C // deform_groups)
    return col


def im2col_terms(x, offset, mask, kh, kw, stride, pad, dil, deform_groups=1):
    """-> A [M, taps, C], n: the column sums over |terms| (bilinear weights are >= 0) and their 4 terms."""
    with torch.no_grad():
        return im2col(x.abs(), offset, None if mask is None else mask.abs(), kh, kw, stride, pad, dil, deform_groups), 4


def col2im(x, offset, mask, gcol, kh, kw, stride, pad, dil, deform_groups=1):
    """Adjoint of im2col at gradient columns gcol [M, taps, C] -> gx, goffset, gmask (None without a mask), by autograd.
    The offset gradient at an integer position is the one-sided derivative towards +inf (floor), as in the kernels."""
    leaves = [t.detach().clone().requires_grad_() for t in (x, offset) + (() if mask is None else (mask,))]
    cols = im2col(leaves[0], leaves[1], leaves[2] if mask is not None else None, kh, kw, stride, pad, dil, deform_groups)
    grads = torch.autograd.grad((cols * gcol).sum(), leaves)
    return grads[0], grads[1], (grads[2] if mask is not None else None)


def col2im_terms(x, offset, mask, gcol, kh, kw, stride, pad, dil, deform_groups=1):
    """Bound terms of the three gradients, a dict:
    A_gx [B, H, W, C]        sum over the corners landing on the element of |gcol| * |mask| * weight
    n_gx [B, H, W, C]        how many corners land there
    A_goffset [M, dg*taps*2] sum over the group's channels of |gcol| |mask| (hw (|v3| + |v1|) + lw (|v4| + |v2|)) for dy,
                             (hh (|v2| + |v1|) + lh (|v4| + |v3|)) for dx
    A_gmask [M, dg*taps]     sum over the group's channels of |gcol| * sum_i weight_i |v_i|
    n_c                      channels per deformable group: the terms of the last two"""
    B, H, W, C = x.shape
    dg, taps = deform_groups, kh * kw
    cpg = C // dg
    amask = None if mask is None else mask.abs()
    xa = x.detach().abs().clone().requires_grad_()
    A_gx, = torch.autograd.grad((im2col(xa, offset, amask, kh, kw, stride, pad, dil, dg) * gcol.abs()).sum(), [xa])
    with torch.no_grad():
        s = sample_points(offset, B, H, W, kh, kw, stride, pad, dil, dg)
        cnt = torch.zeros(B * H * W, dg, dtype=x.dtype, device=x.device)
        for ok, idx in zip(s.ok, s.idx):
            for g in range(dg):
                cnt[:, g].index_add_(0, idx[:, g].reshape(-1), ok[:, g].reshape(-1).to(x.dtype))
        n_gx = cnt.repeat_interleave(cpg, dim=1).reshape(B, H, W, C)
        (v1, v2, v3, v4), (w1, w2, w3, w4) = corners(x.abs(), s, dg)
        # hw = w1 + w3, lw = w2 + w4, hh = w1 + w2, lh = w3 + w4 (rows / columns of the weight square)
        ga = gcol.abs()
        gm = ga if amask is None else ga * per_channel(amask.reshape(-1, dg, taps), cpg)
        a_dy = group_sum(gm * ((w1 + w3) * (v3 + v1) + (w2 + w4) * (v4 + v2)), dg)
        a_dx = group_sum(gm * ((w1 + w2) * (v2 + v1) + (w3 + w4) * (v4 + v3)), dg)
        a_mk = group_sum(ga * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4), dg)
    return dict(A_gx=A_gx, n_gx=n_gx, A_goffset=torch.stack([a_dy, a_dx], 3).reshape(-1, dg * taps * 2),
                A_gmask=a_mk.reshape(-1, dg * taps), n_c=cpg)
