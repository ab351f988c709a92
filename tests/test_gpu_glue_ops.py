"""The small fused kernels of csrc/roi_ops.hip and the two coder kernels of csrc/box_ops.hip, each against its float64
reference in tests/glue_ref.py (pinned on the CPU by tests/test_glue_ref.py), over every kernel form and the edges of each.

Two kinds of check, so that no tolerance is tuned on the kernel.

EXACT: integer-valued inputs whose sums stay far below 2^24 are exact in fp32 in any order of summation, so the device result
must torch.equal the float64 one cast to fp32 (fuse_global backward in both forms, the average pool, BA fusion with one level,
SGD with dyadic constants, the flipped weight image, labels / weights / zeroed rows of the coders, the carried maxima, and the
run-to-run equality of the two workspace forms).

FLOAT: e = max |out - ref64| / max |ref64| per output tensor, held to  F x max(e_cpu, 2^-23),  F = max(8, sqrt(R)):  e_cpu is
the same formula evaluated by torch in fp32 on the CPU, R the longest run of terms one thread of the kernel adds sequentially
(a sequential fp32 sum of R terms loses about sqrt(R) ulp where ATen's blocked sums lose a few; FMA contraction moves single
results by an ulp; F = 8 covers runs up to 64 terms).  Every float check prints e, e_cpu, R and the bound before it asserts.

R, counted from the kernels (bound on centred data = F x max(e_cpu, 1.2e-7), i.e. >= 9.5e-7 at F = 8):
  GroupNorm forward (gn_fwd_kernel<49> for P <= 49, <0> above; y, mean, rstd): a thread adds the P positions of its channel,
      then log2(cpg) shuffles: R = P.  F = 8 up to P = 64, 9 / 9.8 / 10 / 11.3 at P = 80 / 96 / 100 / 128, 64.8 at P = 50 x 84.
  GroupNorm backward, thread per channel (gn_bwd_kernel<49> / <0>): P terms per thread; the parameter gradients then go
      through colsum_rows_kernel, ceil(n / 16) rows per thread and 16 partial sums: R = max(P, ceil(n / 16)).
  GroupNorm backward, tile form (gn_bwd_tile_kernel<PQ>): PQ <= 8 positions per thread, then ONE thread folds the Rr <= 256 row
      groups from LDS, then cpg / 4 <= 16 columns per group; colsum_rows_kernel as above.  gx also consumes the forward's mean
      and rstd (R = P), so every backward output is held to R = max(P, PQ, Rr, cpg / 4, ceil(n / 16)) = max(P, ceil(n / 16)).
  atomic htd_group_norm_relu_bwd: the n per-tile sums meet in float atomics in any order: R = max(P, n).
  fuse_global backward, workspace form: roi_tile_sums ceil(P / 4) positions per wave + 4, image_sums up to 64 RoIs of a chunk,
      chunk_sums ceil(n / 64) chunks: R = max(ceil(P / 4), min(n, 64), ceil(n / 64)) <= 64, F = 8.
  BA fusion: forward L <= 4 products; backward d[l] = ceil(P * C / 1024) float4 dot products per thread (<= 50 at 14 x 14 x 260),
      six shuffles, four waves: F = 8.
  average pool backward (one product), BN folds (forward one product; backward ceil(K / 1024) float4 dot products per thread,
      <= 3 at K = 2304), SGD (three products): F = 8.
The coder kernels are compiled without contraction and follow the reference's order of operations in fp32: they are held to
glue_ref evaluated in fp32 and to the recorded arrays of tests/golden/box_math.npz with the tolerances of
tests/test_oracle_golden.py::test_box_math (device expf / logf differ from the host's by ulps).

ReLU: where the pre-activation is within 1e-3 of zero the fp32 and fp64 activations may fall on different sides, and the
gradient there is discontinuous; the upstream gradient of the float cases is zero at those positions (and only there), so the
comparison never depends on the side.  Exact zeros under ReLU have their own test.

Which case selects which kernel (asserted by test_group_norm_cases_select_every_kernel_form for GroupNorm):
  gn_fwd_kernel<49>            every GroupNorm case with P <= 49 (blocks of 64 threads at C = 16 up to 1024 at C = 1024)
  gn_fwd_kernel<0>             C = 256 at P = 80, 96, 100, 128 and 50 x 84
  gn_bwd_tile_kernel<1>        C = 16 G = 4 P = 49 (V = 4, 49 row groups); C = 1024 G = 32 P = 3
  gn_bwd_tile_kernel<2>..<8>   C = 256 G = 32 (V = 64, 16 row groups) at P = 25, 48, 49, 80, 96, 100, 128;
                               <5> and <8> also C = 1024 (V = 256, 4 row groups) at P = 20 and 32; <7> also C = 576 G = 36 P = 49
  gn_bwd_kernel<49>            C = 64 G = 64 and G = 32 (1 and 2 channels per group) at P = 9, 49; C = 1024 G = 32 P = 49 (13
                               positions per thread, 1024-thread blocks)
  gn_bwd_kernel<0>             C = 256 G = 32 P = 50 x 84 (263 positions per thread)
  colsum_rows_kernel           every GroupNorm backward through the wrapper (n = 17 and 70 walk its row loop twice and more)
  roi_tile_sums / image_sums / chunk_sums    every fuse_global / plain_and_fused backward; n >= 65 has several chunks, C = 260 and
                               1024 take the second and further column passes
  fuse_global_bwd_kernel       htd_fuse_global_bwd_global at C = 6;  fuse_global_bwd_vec_kernel at C = 260
  ba_fuse_fwd / _bwd           L = 1..4, edge 0, 1, 2, 4, four tile sizes; grad_border through the ABI
  gap_fwd / gap_bwd            P around the 8-way unroll; acc = 1 with chain=True and a channels-last second consumer
  bn_fold_fwd / _bwd           K = 4, 216, 260, 2304 (the row loop wraps above 1024)
  bn_fold_many_fwd / _bwd      one and seven layers, Co / Ci off the 32 grid, with and without wT, a flip-only layer
  sgd_kernel                   n < 4 (tail only), n % 4 = 1, 2, 3, many blocks
  decode_clip / roi_targets    n around the 256-thread block, per-image limits, keep, negative and unused slots"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R

pytestmark = pytest.mark.gpu
D64 = torch.float64
CL = torch.channels_last


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture
def h2_state():
    """The H2 switch as the test found it, put back afterwards (tests/test_gpu_h2.py restores it the same way)."""
    from htd_amd import capi, dense
    L = capi.lib()
    before = L.htd_conv2d_set_h2(-1)
    yield L
    L.htd_conv2d_set_h2(before)
    dense.new_step()


def P_(t):
    from htd_amd import capi
    return capi.ptr(t)


def S_():
    from htd_amd import capi
    return capi.current_stream_ptr()


def call(name, *args):
    from htd_amd import capi
    capi.call(name, *args)


def rejected():
    from htd_amd import capi
    return pytest.raises((ValueError, capi.HtdError))


def to_dev(t, dev):
    """logical (n, C, h, w) on the host -> the same on the device in [n][h][w][C] memory, whatever the sizes"""
    return t.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)


def nhwc_empty(n, C, h, w, dev, fill=None):
    t = torch.empty(n, h, w, C, device=dev) if fill is None else torch.full((n, h, w, C), float(fill), device=dev)
    return t.permute(0, 3, 1, 2)


def ints(gen, *shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(D64)


def check_float(name, out, ref64, cpu32, run):
    e, e_cpu = R.rel_err(out, ref64), R.rel_err(cpu32, ref64)
    bound = R.float_bound(e_cpu, run)
    print(f'{name}: e_kernel {e:.3e}  e_cpu {e_cpu:.3e}  R {run}  bound {bound:.3e}')
    assert e <= bound, f'{name}: e_kernel {e:.3e} > bound {bound:.3e} (e_cpu {e_cpu:.3e}, R {run})'


def check_exact(name, out, ref64):
    ref = ref64.detach().to(torch.float32)
    out = out.detach().cpu()
    assert out.shape == ref.shape, (name, tuple(out.shape), tuple(ref.shape))
    assert torch.equal(out, ref), f'{name}: {int((out != ref).sum())} of {ref.numel()} differ, max |diff| {float((out - ref).abs().max()):.3e}'


def make_rois(gen, n, B, empty=None, shuffled=False):
    """(n, 5) RoIs over B images, image `empty` without any; grouped by image unless shuffled"""
    imgs = [b for b in range(B) if b != empty]
    idx = torch.tensor(imgs)[torch.randint(0, len(imgs), (n, ), generator=gen)] if n else torch.zeros(0, dtype=torch.int64)
    if not shuffled:
        idx = torch.sort(idx)[0]
    elif n >= 60 and len(imgs) > 1:
        assert bool((idx[1:] < idx[:-1]).any())
    return torch.cat([idx.to(D64).view(n, 1), torch.rand(n, 4, generator=gen, dtype=D64) * 100], 1)


# ====================================================================== GroupNorm (+ ReLU)
def gn_bwd_form(Pn, C, G):
    """The backward kernel launch_gn_bwd_tile / gn_bwd_ws_impl pick for this shape: ('tile', PQ, row groups) or ('chan', PREG)."""
    cpg = C // G
    if C % 4 or cpg % 4 or C // 4 > 256:
        return ('chan', 49 if Pn <= 49 else 0)
    V = C // 4
    Rr = min(1024 // V, Pn)
    PQ = -(-Pn // Rr)
    return ('tile', PQ, Rr) if PQ <= 8 else ('chan', 49 if Pn <= 49 else 0)


GN_SHAPES = [  # C, G, h, w
    (576, 36, 7, 7), (16, 4, 7, 7), (256, 32, 5, 5), (256, 32, 6, 8), (256, 32, 7, 7), (256, 32, 8, 10), (256, 32, 8, 12),
    (256, 32, 10, 10), (256, 32, 8, 16), (1024, 32, 1, 3), (1024, 16, 4, 5), (1024, 32, 4, 8), (64, 64, 3, 3), (64, 64, 7, 7),
    (64, 32, 3, 3), (64, 32, 7, 7), (1024, 32, 7, 7)]
GN_BIG = (256, 32, 50, 84)


def _gn_cases():
    cases = []
    for C, G, h, w in GN_SHAPES:
        for n in (0, 1, 3, 70 if 70 * C * h * w <= 2200000 else 17):
            cases.append((C, G, h, w, n, 'randn'))
    for C, G, h, w in [(576, 36, 7, 7), (64, 32, 7, 7), (256, 32, 8, 10)]:
        cases += [(C, G, h, w, 3, 'mean50'), (C, G, h, w, 3, 'const')]
    cases += [GN_BIG + (2, 'randn'), GN_BIG + (2, 'mean50')]
    return cases


GN_CASES = _gn_cases()


def test_group_norm_cases_select_every_kernel_form():
    """The case list above, put through the launcher's arithmetic: every gn_bwd_tile_kernel<1..8>, gn_bwd_kernel<49> and <0>,
    gn_fwd_kernel<49> and <0> is taken by at least one case, and htd_group_norm_bwd_amax_supported agrees on tile or not."""
    from htd_amd import capi
    L = capi.lib()
    forms, fwd = set(), set()
    for C, G, h, w, n, _ in GN_CASES:
        form = gn_bwd_form(h * w, C, G)
        assert (form[0] == 'tile') == bool(L.htd_group_norm_bwd_amax_supported(h * w, C, G)), (C, G, h, w, form)
        if n:
            forms.add(form[:2])
            fwd.add(49 if h * w <= 49 else 0)
    assert forms == {('tile', k) for k in range(1, 9)} | {('chan', 49), ('chan', 0)}, sorted(forms)
    assert fwd == {49, 0}
    assert gn_bwd_form(49, 576, 36) == ('tile', 7, 7) and gn_bwd_form(49, 1024, 32) == ('chan', 49)
    assert gn_bwd_form(4200, 256, 32) == ('chan', 0) and gn_bwd_form(9, 64, 32) == ('chan', 49)


@functools.lru_cache(maxsize=4)
def gn_reference(C, G, h, w, n, flavour, relu):
    """inputs (fp64), the fp64 forward and backward, and the same formula in fp32 by ATen on the CPU"""
    gen = torch.Generator().manual_seed(C * 131 + G * 17 + h * w + n)
    x = torch.randn(n, C, h, w, generator=gen, dtype=D64)
    if flavour == 'mean50':
        x = x + 50
    if flavour == 'const':                       # one (tile, group) without variance; 3 * (members of the group) is exact in fp32
        x[1, C // G:2 * (C // G)] = 3.0
    x = x.float().double()
    gamma, beta = (torch.randn(C, generator=gen).double() for _ in range(2))
    gy = torch.randn(n, C, h, w, generator=gen).double()
    if relu:
        pre = R.group_norm_relu(x, gamma, beta, G, 1e-5, False)[0]
        gy = gy * (pre.abs() > 1e-3)
    x64, g64, b64 = (t.clone().requires_grad_() for t in (x, gamma, beta))
    y64, m64, r64 = R.group_norm_relu(x64, g64, b64, G, 1e-5, relu)
    y64.backward(gy)
    x32, g32, b32 = (t.float().requires_grad_() for t in (x, gamma, beta))
    y32, m32, r32 = torch.native_group_norm(x32, g32, b32, n, C, h * w, G, 1e-5)
    y32 = F.relu(y32) if relu else y32
    y32.backward(gy.float())
    ref = dict(y=y64.detach(), mean=m64.detach(), rstd=r64.detach(), gx=x64.grad, ggamma=g64.grad, gbeta=b64.grad)
    cpu = dict(y=y32.detach(), mean=m32.detach().view(n, G), rstd=r32.detach().view(n, G), gx=x32.grad, ggamma=g32.grad, gbeta=b32.grad)
    return x, gamma, beta, gy, ref, cpu


def gn_runs(C, G, h, w, n):
    Pn = h * w
    return Pn, max(Pn, -(-n // 16))


@pytest.mark.parametrize('h2', [0, 1])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('C,G,h,w,n,flavour', GN_CASES)
def test_group_norm_relu(dev, h2_state, C, G, h, w, n, flavour, relu, h2):
    """mmcv_ops.group_norm_relu forward and backward.  The shape selects the kernels (gn_bwd_form, the module docstring's table):
    P <= 49 -> gn_fwd_kernel<49>, else <0>; 4 | channels per group and ceil(P / min(4096 / C, P)) <= 8 -> gn_bwd_tile_kernel<that>,
    else gn_bwd_kernel<49> / <0>.  n = 0, 1, 3 and 70 tiles (17 where 70 would exceed the largest map, 2 x 256 x 50 x 84).  H2 on: htd_group_norm_relu_fwd_amax and, for tile shapes, _bwd_amax; off: _fwd and _bwd_ws.
    n = 0 launches nothing and returns zero parameter gradients."""
    from htd_amd import dense
    from htd_amd import mmcv_ops as M
    h2_state.htd_conv2d_set_h2(h2)
    dense.new_step()
    x, gamma, beta, gy, ref, cpu = gn_reference(C, G, h, w, n, flavour, relu)
    xd = to_dev(x.float(), dev).requires_grad_()
    gd, bd = gamma.float().to(dev).requires_grad_(), beta.float().to(dev).requires_grad_()
    out = M.group_norm_relu(xd, gd, bd, G, 1e-5, relu)
    saved = out.grad_fn.saved_tensors
    if h2 and n:
        am = dense.carried_amax(out)
        assert am is not None and float(am) == float(out.detach().abs().max())
    out.backward(to_dev(gy.float(), dev))
    r_fwd, r_bwd = gn_runs(C, G, h, w, n)
    tag = f'GN C{C} G{G} {h}x{w} n{n} {flavour} relu{int(relu)} h2{h2} {gn_bwd_form(h * w, C, G)}'
    check_float(tag + ' y', out, ref['y'], cpu['y'], r_fwd)
    if n:
        check_float(tag + ' mean', saved[3], ref['mean'], cpu['mean'], r_fwd)
        check_float(tag + ' rstd', saved[4], ref['rstd'], cpu['rstd'], r_fwd)
    check_float(tag + ' gx', xd.grad, ref['gx'], cpu['gx'], r_bwd)
    check_float(tag + ' ggamma', gd.grad, ref['ggamma'], cpu['ggamma'], r_bwd)
    check_float(tag + ' gbeta', bd.grad, ref['gbeta'], cpu['gbeta'], r_bwd)
    if flavour == 'const':
        assert float(saved[4][1, 1]) == pytest.approx(1e-5 ** -0.5, rel=1e-6)      # rstd of the tile without variance: eps^-1/2


def gn_abi_fwd(x, gamma, beta, G, relu, slot=None):
    n, C, h, w = x.shape
    y = nhwc_empty(n, C, h, w, x.device)
    mean, rstd = torch.empty(n, G, device=x.device), torch.empty(n, G, device=x.device)
    if slot is None:
        call('htd_group_norm_relu_fwd', P_(x), P_(gamma), P_(beta), P_(y), P_(mean), P_(rstd), n, h * w, C, G, 1e-5, int(relu), S_())
    else:
        call('htd_group_norm_relu_fwd_amax', P_(x), P_(gamma), P_(beta), P_(y), P_(mean), P_(rstd), n, h * w, C, G, 1e-5, int(relu),
             P_(slot), S_())
    return y, mean, rstd


def gn_abi_bwd(entry, x, y, gamma, mean, rstd, gy, G, relu, slot=None, poison=None):
    n, C, h, w = x.shape
    gx = nhwc_empty(n, C, h, w, x.device)
    if entry == 'htd_group_norm_relu_bwd':                 # float atomics: the sums are ADDED to what the buffers hold
        gg, gb = torch.zeros(C, device=x.device), torch.zeros(C, device=x.device)
        call(entry, P_(x), P_(y), P_(gamma), P_(mean), P_(rstd), P_(gy), P_(gx), P_(gg), P_(gb), n, h * w, C, G, int(relu), S_())
        return gx, gg, gb
    gg, gb = (torch.full((C, ), float('nan') if poison is None else poison, device=x.device) for _ in range(2))    # overwritten
    ws = torch.empty(2 * max(n, 1) * C, device=x.device)
    args = (P_(x), P_(y), P_(gamma), P_(mean), P_(rstd), P_(gy), P_(gx), P_(gg), P_(gb), n, h * w, C, G, int(relu), P_(ws))
    if slot is None:
        call('htd_group_norm_relu_bwd_ws', *args, S_())
    else:
        call('htd_group_norm_relu_bwd_amax', *args, P_(slot), S_())
    return gx, gg, gb


@pytest.mark.parametrize('C,G,h,w,n', [(576, 36, 7, 7, 21), (256, 32, 5, 5, 40), (64, 32, 3, 3, 33), (64, 64, 7, 7, 5), (1024, 32, 7, 7, 3),
                                       (256, 32, 50, 84, 2)])
def test_group_norm_atomic_backward_through_the_abi(dev, C, G, h, w, n):
    """htd_group_norm_relu_bwd (no caller in the package): the same kernels with partial == NULL, the per-tile sums of gamma and
    beta added by float atomics into zeroed buffers.  (576, 36, 49) and (256, 32, 25) take gn_bwd_tile_kernel<7> / <2>, C = 64 and
    (1024, 32, 49) gn_bwd_kernel<49>, 50 x 84 gn_bwd_kernel<0>."""
    x, gamma, beta, gy, ref, cpu = gn_reference(C, G, h, w, n, 'randn', True)
    xd, gyd = to_dev(x.float(), dev), to_dev(gy.float(), dev)
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    y, mean, rstd = gn_abi_fwd(xd, gd, bd, G, True)
    gx, gg, gb = gn_abi_bwd('htd_group_norm_relu_bwd', xd, y, gd, mean, rstd, gyd, G, True)
    run = max(h * w, n)
    tag = f'GN atomic C{C} G{G} {h}x{w} n{n} {gn_bwd_form(h * w, C, G)}'
    check_float(tag + ' gx', gx, ref['gx'], cpu['gx'], run)
    check_float(tag + ' ggamma', gg, ref['ggamma'], cpu['ggamma'], run)
    check_float(tag + ' gbeta', gb, ref['gbeta'], cpu['gbeta'], run)


@pytest.mark.parametrize('C,G,h,w,n', [(576, 36, 7, 7, 21), (256, 32, 8, 16, 9), (64, 32, 7, 7, 33), (256, 32, 50, 84, 2)])
def test_group_norm_workspace_backward_is_bit_reproducible(dev, C, G, h, w, n):
    """htd_group_norm_relu_bwd_ws twice on the same float inputs: gx, ggamma and gbeta bit for bit (tile <7>, tile <8>,
    gn_bwd_kernel<49>, gn_bwd_kernel<0>; all through colsum_rows_kernel), whatever the buffers held before."""
    x, gamma, beta, gy, ref, cpu = gn_reference(C, G, h, w, n, 'randn', True)
    xd, gyd = to_dev(x.float(), dev), to_dev(gy.float(), dev)
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    y, mean, rstd = gn_abi_fwd(xd, gd, bd, G, True)
    a = gn_abi_bwd('ws', xd, y, gd, mean, rstd, gyd, G, True, poison=float('nan'))
    b = gn_abi_bwd('ws', xd, y, gd, mean, rstd, gyd, G, True, poison=7.0)
    for name, s, t in zip(('gx', 'ggamma', 'gbeta'), a, b):
        assert torch.equal(s, t), name
        assert bool(torch.isfinite(s).all()), name


@pytest.mark.parametrize('C,G,h,w,n', [(576, 36, 7, 7, 5), (256, 32, 5, 5, 3), (64, 64, 3, 3, 4), (1024, 32, 7, 7, 2), (256, 32, 50, 84, 1)])
def test_group_norm_maxima(dev, C, G, h, w, n):
    """The maximum _fwd_amax / _bwd_amax leave for an H2 convolution: bit for bit max |tensor stored| (the outputs themselves equal
    the plain entry points'), a larger value already in the slot survives, a NaN in the output leaves a NaN.  The backward leaves
    one for the tile shapes only (the first two); for the others htd_group_norm_relu_bwd_amax refuses before any launch."""
    x, gamma, beta, gy, _, _ = gn_reference(C, G, h, w, n, 'randn', True)
    xd, gyd = to_dev(x.float() * 3, dev), to_dev(gy.float(), dev)
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    y0, mean, rstd = gn_abi_fwd(xd, gd, bd, G, True)
    slot = torch.zeros(1, device=dev)
    y1, m1, r1 = gn_abi_fwd(xd, gd, bd, G, True, slot)
    assert torch.equal(y0, y1) and torch.equal(mean, m1) and torch.equal(rstd, r1)
    assert float(slot) == float(y1.abs().max()) and float(slot) > 0
    slot.fill_(1e30)
    gn_abi_fwd(xd, gd, bd, G, True, slot)
    assert float(slot) == float(torch.tensor(1e30))
    xn = xd.clone()
    xn[n - 1, C - 1, h - 1, w - 1] = float('nan')
    slot.zero_()
    yn = gn_abi_fwd(xn, gd, bd, G, False, slot)[0]
    assert bool(torch.isnan(yn).any()) and bool(torch.isnan(slot).item())
    from htd_amd import capi
    if capi.lib().htd_group_norm_bwd_amax_supported(h * w, C, G):
        g0 = gn_abi_bwd('ws', xd, y0, gd, mean, rstd, gyd, G, True)
        slot.zero_()
        g1 = gn_abi_bwd('amax', xd, y0, gd, mean, rstd, gyd, G, True, slot)
        assert all(torch.equal(s, t) for s, t in zip(g0, g1))
        assert float(slot) == float(g1[0].abs().max()) and float(slot) > 0
        slot.fill_(1e30)
        gn_abi_bwd('amax', xd, y0, gd, mean, rstd, gyd, G, True, slot)
        assert float(slot) == float(torch.tensor(1e30))
        gn_ = gyd.clone()
        gn_[0, 0, 0, 0] = float('nan')
        slot.zero_()
        gxn = gn_abi_bwd('amax', xd, y0, gd, mean, rstd, gn_, G, False, slot)[0]
        assert bool(torch.isnan(gxn).any()) and bool(torch.isnan(slot).item())
    else:
        assert gn_bwd_form(h * w, C, G)[0] == 'chan'
        with rejected():
            gn_abi_bwd('amax', xd, y0, gd, mean, rstd, gyd, G, True, slot)


def test_group_norm_exact_zeros_under_relu_pass_no_gradient(dev):
    """Channels whose activation is exactly 0: gamma = beta = 0 (pre-activation 0, the `!(y > 0)` edge) and gamma = 0, beta = -1
    (clamped).  Their gamma and beta gradients must be exactly 0, as torch's ReLU has it, in the tile form (C = 256, <4>) and in
    gn_bwd_kernel<49> (C = 64, two channels per group)."""
    from htd_amd import mmcv_ops as M
    for C, G in ((256, 32), (64, 32)):
        gen = torch.Generator().manual_seed(C)
        x = torch.randn(5, C, 7, 7, generator=gen)
        gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        gamma[[3, 10]] = 0.0
        beta[3], beta[10] = 0.0, -1.0
        gy = torch.randn(5, C, 7, 7, generator=gen)
        x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
        y64 = R.group_norm_relu(x64, g64, b64, G, 1e-5, True)[0]
        y64.backward(gy.double())
        assert float(g64.grad[3]) == 0 and float(b64.grad[10]) == 0
        xd, gd, bd = to_dev(x, dev).requires_grad_(), gamma.to(dev).requires_grad_(), beta.to(dev).requires_grad_()
        out = M.group_norm_relu(xd, gd, bd, G, 1e-5, True)
        out.backward(to_dev(gy, dev))
        assert bool((out[:, [3, 10]] == 0).all())
        for c in (3, 10):
            assert float(gd.grad[c]) == 0.0 and float(bd.grad[c]) == 0.0, (C, c, float(gd.grad[c]), float(bd.grad[c]))
        assert float(gd.grad.abs().sum()) > 0


def test_group_norm_rejections(dev):
    """Refused by HTD_REQUIRE in gn_fwd_impl / gn_bwd_ws_impl before any launch: channels per group not a power of two (or above
    64), C > 1024, C not divisible by G."""
    from htd_amd import mmcv_ops as M
    for C, G in ((24, 4), (1152, 36), (20, 3), (256, 2)):
        x = to_dev(torch.randn(2, C, 3, 3), dev)
        with rejected():
            M.group_norm_relu(x, torch.ones(C, device=dev), torch.zeros(C, device=dev), G, 1e-5, True)


# ====================================================================== fuse_global / plain_and_fused
FUSE_CASES = [  # n, B, empty image, C, (h, w), shuffled
    (0, 3, 1, 256, (7, 7), False), (1, 1, None, 4, (1, 1), False), (1, 3, 1, 256, (7, 7), False), (1, 3, 0, 1024, (7, 7), False),
    (63, 3, 1, 256, (7, 7), False), (63, 5, 4, 1024, (1, 1), True), (64, 3, 1, 256, (7, 7), True), (64, 1, None, 4, (7, 7), False),
    (65, 5, 2, 260, (7, 7), True), (65, 3, 2, 256, (1, 1), False), (130, 5, 0, 260, (7, 7), False), (130, 3, 1, 1024, (1, 1), True),
    (3000, 1, None, 4, (7, 7), False), (3000, 5, 3, 4, (7, 7), True), (3000, 3, 1, 260, (1, 1), True)]


@pytest.mark.parametrize('n,B,empty,C,hw,shuffled', FUSE_CASES)
def test_fuse_global_and_plain_and_fused_exact(dev, n, B, empty, C, hw, shuffled):
    """mmcv_ops.fuse_global (with extra, alpha = 0.5) and plain_and_fused on integers in [-8, 8]: outputs and every gradient equal
    the float64 ones bit for bit.  The backward of the global feature is htd_fuse_global_bwd_global_ws: roi_tile_sums_kernel (one
    block per RoI; C / 4 > 64 at C = 260 and 1024 takes further column passes), image_sums_kernel (ceil(n / 64) chunks: one up to
    n = 64, two at 65, three at 130, 47 at 3000; an image without RoIs must come out zero; RoIs need not be grouped by image),
    chunk_sums_kernel.  The largest case adds 3000 x 49 terms of at most 8 into one image: < 1.2e6, exact in fp32."""
    from htd_amd import mmcv_ops as M
    h, w = hw
    gen = torch.Generator().manual_seed(n * 7 + C + B)
    x, e, go, go2 = ints(gen, n, C, h, w), ints(gen, n, C, h, w), ints(gen, n, C, h, w), ints(gen, 2 * n, C, h, w)
    g = ints(gen, B, C, 1, 1)
    rois = make_rois(gen, n, B, empty, shuffled)
    x64, e64, g64 = (t.clone().requires_grad_() for t in (x, e, g))
    ref = R.fuse_global(x64, rois, g64, e64, 0.5)
    ref.backward(go)
    xd, ed, gd = to_dev(x.float(), dev).requires_grad_(), to_dev(e.float(), dev).requires_grad_(), g.float().to(dev).requires_grad_()
    out = M.fuse_global(xd, rois.float().to(dev), gd, ed, 0.5)
    out.backward(to_dev(go.float(), dev))
    check_exact('fuse out', out, ref)
    check_exact('fuse gx', xd.grad, x64.grad)
    check_exact('fuse gextra', ed.grad, e64.grad)
    check_exact('fuse gglobal', gd.grad, g64.grad)
    if empty is not None and B > 1:
        assert float(gd.grad[empty].abs().sum()) == 0.0
    x64, g64 = (t.clone().requires_grad_() for t in (x, g))
    ref = R.plain_and_fused(x64, rois, g64)
    ref.backward(go2)
    xd, gd = to_dev(x.float(), dev).requires_grad_(), g.float().to(dev).requires_grad_()
    both = M.plain_and_fused(xd, rois.float().to(dev), gd)
    both.backward(to_dev(go2.float(), dev))
    check_exact('both', both, ref)
    check_exact('both gx', xd.grad, x64.grad)
    check_exact('both gglobal', gd.grad, g64.grad)


@pytest.mark.parametrize('n,B,C,hw', [(130, 3, 260, (7, 7)), (3000, 5, 4, (7, 7)), (65, 3, 1024, (1, 1))])
def test_fuse_global_workspace_backward_float_and_reproducible(dev, n, B, C, hw):
    """htd_fuse_global_bwd_global_ws on float gradients, RoIs not grouped by image: within the float bound (R <= 64: ceil(P / 4)
    positions per wave, 64 RoIs per chunk, ceil(n / 64) chunks) and bit-equal from run to run, whatever the output held."""
    h, w = hw
    gen = torch.Generator().manual_seed(n + C)
    go = torch.randn(n, C, h, w, generator=gen)
    rois = make_rois(gen, n, B, 1, True)
    img = rois[:, 0].long()
    ref = torch.zeros(B, C, dtype=D64).index_add_(0, img, go.double().sum((2, 3)))
    cpu = torch.zeros(B, C).index_add_(0, img, go.sum((2, 3)))
    god, rd = to_dev(go, dev), rois.float().to(dev)
    outs = []
    for fill in (float('nan'), 3.0):
        gg = torch.full((B, C), fill, device=dev)
        ws = torch.empty((n + (n + 63) // 64 * B) * C, device=dev)
        call('htd_fuse_global_bwd_global_ws', P_(god), P_(rd), P_(gg), n, h * w, C, B, P_(ws), S_())
        outs.append(gg)
    assert torch.equal(outs[0], outs[1])
    check_float(f'fuse ws n{n} C{C} P{h * w}', outs[0], ref, cpu, max(-(-h * w // 4), min(n, 64), -(-n // 64)))
    assert float(outs[0][1].abs().sum()) == 0.0


@pytest.mark.parametrize('grouped', [True, False])
@pytest.mark.parametrize('n,C', [(65, 6), (130, 6), (65, 260), (130, 260), (3, 260)])
def test_fuse_global_atomic_backward_through_the_abi(dev, n, C, grouped):
    """htd_fuse_global_bwd_global (the Python backward always takes the workspace form): C = 6 -> fuse_global_bwd_kernel (scalar,
    16 RoIs per block), C = 260 -> fuse_global_bwd_vec_kernel (float4, 4 RoIs per block, 65 float4 columns: the 65th lane group
    is a second grid row).  It ADDS into grad_global; on a zeroed output and integers in [-8, 8] the result is exact in any order
    of the atomics."""
    B, h, w = 3, 7, 7
    gen = torch.Generator().manual_seed(n + C)
    go = ints(gen, n, C, h, w)
    rois = make_rois(gen, n, B, 1, not grouped)
    ref = torch.zeros(B, C, dtype=D64).index_add_(0, rois[:, 0].long(), go.sum((2, 3)))
    gg = torch.zeros(B, C, device=dev)
    god, rd = to_dev(go.float(), dev), rois.float().to(dev)          # named: operands stay alive until the launch is queued
    call('htd_fuse_global_bwd_global', P_(god), P_(rd), P_(gg), n, h * w, C, B, S_())
    check_exact('fuse atomic', gg, ref)
    call('htd_fuse_global_bwd_global', P_(god), P_(rd), P_(gg), n, h * w, C, B, S_())
    check_exact('fuse atomic, added twice', gg, 2 * ref)


def test_fuse_global_rejections(dev):
    """C % 4 != 0 is refused by fuse_global_fwd_impl / plain_and_fused_impl / the _ws backward before any launch."""
    from htd_amd import mmcv_ops as M
    x = to_dev(torch.randn(3, 6, 7, 7), dev)
    rois = torch.zeros(3, 5, device=dev)
    g = torch.randn(1, 6, 1, 1, device=dev)
    with rejected():
        M.fuse_global(x, rois, g)
    with rejected():
        M.plain_and_fused(x, rois, g)
    with rejected():
        call('htd_fuse_global_bwd_global_ws', P_(x), P_(rois), P_(torch.zeros(1, 6, device=dev)), 3, 49, 6, 1, P_(torch.zeros(64, device=dev)), S_())


# ====================================================================== BA fusion
BA_TILES = [(1, 1), (7, 7), (14, 14), (5, 9)]


@pytest.mark.parametrize('edge', [0, 1, 2, 4])
@pytest.mark.parametrize('hw', BA_TILES)
@pytest.mark.parametrize('n,C', [(0, 256), (1, 4), (19, 4), (1, 260), (19, 256), (19, 260)])
def test_ba_fuse_one_level_exact(dev, n, C, hw, edge):
    """mmcv_ops.ba_fuse with L = 1: the softmax weight is exactly 1, so out = x + x on the ring and, backward, grad = g + g on the
    ring and a zero attention gradient (the backward folds four slots whatever L is: three stay zero).  The ring is the
    reference's slice: the whole tile at edge = 0 and at edge >= half the tile (1 x 1 with any edge, 7 x 7 and 5 x 9 at edge 4)."""
    from htd_amd import mmcv_ops as M
    h, w = hw
    gen = torch.Generator().manual_seed(n + C + h)
    x, go = ints(gen, n, C, h, w), ints(gen, n, C, h, w)
    att = torch.randn(1, n, generator=gen).double()
    x64, a64 = x.clone().requires_grad_(), att.clone().requires_grad_()
    ref = R.ba_fuse(a64, [x64], x64, edge)
    ref.backward(go)
    xd, ad = to_dev(x.float(), dev).requires_grad_(), att.float().to(dev).requires_grad_()
    out = M.ba_fuse(ad, [xd], edge)
    out.backward(to_dev(go.float(), dev))
    check_exact('ba out', out, ref)
    check_exact('ba gx', xd.grad, x64.grad)
    assert ad.grad.shape == (1, n) and float(ad.grad.abs().sum()) == 0.0


def ba_inputs(gen, L, n, C, h, w):
    lv = [torch.randn(n, C, h, w, generator=gen).double() for _ in range(L)]
    att = torch.randn(L, n, generator=gen).double()
    if n > 6:
        att[:, 6:] = (torch.rand(L, n - 6, generator=gen).double() * 2 - 1) * 80        # saturated: spread over +-80
    go = torch.randn(n, C, h, w, generator=gen).double()
    return lv, att.float().double(), go


def ba_run_len(h, w, C):
    return max(4, -(-h * w * (C // 4) // 256))


@pytest.mark.parametrize('edge', [0, 1, 2, 4])
@pytest.mark.parametrize('L,n,C,hw', [(2, 19, 256, (7, 7)), (3, 19, 260, (7, 7)), (4, 19, 256, (7, 7)), (4, 1, 4, (1, 1)), (2, 19, 4, (14, 14)),
                                      (3, 19, 256, (5, 9)), (4, 19, 260, (14, 14)), (4, 0, 256, (7, 7)), (3, 1, 260, (5, 9))])
def test_ba_fuse_float(dev, L, n, C, hw, edge):
    """mmcv_ops.ba_fuse with 2 to 4 levels, the first six RoIs with logits of unit spread and the rest spread over +-80 (the
    softmax runs on __expf): output, level gradients (level 0 carries the ring's share) and attention gradient within the float
    bound.  Forward: L products per element; backward: ceil(P * C / 1024) float4 dot products per thread, then the wave."""
    from htd_amd import mmcv_ops as M
    h, w = hw
    gen = torch.Generator().manual_seed(L * 100 + n + C + h + edge)
    lv, att, go = ba_inputs(gen, L, n, C, h, w)
    l64, a64 = [t.clone().requires_grad_() for t in lv], att.clone().requires_grad_()
    ref = R.ba_fuse(a64, l64, l64[0], edge)
    ref.backward(go)
    l32, a32 = [t.float().requires_grad_() for t in lv], att.float().requires_grad_()
    cpu = R.ba_fuse(a32, l32, l32[0], edge)
    cpu.backward(go.float())
    ld, ad = [to_dev(t.float(), dev).requires_grad_() for t in lv], att.float().to(dev).requires_grad_()
    out = M.ba_fuse(ad, ld, edge)
    out.backward(to_dev(go.float(), dev))
    tag = f'BA L{L} n{n} C{C} {h}x{w} edge{edge}'
    check_float(tag + ' out', out, ref, cpu, L)
    for l in range(L):
        check_float(tag + f' glvl{l}', ld[l].grad, l64[l].grad, l32[l].grad, L)
    check_float(tag + ' gatt', ad.grad, a64.grad, a32.grad, ba_run_len(h, w, C))


@pytest.mark.parametrize('edge,hw', [(0, (7, 7)), (1, (7, 7)), (2, (5, 9))])
def test_ba_fuse_separate_border_through_the_abi(dev, edge, hw):
    """htd_ba_fuse_fwd / _bwd with the operands only the ABI has: a `border` map that is not lvl[0], and its gradient in a
    grad_border output (the ring's share of g, zero inside) instead of added into grad_lvl[0]."""
    h, w = hw
    L, n, C = 4, 19, 256
    gen = torch.Generator().manual_seed(edge + h)
    lv, att, go = ba_inputs(gen, L, n, C, h, w)
    border = torch.randn(n, C, h, w, generator=gen).double()
    l64, a64, b64 = [t.clone().requires_grad_() for t in lv], att.clone().requires_grad_(), border.clone().requires_grad_()
    ref = R.ba_fuse(a64, l64, b64, edge)
    ref.backward(go)
    l32, a32, b32 = [t.float().requires_grad_() for t in lv], att.float().requires_grad_(), border.float().requires_grad_()
    cpu = R.ba_fuse(a32, l32, b32, edge)
    cpu.backward(go.float())
    import ctypes
    ld = [to_dev(t.float(), dev) for t in lv]
    bd, ad, god = to_dev(border.float(), dev), att.float().to(dev), to_dev(go.float(), dev)
    out = nhwc_empty(n, C, h, w, dev)
    arr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in ld])
    call('htd_ba_fuse_fwd', arr, L, P_(bd), P_(ad), P_(out), n, h, w, C, edge, S_())
    glv = [nhwc_empty(n, C, h, w, dev) for _ in range(L)]
    gborder, gatt = nhwc_empty(n, C, h, w, dev), torch.empty(L, n, device=dev)
    garr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in glv])
    call('htd_ba_fuse_bwd', arr, L, P_(ad), P_(god), garr, P_(gborder), P_(gatt), n, h, w, C, edge, S_())
    tag = f'BA abi {h}x{w} edge{edge}'
    check_float(tag + ' out', out, ref, cpu, L)
    for l in range(L):
        check_float(tag + f' glvl{l}', glv[l], l64[l].grad, l32[l].grad, L)
    check_float(tag + ' gatt', gatt, a64.grad, a32.grad, ba_run_len(h, w, C))
    check_exact(tag + ' gborder', gborder, b64.grad.float().double())          # a masked copy of g


def test_ba_fuse_rejections(dev):
    """L = 5 and C % 4 != 0 are refused by htd_ba_fuse_fwd before any launch."""
    from htd_amd import mmcv_ops as M
    att = torch.zeros(5, 2, device=dev)
    with rejected():
        M.ba_fuse(att, [to_dev(torch.randn(2, 8, 7, 7), dev) for _ in range(5)], 1)
    with rejected():
        M.ba_fuse(att[:2], [to_dev(torch.randn(2, 6, 7, 7), dev) for _ in range(2)], 1)


# ====================================================================== global average pool
GAP_TILES = [(1, 1), (1, 7), (2, 4), (3, 3), (3, 5), (4, 4), (1, 17), (7, 7), (14, 14)]          # P = 1, 7, 8, 9, 15, 16, 17, 49, 196


@pytest.mark.parametrize('hw', GAP_TILES)
@pytest.mark.parametrize('n,C', [(0, 256), (1, 4), (21, 4), (1, 260), (21, 256), (21, 260), (1, 576), (21, 6)])
def test_global_avg_pool(dev, n, C, hw):
    """mmcv_ops.global_avg_pool on integers: gap_fwd_kernel's sum is exact and its one division correctly rounded, so the forward
    is exact for every P (full 8-way groups and the tail: P = 1, 7, 8, 9, 15, 16, 17, 49, 196).  gap_bwd_kernel multiplies by
    1 / P: exact for P a power of two, one product within the float bound otherwise.  C = 6: the forward kernel takes any C, the
    backward is tensor arithmetic (the float4 kernels need C % 4 == 0)."""
    from htd_amd import mmcv_ops as M
    h, w = hw
    Pn = h * w
    gen = torch.Generator().manual_seed(n + C + Pn)
    x, go = ints(gen, n, C, h, w), ints(gen, n, C, 1, 1)
    x64 = x.clone().requires_grad_()
    ref = R.global_avg_pool(x64)
    ref.backward(go)
    xd = to_dev(x.float(), dev).requires_grad_()
    out = M.global_avg_pool(xd)
    out.backward(go.float().to(dev))
    check_exact('gap out', out, ref)
    if Pn & (Pn - 1) == 0:
        check_exact('gap gx', xd.grad, x64.grad)
    else:
        cpu = (go.float() / Pn).expand(n, C, h, w)
        check_float(f'gap gx n{n} C{C} P{Pn}', xd.grad, x64.grad, cpu, 1)


@pytest.mark.parametrize('consumer', ['channels_last', 'none', 'contiguous'])
@pytest.mark.parametrize('n,C,hw', [(21, 256, (4, 4)), (21, 260, (7, 7)), (1, 4, (1, 1)), (0, 256, (7, 7)), (21, 6, (4, 4)), (3, 576, (3, 5))])
def test_global_avg_pool_chain(dev, n, C, hw, consumer):
    """chain=True (the path the BA extractor trains on): the node also returns an alias of x, and a second consumer's gradient of
    that alias is handed to this node, which adds g / P into it in place with htd_global_avg_pool_bwd_acc (gap_bwd_kernel, acc = 1)
    when it is channels-last; a gradient in another layout is copied into a channels-last map first, none takes the plain kernel.
    Integers: exact at
    P a power of two, within the float bound otherwise."""
    from htd_amd import mmcv_ops as M
    h, w = hw
    Pn = h * w
    gen = torch.Generator().manual_seed(n + C + Pn)
    x, go, w2 = ints(gen, n, C, h, w), ints(gen, n, C, 1, 1), ints(gen, n, C, h, w)
    x64 = x.clone().requires_grad_()
    loss = (R.global_avg_pool(x64) * go).sum()
    if consumer != 'none':
        loss = loss + (x64 * w2).sum()
    loss.backward()
    xd = to_dev(x.float(), dev).requires_grad_()
    pooled, alias = M.global_avg_pool(xd, chain=True)
    assert alias.shape == xd.shape and alias.data_ptr() == xd.data_ptr()
    lossd = (pooled * go.float().to(dev)).sum()
    if consumer == 'channels_last':
        lossd = lossd + (alias * to_dev(w2.float(), dev)).sum()
    elif consumer == 'contiguous':
        lossd = lossd + (alias * w2.float().to(dev).contiguous()).sum()
    lossd.backward()
    check_exact('gap chain out', pooled, R.global_avg_pool(x))
    if Pn & (Pn - 1) == 0:
        check_exact('gap chain gx', xd.grad, x64.grad)
    else:
        cpu = (go.float() / Pn).expand(n, C, h, w) + (w2.float() if consumer != 'none' else 0)
        check_float(f'gap chain gx n{n} C{C} P{Pn} {consumer}', xd.grad, x64.grad, cpu, 2)


# ====================================================================== frozen-BN folds
def bn_params(gen, Co):
    gamma, beta, mean = (torch.randn(Co, generator=gen).double() for _ in range(3))
    var = (torch.rand(Co, generator=gen) + 0.1).double()
    var[Co // 2] = 0.0                                # a channel without variance: s = gamma / sqrt(eps)
    return gamma, beta, mean, var


def fold_reference(gen, w, gamma, beta, mean, var, eps, used=True):
    """fp64: folded weights, and the gradients of w, gamma, beta of L = <go, BN_eval(conv(x, w))> by autograd of the UNFUSED formula;
    the upstream gradients dL/dw', dL/db' the device backward is fed come from the folded formula's leaves.  fp32: the fold's own
    formula on the CPU (forward and, fed the same upstream gradients, backward)."""
    Co, Ci, k, _ = w.shape
    x = torch.randn(2, Ci, 5, 6, generator=gen).double()
    go = torch.randn(2, Co, 5, 6, generator=gen).double()
    leaves = [t.clone().requires_grad_() for t in (w, gamma, beta)]
    y = F.conv2d(x, leaves[0], None, padding=k // 2)
    y = (y - mean.view(1, Co, 1, 1)) / torch.sqrt(var.view(1, Co, 1, 1) + eps) * leaves[1].view(1, Co, 1, 1) + leaves[2].view(1, Co, 1, 1)
    wf, bf, wT = R.bn_fold(w, gamma, beta, mean, var, eps)
    if used:
        (y * go).sum().backward()
        wl, bl = wf.clone().requires_grad_(), bf.clone().requires_grad_()
        (F.conv2d(x, wl, bl, padding=k // 2) * go).sum().backward()
        gwf, gbf = wl.grad.float(), bl.grad.float()
        grads = [t.grad for t in leaves]
    else:
        gwf = gbf = None
        grads = [torch.zeros_like(t) for t in leaves]
    l32 = [t.float().requires_grad_() for t in (w, gamma, beta)]
    wf32, bf32, _ = R.bn_fold(l32[0], l32[1], l32[2], mean.float(), var.float(), eps)
    if used:
        torch.autograd.backward([wf32, bf32], [gwf, gbf])
        g32 = [t.grad for t in l32]
    else:
        g32 = [torch.zeros_like(t) for t in l32]
    return dict(wf=wf, bf=bf, wT=wT, grads=grads, gwf=gwf, gbf=gbf, wf32=wf32.detach(), bf32=bf32.detach(), g32=g32)


@pytest.mark.parametrize('Co,Ci,k', [(1, 4, 1), (33, 24, 3), (64, 256, 3), (7, 260, 1)])
def test_bn_fold_single(dev, Co, Ci, k):
    """bricks._BNFold (htd_bn_fold_fwd / _bwd, one block per output channel): K = Ci * k * k = 4 (one thread), 216, 2304 (above 1024:
    the row loop wraps twice), 260; a channel with var = 0.  Gradients of w, gamma, beta against float64 autograd of the unfused
    convolution-then-BatchNorm."""
    from htd_amd.detector.bricks import _BNFold
    gen = torch.Generator().manual_seed(Co * 3 + Ci)
    w = torch.randn(Co, Ci, k, k, generator=gen).double()
    gamma, beta, mean, var = bn_params(gen, Co)
    ref = fold_reference(gen, w, gamma, beta, mean, var, 1e-5)
    wd = to_dev(w.float(), dev).requires_grad_()
    gd, bd = gamma.float().to(dev).requires_grad_(), beta.float().to(dev).requires_grad_()
    wf, bf = _BNFold.apply(wd, gd, bd, mean.float().to(dev), var.float().to(dev), 1e-5)
    tag = f'fold Co{Co} Ci{Ci} k{k}'
    check_float(tag + ' wf', wf, ref['wf'], ref['wf32'], 1)
    check_float(tag + ' bf', bf, ref['bf'], ref['bf32'], 1)
    torch.autograd.backward([wf, bf], [to_dev(ref['gwf'], dev), ref['gbf'].to(dev)])
    torch.cuda.synchronize()
    run = 4 * -(-Ci * k * k // 1024)
    for name, t, r64, r32 in zip(('gw', 'ggamma', 'gbeta'), (wd, gd, bd), ref['grads'], ref['g32']):
        check_float(f'{tag} {name}', t.grad, r64, r32, run)


MANY_LAYERS = [(33, 24, 3), (64, 256, 3), (7, 260, 1), (1, 4, 1), (40, 36, 3), (32, 32, 1), (65, 100, 1)]


@pytest.mark.parametrize('flips', [True, False])
@pytest.mark.parametrize('layers,unused', [([(33, 24, 3)], None), ([(32, 32, 1)], None), (MANY_LAYERS, 4)])
def test_bn_fold_many(dev, layers, unused, flips):
    """bricks._BNFoldMany (htd_bn_fold_many_fwd / _bwd): one and seven layers in a launch, Co and Ci on and off the 32 x 32 tile
    grid, 1x1 and 3x3, with the flipped images and without.  Every element of every layer is compared, so find_layer is right at
    the first and last tile / row of each layer.  wT must be the permutation of the wf the same launch wrote, bit for bit.  One
    layer's folded weight gets no gradient: its gradients are zero."""
    from htd_amd import dense
    from htd_amd.detector.bricks import _BNFoldMany
    gen = torch.Generator().manual_seed(len(layers) + flips)
    refs, tensors, leaves = [], [], []
    for i, (Co, Ci, k) in enumerate(layers):
        w = torch.randn(Co, Ci, k, k, generator=gen).double()
        gamma, beta, mean, var = bn_params(gen, Co)
        refs.append(fold_reference(gen, w, gamma, beta, mean, var, 1e-5, used=(i != unused)))
        wd = to_dev(w.float(), dev).requires_grad_()
        gd, bd = gamma.float().to(dev).requires_grad_(), beta.float().to(dev).requires_grad_()
        leaves.append((wd, gd, bd))
        tensors += [wd, gd, bd, mean.float().to(dev), var.float().to(dev)]
    outs = _BNFoldMany.apply(1e-5, flips, False, *tensors)
    heads, grads = [], []
    for i, ((Co, Ci, k), ref) in enumerate(zip(layers, refs)):
        wf, bf = outs[2 * i], outs[2 * i + 1]
        tag = f'many[{i}] Co{Co} Ci{Ci} k{k}'
        check_float(tag + ' wf', wf, ref['wf'], ref['wf32'], 1)
        check_float(tag + ' bf', bf, ref['bf'], ref['bf32'], 1)
        wT = dense.take_flipped(wf)
        assert (wT is not None) == flips
        if flips:
            perm = wf.detach().reshape(Co, Ci, k * k).flip(2).permute(1, 2, 0)
            assert torch.equal(wT.view(Ci, k * k, Co), perm), tag + ' wT'
            check_float(tag + ' wT', wT.view(Ci, k * k, Co), ref['wT'], ref['wT'].float(), 1)
        if i != unused:
            heads += [wf, bf]
            grads += [to_dev(ref['gwf'], dev), ref['gbf'].to(dev)]
    torch.autograd.backward(heads, grads)
    torch.cuda.synchronize()
    for i, ((Co, Ci, k), ref, trio) in enumerate(zip(layers, refs, leaves)):
        run = 4 * -(-Ci * k * k // 1024)
        for name, t, r64, r32 in zip(('gw', 'ggamma', 'gbeta'), trio, ref['grads'], ref['g32']):
            check_float(f'many[{i}] Co{Co} Ci{Ci} k{k} {name}', t.grad, r64, r32, run)
        if i == unused:
            assert all(float(t.grad.abs().sum()) == 0.0 for t in trio)


def test_bn_fold_many_table_through_the_abi(dev):
    """htd_bn_fold_many_fwd on a table of its own: a layer without BatchNorm (gamma == NULL: only its flipped image is written, as
    dense.flip_many asks), a folded layer without wT, and a folded layer with both, at sizes off the tile grid."""
    from htd_amd import capi
    gen = torch.Generator().manual_seed(77)
    layers = [(40, 36, 9, False, True), (33, 68, 1, True, False), (70, 24, 9, True, True)]        # Co, Ci, taps, BN, wT
    desc = np.zeros((len(layers), 10), dtype=np.int64)
    keep, tile0 = [], 0
    for i, (Co, Ci, taps, bn, flip) in enumerate(layers):
        w = torch.randn(Co, taps, Ci, generator=gen)                      # [co][tap][ci] memory
        gamma, beta, mean, var = (t.float() for t in bn_params(gen, Co))
        wd, pd = w.to(dev), [t.to(dev) for t in (gamma, beta, mean, var)]
        wf, bf = torch.full((Co, taps, Ci), float('nan'), device=dev), torch.full((Co, ), float('nan'), device=dev)
        wT = torch.full((Ci, taps, Co), float('nan'), device=dev)
        desc[i, :8] = (wd.data_ptr(),) + (tuple(t.data_ptr() for t in pd) if bn else (0, 0, 0, 0)) + \
            (wf.data_ptr() if bn else 0, bf.data_ptr() if bn else 0, wT.data_ptr() if flip else 0)
        desc[i, 8] = Co | (Ci << 32)
        desc[i, 9] = taps | (tile0 << 32)
        tile0 += taps * ((Co + 31) // 32) * ((Ci + 31) // 32)
        keep.append((w, gamma, beta, mean, var, wd, pd, wf, bf, wT))
    table = capi.upload_table(desc, dev)
    call('htd_bn_fold_many_fwd', P_(table), len(layers), tile0, 1e-5, S_())
    for (Co, Ci, taps, bn, flip), (w, gamma, beta, mean, var, wd, pd, wf, bf, wT) in zip(layers, keep):
        src = wd
        if bn:
            s64 = gamma.double() / torch.sqrt(var.double() + 1e-5)
            s32 = gamma / torch.sqrt(var + 1e-5)
            check_float(f'table Co{Co} wf', wf, w.double() * s64.view(Co, 1, 1), w * s32.view(Co, 1, 1), 1)
            check_float(f'table Co{Co} bf', bf, beta.double() - mean.double() * s64, beta - mean * s32, 1)
            src = wf
        if flip:
            assert torch.equal(wT, src.flip(1).permute(2, 1, 0)), f'table Co{Co} wT'
        else:
            assert bool(torch.isnan(wT).all())


def test_bn_fold_rejections(dev):
    """K % 4 != 0 is refused by htd_bn_fold_fwd / _bwd before any launch."""
    z = torch.zeros(64, device=dev)
    with rejected():
        call('htd_bn_fold_fwd', P_(z), P_(z), P_(z), P_(z), P_(z), 1e-5, P_(z), P_(z), 2, 6, S_())
    with rejected():
        call('htd_bn_fold_bwd', P_(z), P_(z), P_(z), P_(z), 1e-5, P_(z), P_(z), P_(z), P_(z), P_(z), 2, 6, S_())


# ====================================================================== SGD with momentum
SGD_N = [1, 2, 3, 4, 5, 1023, 100003]


@pytest.mark.parametrize('n', SGD_N)
def test_sgd_dyadic_constants_exact(dev, n):
    """htd_sgd_momentum_step with lr 0.5, momentum 0.5, weight decay 0.25, grad_scale 0.125 on integer p, g and (non-zero) m: two
    steps stay on a grid of 2^-7 below 2^6 and are exact in fp32, contracted or not.  n < 4 runs in the scalar tail alone,
    n % 4 = 1, 2, 3 in both parts, 100003 over many blocks."""
    from htd_amd import mmcv_ops as M
    gen = torch.Generator().manual_seed(n)
    p, m = ints(gen, n), ints(gen, n)
    pd, md = p.float().to(dev), m.float().to(dev)
    lr = torch.tensor([0.5], device=dev)
    for _ in range(2):
        g = ints(gen, n)
        p, m = R.sgd_momentum(p, g, m, 0.5, 0.5, 0.25, 0.125)
        M.sgd_momentum_step_(pd, g.float().to(dev), md, lr, 0.5, 0.25, 0.125)
    check_exact('sgd p', pd, p)
    check_exact('sgd m', md, m)


@pytest.mark.parametrize('mom,wd,gscale', [(0.9, 1e-4, 1.0), (0.0, 1e-4, 1.0), (0.9, 0.0, 1.0), (0.9, 1e-4, 0.125)])
@pytest.mark.parametrize('n', SGD_N)
def test_sgd_float(dev, n, mom, wd, gscale):
    """Float parameters, a non-zero start momentum, momentum 0, weight decay 0, grad_scale 0.125; the device learning rate is
    overwritten between the two steps with nothing but stream order in between (the kernel reads it on the device)."""
    from htd_amd import mmcv_ops as M
    gen = torch.Generator().manual_seed(n + 1)
    p, m = torch.randn(n, generator=gen).double(), torch.randn(n, generator=gen).double()
    p32, m32 = p.float(), m.float()
    pd, md = p32.to(dev), m32.to(dev)
    lr = torch.tensor([0.02], device=dev)
    for step_lr in (0.02, 0.005):
        g = torch.randn(n, generator=gen).double()
        gd = g.float().to(dev)
        lr.fill_(step_lr)
        M.sgd_momentum_step_(pd, gd, md, lr, mom, wd, gscale)
        lr32 = float(torch.tensor(step_lr, dtype=torch.float32))
        p, m = R.sgd_momentum(p, g, m, lr32, mom, wd, gscale)
        p32, m32 = R.sgd_momentum(p32, g.float(), m32, lr32, mom, wd, gscale)
    tag = f'sgd n{n} mom{mom} wd{wd} gs{gscale}'
    check_float(tag + ' p', pd, p, p32, 3)
    check_float(tag + ' m', md, m, m32, 3)


def test_sgd_rejects_unaligned_buffers(dev):
    """16-byte alignment is required by htd_sgd_momentum_step before the launch."""
    from htd_amd import mmcv_ops as M
    buf = torch.zeros(64, device=dev)
    lr = torch.tensor([0.1], device=dev)
    with rejected():
        M.sgd_momentum_step_(buf[1:33], buf[32:64], torch.zeros(32, device=dev), lr, 0.9, 0.0)


# ====================================================================== coder kernels (csrc/box_ops.hip)
STDS = (0.1, 0.1, 0.2, 0.2)
ZERO4, ONE4 = (0., 0., 0., 0.), (1., 1., 1., 1.)


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_delta2bbox_clip_fixture_arrays(dev, golden):
    """htd_delta2bbox_clip (decode_clip_kernel) on the reference's recorded arrays, tolerances of test_box_math: clipped to a
    90 x 80 image, unclipped with deltas ten times the spread (beyond the width / height clip), and the reference docstring's four
    boxes with their zero-size RoI."""
    from htd_amd.core.bbox import delta2bbox_clip_device as dec
    g = golden('box_math')
    b1, rnd = T(g['b1']).to(dev), T(g['rnd']).to(dev)
    lim = torch.tensor([[90., 80.]], device=dev)
    torch.testing.assert_close(dec(b1, rnd, ZERO4, STDS, lim).cpu(), T(g['dec']), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(dec(b1, rnd * 10, ZERO4, ONE4).cpu(), T(g['dec_noclip']), rtol=1e-6, atol=1e-4)
    kat = dec(T(g['kat_rois']).to(dev), T(g['kat_deltas']).to(dev), ZERO4, ONE4, torch.tensor([[32., 32.]], device=dev))
    torch.testing.assert_close(kat.cpu(), T(g['kat_dec']), rtol=1e-6, atol=1e-6)
    assert kat[3].tolist() == [5., 5., 5., 5.]


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 5000])
def test_delta2bbox_clip(dev, n):
    """Random rows around the 256-thread block: three images with their own [W, H] and rows_per_img rows each, keep with zeros
    (those rows exactly zero), non-zero means, every seventh row's dw / dh far beyond the width / height clip, every ninth RoI
    of zero size; against glue_ref in fp32 (same order of operations) with test_box_math's tolerance for clipped boxes, and
    without limits or keep with its tolerance for unclipped ones."""
    from htd_amd.core.bbox import delta2bbox_clip_device as dec
    gen = torch.Generator().manual_seed(n)
    xy = torch.rand(n, 2, generator=gen) * 100
    rois = torch.cat([xy, xy + torch.rand(n, 2, generator=gen) * 60 + 1], 1)
    rois[::9, 2:] = rois[::9, :2]
    deltas = torch.randn(n, 4, generator=gen)
    deltas[::7, 2:] = torch.tensor([40., -40.])
    means = (0.05, -0.1, 0.1, -0.05)
    lim = torch.tensor([[90., 80.], [50., 120.], [200., 30.]])
    keep = (torch.rand(n, generator=gen) > 0.2)
    rows = max(1, -(-n // 3))
    out = dec(rois.to(dev), deltas.to(dev), means, STDS, lim.to(dev), keep.to(dev), rows)
    ref = R.delta2bbox_clip(rois, deltas, means, STDS, lim, keep, rows)
    assert out.shape == (n, 4)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-6, atol=1e-5)
    assert bool((out.cpu()[~keep] == 0).all())
    if n:
        W, H = lim[torch.arange(n) // rows, 0:1], lim[torch.arange(n) // rows, 1:2]
        o = out.cpu()
        assert bool((o >= 0).all()) and bool((o[:, 0::2] <= W).all()) and bool((o[:, 1::2] <= H).all())
    small = torch.cat([xy, xy + torch.rand(n, 2, generator=gen) * 2], 1)
    out = dec(small.to(dev), deltas.to(dev), means, STDS)
    torch.testing.assert_close(out.cpu(), R.delta2bbox_clip(small, deltas, means, STDS), rtol=1e-6, atol=1e-4)


def test_roi_targets_fixture_arrays(dev, golden):
    """htd_roi_targets (roi_targets_kernel) on the recorded encoder answers, tolerance of test_box_math."""
    from htd_amd.core.bbox import roi_targets_device as tgt
    g = golden('box_math')
    n = 9
    b1, b2 = T(g['b1'])[:n].to(dev), T(g['b2']).to(dev)
    ones = torch.ones(n, device=dev)
    labels, lw, bt, bw = tgt(b1, b2, torch.arange(n, device=dev) + 1, ones, ones, 80, ZERO4, STDS)
    torch.testing.assert_close(bt.cpu(), T(g['deltas']), rtol=1e-6, atol=1e-6)
    assert labels.tolist() == list(range(1, 10)) and bool((lw == 1).all()) and bool((bw == 1).all())


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 5000])
def test_roi_targets(dev, n):
    """Positive, negative and unused slots, non-zero means; the negatives' gt boxes are of zero size (their quotient would be
    non-finite): their targets must be exactly zero.  Labels, label weights, box weights exact; targets against glue_ref in fp32."""
    from htd_amd.core.bbox import roi_targets_device as tgt
    gen = torch.Generator().manual_seed(n + 5)
    xy = torch.rand(n, 2, generator=gen) * 100
    boxes = torch.cat([xy, xy + torch.rand(n, 2, generator=gen) * 60 + 4], 1)
    gxy = xy + torch.randn(n, 2, generator=gen) * 3
    gts = torch.cat([gxy, gxy + torch.rand(n, 2, generator=gen) * 60 + 4], 1)
    pos = torch.rand(n, generator=gen) < 0.3
    valid = torch.rand(n, generator=gen) < 0.9
    gts[~pos] = 0.0
    gl = torch.randint(0, 80, (n, ), generator=gen)
    means = (0.05, -0.1, 0.1, -0.05)
    labels, lw, bt, bw = tgt(boxes.to(dev), gts.to(dev), gl.to(dev), pos.to(dev), valid.to(dev), 80, means, STDS)
    rl, rlw, rbt, rbw = R.roi_targets(boxes, gts, gl, pos, valid, 80, means, STDS)
    assert torch.equal(labels.cpu(), rl) and torch.equal(lw.cpu(), rlw) and torch.equal(bw.cpu(), rbw)
    assert bool((bt.cpu()[~pos] == 0).all())
    torch.testing.assert_close(bt.cpu(), rbt, rtol=1e-6, atol=1e-6)
