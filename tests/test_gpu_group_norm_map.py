"""The whole-map GroupNorm kernels and the weight-standardisation kernels of csrc/group_norm_map.hip, against float64
references: glue_ref.group_norm_relu (extended here with the residual) and the tensor formula of mmcv's ConvWS2d
(mmcv-knowledge: mmcv 1.2.1, unbiased std, eps beside the root).

The FLOAT rule of tests/test_gpu_glue_ops.py, unchanged:  e = max |out - ref64| / max |ref64|  <=  F x max(e_cpu, 2^-23),
F = max(8, sqrt(R)), e_cpu the same formula in fp32 by ATen on the CPU (torch.native_group_norm), R the longest run of terms one
thread adds sequentially.  The upstream gradient is zero where the pre-activation is within 1e-3 of zero.

R, counted from the kernels (map_runs below evaluates it per case; every case here has R <= 64, F = 8):
  forward   gn_map_stats_kernel: a thread takes 8 positions x 4 channels per pass as a pairwise tree (depth 5), merges its
            S / (8 Rr) passes by Chan's formula, then log2(cpg / 4) shuffle merges, the Rr = 256 / min(C / 4, 256) <= 16 row
            groups in order; gn_map_norm_kernel merges the slabs of a sample as J runs of ceil(slabs / J), then the J runs
            (J = 256 / min(G, 256)):  R = max(8, S / (8 Rr), Rr, ceil(slabs / J), J).
  backward  gn_map_bwd_sums_kernel: a thread adds its ceil(S / Rr) positions in order, the Rr row groups in order, 4 channels
            and log2(cpg / 4) shuffles; gn_map_bwd_gx_kernel adds the slabs as in the forward; colsum_rows_kernel adds
            ceil(n slabs / 16) rows per thread and 16 partial sums; gx also consumes mean and rstd:
            R = max(R forward, ceil(S / Rr), 16, ceil(n slabs / 16)).
  weight standardisation: ceil(K / 256) <= 18 terms per thread, six shuffles, four waves: F = 8.

Cases: cpg = 2 (one float4 spans two groups), odd P, many slabs, HTD's (576, 36), cpg = 64 with C above the tile kernels' limit
and two column passes, P = 1 (with equal values per group y is beta), and for C = 256 (slab = 32 positions) P = 31, 32, 33 and 65."""
import functools

import pytest
import torch
import torch.nn.functional as F

import glue_ref as R

pytestmark = pytest.mark.gpu
D64 = torch.float64
EPS = 1e-5

MAP_CASES = [(64, 32, 25, 42, 1), (128, 32, 13, 21, 3), (256, 32, 50, 84, 2), (576, 36, 9, 11, 1), (2048, 32, 4, 5, 2),
             (512, 32, 1, 1, 2), (256, 32, 1, 31, 2), (256, 32, 1, 32, 2), (256, 32, 1, 33, 2), (256, 32, 1, 65, 2)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture
def h2_state():
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
    return t.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)


def nhwc_full(n, C, h, w, dev, fill):
    return torch.full((n, h, w, C), float(fill), device=dev).permute(0, 3, 1, 2)


def check_float(name, out, ref64, cpu32, run):
    e, e_cpu = R.rel_err(out, ref64), R.rel_err(cpu32, ref64)
    bound = R.float_bound(e_cpu, run)
    print(f'{name}: e_kernel {e:.3e}  e_cpu {e_cpu:.3e}  R {run}  bound {bound:.3e}')
    assert e <= bound, f'{name}: e_kernel {e:.3e} > bound {bound:.3e} (e_cpu {e_cpu:.3e}, R {run})'


def gn_res(x, gamma, beta, G, relu, residual):
    """glue_ref.group_norm_relu with the residual joined in front of the ReLU -> y, mean, rstd, pre-activation"""
    pre, mean, rstd = R.group_norm_relu(x, gamma, beta, G, EPS, False)
    if residual is not None:
        pre = pre + residual
    return (torch.relu(pre) if relu else pre), mean, rstd, pre


def map_runs(C, G, P, n):
    from htd_amd import capi
    S = capi.lib().htd_group_norm_map_slab(P, C)
    slabs = -(-P // S)
    Rr = 256 // min(C // 4, 256)
    J = 256 // min(G, 256)
    fwd = max(8, S // (8 * Rr), Rr, -(-slabs // J), J)
    return fwd, max(fwd, -(-S // Rr), 16, -(-(n * slabs) // 16))


@functools.lru_cache(maxsize=8)
def map_reference(C, G, h, w, n, flavour, relu, with_res):
    gen = torch.Generator().manual_seed(C * 131 + G * 17 + h * w + n)
    x = torch.randn(n, C, h, w, generator=gen, dtype=D64)
    if flavour == 'mean50':
        x = x + 50
    if flavour == 'const':                       # one (sample, group) without variance
        x[n - 1, C // G:2 * (C // G)] = 3.0
    x = x.float().double()
    gamma, beta = (torch.randn(C, generator=gen).double() for _ in range(2))
    res = torch.randn(n, C, h, w, generator=gen).double() if with_res else None
    gy = torch.randn(n, C, h, w, generator=gen).double()
    if relu:
        gy = gy * (gn_res(x, gamma, beta, G, False, res)[3].abs() > 1e-3)
    leaves = [t.clone().requires_grad_() for t in (x, gamma, beta)] + ([res.clone().requires_grad_()] if with_res else [None])
    y64, m64, r64, _ = gn_res(leaves[0], leaves[1], leaves[2], G, relu, leaves[3])
    y64.backward(gy)
    l32 = [t.float().requires_grad_() for t in (x, gamma, beta)] + ([res.float().requires_grad_()] if with_res else [None])
    y32, m32, r32 = torch.native_group_norm(l32[0], l32[1], l32[2], n, C, h * w, G, EPS)
    if with_res:
        y32 = y32 + l32[3]
    y32 = F.relu(y32) if relu else y32
    y32.backward(gy.float())
    ref = dict(y=y64.detach(), mean=m64.detach(), rstd=r64.detach(), gx=leaves[0].grad, ggamma=leaves[1].grad, gbeta=leaves[2].grad)
    cpu = dict(y=y32.detach(), mean=m32.detach().view(n, G), rstd=r32.detach().view(n, G), gx=l32[0].grad, ggamma=l32[1].grad,
               gbeta=l32[2].grad)
    return x, gamma, beta, res, gy, ref, cpu


def test_slab_lengths_sit_where_the_cases_expect():
    from htd_amd import capi
    L = capi.lib()
    assert [L.htd_group_norm_map_slab(P, 256) for P in (31, 32, 33, 65, 4200)] == [32, 32, 32, 32, 64]
    assert L.htd_group_norm_map_slab(25 * 42, 64) == 128 and L.htd_group_norm_map_slab(20, 2048) == 8
    assert L.htd_group_norm_map_slab(200 * 336, 256) * 128 >= 200 * 336          # at most 128 slabs per sample
    assert L.htd_group_norm_map_workspace_bytes(2, 4200, 256, 32) >= 2 * 66 * (2 * 256 * 4 + 32 * 8)


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('flavour', ['randn', 'mean50', 'const'])
@pytest.mark.parametrize('C,G,h,w,n', MAP_CASES)
def test_group_norm_map(dev, C, G, h, w, n, flavour, relu, with_res):
    """mmcv_ops.group_norm_map forward and backward through the wrapper, twice: every output within the FLOAT bound, the residual's
    gradient the masked gy bit for bit, the two runs equal in every bit."""
    from htd_amd import dense
    from htd_amd import mmcv_ops as M
    x, gamma, beta, res, gy, ref, cpu = map_reference(C, G, h, w, n, flavour, relu, with_res)
    gyd = to_dev(gy.float(), dev)
    runs = []
    for _ in range(2):
        dense.new_step()
        xd = to_dev(x.float(), dev).requires_grad_()
        gd, bd = gamma.float().to(dev).requires_grad_(), beta.float().to(dev).requires_grad_()
        rd = to_dev(res.float(), dev).requires_grad_() if with_res else None
        out = M.group_norm_map(xd, gd, bd, G, EPS, relu, rd)
        assert type(out.grad_fn).__name__ == 'GroupNormMapFunctionBackward'
        saved = out.grad_fn.saved_tensors
        out.backward(gyd)
        runs.append(dict(y=out.detach(), mean=saved[3], rstd=saved[4], gx=xd.grad, ggamma=gd.grad, gbeta=bd.grad,
                         gres=rd.grad if with_res else None))
    a, b = runs
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), f'{k}: two runs differ'
    r_fwd, r_bwd = map_runs(C, G, h * w, n)
    tag = f'GNmap C{C} G{G} {h}x{w} n{n} {flavour} relu{int(relu)} res{int(with_res)}'
    for k, run in (('y', r_fwd), ('mean', r_fwd), ('rstd', r_fwd), ('gx', r_bwd), ('ggamma', r_bwd), ('gbeta', r_bwd)):
        check_float(f'{tag} {k}', a[k], ref[k], cpu[k], run)
    if with_res:
        want = gyd * (a['y'] > 0) if relu else gyd
        assert torch.equal(a['gres'], want)
    if flavour == 'const':
        # the one group without variance (sample n - 1, group 1; every value 3.0): sums of 3.0 are exact, the mean is 3.0 exactly,
        # every deviation and so M2 is exactly 0, and rstd = rsqrtf(fl(eps)): eps^-1/2 up to the hardware's rsqrt (v_rsq_f32,
        # 1 ulp) and the rounding of eps itself (half an ulp, halved by the root): 2 ulp = 2^-22 relative at most
        assert float(a['mean'][n - 1, 1]) == 3.0
        assert abs(float(a['rstd'][n - 1, 1]) - EPS ** -0.5) <= 2.0 ** -22 * EPS ** -0.5


def test_single_position_of_equal_values_reduces_to_beta(dev):
    """P = 1 with every value v of a group equal: mean = v exactly, the variance is 0 and y = v ga + (beta - v ga) with
    ga = gamma eps^-1/2: beta up to the two roundings of that sum, 2 ulp of |v ga| at most."""
    from htd_amd import mmcv_ops as M
    C, G, n = 512, 32, 2
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, G, 1, generator=gen).expand(n, G, C // G).reshape(n, C, 1, 1).contiguous()
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    y = M.group_norm_map(to_dev(x, dev), gamma.to(dev), beta.to(dev), G, EPS, False)
    saved_mean = x.view(n, G, C // G)[:, :, 0]
    slack = 4 * 2.0 ** -23 * (x.view(n, C) * gamma.view(1, C)).abs() * EPS ** -0.5
    assert bool(((y.cpu().view(n, C) - beta.view(1, C)).abs() <= slack).all())
    y2 = M.group_norm_map(to_dev(x, dev).requires_grad_(), gamma.to(dev), beta.to(dev), G, EPS, False)
    assert torch.equal(y2.grad_fn.saved_tensors[3].cpu(), saved_mean)


def test_empty_batch(dev):
    """n = 0 launches nothing and returns zero parameter gradients."""
    from htd_amd import mmcv_ops as M
    xd = to_dev(torch.zeros(0, 256, 20, 20), dev).requires_grad_()
    gd, bd = torch.ones(256, device=dev, requires_grad=True), torch.zeros(256, device=dev, requires_grad=True)
    out = M.group_norm_map(xd, gd, bd, 32, EPS, True)
    assert out.shape == (0, 256, 20, 20)
    out.backward(torch.zeros_like(out))
    assert xd.grad.shape == xd.shape
    assert torch.equal(gd.grad, torch.zeros_like(gd)) and torch.equal(bd.grad, torch.zeros_like(bd))


def test_exact_zeros_under_relu_pass_no_gradient(dev):
    """gamma = beta = 0 (pre-activation exactly 0) and gamma = 0, beta = -1 (clamped), with a zero residual on those channels:
    nothing reaches x's parameter gradients or the residual there."""
    from htd_amd import mmcv_ops as M
    for C, G in ((256, 32), (64, 32)):
        gen = torch.Generator().manual_seed(C)
        x, res = torch.randn(2, C, 15, 15, generator=gen), torch.randn(2, C, 15, 15, generator=gen)
        gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        gamma[[3, 10]] = 0.0
        beta[3], beta[10] = 0.0, -1.0
        res[:, [3, 10]] = 0.0
        gy = torch.randn(2, C, 15, 15, generator=gen)
        xd, gd, bd = to_dev(x, dev).requires_grad_(), gamma.to(dev).requires_grad_(), beta.to(dev).requires_grad_()
        rd = to_dev(res, dev).requires_grad_()
        out = M.group_norm_map(xd, gd, bd, G, EPS, True, rd)
        out.backward(to_dev(gy, dev))
        assert bool((out[:, [3, 10]] == 0).all())
        for c in (3, 10):
            assert float(gd.grad[c]) == 0.0 and float(bd.grad[c]) == 0.0
            assert bool((rd.grad[:, c] == 0).all())
        assert float(gd.grad.abs().sum()) > 0 and float(rd.grad.abs().sum()) > 0
        # no ReLU-masked gradient term reaches x from the dead channels: with all of a group dead, gx of the group is 0
        gamma2, beta2 = gamma.clone(), beta.clone()
        cpg = C // G
        gamma2[:cpg], beta2[:cpg] = 0.0, -1.0
        x2 = to_dev(x, dev).requires_grad_()
        M.group_norm_map(x2, gamma2.to(dev), beta2.to(dev), G, EPS, True).backward(to_dev(gy, dev))
        assert bool((x2.grad[:, :cpg] == 0).all())


def abi_fwd(x, res, gamma, beta, G, relu, slot=None, fill=float('nan')):
    from htd_amd import capi
    n, C, h, w = x.shape
    y = nhwc_full(n, C, h, w, x.device, fill)
    mean, rstd = (torch.full((n, G), fill, device=x.device) for _ in range(2))
    ws = torch.full((capi.lib().htd_group_norm_map_workspace_bytes(n, h * w, C, G) // 4, ), fill, device=x.device)
    call('htd_group_norm_map_fwd', P_(x), P_(res), P_(gamma), P_(beta), P_(y), P_(mean), P_(rstd), n, h * w, C, G, EPS, int(relu),
         P_(ws), P_(slot), S_())
    return y, mean, rstd


def abi_bwd(x, y, gamma, mean, rstd, gy, G, relu, want_res, slot=None, fill=float('nan')):
    from htd_amd import capi
    n, C, h, w = x.shape
    gx = nhwc_full(n, C, h, w, x.device, fill)
    gres = nhwc_full(n, C, h, w, x.device, fill) if want_res else None
    gg, gb = (torch.full((C, ), fill, device=x.device) for _ in range(2))
    ws = torch.full((capi.lib().htd_group_norm_map_workspace_bytes(n, h * w, C, G) // 4, ), fill, device=x.device)
    call('htd_group_norm_map_bwd', P_(x), P_(y), P_(gamma), P_(mean), P_(rstd), P_(gy), P_(gx), P_(gres), P_(gg), P_(gb), n, h * w,
         C, G, int(relu), P_(ws), P_(slot), S_())
    return gx, gres, gg, gb


@pytest.mark.parametrize('C,G,h,w,n', [(64, 32, 25, 42, 1), (256, 32, 50, 84, 2), (576, 36, 9, 11, 1), (2048, 32, 4, 5, 2)])
def test_raw_abi_overwrites_every_output_and_leaves_the_maximum(dev, C, G, h, w, n):
    """Outputs and workspace pre-filled with NaN hold no NaN afterwards (every element is written, nothing is accumulated);
    amax_out is max |y| / max |gx| bit for bit, a larger value in the slot survives, a NaN in the tensor leaves a NaN."""
    x, gamma, beta, res, gy, _, _ = map_reference(C, G, h, w, n, 'randn', True, True)
    xd, rd, gyd = to_dev(x.float() * 3, dev), to_dev(res.float(), dev), to_dev(gy.float(), dev)
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    slot = torch.zeros(1, device=dev)
    y, mean, rstd = abi_fwd(xd, rd, gd, bd, G, True, slot)
    y7 = abi_fwd(xd, rd, gd, bd, G, True, None, fill=7.0)
    assert all(torch.equal(s, t) for s, t in zip((y, mean, rstd), y7))
    assert all(bool(torch.isfinite(t).all()) for t in (y, mean, rstd))
    assert float(slot) == float(y.abs().max()) and float(slot) > 0
    slot.fill_(1e30)
    abi_fwd(xd, rd, gd, bd, G, True, slot)
    assert float(slot) == float(torch.tensor(1e30))
    for relu in (False, True):
        xn = xd.clone()
        xn[n - 1, C - 1, h - 1, w - 1] = float('nan')
        slot.zero_()
        yn = abi_fwd(xn, None, gd, bd, G, relu, slot)[0]
        assert bool(torch.isnan(yn).any()) and bool(torch.isnan(slot).item())
    slot.zero_()
    gx, gres, gg, gb = abi_bwd(xd, y, gd, mean, rstd, gyd, G, True, True, slot)
    again = abi_bwd(xd, y, gd, mean, rstd, gyd, G, True, True, None, fill=7.0)
    assert all(torch.equal(s, t) for s, t in zip((gx, gres, gg, gb), again))
    assert all(bool(torch.isfinite(t).all()) for t in (gx, gres, gg, gb))
    assert torch.equal(gres, gyd * (y > 0))
    assert float(slot) == float(gx.abs().max()) and float(slot) > 0
    slot.fill_(1e30)
    abi_bwd(xd, y, gd, mean, rstd, gyd, G, True, False, slot)
    assert float(slot) == float(torch.tensor(1e30))
    gn_ = gyd.clone()
    gn_[0, 0, 0, 0] = float('nan')
    slot.zero_()
    gxn, gres0, _, _ = abi_bwd(xd, y, gd, mean, rstd, gn_, G, False, True, slot, fill=5.0)
    assert bool(torch.isnan(gxn).any()) and bool(torch.isnan(slot).item())
    assert bool((gres0 == 5.0).all())            # relu = 0: the residual's gradient is gy itself, nothing is written


def test_refused_shapes_return_before_a_launch(dev):
    """C % 4, three channels per group, C = 4096, one channel per group, C below 64 and null pointers: HTD_ERR_ARG, and the
    NaN-filled outputs are untouched."""
    from htd_amd import mmcv_ops as M
    for C, G in ((66, 33), (96, 32), (4096, 64), (64, 64), (32, 8), (256, 3)):
        x = to_dev(torch.randn(2, C, 15, 15), dev)
        with rejected():
            M.group_norm_map(x, torch.ones(C, device=dev), torch.zeros(C, device=dev), G, EPS, True)
    C, G, n, h, w = 256, 32, 2, 15, 15
    x, g, b = to_dev(torch.randn(n, C, h, w), dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    y = nhwc_full(n, C, h, w, dev, float('nan'))
    mean, rstd = torch.empty(n, G, device=dev), torch.empty(n, G, device=dev)
    ws = torch.empty(1 << 20, device=dev)
    for args in ((None, None, g, b, y, mean, rstd), (x, None, None, b, y, mean, rstd), (x, None, g, b, None, mean, rstd),
                 (x, None, g, b, y, None, rstd)):
        with rejected():
            call('htd_group_norm_map_fwd', *[P_(t) for t in args], n, h * w, C, G, EPS, 1, P_(ws), None, S_())
    with rejected():
        call('htd_group_norm_map_fwd', P_(x), None, P_(g), P_(b), P_(y), P_(mean), P_(rstd), n, h * w, C, G, EPS, 1, None, None, S_())
    gx = nhwc_full(n, C, h, w, dev, float('nan'))
    with rejected():
        call('htd_group_norm_map_bwd', P_(x), P_(x), P_(g), P_(mean), P_(rstd), P_(x), P_(gx), None, None, P_(b), n, h * w, C, G, 1,
             P_(ws), None, S_())
    with rejected():
        call('htd_group_norm_map_bwd', P_(x), P_(x), P_(g), P_(mean), P_(rstd), None, P_(gx), None, P_(g), P_(b), n, h * w, C, G, 1,
             P_(ws), None, S_())
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(gx).all())


def test_conv_module_dispatch(dev):
    """ConvModule sends a (2, 256, 50, 84) GroupNorm to the map kernels and a (70, 256, 7, 7) one to the RoI-tile kernels; the
    rule is mmcv_ops.use_group_norm_map: fp32 on the GPU, n < 256, h * w > 196."""
    from htd_amd import mmcv_ops as M
    from htd_amd.detector.bricks import ConvModule
    m = ConvModule(256, 256, 3, padding=1, norm_cfg=dict(type='GN', num_groups=32)).to(dev)
    big = m(to_dev(torch.randn(2, 256, 50, 84), dev))
    assert type(big.grad_fn).__name__ == 'GroupNormMapFunctionBackward'
    tiles = m(to_dev(torch.randn(70, 256, 7, 7), dev))
    assert type(tiles.grad_fn).__name__ == 'GroupNormReLUFunctionBackward'
    # a shape the map kernels refuse (C < 64) stays where it ran before
    small = ConvModule(32, 32, 3, padding=1, norm_cfg=dict(type='GN', num_groups=8)).to(dev)
    assert type(small(to_dev(torch.randn(2, 32, 20, 20), dev)).grad_fn).__name__ == 'GroupNormReLUFunctionBackward'
    e = torch.empty
    assert not M.use_group_norm_map(e(2, 32, 20, 20, device=dev), 8) and not M.use_group_norm_map(e(2, 96, 20, 20, device=dev), 32)
    assert not M.use_group_norm_map(e(2, 4096, 20, 20, device=dev), 64) and M.use_group_norm_map(e(2, 576, 20, 20, device=dev), 36)
    assert M.use_group_norm_map(e(255, 64, 14, 15, device=dev)) and not M.use_group_norm_map(e(256, 64, 14, 15, device=dev))
    assert not M.use_group_norm_map(e(2, 64, 14, 14, device=dev)) and not M.use_group_norm_map(e(2, 64, 14, 15))
    assert not M.use_group_norm_map(e(2, 64, 14, 15, device=dev, dtype=torch.bfloat16))


def test_map_output_carries_its_maximum_for_an_h2_consumer(dev, h2_state):
    from htd_amd import dense
    from htd_amd import mmcv_ops as M
    h2_state.htd_conv2d_set_h2(1)
    dense.new_step()
    x = to_dev(torch.randn(2, 256, 20, 21), dev).requires_grad_()
    g, b = torch.randn(256, device=dev, requires_grad=True), torch.randn(256, device=dev, requires_grad=True)
    out = M.group_norm_map(x, g, b, 32, EPS, True)
    am = dense.carried_amax(out)
    assert am is not None and float(am) == float(out.detach().abs().max())
    h2_state.htd_conv2d_set_h2(0)
    dense.new_step()
    assert dense.carried_amax(M.group_norm_map(x, g, b, 32, EPS, True)) is None


def ws_formula(w, eps):
    flat = w.reshape(w.size(0), -1)
    return ((flat - flat.mean(1, keepdim=True)) / (flat.std(1, keepdim=True) + eps)).view_as(w)


@pytest.mark.parametrize('Co,K', [(64, 147), (256, 2304), (2048, 512), (7, 5), (1, 4608)])
def test_weight_standardize(dev, Co, K):
    """htd_weight_standardize_fwd / _bwd through mmcv_ops.weight_standardize against the fp64 tensor formula (mmcv-knowledge:
    unbiased std, eps beside the root), under the FLOAT rule with R = ceil(K / 256) <= 18; two runs equal in every bit.  K = 147 is
    the stem's 7 x 7 x 3 row (no 16-byte alignment), 2304 a 3 x 3 x 256 one, K = 5 less than a wavefront, 4608 the longest."""
    from htd_amd import mmcv_ops as M
    gen = torch.Generator().manual_seed(Co * 7 + K)
    w = (torch.randn(Co, K, generator=gen) * 0.05 + 0.01).double().float().double()
    g = torch.randn(Co, K, generator=gen).double()
    w64 = w.clone().requires_grad_()
    o64 = ws_formula(w64, EPS)
    o64.backward(g)
    w32 = w.float().requires_grad_()
    o32 = ws_formula(w32, EPS)
    o32.backward(g.float())
    shape = (Co, 3, 7, 7) if K == 147 else (Co, K // 9, 3, 3) if K % 9 == 0 and K > 9 else (Co, K, 1, 1)
    outs = []
    for _ in range(2):
        wd = w.float().view(Co, *shape[2:], shape[1]).permute(0, 3, 1, 2).to(dev).requires_grad_()       # KRSC memory
        assert wd.is_contiguous(memory_format=torch.channels_last) or K == shape[1]
        od = M.weight_standardize(wd, EPS)
        assert type(od.grad_fn).__name__ == 'WeightStandardizeFunctionBackward'
        od.backward(g.float().view(Co, *shape[2:], shape[1]).permute(0, 3, 1, 2).to(dev))
        outs.append((od.detach().permute(0, 2, 3, 1).reshape(Co, K), wd.grad.permute(0, 2, 3, 1).reshape(Co, K)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    run = -(-K // 256)
    check_float(f'WS Co{Co} K{K} w_hat', outs[0][0], o64.detach(), o32.detach(), run)
    check_float(f'WS Co{Co} K{K} gw', outs[0][1], w64.grad, w32.grad, run)
