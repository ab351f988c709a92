"""tests/glue_ref.py (the float64 references of tests/test_gpu_glue_ops.py) pinned from outside the code under test: against
torch's own operators in float64 where torch has the operation, against the CPU oracle (which the golden fixtures pin to the
reference project), and against the reference's recorded box arithmetic in tests/golden/box_math.npz."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R

D64 = torch.float64


def T(a):
    return torch.from_numpy(np.asarray(a))


def close64(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('n,C,G,h,w', [(3, 576, 36, 7, 7), (2, 64, 64, 3, 3), (1, 64, 32, 5, 9), (0, 16, 4, 7, 7), (2, 32, 4, 10, 12)])
@pytest.mark.parametrize('relu', [True, False])
def test_group_norm_relu_is_torch_group_norm(n, C, G, h, w, relu):
    gen = torch.Generator().manual_seed(C + h)
    x = (torch.randn(n, C, h, w, generator=gen, dtype=D64) + 3).requires_grad_()
    ga, be = torch.randn(C, generator=gen, dtype=D64).requires_grad_(), torch.randn(C, generator=gen, dtype=D64).requires_grad_()
    y, mean, rstd = R.group_norm_relu(x, ga, be, G, 1e-5, relu)
    x2, ga2, be2 = (t.detach().clone().requires_grad_() for t in (x, ga, be))
    ref = F.group_norm(x2, G, ga2, be2, 1e-5)
    ref = F.relu(ref) if relu else ref
    close64(y, ref)
    xg = x.detach().reshape(n, G, C // G * h * w)
    if n:
        close64(mean, xg.mean(2))
        close64(rstd, (xg.var(2, unbiased=False) + 1e-5).rsqrt())
    assert mean.shape == rstd.shape == (n, G)
    go = torch.randn(y.shape, generator=gen, dtype=D64)
    y.backward(go)
    ref.backward(go)
    for a, b in ((x, x2), (ga, ga2), (be, be2)):
        close64(a.grad, b.grad)


def test_fuse_global_is_the_oracle():
    from oracle import detector as D
    gen = torch.Generator().manual_seed(5)
    n, C, B = 23, 12, 3
    x, e = torch.randn(n, C, 7, 7, generator=gen, dtype=D64), torch.randn(n, C, 7, 7, generator=gen, dtype=D64)
    g = torch.randn(B, C, 1, 1, generator=gen, dtype=D64)
    rois = torch.cat([torch.randint(0, B, (n, 1), generator=gen).double(), torch.rand(n, 4, generator=gen, dtype=D64)], 1)
    assert torch.equal(R.fuse_global(x, rois, g), D.fuse_global(x, g, rois))
    assert torch.equal(R.fuse_global(x, rois, g, e, 0.5), D.fuse_global(x, g, rois) + 0.5 * e)
    both = R.plain_and_fused(x, rois, g)
    assert torch.equal(both[:n], x) and torch.equal(both[n:], D.fuse_global(x, g, rois))
    assert R.fuse_global(x[:0], rois[:0], g).shape == (0, C, 7, 7)


@pytest.mark.parametrize('edge', [0, 1, 2, 4])
def test_ba_fuse_is_the_oracle_extractor(edge):
    """The oracle's BA extractor end to end against glue_ref.ba_fuse fed with the per-level tiles and attention logits recomputed
    by the oracle's own operators; edge = 0 and edge = 4 (more than half of 7) keep the whole P2 tile in both."""
    from oracle import detector as D
    from oracle import ops
    gen = torch.Generator().manual_seed(edge)
    C, n, pre = 8, 11, 'ba.'
    strides = (4, 8, 16, 32)
    feats = [torch.randn(2, C, 128 // s, 160 // s, generator=gen) for s in strides]
    sd = {pre + 'conv1.weight': torch.randn(4, C, 1, 1, generator=gen), pre + 'conv1.bias': torch.randn(4, generator=gen),
          pre + 'conv2.weight': torch.randn(1, 4, 1, 1, generator=gen) * 3, pre + 'conv2.bias': torch.randn(1, generator=gen)}
    xy = torch.rand(n, 2, generator=gen) * torch.tensor([100., 80.])
    wh = torch.rand(n, 2, generator=gen) * 60 + 4
    rois = torch.cat([torch.randint(0, 2, (n, 1), generator=gen).float(), xy, xy + wh], 1)
    out = D.ba_extract(sd, feats, rois, strides, edge=edge, prefix=pre)
    lvl, att = [], []
    for f, s in zip(feats, strides):
        t = ops.roi_align(f, rois, 7, 1.0 / s, 0, True)
        a = torch.tanh(F.conv2d(F.adaptive_avg_pool2d(t, 1), sd[pre + 'conv1.weight'], sd[pre + 'conv1.bias']))
        att.append(F.conv2d(a, sd[pre + 'conv2.weight'], sd[pre + 'conv2.bias']).reshape(n))
        lvl.append(t)
    mine = R.ba_fuse(torch.stack(att).double(), [t.double() for t in lvl], lvl[0].double(), edge)
    torch.testing.assert_close(mine, out.double(), rtol=1e-5, atol=1e-5)           # the oracle's sum runs in fp32
    if edge in (0, 4):
        w = torch.stack(att).double().softmax(0)
        whole = sum(w[l].view(n, 1, 1, 1) * lvl[l].double() for l in range(4)) + lvl[0].double()
        close64(mine, whole)


def test_ba_fuse_ring_is_the_reference_slice():
    ones = torch.ones(1, 1, 5, 9, dtype=D64)
    zero_att = torch.zeros(1, 1, dtype=D64)
    for edge, kept in ((0, 45), (1, 45 - 3 * 7), (2, 45 - 1 * 5), (3, 45), (4, 45), (9, 45)):
        ring = R.ba_fuse(zero_att, [torch.zeros_like(ones)], ones, edge)
        assert int(ring.sum()) == kept, (edge, int(ring.sum()))
    assert int(R.ba_fuse(zero_att, [torch.zeros(1, 1, 1, 1, dtype=D64)], torch.ones(1, 1, 1, 1, dtype=D64), 1).sum()) == 1


@pytest.mark.parametrize('h,w', [(1, 1), (1, 7), (3, 3), (7, 7), (14, 14)])
def test_global_avg_pool_is_adaptive_avg_pool(h, w):
    x = torch.randn(3, 6, h, w, generator=torch.Generator().manual_seed(h * w), dtype=D64).requires_grad_()
    x2 = x.detach().clone().requires_grad_()
    a, b = R.global_avg_pool(x), F.adaptive_avg_pool2d(x2, 1)
    close64(a, b)
    go = torch.randn(a.shape, generator=torch.Generator().manual_seed(1), dtype=D64)
    a.backward(go)
    b.backward(go)
    close64(x.grad, x2.grad)


@pytest.mark.parametrize('Co,Ci,k', [(1, 4, 1), (33, 24, 3), (7, 20, 1)])
def test_bn_fold_is_eval_batchnorm_behind_a_convolution(Co, Ci, k):
    gen = torch.Generator().manual_seed(Co)
    w = torch.randn(Co, Ci, k, k, generator=gen, dtype=D64)
    bn = torch.nn.BatchNorm2d(Co).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(Co, generator=gen, dtype=D64))
        bn.bias.copy_(torch.randn(Co, generator=gen, dtype=D64))
        bn.running_mean.copy_(torch.randn(Co, generator=gen, dtype=D64))
        bn.running_var.copy_(torch.rand(Co, generator=gen, dtype=D64) + 0.1)
        bn.running_var[0] = 0.0
    x = torch.randn(2, Ci, 9, 11, generator=gen, dtype=D64)
    wf, bf, wT = R.bn_fold(w, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    torch.testing.assert_close(F.conv2d(x, wf, bf, padding=k // 2), bn(F.conv2d(x, w, None, padding=k // 2)), rtol=1e-10, atol=1e-10)
    # the flipped image is the weight of the data gradient written as a convolution of the output gradient
    gy = torch.randn(2, Co, 9, 11, generator=gen, dtype=D64)
    gx = torch.nn.grad.conv2d_input(x.shape, wf, gy, padding=k // 2)
    wd = wT.reshape(Ci, k, k, Co).permute(0, 3, 1, 2)            # [ci][co][r][s] of the flipped taps
    close64(F.conv2d(gy, wd, None, padding=k // 2), gx)
    assert wT.shape == (Ci, k * k, Co) and torch.equal(wT[2 % Ci, k * k - 1, Co - 1], wf[Co - 1, 2 % Ci, 0, 0])


@pytest.mark.parametrize('mom,wd,gscale', [(0.9, 1e-4, 1.0), (0.0, 1e-4, 1.0), (0.9, 0.0, 1.0), (0.5, 0.25, 0.125)])
def test_sgd_momentum_is_torch_sgd(mom, wd, gscale):
    gen = torch.Generator().manual_seed(3)
    p, m = torch.randn(101, generator=gen, dtype=D64), torch.randn(101, generator=gen, dtype=D64)
    pt = p.clone().requires_grad_()
    opt = torch.optim.SGD([pt], lr=0.02, momentum=mom, weight_decay=wd)
    if mom:
        opt.state[pt]['momentum_buffer'] = m.clone()          # a non-zero start momentum
    for step in range(3):
        g = torch.randn(101, generator=gen, dtype=D64)
        pt.grad = g * gscale
        for grp in opt.param_groups:
            grp['lr'] = 0.02 / (step + 1)
        opt.step()
        p, m = R.sgd_momentum(p, g, m, 0.02 / (step + 1), mom, wd, gscale)
        close64(p, pt.detach())


def test_coders_reproduce_the_recorded_reference_answers(golden):
    """The arrays and tolerances of tests/test_oracle_golden.py::test_box_math."""
    g = golden('box_math')
    b1, b2, rnd = T(g['b1']).double(), T(g['b2']).double(), T(g['rnd']).double()
    stds = (0.1, 0.1, 0.2, 0.2)
    lim = torch.tensor([[90., 80.]], dtype=D64)
    dec = R.delta2bbox_clip(b1, rnd, (0., 0., 0., 0.), stds, lim)
    torch.testing.assert_close(dec.float(), T(g['dec']), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(R.delta2bbox_clip(b1, rnd * 10, (0., ) * 4, (1., ) * 4).float(), T(g['dec_noclip']), rtol=1e-6, atol=1e-4)
    kat = R.delta2bbox_clip(T(g['kat_rois']).double(), T(g['kat_deltas']).double(), (0., ) * 4, (1., ) * 4,
                            torch.tensor([[32., 32.]], dtype=D64))
    torch.testing.assert_close(kat.float(), T(g['kat_dec']), rtol=1e-6, atol=1e-6)
    expected = torch.tensor([[0.0000, 0.0000, 1.0000, 1.0000], [0.1409, 0.1409, 2.8591, 2.8591],         # delta_xywh_bbox_coder.py:166-169
                             [0.0000, 0.3161, 4.1945, 0.6839], [5.0000, 5.0000, 5.0000, 5.0000]])
    torch.testing.assert_close(kat.float(), expected, rtol=0, atol=1e-4)
    n = 9
    labels, lw, bt, bw = R.roi_targets(b1[:n], b2, torch.arange(n) + 1, torch.ones(n), torch.ones(n), 80, (0., ) * 4, stds)
    torch.testing.assert_close(bt.float(), T(g['deltas']), rtol=1e-6, atol=1e-6)
    assert labels.tolist() == list(range(1, 10)) and bool((lw == 1).all()) and bool((bw == 1).all())


def test_coders_rows_images_and_slots():
    from oracle import boxes as B
    gen = torch.Generator().manual_seed(8)
    n = 12
    xy = torch.rand(n, 2, generator=gen, dtype=D64) * 100
    rois = torch.cat([xy, xy + torch.rand(n, 2, generator=gen, dtype=D64) * 80 + 1], 1)
    deltas = torch.randn(n, 4, generator=gen, dtype=D64) * 3
    means, stds = (0.1, -0.2, 0.05, 0.0), (0.1, 0.1, 0.2, 0.2)
    lim = torch.tensor([[90., 80.], [50., 120.], [200., 30.]], dtype=D64)
    keep = torch.ones(n, dtype=torch.uint8)
    keep[[2, 7]] = 0
    out = R.delta2bbox_clip(rois, deltas, means, stds, lim, keep, 4)
    for b in range(3):                     # image by image through the oracle's coder (max_shape = (H, W))
        rows = slice(4 * b, 4 * b + 4)
        ref = B.delta2bbox(rois[rows], deltas[rows], means, stds, max_shape=(float(lim[b, 1]), float(lim[b, 0])))
        ref = ref * keep[rows].double().view(4, 1)
        close64(out[rows], ref)
    assert bool((out[2] == 0).all()) and bool((out[7] == 0).all())
    gts = torch.cat([xy + 3, xy + 50], 1)
    pos = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0], dtype=torch.uint8)
    valid = torch.tensor([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], dtype=torch.uint8)
    gl = torch.randint(0, 80, (n, ), generator=gen)
    labels, lw, bt, bw = R.roi_targets(rois, gts, gl, pos, valid, 80, means, stds)
    # (the oracle's encoder casts its operands to fp32, as the reference's does, :98-99)
    torch.testing.assert_close(bt[pos.bool()].float(), B.bbox2delta(rois[pos.bool()], gts[pos.bool()], means, stds), rtol=1e-5, atol=1e-5)
    assert bool((bt[~pos.bool()] == 0).all()) and torch.equal(bw, pos.double().view(n, 1).expand(n, 4))
    assert torch.equal(labels, torch.where(pos.bool(), gl, torch.tensor(80))) and torch.equal(lw, valid.double())


def test_metric_and_bound():
    ref = torch.tensor([1.0, -4.0], dtype=D64)
    assert R.rel_err(torch.tensor([1.0, -3.0]), ref) == 0.25
    assert R.rel_err(torch.zeros(0), torch.zeros(0, dtype=D64)) == 0.0
    assert R.rel_err(torch.zeros(3), torch.zeros(3, dtype=D64)) == 0.0 and R.rel_err(torch.ones(3), torch.zeros(3, dtype=D64)) == float('inf')
    assert R.float_bound(0.0, 49) == 8 * 2.0 ** -23 and R.float_bound(1e-6, 4200) == 4200 ** 0.5 * 1e-6
