"""htd_rpn_loss and htd_rpn_loss_l1 (rpn_loss_kernel<false> / <true> of csrc/box_ops.hip) through the C ABI against
pgraph_ref.rpn_loss in float64 (pinned to torch's loss operators and the project's coder by tests/test_pgraph_ref.py), with
gradients from autograd.  Every output buffer goes in filled with NaN; cls holds NaN on the rows that are not sampled and reg on
the rows that are not positive, since the kernel has no reason to read them.

The kernel runs on a fixed grid of 1024 blocks x 256 threads = 262 144 threads that stride over the B x A anchor rows:
  A = 100      200 rows: block 0 alone has work, the other 1023 blocks must still write zero partials
  A = 131 149  262 298 rows: the grid wraps, the first 154 threads take a second row (production: B x 268 569 anchors)
B = 2 images, K = 3 gts.  About 1 % of the rows are positive and 5 % negative, a few are flagged both (counted once, as positives);
logits reach +-60; pos_weight -1 (off) and 2.5; beta 1 / 9 and 1.0; stds (1, 1, 1, 1) and (0.1, 0.1, 0.2, 0.2), means 0.  Several
anchors equal their gt with reg 0: target and difference are exactly 0, so grad_reg must be exactly 0 under both losses.  Elsewhere
reg = the float64 target + s with 0.01 <= |s| and |s| further than 1e-3 from both betas, so fp32 and fp64 agree on the sign and on
the branch of every component; under L1 the gradient on the positives is then the reference's sign exactly.

FLOAT checks: the rule of tests/test_gpu_glue_ops.py, e = max |out - ref64| / max |ref64| <= F x max(e_cpu, 2^-23), F = max(8, sqrt(R)).
R, counted from rpn_loss_kernel: a thread adds one BCE term per row it takes and the four box components of a positive row one after
the other, so at most 2 (cls) and 2 x 4 = 8 (box) terms at A = 131 149, 1 and 4 at A = 100; then six shuffle steps, four waves, and
the 1024 partials go through torch's blocked sum as in _RPNLossFunction.  F = 8 either way.  The gradients are one expression per
element: R = 1.  Every float check prints e, e_cpu, R, the bound and their ratio before it asserts."""
import pytest
import torch

import pgraph_ref as R

pytestmark = pytest.mark.gpu
D64 = torch.float64
NAN = float('nan')
B, K = 2, 3
BETAS = (1. / 9., 1.0)
# beta (None: L1), pos_weight, stds
CASES = [(BETAS[0], -1., (1., 1., 1., 1.)), (BETAS[1], 2.5, (0.1, 0.1, 0.2, 0.2)), (None, -1., (0.1, 0.1, 0.2, 0.2)), (None, 2.5, (1., 1., 1., 1.))]
MEANS = (0., 0., 0., 0.)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return torch.device('cuda:0')


def make_inputs(A):
    """Everything but reg (which depends on the stds): fp32 values held in float64."""
    gen = torch.Generator().manual_seed(A)
    gc = torch.rand(B, K, 2, generator=gen, dtype=D64) * 400 + 100
    gwh = torch.rand(B, K, 2, generator=gen, dtype=D64) * 120 + 24
    gts = torch.cat([gc - gwh / 2, gc + gwh / 2], -1).float().double()
    c = torch.rand(A, 2, generator=gen, dtype=D64) * 600
    wh = torch.rand(A, 2, generator=gen, dtype=D64) * 100 + 16
    anchors = torch.cat([c - wh / 2, c + wh / 2], 1)
    u = torch.rand(B, A, generator=gen)
    pos, neg = u < 0.01, (u >= 0.009) & (u < 0.06)                  # 0.009 <= u < 0.01: flagged both
    pos[0, 0] = pos[0, 3] = pos[1, A - 1] = pos[0, 5] = neg[0, 5] = True
    pos[1] &= ~pos[0]                                               # an anchor is positive in one image at most (its gt is near it)
    assert int((pos & neg).sum()) > 0 and int(pos.sum()) >= 4
    assigned = torch.where(pos, torch.randint(1, K + 1, (B, A), generator=gen), torch.randint(-1, 1, (B, A), generator=gen))
    b_idx, a_idx = pos.nonzero(as_tuple=True)
    g = gts[b_idx, assigned[pos] - 1]
    gsz = torch.cat([g[:, 2:] - g[:, :2]] * 2, 1)
    anchors[a_idx] = g + (torch.rand(g.shape, generator=gen, dtype=D64) - 0.5) * 0.3 * gsz      # a positive's anchor lies near its gt
    same = torch.arange(0, a_idx.numel(), 2)[:8]                                                # several anchors ARE their gt
    anchors[a_idx[same]] = g[same]
    anchors = anchors.float().double()
    cls = torch.randn(B, A, generator=gen, dtype=D64) * 5
    sampled = (pos | neg).nonzero(as_tuple=False)
    for (b_, a_), v in zip(sampled[[1, 2, -2, -1]].tolist(), (60., -60., 59.5, -60.)):
        cls[b_, a_] = v
    cls[0, 0], cls[1, A - 1] = 60., -60.                             # a positive at each end of the range
    cls[~(pos | neg)] = NAN
    cls = cls.float().double()
    # |s| in [0.01, 2), at least 2e-3 away from both betas (1e-3 asked, the rest for the fp32 rounding of reg), random sign
    mag = torch.rand(B, A, 4, generator=gen, dtype=D64) * 1.99 + 0.01
    for beta in BETAS:
        near = (mag - beta).abs() < 2e-3
        mag = torch.where(near, mag + 4e-3, mag)
    s = mag * (torch.randint(0, 2, (B, A, 4), generator=gen) * 2 - 1)
    is_same = torch.zeros(B, A, dtype=torch.bool)
    is_same[b_idx[same], a_idx[same]] = True
    return dict(A=A, gts=gts, anchors=anchors, pos=pos, neg=neg, assigned=assigned, cls=cls, s=s, is_same=is_same)


_INPUTS = {}


def inputs(A, stds):
    if A not in _INPUTS:
        _INPUTS[A] = make_inputs(A)
    d = dict(_INPUTS[A])
    pos = d['pos']
    tgt = R.rpn_targets(d['anchors'], d['gts'], d['assigned'], pos) / torch.tensor(stds, dtype=D64)
    reg = torch.full((B, A, 4), NAN, dtype=D64)
    reg[pos] = torch.where(d['is_same'][pos][:, None], torch.zeros_like(tgt), tgt + d['s'][pos])
    d['reg'] = reg.float().double()
    return d


def reference(d, stds, beta, pos_weight, dtype):
    cls, reg = d['cls'].to(dtype).clone().requires_grad_(), d['reg'].to(dtype).clone().requires_grad_()     # copies: the inputs are shared
    s_cls, s_box = R.rpn_loss(cls, reg, d['anchors'].to(dtype), d['gts'].to(dtype), d['assigned'], d['pos'], d['neg'], MEANS, stds, beta,
                              pos_weight)
    g_cls, = torch.autograd.grad(s_cls, cls)
    g_reg, = torch.autograd.grad(s_box, reg)
    return s_cls.detach(), s_box.detach(), g_cls, g_reg


def launch(dev, t, stds, beta, pos_weight, A=None, Kn=K, null=None):
    """t: the device tensors in ABI order -> partial, grad_cls, grad_reg (NaN-filled before the call)"""
    from htd_amd import capi
    from htd_amd.core.bbox import _f4
    A = t['cls'].size(1) if A is None else A
    out = [torch.full((capi.lib().htd_rpn_loss_partial_rows(), 2), NAN, device=dev), torch.full((B, A), NAN, device=dev),
           torch.full((B, A, 4), NAN, device=dev)]
    ptrs = [capi.ptr(t[k]) for k in ('cls', 'reg', 'anchors', 'gts', 'assigned', 'pos', 'neg')] + [_f4(MEANS), _f4(stds)] + \
        [capi.ptr(o) for o in out]
    if null is not None:
        ptrs[null] = None
    head, tail = ptrs[:7] + [B, A, Kn] + ptrs[7:9], ptrs[9:] + [capi.current_stream_ptr()]
    if beta is None:
        capi.call('htd_rpn_loss_l1', *head, pos_weight, *tail)
    else:
        capi.call('htd_rpn_loss', *head, beta, pos_weight, *tail)
    return out


def device_tensors(d, dev):
    t = {k: d[k].float().to(dev).contiguous() for k in ('cls', 'reg', 'anchors', 'gts')}
    t['assigned'] = d['assigned'].to(dev)
    t['pos'], t['neg'] = d['pos'].to(torch.uint8).to(dev), d['neg'].to(torch.uint8).to(dev)
    return t


@pytest.mark.parametrize('beta,pos_weight,stds', CASES)
@pytest.mark.parametrize('A', [100, 131149])
def test_rpn_loss(dev, A, beta, pos_weight, stds):
    d = inputs(A, stds)
    pos, sampled = d['pos'], d['pos'] | d['neg']
    s_cls, s_box, g_cls, g_reg = reference(d, stds, beta, pos_weight, D64)
    c_cls, c_box, cg_cls, cg_reg = reference(d, stds, beta, pos_weight, torch.float32)
    t = device_tensors(d, dev)
    partial, gcls, greg = launch(dev, t, stds, beta, pos_weight)
    again = launch(dev, t, stds, beta, pos_weight)
    sums = partial.sum(0).cpu()                                      # the reduction of _RPNLossFunction.forward
    for x, y in zip((partial, gcls, greg), again):
        assert torch.equal(x, y), 'two runs differ'
    partial, gcls, greg = partial.cpu(), gcls.cpu(), greg.cpu()
    assert torch.isfinite(partial).all() and torch.isfinite(gcls).all() and torch.isfinite(greg).all(), 'entries the kernel did not write'
    if B * A <= 256:
        assert float(partial[1:].abs().sum()) == 0.0                 # blocks without rows
    wraps = B * A > 1024 * 256
    name = f'rpn_loss{"_l1" if beta is None else ""} A={A} beta={beta} pw={pos_weight}'
    R.check_float(name + ' sum_cls', sums[0], s_cls, c_cls, 2 if wraps else 1)
    R.check_float(name + ' sum_box', sums[1], s_box, c_box, 8 if wraps else 4)
    assert float(gcls[~sampled].abs().sum()) == 0.0
    assert float(greg[~pos].abs().sum()) == 0.0
    assert int(d['is_same'].sum()) >= 3 and float(greg[d['is_same']].abs().sum()) == 0.0
    R.check_float(name + ' grad_cls', gcls, g_cls, cg_cls, 1)
    if beta is None:
        assert torch.equal(greg[pos], g_reg[pos].float())           # -1, 0 or 1
        assert set(g_reg[pos].unique().tolist()) == {-1.0, 0.0, 1.0}
    else:
        R.check_float(name + ' grad_reg', greg, g_reg, cg_reg, 1)


def test_rpn_loss_rejects_bad_arguments(dev):
    from htd_amd import capi
    d = inputs(100, CASES[0][2])
    t = device_tensors(d, dev)
    with pytest.raises(ValueError):
        launch(dev, t, CASES[0][2], 0.0, -1.)                        # beta = 0 for the smooth form
    for beta in (1.0, None):
        with pytest.raises(ValueError):
            launch(dev, t, CASES[0][2], beta, -1., Kn=0)
        for k in range(12):
            with pytest.raises(ValueError, match='null pointer'):
                launch(dev, t, CASES[0][2], beta, -1., null=k)
    assert capi.lib().htd_last_error()
    torch.cuda.synchronize()
