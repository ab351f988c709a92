"""The ordering rules of the weight-gradient stream (dense._wgrad_raw, bricks._BNFold / _BNFoldMany) and the address-keyed
registries of dense.py / bricks.py, each tested directly on small layers.

Part A.  Every case runs forward + backward twice from identical inputs: first with dense.overlap_wgrad(True) while ONE of the
two streams is late (a bounded run of dense torch.mm launches queued on it immediately before backward()), then with
dense.overlap_wgrad(False).  Every gradient of the two runs is compared with torch.equal -- the claim of
test_weight_gradient_stream_gives_identical_step, here without a Trainer whose flat-buffer sinks hide a late side stream --
and the single-stream run against an fp64 autograd reference of the same layers, so that the two cannot be equal and both wrong.
late='side' shows a missing main.wait_stream(side): the consumer on the main stream is reached while the producer has not
started.  late='main' shows a missing side.wait_stream(main): the side stream reads a gradient map that the main stream has
not written.  A race reads whatever the recycled block holds, so the overlapped run goes FIRST, after NaN has been written
over more free memory of both allocator pools than the case's gradients take, and every case has its own seed.

The delay (DELAY_LAUNCHES launches of a DELAY_N^3 fp32 product) is far longer than the backward of the largest case; both
numbers are measured in DESIGN.md ("The weight-gradient stream and the address-keyed registries, tested directly") and
test_delay_outlasts_the_largest_backward holds the ratio.

Tolerance against fp64: rtol 1e-4 and atol 2e-5 x rms(reference).  test_conv2d_fwd_bwd allows 2e-5 x sqrt(terms) on sums of
unit-variance products, i.e. 2e-5 x the rms of the result; the cases here compose layers (standardised or folded weights, a
residual stage), so the scale is taken from the reference itself instead of the term count.

Parts B and C.  An entry of a registry keyed by data_ptr() is served only to the tensor it was made for: a NEW tensor at the
address of a dead one misses.  Slot makes such an address: a free block of an odd size between two live tensors, the only free
block of its size, so that the next allocation of that byte count is an exact best fit there (reborn()).
"""
import copy
import gc
import weakref

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DEV = 'cuda:0'
B, H, W = 2, 12, 14
EPS = 1e-5
DELAY_N, DELAY_LAUNCHES = 4096, 96
ODD_SHAPE = (72, 40, 3, 3)          # 103 680 bytes: no other weight, map or buffer of the suite has this size


# ---------------------------------------------------------------------------------------------------- the two tools
_SCRATCH = {}


def delay(stream, launches=DELAY_LAUNCHES):
    """Queue a bounded amount of ordinary work on `stream`: dense products into a scratch tensor."""
    if 'a' not in _SCRATCH:
        _SCRATCH['a'] = torch.full((DELAY_N, DELAY_N), 1.0 / DELAY_N, device=DEV)
        _SCRATCH['out'] = torch.empty(DELAY_N, DELAY_N, device=DEV)
        from htd_amd import dense
        for s in (torch.cuda.current_stream(), dense.side_stream(DEV)):       # the first product on a stream sets its handle up
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                torch.mm(_SCRATCH['a'], _SCRATCH['a'], out=_SCRATCH['out'])
        torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(launches):
            torch.mm(_SCRATCH['a'], _SCRATCH['a'], out=_SCRATCH['out'])


def poison(nbytes):
    """NaN over free memory of both allocator pools (blocks of 1 MiB belong to the small pool), then free it again."""
    nan = float('nan')
    small = [torch.full((1 << 18, ), nan, device=DEV) for _ in range(max(8, 4 * nbytes // (1 << 20) + 1))]
    large = torch.full((max(4 * nbytes, 1 << 23) // 4, ), nan, device=DEV)
    torch.cuda.synchronize()
    del small, large


def reborn(ptr, shape):
    """A NEW tensor at the address `ptr` of a tensor of this shape that the caller has just dropped.  A miss is kept alive and
    the allocation repeated, eight times at the most; no hit is a failed precondition, never a skip."""
    misses = []
    for _ in range(8):
        z = torch.empty(shape, device=DEV, memory_format=CL) if len(shape) == 4 else torch.empty(shape, device=DEV)
        if z.data_ptr() == ptr:
            return z
        misses.append(z)
    pytest.fail(f'precondition not met: the allocator never handed out the freed address again ({len(misses)} allocations)')


def hole(shape=ODD_SHAPE, n=24, most=480):
    """-> (address, guards): a FREE block of exactly this tensor's size between two live tensors (so it cannot merge with a free
    neighbour), and the only free block of its size: the allocations fill every older one first.  n at a time, until three
    lie side by side: where the earlier tests of a run left the pool with many free blocks of about this size, each of the first
    allocations lands in a block of its own, and only the ones after them are cut from one larger block in a row."""
    vs, first = [], 1
    while len(vs) < most:
        vs += [victim(shape) for _ in range(n)]
        step = (vs[0].numel() * 4 + 511) // 512 * 512
        for i in range(first, len(vs) - 1):
            if vs[i].data_ptr() - vs[i - 1].data_ptr() == step and vs[i + 1].data_ptr() - vs[i].data_ptr() == step:
                print(f'hole: three adjacent blocks after {len(vs)} allocations')
                ptr = vs[i].data_ptr()
                vs[i] = None
                return ptr, vs
        first = len(vs) - 1
    pytest.fail(f'precondition not met: no three adjacent blocks among {len(vs)} allocations')


class Slot:
    """An address that the allocator hands out again: take() -> a new tensor there, once the previous tenant has died."""

    def __init__(self, shape=ODD_SHAPE):
        self.shape = shape
        self.ptr, self.guards = hole(shape)

    def take(self):
        return reborn(self.ptr, self.shape).normal_()


def victim(shape=ODD_SHAPE):
    t = torch.empty(shape, device=DEV, memory_format=CL) if len(shape) == 4 else torch.empty(shape, device=DEV)
    return t.normal_()


# ---------------------------------------------------------------------------------------------------- one program, two arithmetics
class DevOps:
    """The layers under test."""

    def __init__(self, ws=None):
        self._ws = ws

    def conv(self, x, w, b=None, pad=0, relu=False, res=None):
        from htd_amd import dense
        return dense.conv2d(x, w, b, 1, pad, 1, relu, res)

    def ws(self, w):
        from htd_amd import mmcv_ops as M
        return M.weight_standardize(w, EPS) if self._ws is None else self._ws(w)

    def fold(self, w, gamma, beta, mean, var):
        from htd_amd.detector import bricks
        bn = nn.BatchNorm2d(w.size(0), eps=EPS).eval()
        bn.weight, bn.bias, bn.running_mean, bn.running_var = gamma, beta, mean, var
        return bricks.frozen_bn_fold(w, bn)

    def head(self, x, w1, b1, w2, b2):
        from htd_amd import dense
        return dense.conv_relu_head(x, w1, b1, w2, b2, 1)

    def merged(self, parts):
        from htd_amd import dense
        t = torch.cat(parts)
        dense.temp_grad_sink(t)
        return t


class RefOps:
    """The same layers as plain tensor formulas (run in fp64 on the CPU, differentiated by autograd)."""

    def conv(self, x, w, b=None, pad=0, relu=False, res=None):
        y = F.conv2d(x, w, b, 1, pad)
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    def ws(self, w):
        flat = w.flatten(1)
        return ((flat - flat.mean(1, keepdim=True)) / (flat.std(1, keepdim=True) + EPS)).reshape(w.shape)

    def fold(self, w, gamma, beta, mean, var):
        s = gamma * torch.rsqrt(var + EPS)
        return w * s.view(-1, 1, 1, 1), beta - mean * s

    def head(self, x, w1, b1, w2, b2):
        return F.conv2d(F.relu(F.conv2d(x, w1, b1, 1, 1)), w2, b2)

    def merged(self, parts):
        return torch.cat(parts)


class Case:
    """make(R) -> dict of fp32 CPU tensors (R(*shape): standard normal); prog(ops, t) -> [(output, name of its gradient)].
    const: inputs without a gradient; flat: the parameters registered in a runner.FlatParams (None: no FlatParams)."""

    def __init__(self, name, make, prog, const=(), flat=None):
        self.name, self.make, self.prog, self.const, self.flat = name, make, prog, tuple(const), flat

    def data(self, seed):
        g = torch.Generator().manual_seed(seed)
        return self.make(lambda *s: torch.randn(*s, generator=g))

    def is_leaf(self, k):
        return not k.startswith('gy') and k not in self.const

    def leaves(self, d):
        t = {}
        for k, v in d.items():
            v = v.to(DEV)
            v = v.contiguous(memory_format=CL) if v.dim() == 4 else v
            t[k] = v.requires_grad_() if (self.is_leaf(k) and k.startswith('x')) else (nn.Parameter(v) if self.is_leaf(k) else v)
        return t

    def reference(self, d):
        t = {k: v.double().requires_grad_(self.is_leaf(k)) for k, v in d.items()}
        outs = self.prog(RefOps(), t)
        torch.autograd.backward([y for y, _ in outs], [t[g] for _, g in outs])
        return {k: v.grad for k, v in t.items() if self.is_leaf(k)}


def once(case, d, overlap, late=None, ops=None, before=None):
    """One forward + backward of `case` on the device -> {name: gradient}.  The gradients are read on the main stream in stream
    order, as an optimizer would (after dense.join_side_stream() where a FlatParams owns them): nothing synchronises the device
    between backward() and the read."""
    from htd_amd import dense
    from htd_amd.runner import FlatParams
    dense.new_step()
    t = case.leaves(d)
    fp = None
    if case.flat is not None:
        holder = nn.Module()
        for k in case.flat:
            holder.register_parameter(k, t[k])
        fp = FlatParams(holder)
        fp.zero_grad()
    try:
        with dense.overlap_wgrad(overlap):
            if before is not None:
                before()
            outs = case.prog(ops or DevOps(), t)
            torch.cuda.synchronize()
            if late is not None:
                delay(dense.side_stream(DEV) if late == 'side' else torch.cuda.current_stream())
            torch.autograd.backward([y for y, _ in outs], [t[g] for _, g in outs])
            if fp is not None:
                dense.join_side_stream()
                fp.collect()
            grads = {k: v.grad.clone() for k, v in t.items() if case.is_leaf(k)}
        torch.cuda.synchronize()
    finally:
        if fp is not None:
            fp.close()
        dense.new_step()
    return grads


def assert_close_to_fp64(got, ref, what):
    assert set(got) == set(ref)
    for k in ref:
        rms = float(ref[k].pow(2).mean().sqrt())
        torch.testing.assert_close(got[k].cpu().double(), ref[k], rtol=1e-4, atol=2e-5 * rms, msg=lambda m: f'{what} {k}: {m}')


def pair(case, seed, late, ops=None, before=None):
    """The overlapped run with one stream late (first, over poisoned memory), the single-stream run, bit equality, fp64."""
    once(case, case.data(seed + 5000), True)        # nobody looks at this one: it loads every kernel of the case, so that no
    d = case.data(seed)                             # first-launch set-up orders the two streams by accident
    poison(sum(v.numel() * 4 for v in d.values()))
    got = once(case, d, True, late, ops=ops, before=before)
    ref = once(case, d, False)
    for k in ref:
        assert torch.equal(got[k], ref[k]), \
            f'{case.name}, late={late}: gradient of {k} differs from the single-stream run ' \
            f'({int((got[k] != ref[k]).sum())} of {ref[k].numel()} elements, {int(torch.isnan(got[k]).sum())} NaN)'
    assert_close_to_fp64(ref, case.reference(d), case.name)
    return got


def _scaled(R, Co, Ci, k):
    return R(Co, Ci, k, k) / (Ci * k * k) ** 0.5


def _plain(Ci, Co, k):
    return Case(f'plain{k}x{k}',
                lambda R: dict(x=R(B, Ci, H, W), w=_scaled(R, Co, Ci, k), b=R(Co), gy=R(B, Co, H, W)),
                lambda ops, t: [(ops.conv(t['x'], t['w'], t['b'], k // 2, True), 'gy')])


def _ws(Ci, Co, k):
    return Case(f'ws{k}x{k}',
                lambda R: dict(x=R(B, Ci, H, W), w=_scaled(R, Co, Ci, k), b=R(Co), gy=R(B, Co, H, W)),
                lambda ops, t: [(ops.conv(t['x'], ops.ws(t['w']), t['b'], k // 2, True), 'gy')])


def _bn_stats(R, Co):
    return dict(gamma=R(Co).abs() + 0.5, beta=0.1 * R(Co), mean=0.1 * R(Co), var=R(Co).abs() + 0.5)


def _fold(Ci, Co, k, flat):
    def prog(ops, t):
        wf, bf = ops.fold(t['w'], t['gamma'], t['beta'], t['mean'], t['var'])
        return [(ops.conv(t['x'], wf, bf, k // 2, True), 'gy')]
    return Case(f'fold{k}x{k}' + ('-flat' if flat else ''),
                lambda R: dict(x=R(B, Ci, H, W), w=_scaled(R, Co, Ci, k), gy=R(B, Co, H, W), **_bn_stats(R, Co)),
                prog, const=('mean', 'var'), flat=('w', 'gamma', 'beta') if flat else None)


def _head(Ci, Cm, Co):
    return Case('head',
                lambda R: dict(x=R(B, Ci, H, W), w1=_scaled(R, Cm, Ci, 3), b1=R(Cm), w2=_scaled(R, Co, Cm, 1), b2=R(Co),
                               gy=R(B, Co, H, W)),
                lambda ops, t: [(ops.head(t['x'], t['w1'], t['b1'], t['w2'], t['b2']), 'gy')])


def _shared(Ci, Co, k, aliased):
    """One weight read on two maps.  Backward runs the node made LAST first: its gradient takes the flat-buffer slice, the other
    one is added there (htd_conv2d_bwd_weight_acc).  aliased: that second launch belongs to a layer with a same-size residual
    that needs a gradient -- it stays on the main stream and has to wait for the first one."""
    def make(R):
        d = dict(xa=R(B, Ci, H, W), xb=R(B, Ci, 9, 11), w=_scaled(R, Co, Ci, k), b=R(Co), gya=R(B, Co, H, W), gyb=R(B, Co, 9, 11))
        if aliased:
            d['xr'] = R(B, Co, H, W)
        return d

    def prog(ops, t):
        ya = ops.conv(t['xa'], t['w'], t['b'], k // 2, False, t.get('xr'))
        yb = ops.conv(t['xb'], t['w'], t['b'], k // 2, False)
        return [(ya, 'gya'), (yb, 'gyb')]
    return Case('shared' + ('-aliased' if aliased else ''), make, prog, flat=('w', 'b'))


def _merged(Ci, Ca, Cb):
    """The RPN's merged head: a non-leaf concatenation of two leaves with a temporary gradient buffer, read on two maps."""
    def prog(ops, t):
        w, b = ops.merged([t['wa'], t['wb']]), ops.merged([t['ba'], t['bb']])
        return [(ops.conv(t['xa'], w, b), 'gya'), (ops.conv(t['xb'], w, b), 'gyb')]
    return Case('merged',
                lambda R: dict(xa=R(B, Ci, H, W), xb=R(B, Ci, 9, 11), wa=_scaled(R, Ca, Ci, 1), wb=_scaled(R, Cb, Ci, 1), ba=R(Ca),
                               bb=R(Cb), gya=R(B, Ca + Cb, H, W), gyb=R(B, Ca + Cb, 9, 11)), prog)


def _residual(Ci, Co, k):
    return Case('residual',
                lambda R: dict(x=R(B, Ci, H, W), w=_scaled(R, Co, Ci, k), b=R(Co), xr=R(B, Co, H, W), gy=R(B, Co, H, W)),
                lambda ops, t: [(ops.conv(t['x'], t['w'], t['b'], k // 2, True, t['xr']), 'gy')])


CASES = [_plain(40, 64, 3), _plain(72, 40, 1), _ws(40, 64, 3), _ws(64, 48, 1), _fold(40, 56, 3, False), _fold(40, 56, 3, True),
         _fold(72, 48, 1, False), _head(40, 56, 16), _shared(40, 48, 3, False), _shared(40, 48, 3, True), _merged(56, 8, 32),
         _residual(40, 48, 3)]


@pytest.mark.parametrize('late', ['side', 'main'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=[c.name for c in CASES])
def test_late_stream_leaves_every_gradient_bit_for_bit(i, late):
    pair(CASES[i], 100 + 2 * i + (late == 'main'), late)


# ---------------------------------------------------------------------------------------------------- case 4: a residual stage
def _stage_reference(layer, x, gy):
    """ResLayer of bottlenecks on running statistics, block by block in fp64."""
    def cb(conv, bn, t):
        y = F.conv2d(t, conv.weight, None, conv.stride, conv.padding, conv.dilation)
        return F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    layer = copy.deepcopy(layer).double()
    x = x.double().requires_grad_()
    t = x
    for blk in layer:
        h = F.relu(cb(blk.conv1, blk.norm1, t))
        h = F.relu(cb(blk.conv2, blk.norm2, h))
        idn = t if blk.downsample is None else cb(blk.downsample[0], blk.downsample[1], t)
        t = F.relu(cb(blk.conv3, blk.norm3, h) + idn)
    t.backward(gy.double())
    return dict({n: p.grad for n, p in layer.named_parameters()}, x=x.grad)


def _stage_once(base, x, gy, overlap, late, flat):
    from htd_amd import dense
    from htd_amd.runner import FlatParams
    dense.new_step()
    layer = copy.deepcopy(base).to(DEV).eval()
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_()
    gyd = gy.to(DEV).contiguous(memory_format=CL)
    fp = FlatParams(layer) if flat else None
    if fp is not None:
        fp.zero_grad()
    try:
        with dense.overlap_wgrad(overlap):
            y = layer(xd)
            assert len(dense._FLIPPED) == 0                        # every offered image was taken by the stage's node
            torch.cuda.synchronize()
            if late is not None:
                delay(dense.side_stream(DEV) if late == 'side' else torch.cuda.current_stream())
            y.backward(gyd)
            if fp is not None:
                dense.join_side_stream()
                fp.collect()
            grads = dict({n: p.grad.clone() for n, p in layer.named_parameters()}, x=xd.grad.clone())
        torch.cuda.synchronize()
    finally:
        if fp is not None:
            fp.close()
        dense.new_step()
    assert len(dense._FLIPPED) == 0
    return grads


@pytest.mark.parametrize('late', ['side', 'main'])
@pytest.mark.parametrize('flat', [False, True], ids=['plain', 'flat'])
def test_late_stream_under_a_fused_residual_stage(flat, late):
    """frozen_bn_fold_many + ResStageFunction + _BNFoldMany.backward: two bottlenecks of 32 mid channels on an 8x10 map."""
    from htd_amd.detector.resnet import Bottleneck, ResLayer
    seed = 300 + 2 * flat + (late == 'main')
    torch.manual_seed(seed)
    base = ResLayer(Bottleneck, 64, 32, 2)
    for m in base.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    base.eval()
    x, gy = torch.randn(B, 64, 8, 10), torch.randn(B, 128, 8, 10)
    _stage_once(base, 2.0 * x, gy, True, None, flat)                   # (loads the kernels, as in pair())
    poison(4 * (x.numel() + gy.numel() + sum(p.numel() for p in base.parameters())))
    got = _stage_once(base, x, gy, True, late, flat)
    ref = _stage_once(base, x, gy, False, None, flat)
    for k in ref:
        assert torch.equal(got[k], ref[k]), f'late={late}: gradient of {k} differs from the single-stream run'
    assert_close_to_fp64(ref, _stage_reference(base, x, gy), 'stage')


# ---------------------------------------------------------------------------------------------------- case 8: where the launch runs
@pytest.fixture
def launches(monkeypatch):
    """[(entry point, ran on the weight-gradient stream)] of every library call made while the fixture lives."""
    from htd_amd import capi, dense
    log, real, side = [], capi.call, dense.side_stream(DEV)

    def spy(name, *args, **kw):
        log.append((name, torch.cuda.current_stream() == side))
        return real(name, *args, **kw)
    monkeypatch.setattr(capi, 'call', spy)
    return log


def test_aliased_residual_keeps_its_weight_gradient_on_the_main_stream(launches):
    """Conv2dFunction hands `g` itself to a same-size residual that needs a gradient: autograd may add into that tensor in place
    on the main stream, so the layer's weight gradient must not read it on the side stream.  Control: without the residual the
    same launch does go to the side stream (the spy sees it)."""
    d = _residual(40, 48, 3).data(77)
    once(_residual(40, 48, 3), d, True)
    wgrad = [(n, s) for n, s in launches if n.startswith('htd_conv2d_bwd_weight')]
    assert len(wgrad) == 1 and not any(s for _, s in launches), launches
    del launches[:]
    once(_plain(40, 48, 3), _plain(40, 48, 3).data(78), True)
    wgrad = [(n, s) for n, s in launches if n.startswith('htd_conv2d_bwd_weight')]
    assert len(wgrad) == 1 and wgrad[0][1], launches


def test_delay_outlasts_the_largest_backward():
    """The delay has to be reached by the consumer first with certainty: at least 20 backward passes of the largest case (the
    residual stage, single stream, device events) and at least 3 ms."""
    from htd_amd import dense
    from htd_amd.detector.resnet import Bottleneck, ResLayer
    torch.manual_seed(5)
    layer = ResLayer(Bottleneck, 64, 32, 2).to(DEV).eval()
    x = torch.randn(B, 64, 8, 10, device=DEV).contiguous(memory_format=CL).requires_grad_()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with dense.overlap_wgrad(False):
        for rep in range(3):                                       # the third pass is the measured one
            dense.new_step()
            y = layer(x)
            gy = torch.ones_like(y)
            torch.cuda.synchronize()
            ev[0].record()
            y.backward(gy)
            ev[1].record()
    delay(torch.cuda.current_stream(), 2)                         # (the first product also loads its kernel)
    ev[2].record()
    delay(torch.cuda.current_stream())
    ev[3].record()
    torch.cuda.synchronize()
    dense.new_step()
    t_bwd, t_delay = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])
    print(f'single-stream backward of the stage {t_bwd:.3f} ms, delay {t_delay:.3f} ms')
    assert t_delay >= 20 * t_bwd and t_delay >= 3.0, (t_bwd, t_delay)
    assert t_delay <= 400.0, t_delay                              # ... and every test stays quick


# ---------------------------------------------------------------------------------------------------- B: side-consumed marks
def test_side_consumed_mark_dies_with_its_tensor():
    from htd_amd import dense
    dense.new_step()
    n0 = len(dense._SIDE_CONSUMED)
    slot = Slot()
    t = slot.take()
    assert not dense.side_consumed(t)
    dense.mark_side_consumed(t)
    assert dense.side_consumed(t) and dense.side_consumed(t.view_as(t)) and dense.side_consumed(t.detach())
    assert dense.side_consumed(t.permute(0, 2, 3, 1).permute(0, 3, 1, 2))          # a channels_last view of the same elements
    assert not dense.side_consumed(t[:36]) and not dense.side_consumed(t.clone())
    del t
    z = slot.take()
    assert not dense.side_consumed(z)                                               # another tensor: nobody marked it
    t2 = victim()
    dense.mark_side_consumed(t2)
    assert len(dense._SIDE_CONSUMED) == n0 + 1
    del t2
    dense.new_step()                                                                # drops the entries of dead tensors ...
    assert len(dense._SIDE_CONSUMED) == n0
    dense.mark_side_consumed(z)
    dense.new_step()
    assert dense.side_consumed(z)                                                   # ... and only those
    dense.reset_grad_sinks()
    assert len(dense._SIDE_CONSUMED) == 0 and not dense.side_consumed(z)


def test_weight_on_a_dead_fold_address_still_makes_the_main_stream_wait():
    """The suspected cause of a wrong convolution weight gradient seen only in the whole suite, in miniature.  Folded weights
    (bricks.frozen_bn_fold, once in inference and once with a backward) are recorded as consumed on the side stream and die; no
    FlatParams, nobody calls reset_grad_sinks.  A standardised weight of the same byte size then lands on one of their addresses
    (the precondition, asserted).  Its gradient is consumed by WeightStandardizeFunction.backward on the MAIN stream: with the
    side stream late, the gradient of `w` is right only if the main stream waited."""
    from htd_amd import dense
    from htd_amd import mmcv_ops as M
    Co, Ci, k, _ = ODD_SHAPE
    case = _ws(Ci, Co, k)
    recorded, hits, keep = set(), [], []

    def predecessors():
        fold = _fold(Ci, Co, k, False)
        inputs = [fold.leaves(fold.data(900 + grad)) for grad in (False, True)]
        keep.append(inputs)                                         # inputs and parameters stay: only the folded weights die
        keep.append(hole()[1])                                      # where the folded weights will live
        for grad, t in zip((False, True), inputs):
            with torch.set_grad_enabled(grad):
                ops = DevOps()
                wf, bf = ops.fold(t['w'], t['gamma'], t['beta'], t['mean'], t['var'])
                recorded.add(wf.data_ptr())
                y = ops.conv(t['x'], wf, bf, 1, True)
            if grad:
                y.backward(t['gy'])
            del wf, bf, y
        torch.cuda.synchronize()
        dense.new_step()                                            # (the step's weight images hold their weights until then)
        gc.collect()

    def ws_on_a_dead_address(w):
        misses = []
        for _ in range(8):
            out = M.weight_standardize(w, EPS)
            if out.data_ptr() in recorded:
                hits.append(out.data_ptr())
                return out
            misses.append(out)
        pytest.fail('precondition not met: the standardised weight never landed on the address of a dead folded weight')

    got = pair(case, 950, 'side', ops=DevOps(ws=ws_on_a_dead_address), before=predecessors)
    assert len(hits) == 1 and hits[0] in recorded
    assert torch.isfinite(got['w']).all()
    del keep[:]


# ---------------------------------------------------------------------------------------------------- C: the other registries
def test_flipped_image_is_served_to_its_own_weight_only():
    from htd_amd import dense
    dense.new_step()
    slot = Slot()
    w = slot.take()
    wT = torch.empty(w.numel() + 1, device=DEV)[:w.numel()]
    dense.offer_flipped(w, wT)
    assert dense.take_flipped(w) is wT and dense.take_flipped(w) is None             # taken once
    dense.offer_flipped(w, wT)
    assert dense.take_flipped(w.view_as(w)) is wT                                     # the weight as another tensor object
    dense.offer_flipped(w, wT)
    other = w.permute(0, 2, 3, 1).reshape(w.size(0), -1, 1, 1)                        # same address and elements, other shape
    assert other.data_ptr() == w.data_ptr()
    assert dense.take_flipped(other) is None
    dense.offer_flipped(w, wT)
    assert dense.take_flipped(w[:36]) is None                                         # same address, fewer elements
    dense.offer_flipped(w, wT)                                                        # offered and never taken: the weight dies
    del w, other
    z = slot.take()
    assert dense.take_flipped(z) is None
    dense.offer_flipped(z, wT)
    dense.new_step()                                                                  # a new step drops what nobody took
    assert len(dense._FLIPPED) == 0 and dense.take_flipped(z) is None


@pytest.mark.parametrize('shape', [ODD_SHAPE, (64, 48, 3, 3)], ids=['flips', 'planes'])
def test_step_images_hold_their_weight_and_a_new_weight_gets_new_images(shape):
    """_STEP_FLIPS (72 output channels: the data gradient of conv_igemm_kernel) / _STEP_PLANES (64 x 48: conv_x3p_kernel both ways).
    An entry holds its weight, so the address cannot recur while it lives; new_step() empties the dicts, and a NEW weight at the
    old address is read through images of its own (forward and data gradient against fp64)."""
    from htd_amd import dense
    Co, Ci, k, _ = shape
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, Ci, H, W, generator=g)
    gy = torch.randn(B, Co, H, W, generator=g)
    w1, w2 = _scaled(lambda *s: torch.randn(*s, generator=g), Co, Ci, k), _scaled(lambda *s: torch.randn(*s, generator=g), Co, Ci, k)
    xd, gyd = x.to(DEV).contiguous(memory_format=CL), gy.to(DEV).contiguous(memory_format=CL)
    dense.new_step()
    assert len(dense._STEP_FLIPS) + len(dense._STEP_PLANES) == 0
    slot = Slot(shape)
    w = slot.take().copy_(w1)

    def check(w, wc):
        y = dense._fwd_raw(xd, w, None, None, 1, 1, 1, False)
        gx = dense._dgrad_raw(gyd, w, tuple(xd.shape), 1, 1, 1)
        xr = x.double().requires_grad_()
        yr = F.conv2d(xr, wc.double(), None, 1, 1)
        yr.backward(gy.double())
        torch.testing.assert_close(y.cpu().double(), yr.detach(), rtol=1e-4, atol=1e-5 * (Ci * k * k) ** 0.5)
        torch.testing.assert_close(gx.cpu().double(), xr.grad, rtol=1e-4, atol=2e-5 * (Co * k * k) ** 0.5)
    check(w, w1)
    assert len(dense._STEP_FLIPS) + len(dense._STEP_PLANES) > 0
    ptr, alive = w.data_ptr(), weakref.ref(w)
    del w
    gc.collect()
    assert alive() is not None and alive().data_ptr() == ptr         # the registry's own reference keeps the weight
    held = [torch.empty(shape, device=DEV, memory_format=CL) for _ in range(8)]
    assert all(h.data_ptr() != ptr for h in held)                    # ... so nobody else gets its address
    dense.new_step()
    gc.collect()
    assert len(dense._STEP_FLIPS) == 0 and len(dense._STEP_PLANES) == 0 and alive() is None
    z = slot.take()
    del held
    z.copy_(w2)                                                       # same address, version, shape and epoch as w had
    check(z, w2)
    dense.new_step()


def test_temporary_sink_is_not_served_to_a_later_tensor():
    from htd_amd import dense
    dense.new_step()
    slot = Slot()
    t = slot.take().requires_grad_()
    dense.temp_grad_sink(t)
    with torch.no_grad():
        buf, is_sink = dense.grad_out2(t)
        again = dense.grad_sink_again(t)
        assert not is_sink and again is not None and again.data_ptr() == buf.data_ptr()
    del t, again
    gc.collect()
    z = slot.take().requires_grad_()
    with torch.no_grad():                                             # the tensor died: its buffer is nobody's, new_step() or not
        assert dense.grad_sink_again(z) is None
        a, sa = dense.grad_out2(z)
        b, sb = dense.grad_out2(z)
    assert not sa and not sb and len({a.data_ptr(), b.data_ptr(), buf.data_ptr()}) == 3
    dense.temp_grad_sink(z * 1.0)
    dense.new_step()
    assert len(dense._TEMP_KEYS) == 0 and len(dense._TEMP_USED) == 0
    with torch.no_grad():
        assert dense.grad_sink_again(z) is None and not dense.grad_out2(z)[1]


def test_carried_maximum_is_not_served_to_a_later_tensor():
    from htd_amd import dense
    assert dense.H2_VIEWS
    dense.new_step()
    slot = Slot()
    y = slot.take()
    dense.tag_amax(y, dense.absmax(y))
    assert dense.carried_amax(y.view_as(y)) is not None                # found by address
    del y
    z = slot.take()
    assert dense.carried_amax(z) is None and dense.carried_amax(z.view_as(z)) is None
    dense.new_step()


def test_inference_fold_cache_follows_its_five_tensors():
    """bn._htd_fold_cache of bricks.frozen_bn_fold: the same objects while nothing changed, rebuilt after mmcv_ops.PARAM_EPOCH
    moved and after an in-place change of the weight or of any of the four BatchNorm tensors."""
    from htd_amd import mmcv_ops as M
    from htd_amd.detector import bricks
    Co, Ci, k = 56, 40, 3
    g = torch.Generator().manual_seed(61)
    R = lambda *s: torch.randn(*s, generator=g)
    w = _scaled(R, Co, Ci, k).to(DEV).contiguous(memory_format=CL)
    bn = nn.BatchNorm2d(Co, eps=EPS).to(DEV).eval()
    st = _bn_stats(R, Co)
    with torch.no_grad():
        bn.weight.copy_(st['gamma']), bn.bias.copy_(st['beta']), bn.running_mean.copy_(st['mean']), bn.running_var.copy_(st['var'])

    def check(out):
        rw, rb = RefOps().fold(w.cpu().double(), bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double(),
                               bn.running_mean.cpu().double(), bn.running_var.cpu().double())
        torch.testing.assert_close(out[0].cpu().double(), rw, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out[1].cpu().double(), rb, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        first = bricks.frozen_bn_fold(w, bn)
        check(first)
        again = bricks.frozen_bn_fold(w, bn)
        assert again[0] is first[0] and again[1] is first[1]
        M.PARAM_EPOCH += 1                                             # what the optimizer kernel does
        last = bricks.frozen_bn_fold(w, bn)
        assert last[0] is not first[0]
        check(last)
        for t in (w, bn.weight, bn.bias, bn.running_mean, bn.running_var):
            t.mul_(1.25)
            out = bricks.frozen_bn_fold(w, bn)
            assert out[0] is not last[0] and out[1] is not last[1]
            check(out)
            assert bricks.frozen_bn_fold(w, bn)[0] is out[0]
            last = out
