"""The chained-gradient hand-off ("The gradient hand-off"): a node returns an identity alias of its input, a later
consumer reads the alias, its gradient arrives at the first node's backward and joins there, so one gradient map reaches the
producer.  Every test runs the chained nodes and the same ops unchained on cloned leaves, where autograd adds the maps, and
compares the producer's gradient -- over every way the handed gradient can arrive (channels-last: written in place; NCHW: copied
first; absent; present while the node's own output is unused) and every backward form of the RoIAlign nodes."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
NCHW = torch.contiguous_format

SHAPES = [(2, 8, 16, 24), (2, 8, 8, 12)]            # two pyramid levels of a 64 x 96 image
SCALES = [1 / 4, 1 / 8]
NODES = ['single', 'levels', 'all']
CONSUMERS = ['cl', 'nchw', 'absent', 'only']        # 'only': the alias is read, the node's own output is not (g is None)


def _dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _roi_case(ph):
    """Fixed inputs, made once per output size and never modified: the maps, 24 RoIs over both images (four of them reach past
    the border), their levels, the output gradients of the nodes and the second consumer's factor and gradient per level."""
    from htd_amd.detector.roi_extractors import map_roi_levels
    dev, g = _dev(), torch.Generator().manual_seed(11)
    feats = [torch.randn(s, generator=g).to(dev).contiguous(memory_format=CL) for s in SHAPES]
    n = 24
    img = (torch.arange(n) // 12).float()
    size = torch.exp(torch.rand(n, generator=g) * 2.0 + 2.3)                  # 10 .. 74 px
    cx, cy = torch.rand(n, generator=g) * 96, torch.rand(n, generator=g) * 64
    rois = torch.stack([img, cx - size / 2, cy - size / 3, cx + size / 2, cy + size / 3], 1)
    rois[:, 1::2] = rois[:, 1::2].clamp(0, 96)
    rois[:, 2::2] = rois[:, 2::2].clamp(0, 64)
    rois[0] = torch.tensor([0., -9., -7., 30., 20.])
    rois[5] = torch.tensor([0., 70., 40., 104., 71.])
    rois[13] = torch.tensor([1., -12., 30., 50., 75.])
    rois[20] = torch.tensor([1., 60., -5., 101., 30.])
    rois = rois.to(dev)
    lvls = map_roi_levels(rois, 2, finest_scale=16)                           # sqrt(w h) < 32 px -> level 0, else level 1
    assert 0 < int(lvls.sum()) < n                                            # both levels have RoIs
    gos = [torch.randn(n, 8, ph, ph, generator=g).to(dev).contiguous(memory_format=CL) for _ in SHAPES]
    factor = [torch.randn(s, generator=g).to(dev) for s in SHAPES]
    gz = [torch.randn(s, generator=g).to(dev) for s in SHAPES]
    return feats, rois, lvls, gos, factor, gz


def _second_consumer(aliases, factor, gz, fmt, heads, grads, seen=None):
    """alias * factor per level, both and the product's gradient in layout `fmt`: the gradient handed to the alias is then in
    that layout too (recorded in `seen` as (data_ptr, is channels-last))."""
    for a, r, z in zip(aliases, factor, gz):
        if seen is not None:
            a.register_hook(lambda t: seen.append((t.data_ptr(), t.is_contiguous(memory_format=CL))))
        heads.append(a * r.contiguous(memory_format=fmt))
        grads.append(z.contiguous(memory_format=fmt))


def _run_roi(node, consumer, chained, ph):
    """-> (gradients of the leaves, [(data_ptr, channels-last?) of every gradient handed to an alias])"""
    from htd_amd import mmcv_ops as M
    feats, rois, lvls, gos, factor, gz = _roi_case(ph)
    xs = [f.clone().requires_grad_() for f in feats]
    hs = [x * 1.0 for x in xs]                      # produced maps, not leaves: their gradient is what gets summed
    src = M.PyramidTaps(hs) if chained else hs
    if node == 'single':
        outs = [M.roi_align(h, rois, ph, s, 0, 'avg', True, chain=chained) for h, s in zip(hs, SCALES)]
        if chained:
            outs, aliases = [o for o, _ in outs], [a for _, a in outs]
    elif node == 'levels':
        outs = [M.roi_align_levels(src, rois, lvls, ph, SCALES)]
    else:
        outs = M.roi_align_all_levels(src, rois, ph, SCALES)
    if node != 'single' or not chained:
        aliases = list(src.levels) if chained else hs
    heads, grads, seen = [], [], []
    if consumer != 'only':
        heads += outs
        grads += gos[:len(outs)]
    if consumer != 'absent':
        _second_consumer(aliases, factor, gz, NCHW if consumer == 'nchw' else CL, heads, grads, seen if chained else None)
    torch.autograd.backward(heads, grads)
    return [x.grad for x in xs], seen


def _check(name, got, ref, rtol, atol_rel):
    """|got - ref| <= atol_rel * max|ref| + rtol * |ref|; prints the worst error in units of max|ref| first"""
    scale = float(ref.abs().max())
    print('%s: max|err| / max|ref| = %.3g' % (name, float((got - ref).abs().max()) / scale))
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol_rel * scale)


@pytest.fixture(params=['gather', 'per_level', 'scatter', 'ph9'])
def roi_form(request, monkeypatch):
    """The backward forms: one gather launch, one gather launch per level, the atomic scatter kernels, and a 9 x 9 output,
    which is past the gather kernels' 8 x 8 and takes the scatter kernels too.  -> output size"""
    from htd_amd import mmcv_ops as M
    if request.param == 'per_level':
        monkeypatch.setattr(M, 'ROI_BWD_ONE_LAUNCH', False)
    if request.param == 'scatter':
        monkeypatch.setattr(M, 'ROI_BWD', 'scatter')
    return 9 if request.param == 'ph9' else 7


@pytest.mark.parametrize('consumer', CONSUMERS)
@pytest.mark.parametrize('node', NODES)
def test_roi_align_hand_off_equals_autograd_adding_the_maps(node, consumer, roi_form):
    """rtol 2e-5, atol 2e-6 max|ref|: the bound of test_all_levels_backward_adds_into_chained_maps, in every form.  The scatter
    forms, which sum with float atomics, need no wider one: measured before the hand-off had one implementation, the worst error
    was 2.1e-7 max|ref| with ROI_BWD = 'scatter' and 5.8e-7 at 9 x 9 (levels node, NCHW gradient); both gather forms gave 0."""
    ref, _ = _run_roi(node, consumer, False, roi_form)
    got, seen = _run_roi(node, consumer, True, roi_form)
    if consumer != 'absent':                        # the handed gradients arrived, in the layout this case is about
        assert len(seen) == len(SHAPES) and all(is_cl == (consumer != 'nchw') for _, is_cl in seen)
    for i, (a, b) in enumerate(zip(got, ref)):
        _check('%s %s level %d' % (node, consumer, i), a, b, 2e-5, 2e-6)


@pytest.mark.parametrize('consumer', CONSUMERS)
def test_one_gather_launch_and_one_per_level_hand_off_the_same_bits(consumer, monkeypatch):
    """the same strips sum the same RoIs in the same order onto the same handed maps: bit for bit"""
    from htd_amd import mmcv_ops as M
    one, _ = _run_roi('levels', consumer, True, 7)
    monkeypatch.setattr(M, 'ROI_BWD_ONE_LAUNCH', False)
    per, _ = _run_roi('levels', consumer, True, 7)
    for a, b in zip(one, per):
        assert torch.equal(a, b)


def _gather_writes(calls):
    """[(pointer of the map written, accumulate flag)] of every map a recorded gather backward launch writes"""
    out = []
    for name, a in calls:
        if name == 'htd_roi_align_bwd_gather':
            out.append((a[4].value, a[15]))
        elif name == 'htd_roi_align_levels_bwd_gather':
            out += [(a[3][i], a[7][i]) for i in range(a[8])]
        elif name == 'htd_roi_align_all_levels_bwd_gather':
            out += [(a[2][i], a[6][i]) for i in range(a[7])]
    return out


@pytest.mark.parametrize('consumer', ['cl', 'nchw', 'absent'])
@pytest.mark.parametrize('node,one_launch', [('single', True), ('levels', True), ('levels', False), ('all', True)])
def test_handed_maps_are_written_in_place_exactly_when_they_can_be(node, one_launch, consumer, monkeypatch):
    """A channels-last handed map is the map the kernel accumulates into (acc = 1, same pointer: nothing allocated, nothing
    copied); an NCHW one is copied into a fresh map that is then accumulated into (acc = 1, another pointer); with nothing
    handed the kernel writes a fresh map (acc = 0)."""
    from htd_amd import capi
    from htd_amd import mmcv_ops as M
    monkeypatch.setattr(M, 'ROI_BWD_ONE_LAUNCH', one_launch)
    calls, real = [], capi.call

    def spy(name, *args, **kw):
        calls.append((name, args))
        return real(name, *args, **kw)
    monkeypatch.setattr(capi, 'call', spy)
    _, seen = _run_roi(node, consumer, True, 7)
    names = {name for name, _ in calls if 'bwd' in name}
    assert names == {{'single': 'htd_roi_align_bwd_gather', 'all': 'htd_roi_align_all_levels_bwd_gather',
                      'levels': 'htd_roi_align_levels_bwd_gather' if one_launch else 'htd_roi_align_bwd_gather'}[node]}
    writes = _gather_writes(calls)
    handed = {p for p, _ in seen}
    assert len(writes) == len(SHAPES) and len({p for p, _ in writes}) == len(SHAPES)
    if consumer == 'cl':
        assert set(writes) == {(p, 1) for p in handed}
    elif consumer == 'nchw':
        assert all(acc == 1 and p not in handed for p, acc in writes)
    else:
        assert not seen and all(acc == 0 for _, acc in writes)


def test_ba_extractor_taps_level_by_level_as_in_one_launch(monkeypatch):
    """AdptRoIExtractor over a PyramidTaps with BA_ONE_LAUNCH off (one chained roi_align per level) against the one-launch
    form: the same features bit for bit, the same gradient maps within the bound above; a second consumer reads the levels the
    extractor left in the taps."""
    from htd_amd import mmcv_ops as M
    from htd_amd.detector import roi_extractors as E
    dev, g = _dev(), torch.Generator().manual_seed(17)
    _, rois, _, _, _, _ = _roi_case(7)
    feats = [torch.randn(2, 256, h, w, generator=g).to(dev).contiguous(memory_format=CL) for h, w in ((16, 24), (8, 12))]
    factor = [torch.randn(f.shape, generator=g).to(dev).contiguous(memory_format=CL) for f in feats]
    go = torch.randn(rois.size(0), 256, 7, 7, generator=g).to(dev).contiguous(memory_format=CL)
    torch.manual_seed(17)
    ext = E.AdptRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                             featmap_strides=[4, 8]).to(dev)

    def run(one_launch):
        monkeypatch.setattr(E, 'BA_ONE_LAUNCH', one_launch)
        xs = [f.clone().requires_grad_() for f in feats]
        taps = M.PyramidTaps([x * 1.0 for x in xs])
        out = ext(taps, rois)
        torch.autograd.backward([out] + [a * r for a, r in zip(taps.levels, factor)], [go] + factor)
        return out.detach(), [x.grad for x in xs]
    (ref_out, ref), (out, got) = run(True), run(False)
    assert torch.equal(out, ref_out)
    for i, (a, b) in enumerate(zip(got, ref)):
        _check('BA level %d' % i, a, b, 2e-5, 2e-6)


# ------------------------------------------------------------------------------------------------ convolutions
@functools.lru_cache(maxsize=None)
def _conv_case():
    dev, g = _dev(), torch.Generator().manual_seed(13)

    def t(*shape, s=1.0):
        v = (torch.randn(*shape, generator=g) * s).to(dev)
        return v.contiguous(memory_format=CL) if v.dim() == 4 else v
    return dict(x=t(2, 16, 12, 20), w1=t(16, 16, 3, 3, s=0.1), b1=t(16, s=0.1), w2=t(16, 16, 1, 1, s=0.1), b2=t(16, s=0.1),
                wb=t(8, 16, 1, 1, s=0.1), ry=t(2, 16, 12, 20), ry2=t(2, 16, 6, 10), rb=t(2, 8, 12, 20), factor=t(2, 16, 12, 20),
                gz=t(2, 16, 12, 20))


def _run_conv(first, second, chained, use_first=True):
    """first: 'head' (ConvReluHeadFunction: 3x3 16->16 + ReLU + merged 1x1 16->16) | 'conv' (Conv2dFunction 3x3) | 'conv_s2' (the
    same with stride 2); second reader of the map: '1x1' (a convolution) | 'nchw' (a product whose gradient is NCHW-contiguous).
    -> gradients of x and of every weight, [(data_ptr, channels-last?) of the handed gradient]"""
    from htd_amd import dense
    c = _conv_case()
    x = c['x'].clone().requires_grad_()
    p = {k: c[k].clone().requires_grad_() for k in ('w1', 'b1', 'w2', 'b2', 'wb')}
    h = x * 1.0
    if first == 'head':
        y = dense.conv_relu_head(h, p['w1'], p['b1'], p['w2'], p['b2'], 1, chained)
    else:
        y = dense.conv2d(h, p['w1'], p['b1'], 2 if first == 'conv_s2' else 1, 1, 1, chain=chained)
    y, alias = y if chained else (y, h)
    heads, grads, seen = [], [], []
    if use_first:
        heads.append(y)
        grads.append(c['ry2'] if first == 'conv_s2' else c['ry'])
    if second == '1x1':
        if chained:
            alias.register_hook(lambda t: seen.append((t.data_ptr(), t.is_contiguous(memory_format=CL))))
        heads.append(dense.conv2d(alias, p['wb'], None, 1, 0, 1))
        grads.append(c['rb'])
    else:
        _second_consumer([alias], [c['factor']], [c['gz']], NCHW, heads, grads, seen if chained else None)
    torch.autograd.backward(heads, grads)
    return [x.grad] + [p[k].grad for k in ('w1', 'b1', 'w2', 'b2', 'wb')], seen


@pytest.mark.parametrize('first,second,use_first', [('head', '1x1', True), ('conv_s2', '1x1', True), ('conv', 'nchw', True),
                                                    ('head', '1x1', False)],
                         ids=['head', 'conv-stride2-add-afterwards', 'conv-nchw-gradient', 'head-output-unused'])
def test_conv_hand_off_equals_autograd_adding_the_maps(first, second, use_first):
    """rtol 1e-5, atol 1e-5 max|ref|: the bound of test_chained_conv_consumers_hand_one_gradient_to_the_producer"""
    ref, _ = _run_conv(first, second, False, use_first)
    got, seen = _run_conv(first, second, True, use_first)
    assert len(seen) == 1 and seen[0][1] == (second != 'nchw')
    assert ref[0] is not None
    for name, a, b in zip(('x', 'w1', 'b1', 'w2', 'b2', 'wb'), got, ref):
        assert (a is None) == (b is None), name
        if b is not None:
            _check('%s-%s %s' % (first, second, name), a, b, 1e-5, 1e-5)
