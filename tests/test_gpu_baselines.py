"""Faster R-CNN and Cascade R-CNN on a real MI355X: htd_roi_head_loss_classes and htd_rpn_loss_l1 against fp64 references and the
reference's own fp32 error (tests/golden/baselines.npz), both detectors against the reference run, the static-shape training path
against the per-image path, the whole-batch test post-processing against the per-image loop, reproducibility and checkpoints.

The ratios measured on the MI355X are in DESIGN.md section 8 f10."""
import copy

import numpy as np
import pytest
import torch

import baselines_util as U
from golden_util import match_detections

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
DEV = 'cuda:0'


def T(a):
    return torch.from_numpy(np.asarray(a))


# ---------------------------------------------------------------------------------------------------- the fused head loss
def _raw(entry, cls, labels, lw, pred, tgt, bw, nc, reg, box_loss=0, beta=1.0):
    """One call of htd_roi_head_loss / htd_roi_head_loss_classes on device tensors -> (partial, grad_cls, grad_box), every output
    buffer pre-filled with NaN: what the kernel does not write shows."""
    from htd_amd import capi
    n = cls.size(0)
    blocks = capi.lib().htd_roi_head_loss_partial_rows()
    partial = torch.full((blocks, 4), float('nan'), device=cls.device)
    gcls, gbox = torch.full_like(cls, float('nan')), torch.full_like(pred, float('nan'))
    if entry == 'htd_roi_head_loss':
        capi.call(entry, capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(pred), capi.ptr(tgt), capi.ptr(bw), n, nc, nc - 1,
                  float(beta), capi.ptr(partial), capi.ptr(gcls), capi.ptr(gbox), capi.current_stream_ptr())
    else:
        capi.call(entry, capi.ptr(cls), capi.ptr(labels), capi.ptr(lw), capi.ptr(pred), capi.ptr(tgt), capi.ptr(bw), n, nc, nc - 1,
                  int(reg), int(box_loss), float(beta), capi.ptr(partial), capi.ptr(gcls), capi.ptr(gbox), capi.current_stream_ptr())
    torch.cuda.synchronize()
    return partial, gcls, gbox


@pytest.mark.parametrize('loss', list(U.HEAD_LOSSES))
@pytest.mark.parametrize('spec', [False, True], ids=['agn', 'spec'])
@pytest.mark.parametrize('nc', U.CASE_NC)
@pytest.mark.parametrize('n', U.CASE_ROWS)
def test_head_loss_classes_kernel(golden, n, nc, spec, loss):
    """htd_roi_head_loss_classes with reg_classes = 1 ('agn') and NC - 1 ('spec'), smooth-L1 and L1, on n rows of NC logits: fewer
    rows than the four waves of a block, rows that are no multiple of them, one row more than two sweeps of the 64 x 4 grid; a
    row of 4 columns, of 16 (a quarter wave) and of 320 (five sweeps of the wave).  Each case holds a row of the last class,
    unused slots of weight 0 and pred == target rows, and comes a second time with every row background.

    loss_cls, loss_bbox (through BBoxHead.loss, num_samples = n) against the reference's fp64 run: within 4 x max(the reference's own
    fp32 error on the case, one fp32 ulp of the value) -- only the summation order differs.  grad_box (the kernel's raw output)
    against the fp64 tensor formulation: nonzero entries to 4 * 2^-23 relative (three fp32 roundings: the difference, the division
    by beta, the weight), every other entry exactly 0 although the buffer went in as NaN.  loss_cls, acc and grad_cls bitwise those
    of htd_roi_head_loss; with reg_classes = 1 and smooth-L1 every output bitwise; two runs bitwise equal."""
    from htd_amd import capi
    g = golden('baselines')
    dev = torch.device(DEV)
    fg = nc - 1
    reg = fg if spec else 1
    for variant in ('mixed', 'allbg'):
        cls, full, labels, lw, tgt, bw = U.head_case(n, nc, variant)
        pred = full if spec else U.own_columns(full, labels, fg)
        head = U.make_head(loss, fg, not spec)
        ref = U.head_loss_fp64(head, cls, pred, labels, lw, tgt, bw, num_samples=n)
        p = f'case.{n}.{nc}.{reg}.{loss}.{variant}.'
        scalars, err32 = g[p + 'scalars64'], g[p + 'err32']                  # [loss_cls, loss_bbox]
        np.testing.assert_allclose([float(ref['loss_cls']), float(ref['loss_bbox'])], scalars, rtol=1e-12, atol=1e-300)
        d = [t.to(dev) for t in (cls, labels, lw, pred.contiguous(), tgt, bw)]
        # ---- through BBoxHead.loss
        calls, real = [], capi.call

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        capi.call = spy
        try:
            c, q = d[0].clone().requires_grad_(), d[3].clone().requires_grad_()
            losses = head.loss(c, q, None, d[1], d[2], d[4], d[5], num_samples=torch.tensor(n, device=dev))
        finally:
            capi.call = real
        (losses['loss_cls'] + losses['loss_bbox']).backward()
        assert calls == ['htd_roi_head_loss' if (loss == 'smooth_l1' and not spec) else 'htd_roi_head_loss_classes'], calls
        for i, k in enumerate(('loss_cls', 'loss_bbox')):
            e = abs(float(losses[k].detach().double()) - float(scalars[i]))
            bound = 4.0 * max(float(err32[i]), EPS32 * abs(float(scalars[i])))
            print(f'{p}{k}: |kernel - fp64| {e:.3e}  |reference fp32 - fp64| {float(err32[i]):.3e}  bound {bound:.3e}')
            assert e <= bound, (k, e, bound)
        assert float(losses['acc']) == pytest.approx(float(ref['acc']), abs=1e-4)
        assert tuple(q.grad.shape) == (n, 4 * reg) and torch.isfinite(q.grad).all() and torch.isfinite(c.grad).all()
        # ---- the entry point itself
        box_loss = int(loss == 'l1')
        new = _raw('htd_roi_head_loss_classes', d[0], d[1], d[2], d[3], d[4], d[5], nc, reg, box_loss)
        again = _raw('htd_roi_head_loss_classes', d[0], d[1], d[2], d[3], d[4], d[5], nc, reg, box_loss)
        own = U.own_columns(d[3], d[1], fg).contiguous() if spec else d[3]
        old = _raw('htd_roi_head_loss', d[0], d[1], d[2], own, d[4], d[5], nc, 1)
        for a, b in zip(new, again):
            assert torch.isfinite(a).all() and torch.equal(a, b)
        assert torch.equal(new[0][:, [0, 1, 3]], old[0][:, [0, 1, 3]]) and torch.equal(new[1], old[1])
        if loss == 'smooth_l1':                     # the same four terms in the same order: the box sum as well
            assert torch.equal(new[0], old[0])
            got_own = U.own_columns(new[2], d[1], fg) if spec else new[2]
            is_fg = (d[1] < fg)[:, None]
            assert torch.equal(got_own * is_fg, old[2] * is_fg)
            if not spec:
                assert torch.equal(new[2], old[2])
        want = ref['grad_box'] * n                                            # d(sum)/d(pred): loss_weight 1, avg_factor n
        got = new[2].cpu().double()
        nz = want != 0
        assert float(got[~nz].abs().max() if (~nz).any() else 0.0) == 0.0     # other classes' columns, idle rows, pred == target
        if nz.any():
            rel = float(((got[nz] - want[nz]).abs() / want[nz].abs()).max())
            print(f'{p}grad_box: {int(nz.sum())} nonzero entries, worst relative error {rel / EPS32:.2f} x 2^-23')
            assert rel <= 4 * EPS32, rel
        else:
            assert variant == 'allbg' or n == 1
        if variant == 'allbg':
            assert float(losses['loss_bbox'].detach()) == 0.0 and float(q.grad.abs().max()) == 0.0
        else:
            assert int(labels[0]) == fg - 1 and (float(want[0].abs().sum()) > 0 or n == 1)


def test_head_loss_classes_argument_checks():
    from htd_amd import capi
    dev = torch.device(DEV)
    cls, full, labels, lw, tgt, bw = (t.to(dev) for t in U.head_case(7, 5))
    with pytest.raises(ValueError, match='reg_classes'):
        _raw('htd_roi_head_loss_classes', cls, labels, lw, full, tgt, bw, 5, 3)
    with pytest.raises(ValueError, match='beta'):
        _raw('htd_roi_head_loss_classes', cls, labels, lw, full, tgt, bw, 5, 4, 0, 0.0)
    with pytest.raises(ValueError, match='box_loss'):
        _raw('htd_roi_head_loss_classes', cls, labels, lw, full, tgt, bw, 5, 4, 2)
    assert capi.lib().htd_abi_version() == 8


# ---------------------------------------------------------------------------------------------------- the two detectors
def small_cfg(name):
    from htd_amd.configs import cascade_rcnn_config, faster_rcnn_config
    cfg = dict(faster_rcnn=faster_rcnn_config, cascade_rcnn=cascade_rcnn_config)[name]()
    U.small_counts(cfg.train_cfg, cfg.test_cfg)
    return cfg


def inputs(dev):
    imgs, metas, gts, labels = U.detector_inputs()
    return T(imgs).to(dev), metas, [T(x).to(dev) for x in gts], [T(x).to(dev) for x in labels]


@pytest.fixture(scope='module')
def dets(golden):
    """Both detectors with the fixture's weights, sampling replayed from the CPU generator."""
    from htd_amd.configs import build_baseline_detector
    from htd_amd.core import set_randperm
    scale = float(golden('baselines')['fc_reg_scale'])
    models = {name: U.load_fixture_weights_(build_baseline_detector(cfg=small_cfg(name)), scale).to(torch.device(DEV))
              for name in U.MODELS}
    set_randperm(lambda n, device: torch.randperm(n).to(device))
    yield models
    set_randperm(None)


def box_keys(dev):
    coef = torch.tensor([12.9898, 78.233, 37.719, 93.989], device=dev)
    return lambda cand: torch.frac(torch.sin((torch.round(cand * 64.0) / 64.0 * coef).sum(-1)) * 43758.5453).abs()


def _stages(name):
    return 3 if name == 'cascade_rcnn' else 1


def _bbox_forward(head, name, stage, feats, rois):
    return head._bbox_forward(stage, feats, rois) if name == 'cascade_rcnn' else head._bbox_forward(feats, rois)


@pytest.mark.parametrize('name', U.MODELS)
def test_train_step_matches_reference_fixture(dets, golden, name):
    """Bounds of test_gpu_detector.py::test_train_step_matches_reference_fixture: losses rtol 5e-4 / atol 1e-4; gradient digests in
    units of 2e-4 * max(1, max |ref|) + 1e-3 * |ref|: no element over 2 units, rms at most 0.2."""
    g, det = golden('baselines'), dets[name]
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    det.train()
    torch.manual_seed(int(g[f'{name}.seed_sampler']))
    losses = det.forward_train(img, metas, gts, labels)
    loss, log_vars = det._parse_losses(losses)
    assert set(log_vars.keys()) == {f[len(name) + 6:] for f in g.files if f.startswith(f'{name}.loss.')}
    worst_loss = 0.0
    for k, v in log_vars.items():
        ref = float(g[f'{name}.loss.{k}'])
        worst_loss = max(worst_loss, abs(v - ref) / (1e-4 + 5e-4 * abs(ref)))
    det.zero_grad()
    loss.backward()
    params = dict(det.named_parameters())
    keys = U.grad_keys(det)
    assert any(k.endswith('fc_reg.weight') for k in keys) and len(keys) == 7 + 3 * _stages(name)
    worst, worst_rms = (0.0, ''), (0.0, '')
    assert all(np.abs(g[f'{name}.grad.{k}.sample']).max() > 0 for k in keys if k.startswith('roi_head.'))
    for k in keys:
        gr = params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
        ref = g[f'{name}.grad.{k}.sample']
        tol = 2e-4 * max(1.0, np.abs(ref).max()) + 1e-3 * np.abs(ref)
        ratio = np.abs(U.digest(gr.cpu())[1] - ref) / tol
        worst, worst_rms = max(worst, (float(ratio.max()), k)), max(worst_rms, (float(np.sqrt(np.mean(ratio ** 2))), k))
    print(f'{name}: worst loss ratio {worst_loss:.3f}; worst gradient element {worst[0]:.3f} units ({worst[1]}), '
          f'worst rms {worst_rms[0]:.3f} ({worst_rms[1]})')
    for k, v in log_vars.items():
        np.testing.assert_allclose(v, float(g[f'{name}.loss.{k}']), rtol=5e-4, atol=1e-4, err_msg=k)
    assert worst[0] <= 2.0 and worst_rms[0] <= 0.2, (worst, worst_rms)


@pytest.mark.parametrize('name', U.MODELS)
def test_inference_matches_reference_fixture(dets, golden, name):
    """Bounds of test_gpu_detector.py::test_inference_matches_reference_fixture: proposals rtol 1e-5 / atol 2e-3, detections matched
    one to one within 1e-3 + 1e-5 * the largest coordinate, same class."""
    g, det = golden('baselines'), dets[name]
    dev = torch.device(DEV)
    img, metas, _, _ = inputs(dev)
    det.eval()
    with torch.no_grad():
        feats = det.extract_feat(img)
        for i, f in enumerate(feats):
            np.testing.assert_allclose(f.double().abs().sum().item(), float(g[f'{name}.feat{i}_abs']), rtol=1e-5)
        props = det.rpn_head.simple_test_rpn(feats, metas)
        res = det.roi_head.simple_test(feats, props, metas, rescale=False)
        whole = det.simple_test(img, metas)
    worst = 0.0
    for i in range(2):
        ref_p = g[f'{name}.test_props{i}']
        assert props[i].shape == ref_p.shape
        np.testing.assert_allclose(props[i].cpu().numpy(), ref_p, rtol=1e-5, atol=2e-3)
        mine, ref = U.dets_array(res[i]), g[f'{name}.test_dets{i}']
        assert mine.shape == ref.shape and len(ref) > 0
        assert np.array_equal(mine, U.dets_array(whole[i]))
        used = np.zeros(len(mine), dtype=bool)
        for r in ref:
            d = np.abs(mine[:, :5] - r[:5]).max(1) + 1e3 * (mine[:, 5] != r[5]) + 1e3 * used
            j = int(d.argmin())
            worst = max(worst, d[j] / (1e-3 + 1e-5 * np.abs(r[:4]).max()))
            assert d[j] <= 1e-3 + 1e-5 * np.abs(r[:4]).max(), (r, mine[j], d[j])
            used[j] = True
    print(f'{name}: worst detection ratio {worst:.3f}')


@pytest.mark.parametrize('name', U.MODELS)
def test_train_stage_logits_match_reference_fixture(dets, golden, name):
    """Bounds of test_gpu_detector.py::test_train_stage_logits_match_reference_fixture: end to end the rois of every stage rtol 5e-5 /
    atol 1e-3 and its logits and deltas within 2.5e-4; within 1e-4 once a stage is fed the reference's own rois (train and test)."""
    g, det = golden('baselines'), dets[name]
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    det.train()
    head = det.roi_head
    trail = {}
    orig = head._bbox_forward

    def rec(*a, **k):
        r = orig(*a, **k)
        stage, rois = (a[0], a[2]) if name == 'cascade_rcnn' else (0, a[1])
        trail[stage] = (rois.detach().cpu(), r['cls_score'].detach().cpu(), r['bbox_pred'].detach().cpu())
        return r
    head._bbox_forward = rec
    try:
        torch.manual_seed(int(g[f'{name}.seed_sampler']))
        det.forward_train(img, metas, gts, labels)
    finally:
        del head._bbox_forward
    assert sorted(trail) == list(range(_stages(name)))
    worst = [0.0, 0.0]
    for st in sorted(trail):
        rois, cls, reg = trail[st]
        ref = [T(g[f'{name}.train_s{st}_{k}']) for k in ('rois', 'cls', 'reg')]
        assert rois.shape == ref[0].shape and reg.shape == ref[2].shape
        worst[0] = max(worst[0], float((cls - ref[1]).abs().max()) / 2.5e-4, float((reg - ref[2]).abs().max()) / 2.5e-4)
        torch.testing.assert_close(rois, ref[0], rtol=5e-5, atol=1e-3)
        torch.testing.assert_close(cls, ref[1], rtol=0, atol=2.5e-4)
        torch.testing.assert_close(reg, ref[2], rtol=0, atol=2.5e-4)
    with torch.no_grad():
        feats = det.extract_feat(img)
        for phase in ('train', 'test'):
            for st in range(_stages(name)):
                ref = [T(g[f'{name}.{phase}_s{st}_{k}']) for k in ('rois', 'cls', 'reg')]
                res = _bbox_forward(head, name, st, feats, ref[0].to(dev))
                for a, b in ((res['cls_score'], ref[1]), (res['bbox_pred'], ref[2])):
                    worst[1] = max(worst[1], float((a.cpu() - b).abs().max()) / 1e-4)
                    torch.testing.assert_close(a.cpu(), b, rtol=0, atol=1e-4)
    print(f'{name}: worst stage-logit ratio end to end {worst[0]:.3f}, fed the reference rois {worst[1]:.3f}')


def test_fused_l1_rpn_loss_matches_tensor_formulation(dets):
    """htd_rpn_loss_l1 against the tensor formulation of the same batched loss, as
    test_gpu_detector.py::test_fused_rpn_loss_matches_tensor_formulation does for smooth-L1: values to 1e-5, gradients of every level's
    maps to rtol 1e-4 / atol 1e-6 of the largest entry."""
    from htd_amd import capi
    from htd_amd.core.bbox import set_sample_keys
    from htd_amd.detector.losses import L1Loss
    det = dets['faster_rcnn']
    dev = torch.device(DEV)
    img, metas, gts, _ = inputs(dev)
    det.train()
    rpn = det.rpn_head
    assert type(rpn.loss_bbox) is L1Loss
    with torch.no_grad():
        cls0, reg0 = rpn(det.extract_feat(img))
    coef = torch.tensor([12.9898, 78.233, 37.719, 93.989], device=dev)
    set_sample_keys(lambda cand: torch.frac(torch.sin((cand * coef).sum(-1)) * 43758.5453).abs())
    out, calls, real = {}, [], capi.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    try:
        for fused in (True, False):
            rpn.fused_loss = fused
            cls = [c.clone().requires_grad_() for c in cls0]
            reg = [r.clone().requires_grad_() for r in reg0]
            capi.call = spy
            try:
                losses = rpn.loss_batched(cls, reg, gts, metas)
            finally:
                capi.call = real
            assert ('htd_rpn_loss_l1' in calls) == fused and 'htd_rpn_loss' not in calls
            total = sum(losses['loss_rpn_cls']) + 2.0 * sum(losses['loss_rpn_bbox'])
            total.backward()
            out[fused] = ([float(sum(losses[k]).detach()) for k in ('loss_rpn_cls', 'loss_rpn_bbox')],
                          [t.grad.clone() for t in cls + reg])
            calls.clear()
    finally:
        rpn.fused_loss = True
        set_sample_keys(None)
    (lf, gf), (lt, gt_) = out[True], out[False]
    for a, b in zip(lf, lt):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (lf, lt)
    assert lt[1] > 0
    for a, b in zip(gf, gt_):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * max(1.0, float(b.abs().max())))


@pytest.mark.parametrize('arith', ['six_product', 'h2'])
@pytest.mark.parametrize('scenario', ['plain', 'no_gt_image_and_few_proposals'])
@pytest.mark.parametrize('name', U.MODELS)
def test_static_shape_train_path_matches_per_image_path(dets, name, scenario, arith):
    """forward_train_static against the per-image lists on the same samples (sampler keys a function of the candidate boxes), with the
    bounds of test_gpu_detector.py::test_static_shape_train_path_matches_per_image_path: losses to 2e-5; six-product arithmetic:
    every gradient to 2e-4 of its largest entry; H2 (a layer scales by its tensor's maximum, so padded and per-image tensors round
    differently): every gradient to 1e-2 of its root mean square."""
    from htd_amd import capi
    from htd_amd.core import set_randperm
    from htd_amd.core.bbox import set_sample_keys
    L = capi.lib()
    if arith == 'h2' and L.htd_conv2d_set_h2(-1) != 1:
        pytest.skip('H2 arithmetic switched off')
    prev_h2 = L.htd_conv2d_set_h2(1 if arith == 'h2' else 0)
    det = dets[name]
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    saved_post = det.train_cfg.rpn_proposal.nms_post
    if scenario == 'no_gt_image_and_few_proposals':
        gts, labels = [gts[0], gts[1][:0]], [labels[0], labels[1][:0]]
        det.train_cfg.rpn_proposal.nms_post = 30          # < sampler.num = 48
    det.train()
    head = det.roi_head
    set_randperm(None)                       # the batched samplers (keys), not the replayed CPU permutation
    set_sample_keys(box_keys(dev))
    out = {}
    try:
        for static in (True, False):
            head.static_shapes = static
            if hasattr(head, '_last_static'):
                del head._last_static
            det.zero_grad()
            losses = det(img=img, img_metas=metas, gt_bboxes=gts, gt_labels=labels)
            loss, log_vars = det._parse_losses(losses)
            loss.backward()
            grads = {n: p.grad.detach().clone() for n, p in det.named_parameters() if p.grad is not None}
            out[static] = ({k: float(v) for k, v in log_vars.items()}, grads)
            assert hasattr(head, '_last_static') == static
            if static:
                S = head._last_static
                assert len(S) == _stages(name) and all(int(s.is_pos.sum()) > 0 for s in S)
                if scenario == 'no_gt_image_and_few_proposals':
                    assert all(int((~s.valid).sum()) > 0 for s in S)      # unused slots really occur
    finally:
        L.htd_conv2d_set_h2(prev_h2)
        det.train_cfg.rpn_proposal.nms_post = saved_post
        head.static_shapes = True
        set_sample_keys(None)
        set_randperm(lambda n, device: torch.randperm(n).to(device))
    (l_s, g_s), (l_d, g_d) = out[True], out[False]
    assert set(l_s) == set(l_d)
    for k in l_d:
        assert abs(l_s[k] - l_d[k]) <= 2e-5 * max(1.0, abs(l_d[k])), (k, l_s[k], l_d[k])
    errs = []
    for n in set(g_s) | set(g_d):
        if n not in g_s or n not in g_d:
            assert float((g_s.get(n, g_d.get(n))).abs().max()) == 0.0, n
            continue
        scale = float(g_d[n].abs().max())
        if scale == 0.0:
            assert float(g_s[n].abs().max()) == 0.0, n
            continue
        if arith == 'h2':
            rms = float(g_d[n].double().square().mean().sqrt())
            errs.append((float((g_s[n] - g_d[n]).double().square().mean().sqrt()) / max(rms, 1e-6), n, rms))
        else:
            errs.append((float((g_s[n] - g_d[n]).abs().max()) / max(scale, 1e-5), n, scale))
    errs.sort(reverse=True)
    print(f'{name}.{scenario}.{arith}: worst gradient ratio {errs[0][0]:.3e} ({errs[0][1]})')
    assert errs[0][0] < (1e-2 if arith == 'h2' else 2e-4), errs[:8]


def test_standard_head_static_path_reads_nothing_on_the_host(dets, monkeypatch):
    """StandardRoIHead.forward_train_static -- sampling, RoIAlign, the FC stack, the fused class-specific L1 loss -- and its backward
    run with .item() / .tolist() / bool() / any() / all() / nonzero() of tensors made to raise."""
    from htd_amd import capi
    from htd_amd.core import set_randperm
    from test_iou_losses import _no_host_reads
    det = dets['faster_rcnn']
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    det.train()
    set_randperm(None)
    try:
        with torch.no_grad():
            x = det.extract_feat(img)
        proposal_cfg = det.train_cfg.get('rpn_proposal', det.test_cfg.rpn)
        with torch.no_grad():
            _, (proposals, n_keep) = det.rpn_head.forward_train(x, metas, gts, gt_labels=None, gt_bboxes_ignore=None,
                                                                proposal_cfg=proposal_cfg, padded=True)
        assert det.roi_head.can_train_static(None)
        x = tuple(f.detach().requires_grad_() for f in x)
        calls, real = [], capi.call

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        capi.call = spy
        _no_host_reads(monkeypatch)
        try:
            losses = det.roi_head.forward_train_static(x, metas, proposals, n_keep, gts, labels)
            (losses['loss_cls'] + losses['loss_bbox']).backward()
        finally:
            monkeypatch.undo()
            capi.call = real
    finally:
        set_randperm(lambda n, device: torch.randperm(n).to(device))
    assert 'htd_roi_head_loss_classes' in calls
    assert set(losses) == {'loss_cls', 'acc', 'loss_bbox'}
    assert all(torch.isfinite(v.detach()).all().item() for v in losses.values()) and float(losses['loss_bbox'].detach()) > 0
    assert all(f.grad is not None and torch.isfinite(f.grad).all().item() for f in x[:4])


@pytest.mark.parametrize('scale', ['array', 'float', None])
@pytest.mark.parametrize('name', U.MODELS)
def test_batched_test_postprocessing_equals_the_per_image_loop(dets, name, scale):
    """simple_test of both heads post-processes the whole batch in one pass -- (n, 4 * 80) class-specific boxes in StandardRoIHead --
    and must agree BIT FOR BIT with the reference's per-image loop: images of different shapes and scale factors, a blank image, the
    cut to max_per_img active (the form of test_gpu_detector.py's test of the same name)."""
    det = dets[name]
    dev = torch.device(DEV)
    img, _, _, _ = inputs(dev)
    H, W = img.shape[-2:]
    img = torch.cat([img, img.flip(0) * 0.5, img[:1] * 0.0])                     # 5 images, the last one blank
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas = []
    for i, (h, w) in enumerate(shapes):
        sf = {'array': np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32), 'float': 0.7 + 0.3 * i,
              None: np.ones(4, dtype=np.float32)}[scale]
        metas.append(dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), scale_factor=sf, flip=False))
    det.eval()
    head = det.roi_head
    old_cfg = copy.deepcopy(head.test_cfg)
    rescale = scale is not None
    try:
        head.test_cfg.max_per_img = 37
        with torch.no_grad():
            feats = det.extract_feat(img)
            props = det.rpn_head.simple_test_rpn(feats, metas)
            out = {}
            for mode in (True, False):
                head.batched_test = mode
                if name == 'cascade_rcnn':
                    b, l = head.simple_test_bboxes(feats, props, metas, rescale=rescale)
                else:
                    b, l = head.simple_test_bboxes(feats, metas, props, head.test_cfg, rescale=rescale)
                out[mode] = (b, l, head.simple_test(feats, props, metas, rescale=rescale))
    finally:
        head.batched_test = True
        head.test_cfg = old_cfg
    counts = [int(x.shape[0]) for x in out[False][0]]
    assert max(counts) == 37 and sum(counts) > 60, counts                        # the cut is active; boxes to compare
    for i in range(len(shapes)):
        assert torch.equal(out[True][0][i], out[False][0][i]), i
        assert torch.equal(out[True][1][i], out[False][1][i]), i
        for a, b in zip(out[True][2][i], out[False][2][i]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('name', U.MODELS)
def test_two_trainers_end_bitwise_equal(name):
    """Two Trainers from one seed, two steps each on the static path, end with bitwise equal flat parameters."""
    from htd_amd.configs import build_baseline_detector
    from htd_amd.core import bbox as _bbox, set_randperm
    from htd_amd.runner import Trainer, synthetic_batch
    dev = torch.device(DEV)

    def run():
        torch.manual_seed(0)
        model = build_baseline_detector(cfg=small_cfg(name)).to(dev).train()
        tr = Trainer(model, lr=0.01)
        data = synthetic_batch(2, 256, 320, 311, device=dev, seed=1)
        for _ in range(2):
            out = tr.train_step(data)
        assert hasattr(model.roi_head, '_last_static')
        assert torch.isfinite(out['loss'].detach()).item()
        return tr.flat.flat.detach().clone()
    saved = _bbox._randperm
    set_randperm(None)                       # the device sampler of a production run, whatever an earlier fixture installed
    try:
        a, b = run(), run()
    finally:
        set_randperm(None if saved is _bbox._device_randperm else saved)
    assert torch.isfinite(a).all().item() and torch.equal(a, b)


@pytest.mark.parametrize('name', U.MODELS)
def test_reference_format_checkpoint_loads_and_reproduces_the_fixture(golden, tmp_path, name):
    """A `.pth` in the reference's wire format (meta + state_dict with the reference's keys and logical shapes under a `module.`
    prefix) goes through load_checkpoint(strict=True) into a freshly built detector, which reproduces the reference's detections."""
    from golden_util import seeded_state_value
    from htd_amd.checkpoint import load_checkpoint
    from htd_amd.configs import build_baseline_detector
    g = golden('baselines')
    dev = torch.device(DEV)
    scale = float(g['fc_reg_scale'])
    ref = {}
    for k, shape in zip(g[f'{name}.state_keys'], g[f'{name}.state_shapes']):
        k = str(k)
        if k.endswith('num_batches_tracked'):
            ref[k] = torch.zeros((), dtype=torch.int64)
            continue
        v = torch.from_numpy(np.asarray(seeded_state_value('det.' + k, [int(s) for s in shape if s])))
        ref[k] = v * scale if '.fc_reg.' in k else v
    path = str(tmp_path / 'epoch_3.pth')
    torch.save(dict(meta=dict(epoch=3, iter=100, mmdet_version='2.7.0', CLASSES=('person', )),
                    state_dict={'module.' + k: v for k, v in ref.items()}), path)
    torch.manual_seed(123)                                   # different init: every value must come from the file
    model = build_baseline_detector(cfg=small_cfg(name))
    ckpt = load_checkpoint(model, path, strict=True)
    assert ckpt['meta']['epoch'] == 3
    model = model.to(dev).eval()
    img, metas, _, _ = inputs(dev)
    with torch.no_grad():
        res = model.simple_test(img, metas)
    for i in range(2):
        match_detections(U.dets_array(res[i]), g[f'{name}.test_dets{i}'])
