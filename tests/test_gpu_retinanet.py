"""RetinaNet on a real MI355X: htd_sigmoid_focal_loss and htd_retina_loss against fp64 references and the reference's own fp32
error (tests/golden/retinanet.npz), the detector against the reference run, the fused head loss against its tensor path, the
whole-batch post-processing against the per-image loop, reproducibility, checkpoints and shape changes inside one process.

The ratios measured on the MI355X are in DESIGN.md section 8 f11."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import baselines_util as BU
import dense_fixture_util as D
from dense_fixture_util import EPS32, T, bound as _bound, err as _err  # noqa: F401
import retina_util as U

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------------- the matrix kernel
def _matrix(pred, labels, weight, gamma, alpha, want_loss=True):
    """One raw call of htd_sigmoid_focal_loss -> (loss_out, partial, grad); outputs pre-filled with NaN."""
    from htd_amd import capi
    N, C = pred.shape
    loss = torch.full_like(pred, float('nan')) if want_loss else None
    grad = torch.full_like(pred, float('nan'))
    partial = torch.full((capi.lib().htd_focal_loss_partial_rows(), ), float('nan'), device=pred.device)
    capi.call('htd_sigmoid_focal_loss', capi.ptr(pred), capi.ptr(labels), capi.ptr(weight), N, C, float(gamma), float(alpha),
              capi.ptr(loss), capi.ptr(partial), capi.ptr(grad), capi.current_stream_ptr())
    torch.cuda.synchronize()
    return loss, partial, grad


@pytest.mark.parametrize('i', range(len(U.FOCAL_PARAMS)))
def test_matrix_kernel_against_reference_fp64(golden, i):
    """Element losses, their sum and the gradient against the reference's fp64 run, each within 4 x max(the reference's own fp32
    error, one fp32 ulp of the largest entry); finite at +-90; two runs bitwise equal; the autograd surface agrees."""
    from htd_amd import mmcv_ops as M
    g = golden('retinanet')
    gamma, alpha = U.FOCAL_PARAMS[i]
    pred, labels, weight = (t.to(DEV) for t in U.focal_rows())
    assert float(pred.abs().max()) == 90.0
    loss, partial, grad = _matrix(pred, labels, weight, gamma, alpha)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and torch.isfinite(partial).all()
    p = f'focal.{i}.'
    err32 = g[p + 'err32']
    refs = dict(loss=T(g[p + 'none64']), grad=T(g[p + 'gnone64']), total=T(g[p + 'red64'][2]).reshape(1))
    figures = dict(loss=(_err(loss, refs['loss']), err32[0]), grad=(_err(grad, refs['grad']), err32[1]),
                   total=(_err(partial.double().sum().reshape(1), refs['total']), err32[2]))
    print(f'gamma {gamma} alpha {alpha}: ' + ', '.join(f'{k} {e / _bound(e32, refs[k]):.3f} of the bound' for k, (e, e32) in figures.items()))
    for k, (e, e32) in figures.items():
        assert e <= _bound(e32, refs[k]), (k, e, e32)
    loss2, partial2, grad2 = _matrix(pred, labels, weight, gamma, alpha)
    assert torch.equal(loss, loss2) and torch.equal(partial, partial2) and torch.equal(grad, grad2)
    # without loss_out the sums and the gradient are the same bits
    _, partial3, grad3 = _matrix(pred, labels, weight, gamma, alpha, want_loss=False)
    assert torch.equal(partial, partial3) and torch.equal(grad, grad3)
    x = pred.clone().requires_grad_()
    out = M.sigmoid_focal_loss(x, labels, gamma, alpha, weight, 'sum')
    (out * 2.0).backward()
    assert torch.equal(out.detach(), partial.sum()) and torch.equal(x.grad, grad * 2.0)


@pytest.mark.parametrize('variant', ['mixed', 'allbg', 'w0'])
@pytest.mark.parametrize('C', [1, 3, 80, 81, 128])
@pytest.mark.parametrize('N', [1, 3, 257])
def test_matrix_kernel_shapes(N, C, variant):
    """Fewer rows than a wave, rows x classes that fill no whole float4 / block, the scalar (C % 4 != 0) and the vector path, every row
    background, every weight 0: against the fp64 tensor formula under the same rule, the reference's fp32 error taken from the
    formula's own fp32 run on the case."""
    pred, labels, weight = U.focal_rows(N, C)
    if variant == 'allbg':
        labels[:] = C
    if variant == 'w0':
        weight[:] = 0.
    for gamma, alpha in ((2.0, 0.25), (1.5, 0.5)):
        l64, g64 = U.focal_ref(pred, labels, weight, gamma, alpha)
        l32, g32 = U.focal_ref(pred, labels, weight, gamma, alpha, torch.float32)
        loss, partial, grad = _matrix(pred.to(DEV), labels.to(DEV), weight.to(DEV), gamma, alpha)
        assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and torch.isfinite(partial).all()
        total64 = l64.sum().reshape(1)
        figs = dict(loss=(_err(loss, l64), _err(l32, l64), l64), grad=(_err(grad, g64), _err(g32, g64), g64),
                    total=(_err(partial.double().sum().reshape(1), total64), _err(l32.sum().reshape(1), total64), total64))
        for k, (e, e32, ref) in figs.items():
            assert e <= _bound(e32, ref), (k, gamma, e, e32)
        if variant == 'w0':
            assert float(loss.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0 and float(partial.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- the head kernel
def _head_raw(case, gamma, alpha, pos_weight, box_loss, beta, cw, bw):
    """One raw call of htd_retina_avg_factor + htd_retina_loss on the case (regression maps channel-padded, read in place) ->
    (partial, gcls list, greg list incl. padding, num_pos, avg); gradient buffers pre-filled with NaN."""
    from htd_amd import capi, mmcv_ops as M
    na, C = case['na'], case['C']
    cl = [c.to(DEV).contiguous(memory_format=torch.channels_last) for c in case['cls']]
    rg_full = [r.to(DEV).contiguous(memory_format=torch.channels_last) for r in case['reg']]
    rg = [r[:, :na * 4] for r in rg_full]
    gcls = [torch.full_like(c, float('nan')) for c in cl]
    greg_full = [torch.full_like(r, float('nan')) for r in rg_full]
    anchors, gts = case['anchors'].to(DEV).contiguous(), case['gts'].to(DEV).contiguous()
    labels, assigned = case['gt_labels'].to(DEV).contiguous(), case['assigned'].to(DEV).contiguous()
    B, A = assigned.shape
    num_pos, avg = M.retina_avg_factor(assigned)
    ct, cs, pix = M._level_tables(cl)
    rt, rs, _ = M._level_tables(rg)
    gct, _, _ = M._level_tables(gcls)
    grt, grs, _ = M._level_tables([g_[:, :na * 4] for g_ in greg_full])
    assert list(rs) == [na * 4 + case['reg_pad']] * len(rg) == list(grs)
    partial = torch.full((capi.lib().htd_focal_loss_partial_rows(), 2), float('nan'), device=DEV)
    f4 = (ctypes.c_float * 4)
    capi.call('htd_retina_loss', ct, cs, rt, rs, pix, len(cl), B, na, C, capi.ptr(anchors), capi.ptr(gts), capi.ptr(labels),
              capi.ptr(assigned), A, gts.size(1), f4(0, 0, 0, 0), f4(1, 1, 1, 1), float(gamma), float(alpha), float(pos_weight),
              int(box_loss), float(beta), capi.ptr(avg), float(cw), float(bw), capi.ptr(partial), gct, grt,
              capi.current_stream_ptr())
    torch.cuda.synchronize()
    return partial, gcls, greg_full, num_pos, avg


@pytest.mark.parametrize('box_loss,beta,pos_weight,gamma', [(1, 0.0, -1.0, 2.0), (0, 0.11, -1.0, 2.0), (1, 0.0, 2.0, 2.0),
                                                            (0, 1.0, 2.0, 1.5)])
def test_head_kernel_against_tensor_path_fp64(box_loss, beta, pos_weight, gamma):
    """htd_retina_loss on five levels of 4x5 .. 1x1 pixels, B = 3, channel-padded regression maps, an image without ground truth, an
    image without a positive (the max(., 1) clamp) and invalid anchors: partial sums and both gradient sets against the tensor path
    in fp64 under the rule of the matrix kernel (fp32 error: the tensor path's own fp32 run); padding channels and invalid anchors
    get exact zeros; every element is written (the buffers went in as NaN); two runs are bitwise equal."""
    case = U.head_case()
    na, C = case['na'], case['C']
    alpha, cw, bw = 0.25, 1.0, 0.5
    # level boundaries fall inside a block: the regression units of level 0 (B x 20 pixels x 10 float4s) are no whole number of
    # 256-thread blocks, and the pixel rows of levels 0 and 1 (one wavefront each) no whole number of four-wave blocks
    pix = [h * w for h, w in U.HEAD_CASE_SIZES]
    n_img = case['assigned'].size(0)
    assert (n_img * pix[0] * (na * 4 + case['reg_pad']) // 4) % 256 != 0 and (n_img * (pix[0] + pix[1])) % 4 != 0
    r64 = U.head_ref(case, gamma, alpha, pos_weight, box_loss, beta, cw, bw)
    r32 = U.head_ref(case, gamma, alpha, pos_weight, box_loss, beta, cw, bw, torch.float32)
    partial, gcls, greg_full, num_pos, avg = _head_raw(case, gamma, alpha, pos_weight, box_loss, beta, cw, bw)
    assert num_pos.tolist() == r64['num_pos'].tolist() and int(num_pos[2]) == 0 and float(avg) == r64['avg'] == 23.0
    assert torch.isfinite(partial).all() and all(torch.isfinite(t).all() for t in gcls + greg_full)
    sums = partial.double().sum(0).cpu()
    worst = {}
    for j, name in enumerate(('sum focal', 'sum box')):
        ref = r64['sums'][j].reshape(1)
        e, e32 = _err(sums[j].reshape(1), ref), _err(r32['sums'][j].reshape(1), ref)
        worst[name] = e / _bound(e32, ref)
        assert e <= _bound(e32, ref), (name, e, e32)
    for name, mine, ref64, ref32 in (('grad cls', gcls, r64['gcls'], r32['gcls']),
                                     ('grad reg', [t[:, :na * 4] for t in greg_full], r64['greg'], r32['greg'])):
        big = max(float(t.abs().max()) for t in ref64)
        e32 = max(_err(a, b) for a, b in zip(ref32, ref64))
        bound = 4.0 * max(e32, EPS32 * big)
        e = max(_err(a, b) for a, b in zip(mine, ref64))
        worst[name] = e / bound
        assert e <= bound, (name, e, e32)
    print(f'box_loss {box_loss} pos_weight {pos_weight} gamma {gamma}: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    # exact zeros: padding channels, anchors with assigned < 0 (both maps), non-positive anchors (regression)
    B = case['assigned'].size(0)
    assert all(float(t[:, na * 4:].abs().max()) == 0.0 for t in greg_full)
    gc = torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, C) for t in gcls], 1).cpu()
    gr = torch.cat([t[:, :na * 4].permute(0, 2, 3, 1).reshape(B, -1, 4) for t in greg_full], 1).cpu()
    invalid = case['assigned'] < 0
    assert int(invalid.sum()) > 30 and float(gc[invalid].abs().max()) == 0.0
    assert float(gr[case['assigned'] <= 0].abs().max()) == 0.0
    if box_loss == 1:           # L1: every component of a positive gets the slope +-1 (seeded deltas never equal their target)
        want = bw / r64['avg']
        assert float((gr[case['assigned'] > 0].abs() - want).abs().max()) <= 4 * EPS32 * want
    assert float(gc[case['assigned'] == 0].abs().min()) > 0.0
    again = _head_raw(case, gamma, alpha, pos_weight, box_loss, beta, cw, bw)
    assert torch.equal(partial, again[0]) and all(torch.equal(a, b) for a, b in zip(gcls + greg_full, again[1] + again[2]))


def test_head_kernel_scalar_path_and_autograd_scaling():
    """C = 3 (27 classification channels per pixel: the scalar path) through the autograd surface, with incoming gradients other
    than 1: against the tensor path in fp64."""
    from htd_amd import mmcv_ops as M
    case = U.head_case(C=3, reg_pad=0)
    case['gt_labels'] = case['gt_labels'] % 3
    r64 = U.head_ref(case, 2.0, 0.25, -1.0, 1, 0.0, 1.0, 1.0)
    for scale in (1.0, 3.0):
        cl = [c.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_() for c in case['cls']]
        rg = [r.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_() for r in case['reg']]
        assigned = case['assigned'].to(DEV)
        _, avg = M.retina_avg_factor(assigned)
        lc, lb = M.retina_loss(cl, rg, case['na'], 3, case['anchors'].to(DEV), case['gts'].to(DEV), case['gt_labels'].to(DEV),
                               assigned, avg, (0., 0., 0., 0.), (1., 1., 1., 1.), 2.0, 0.25, -1.0, 1, 0.0)
        ((lc + lb) * scale).backward()
        np.testing.assert_allclose([float(lc.detach()), float(lb.detach())], (r64['sums'] / r64['avg']).numpy(), rtol=1e-5)
        for a, b in zip([t.grad for t in cl + rg], r64['gcls'] + r64['greg']):
            torch.testing.assert_close(a.cpu().double(), b * scale, rtol=1e-4, atol=1e-6 * max(1.0, float(b.abs().max())))


# ---------------------------------------------------------------------------------------------------- the detector
def small_cfg(g):
    from htd_amd.configs import retinanet_config
    cfg = retinanet_config()
    cfg.test_cfg.nms_pre = int(g['nms_pre'])
    return cfg


def inputs(dev):
    return D.inputs(dev, BU.detector_inputs)


@pytest.fixture(scope='module')
def det(golden):
    from htd_amd.configs import build_retinanet_detector
    g = golden('retinanet')
    model = build_retinanet_detector(cfg=small_cfg(g))
    return U.load_fixture_weights_(model, float(g['cls_scale'])).to(torch.device(DEV))


def test_train_step_matches_reference_fixture(det, golden):
    """The bounds of dense_fixture_util.check_train_step; `assigned` equals the fixture's and the step takes one htd_retina_loss."""
    g = golden('retinanet')
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    losses, calls = D.spied(lambda: det.forward_train(img, metas, gts, labels))
    assert 'htd_retina_loss' in calls and calls.count('htd_retina_loss') == 1
    assigned, num_pos, avg = det.bbox_head._last_assigned
    assert torch.equal(assigned.cpu(), T(g['assigned']).long())
    assert num_pos.tolist() == g['num_pos'].tolist() and float(avg) == float(g['num_pos'].sum())
    keys = U.grad_keys(det)
    assert len(keys) == 5 + len(U.EXTRA_GRAD_KEYS), keys
    D.check_train_step(det, g, '', 'retinanet', losses, ('loss_cls', 'loss_bbox'), keys, len(keys))


def test_logits_and_detections_match_reference_fixture(det, golden):
    """Per-level logits and deltas of the training forward within 2.5e-4 (the fixture's strided samples); detections under the
    bounds of dense_fixture_util.check_detections."""
    g = golden('retinanet')
    img, metas, _, _ = inputs(torch.device(DEV))
    det.train()
    with torch.no_grad():
        cls, reg = det.bbox_head(det.extract_feat(img))
    assert tuple(tuple(c.shape[-2:]) for c in cls) == U.LEVEL_SIZES
    worst = 0.0
    for l, (c, r) in enumerate(zip(cls, reg)):
        for name, t in (('cls', c), ('reg', r)):
            ref = g[f'{name}{l}.sample']
            mine = BU.digest(t.cpu())[1]
            worst = max(worst, float(np.abs(mine - ref).max()) / 2.5e-4)
            np.testing.assert_allclose(mine, ref, rtol=0, atol=2.5e-4, err_msg=f'{name}{l}')
    det.eval()
    with torch.no_grad():
        res = det.simple_test(img, metas)
    print(f'retinanet: worst logit ratio {worst:.3f}, worst detection ratio {D.check_detections(res, g, ""):.3f}')


def test_fused_head_loss_matches_tensor_path_bitwise_repeatable_and_reads_nothing(det, monkeypatch):
    """The fused RetinaHead.loss against its tensor path on the small detector (bounds of
    test_gpu_baselines.py::test_fused_l1_rpn_loss_matches_tensor_formulation: values to 1e-5, gradients of every level's maps to
    rtol 1e-4 / atol 1e-6 of the largest entry); two fused runs bitwise equal; the fused path and its backward run with .item() /
    .tolist() / bool() / any() / all() / nonzero() of tensors made to raise."""
    from htd_amd import capi
    from test_iou_losses import _no_host_reads
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    head = det.bbox_head
    with torch.no_grad():
        cls0, reg0 = head(det.extract_feat(img))
    out = {}
    for mode in ('fused', 'fused2', 'tensor'):
        head.fused_loss = mode != 'tensor'
        cls = [c.clone().requires_grad_() for c in cls0]
        reg = [r.clone().requires_grad_() for r in reg0]
        calls, real = [], capi.call

        def spy(name, *a, **k):
            calls.append(name)
            return real(name, *a, **k)
        capi.call = spy
        if mode == 'fused2':
            head.loss(cls, reg, gts, labels, metas)            # caches (anchors, gt padding) are warm: a production step
            _no_host_reads(monkeypatch)
        try:
            losses = head.loss(cls, reg, gts, labels, metas)
            total = sum(losses['loss_cls']) + 2.0 * sum(losses['loss_bbox'])
            total.backward()
        finally:
            monkeypatch.undo()
            capi.call = real
            head.fused_loss = True
        assert ('htd_retina_loss' in calls) == (mode != 'tensor')
        out[mode] = ([sum(losses[k]).detach() for k in ('loss_cls', 'loss_bbox')], [t.grad.clone() for t in cls + reg])
    (lf, gf), (l2, g2), (lt, gt_) = out['fused'], out['fused2'], out['tensor']
    assert all(torch.equal(a, b) for a, b in zip(lf + gf, l2 + g2))
    for a, b in zip(lf, lt):
        assert abs(float(a) - float(b)) <= 1e-5 * max(1.0, abs(float(b))), (lf, lt)
    assert float(lt[1]) > 0
    for a, b in zip(gf, gt_):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * max(1.0, float(b.abs().max())))


@pytest.mark.parametrize('scale', ['array', None])
def test_batched_get_bboxes_equals_the_per_image_loop(det, scale):
    """get_bboxes of the whole batch -- one key launch, one segmented top-k, one NMS -- agrees BIT FOR BIT with the per-image loop:
    images of different shapes and scale factors, a blank image, the cuts to nms_pre and max_per_img active.  NCHW-contiguous copies
    of the maps give, in both forms, exactly what the head's own channels_last maps give."""
    img, _, _, _ = inputs(torch.device(DEV))
    H, W = img.shape[-2:]
    img = torch.cat([img, img.flip(0) * 0.5, img[:1] * 0.0])
    shapes = [(H, W - 24), (H - 16, W), (H - 32, W - 40), (H, W), (H - 8, W - 8)]
    metas = []
    for i, (h, w) in enumerate(shapes):
        sf = np.array([1.0 + 0.13 * i, 0.9 + 0.07 * i] * 2, dtype=np.float32) if scale == 'array' else np.ones(4, dtype=np.float32)
        metas.append(dict(img_shape=(h, w, 3), pad_shape=(H, W, 3), ori_shape=(h, w, 3), scale_factor=sf, flip=False))
    det.eval()
    head = det.bbox_head
    old_cfg = copy.deepcopy(head.test_cfg)
    try:
        head.test_cfg.max_per_img = 37
        with torch.no_grad():
            outs = head(det.extract_feat(img))
            nchw = [[t.contiguous() for t in maps] for maps in outs]
            assert not any(maps[0].is_contiguous(memory_format=torch.channels_last) for maps in nchw)
            res, res_nchw = {}, {}
            for mode in (True, False):
                head.batched_get_bboxes = mode
                res[mode] = head.get_bboxes(*outs, metas, rescale=scale is not None)
                res_nchw[mode] = head.get_bboxes(*nchw, metas, rescale=scale is not None)
    finally:
        head.batched_get_bboxes = True
        head.test_cfg = old_cfg
    counts = [int(d.shape[0]) for d, _ in res[False]]
    assert max(counts) == 37 and sum(counts) > 60, counts
    for (d1, l1), (d2, l2) in zip(res[True], res[False]):
        assert torch.equal(d1, d2) and torch.equal(l1, l2)
    for mode in (True, False):                  # NCHW-contiguous copies of the maps: the same detections in both forms
        for (d1, l1), (d2, l2) in zip(res_nchw[mode], res[mode]):
            assert torch.equal(d1, d2) and torch.equal(l1, l2)


def test_reference_format_checkpoint_round_trip(golden, tmp_path):
    """dense_fixture_util.check_checkpoint_round_trip on the RetinaNet fixture."""
    from htd_amd.configs import build_retinanet_detector
    g = golden('retinanet')
    state = U.fixture_state(g['state_keys'], g['state_shapes'], float(g['cls_scale']))
    img, metas, _, _ = inputs(torch.device(DEV))
    ckpt = D.check_checkpoint_round_trip(lambda: build_retinanet_detector(cfg=small_cfg(g)), state, g, '', img, metas, tmp_path, tol=1e-2)
    assert ckpt['meta']['epoch'] == 3


def test_transposed_batch_after_a_batch_gives_the_result_of_a_fresh_head(det):
    """An H x W batch and then a W x H batch in one process: losses, gradients and detections of the second equal those of a head
    that has seen nothing before (caches key on the feature-map shapes, not on their products)."""
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    img_t = img.transpose(2, 3).contiguous()
    H, W = img_t.shape[-2:]
    metas_t = [dict(m, img_shape=(H - 3, W, 3), pad_shape=(H, W, 3), ori_shape=(H - 3, W, 3)) for m in metas]
    gts_t = [x[:, [1, 0, 3, 2]].contiguous() for x in gts]

    def run(model, first):
        out = []
        for im, ms, gs in ([(img, metas, gts)] if first else []) + [(img_t, metas_t, gts_t)]:
            model.train()
            model.zero_grad()
            losses = model.forward_train(im, ms, gs, labels)
            loss, _ = model._parse_losses(losses)
            loss.backward()
            model.eval()
            with torch.no_grad():
                res = model.simple_test(im, ms)
            out = [loss.detach().clone(), model.bbox_head.retina_cls.weight.grad.clone(), model.bbox_head.retina_reg.bias.grad.clone(),
                   [BU.dets_array(r) for r in res]]
        return out
    fresh = copy.deepcopy(det)
    for m in (det, fresh):
        m.bbox_head.__dict__.pop('_inside_cache', None)
        m.bbox_head.__dict__.pop('_prior_cache', None)
    a, b = run(det, True), run(fresh, False)
    assert torch.isfinite(a[0]).item() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and sum(len(x) for x in a[3]) > 0


def test_train_and_test_cli_run_the_retinanet_config(golden, tmp_path):
    """`python -m htd_amd.train` for one epoch with evaluation and `python -m htd_amd.test` on its checkpoint, from a config file
    that holds retinanet_config() (the reference's merged retinanet_r50_fpn_1x_coco, test_retinanet.py) on a tiny COCO-format set."""
    import json
    import os
    import re
    import subprocess
    import sys
    from test_datasets import write_png_set
    from test_gpu_test_loop import SHAPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data_root = str(tmp_path / 'data')
    os.makedirs(data_root)
    ann = write_png_set(data_root, SHAPES, seed=4)
    cfg = small_cfg(golden('retinanet'))
    cfg.test_cfg.score_thr = 0.0
    for split in (cfg.data.train, cfg.data.val, cfg.data.test):
        split.ann_file, split.img_prefix = ann, os.path.join(data_root, 'imgs')
    cfg.data.test.pipeline[1]['img_scale'] = (128, 128)
    cfg.data.val.pipeline[1]['img_scale'] = (128, 128)
    cfg.data.train.pipeline[2]['img_scale'] = (128, 128)
    cfg.model.pretrained = None
    cfg.data.workers_per_gpu = 0
    cfg.total_epochs = 1
    cfg.log_config = dict(interval=2, hooks=[dict(type='TextLoggerHook')])
    cfg_file = tmp_path / 'retinanet_tiny.py'
    cfg_file.write_text(''.join(f'{k} = {v!r}\n' for k, v in cfg.to_dict().items()))
    work = tmp_path / 'work'

    def cli(args):
        return subprocess.run([sys.executable] + args, cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True,
                              text=True, timeout=600)
    p = cli(['-m', 'htd_amd.train', str(cfg_file), '--work-dir', str(work), '--seed', '1'])
    assert p.returncode == 0, p.stderr[-4000:]
    (name, ) = [f for f in os.listdir(work) if f.endswith('.log.json')]
    lines = [json.loads(l) for l in open(os.path.join(work, name))]
    train = [l for l in lines if l.get('mode') == 'train']
    assert train and all({'loss_cls', 'loss_bbox', 'loss'} <= set(l) and np.isfinite(l['loss']) for l in train)
    assert any(l.get('mode') == 'val' and 'bbox_mAP' in l for l in lines)
    p = cli(['-m', 'htd_amd.test', str(cfg_file), os.path.join(str(work), 'epoch_1.pth'), '--eval', 'bbox'])
    assert p.returncode == 0, p.stderr[-3000:]
    assert re.search(r"'bbox_mAP'(?::|,) ([^,)}]+)", p.stdout) is not None, (p.stdout[-3000:], p.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- more than one sweep of a grid
def test_matrix_kernel_wraps_its_grid():
    """30 000 x 80: 600 000 float4 units against the 524 288 threads of the fixed grid, so the grid-stride loop takes a second
    sweep; and 7 000 x 81 on the scalar path (567 000 units).  Against the fp64 formula under the rule of the shape cases."""
    for N, C in ((30000, 80), (7000, 81)):
        pred, labels, weight = U.focal_rows(N, C)
        assert N * (C // 4 if C % 4 == 0 else C) > 2048 * 256
        l64, g64 = U.focal_ref(pred, labels, weight, 2.0, 0.25)
        l32, g32 = U.focal_ref(pred, labels, weight, 2.0, 0.25, torch.float32)
        loss, partial, grad = _matrix(pred.to(DEV), labels.to(DEV), weight.to(DEV), 2.0, 0.25)
        total64 = l64.sum().reshape(1)
        figs = dict(loss=(_err(loss, l64), _err(l32, l64), l64), grad=(_err(grad, g64), _err(g32, g64), g64),
                    total=(_err(partial.double().sum().reshape(1), total64), _err(l32.sum().reshape(1), total64), total64))
        for k, (e, e32, ref) in figs.items():
            assert e <= _bound(e32, ref), (N, C, k, e, e32)


def test_head_kernels_wrap_their_grids():
    """B = 2 on levels of 64 x 72 and 2 x 3 pixels: 9 228 pixel rows against 8 192 wavefronts (classification part), 590 592
    regression float4s against 524 288 threads (the maps padded to 256 channels), 41 526 anchors per image against the 16 384 of a
    counting sweep and 83 052 keys against 32 768 per sweep.  htd_retina_loss, htd_retina_avg_factor, htd_retina_grad_scale and
    htd_retina_keys against the tensor path in fp64 / the tensor formula."""
    from htd_amd import capi, mmcv_ops as M
    case = U.head_case(B=2, reg_pad=220, sizes=((64, 72), (2, 3)), strides=(8, 256), scale=14.0, tag='retina.wrap')
    na, C = case['na'], case['C']
    B, A = case['assigned'].shape
    rows = B * (64 * 72 + 6)
    assert rows > 2048 * 4 and rows * 64 > 2048 * 256 and A > 64 * 256 and B * A > 2048 * 16
    args = (2.0, 0.25, -1.0, 1, 0.0, 1.0, 0.5)
    r64, r32 = U.head_ref(case, *args), U.head_ref(case, *args, torch.float32)
    assert int(r64['num_pos'].min()) == 0 and int(r64['num_pos'].max()) > 20
    partial, gcls, greg_full, num_pos, avg = _head_raw(case, *args)
    assert num_pos.tolist() == r64['num_pos'].tolist() and float(avg) == r64['avg']
    sums = partial.double().sum(0).cpu()
    for j in range(2):
        ref = r64['sums'][j].reshape(1)
        assert _err(sums[j].reshape(1), ref) <= _bound(_err(r32['sums'][j].reshape(1), ref), ref), j
    greg = [t[:, :na * 4] for t in greg_full]
    for mine, ref64, ref32 in ((gcls, r64['gcls'], r32['gcls']), (greg, r64['greg'], r32['greg'])):
        big = max(float(t.abs().max()) for t in ref64)
        e32 = max(_err(a, b) for a, b in zip(ref32, ref64))
        assert max(_err(a, b) for a, b in zip(mine, ref64)) <= 4.0 * max(e32, EPS32 * big)
    assert all(float(t[:, na * 4:].abs().max()) == 0.0 for t in greg_full)
    # the in-place scaling: factor 1 leaves the bits, any other factor multiplies every element once
    before = [t.clone() for t in gcls + greg_full]
    gct, gcs, pix = M._level_tables(gcls)
    grt, grs, _ = M._level_tables(greg)
    one, f = torch.ones(1, device=DEV), torch.tensor([3.0], device=DEV)
    for g_c, g_b in ((one, one), (f, one), (one, f)):
        capi.call('htd_retina_grad_scale', gct, gcs, grt, grs, pix, len(gcls), B, na, C, capi.ptr(g_c), capi.ptr(g_b),
                  capi.current_stream_ptr())
    assert all(torch.equal(a, b * 3.0) for a, b in zip(gcls + greg_full, before))
    # keys
    cl = [c.to(DEV).contiguous(memory_format=torch.channels_last) for c in case['cls']]
    keys = M.retina_keys(cl, na, C)
    ref = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1, C) for c in case['cls']], 1).max(-1)[0].double().sigmoid()
    assert keys.shape == (B, A) and _err(keys, ref) <= 2 * EPS32


def test_keys_of_unaligned_image_slices_and_layout_gate():
    """A one-class head (9 channels per pixel) on a 3 x 5 level: image 1 of the batch starts 540 bytes into the map, which the
    scalar form of htd_retina_keys must take (the per-image loop of get_bboxes hands it such slices).  And NCHW-contiguous maps,
    which the fused loss cannot read in place, take the tensor path instead of raising."""
    from htd_amd import mmcv_ops as M
    x = seeded = torch.randn(3, 9, 3, 5, generator=torch.Generator().manual_seed(3)).to(DEV).contiguous(memory_format=torch.channels_last)
    assert x[1].data_ptr() % 16 != 0
    whole = M.retina_keys([x], 9, 1)
    for b in range(3):
        assert torch.equal(M.retina_keys([x[b][None]], 9, 1)[0], whole[b])
    assert _err(whole, seeded.permute(0, 2, 3, 1).reshape(3, -1).cpu().double().sigmoid()) <= 2 * EPS32
    case = U.head_case()
    assert M.nhwc_channel_stride(case['cls'][0].to(DEV)) is None
    assert M.nhwc_channel_stride(case['cls'][0].to(DEV).contiguous(memory_format=torch.channels_last)) == 720


def test_nchw_maps_take_the_tensor_path_and_second_backward_raises(det):
    from htd_amd import capi
    img, metas, gts, labels = inputs(torch.device(DEV))
    det.train()
    head = det.bbox_head
    with torch.no_grad():
        cls0, reg0 = head(det.extract_feat(img))
    calls, real = [], capi.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    out = {}
    for layout in ('nhwc', 'nchw'):
        fmt = torch.channels_last if layout == 'nhwc' else torch.contiguous_format
        cls = [c.clone(memory_format=fmt).requires_grad_() for c in cls0]
        reg = [r.clone(memory_format=fmt).requires_grad_() for r in reg0]
        calls.clear()
        capi.call = spy
        try:
            losses = head.loss(cls, reg, gts, labels, metas)
        finally:
            capi.call = real
        # level 0 is 16 x 20: its contiguous form is not channels_last
        assert ('htd_retina_loss' in calls) == (layout == 'nhwc')
        out[layout] = (losses, cls)
    for k in ('loss_cls', 'loss_bbox'):
        a, b = float(sum(out['nhwc'][0][k]).detach()), float(sum(out['nchw'][0][k]).detach())
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b))
    losses, cls = out['nhwc']
    total = sum(losses['loss_cls']) + 2.0 * sum(losses['loss_bbox'])
    total.backward(retain_graph=True)
    first = cls[0].grad.clone()
    with pytest.raises(RuntimeError, match='second backward'):
        total.backward()
    assert torch.equal(cls[0].grad, first)


# ---------------------------------------------------------------------------------------------------- FPN with extra convolutions
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('mode', ['on_input', 'on_lateral', 'on_output'])
def test_fpn_extra_convs_against_torch_fp64(mode, relu):
    """FPN(start_level=1, add_extra_convs=mode) on the GPU in its three forms -- the chained fused top-down path of a training
    step, the fused path without autograd, interpolate + add (fused_top_down=False) -- against F.conv2d / F.interpolate in fp64 with
    the same weights: outputs, and the input gradients of the training form."""
    import torch.nn.functional as F
    from htd_amd.detector.fpn import FPN
    torch.manual_seed(5)
    ins = [32, 64, 128, 256]
    neck = FPN(ins, 32, 5, start_level=1, add_extra_convs=mode, relu_before_extra_convs=relu)
    neck.init_weights()
    for m in neck.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.normal_(m.bias, std=0.1)
    feats = [torch.randn(2, c, 40 // 2 ** i, 56 // 2 ** i) for i, c in enumerate(ins)]

    def reference(xs):
        conv = lambda m, x: F.conv2d(x, m.conv.weight.detach().double().contiguous(), m.conv.bias.detach().double(), m.conv.stride,
                                     m.conv.padding)
        lat = [conv(m, xs[i + 1]) for i, m in enumerate(neck.lateral_convs)]
        for i in range(2, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode='nearest')
        outs = [conv(neck.fpn_convs[i], lat[i]) for i in range(3)]
        outs.append(conv(neck.fpn_convs[3], dict(on_input=xs[3], on_lateral=lat[2], on_output=outs[2])[mode]))
        outs.append(conv(neck.fpn_convs[4], F.relu(outs[3]) if relu else outs[3]))
        return outs
    xs64 = [f.double().requires_grad_() for f in feats]
    ref = reference(xs64)
    coef = [torch.randn_like(o) for o in ref]
    sum((o * c).sum() for o, c in zip(ref, coef)).backward()
    neck = neck.to(DEV)

    def run(grad, fused):
        neck.fused_top_down = fused
        xs = [f.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(grad) for f in feats]
        with torch.set_grad_enabled(grad):
            outs = neck(xs)
        return xs, outs
    try:
        for grad, fused in ((True, True), (False, True), (True, False)):
            xs, outs = run(grad, fused)
            assert len(outs) == 5
            for o, r in zip(outs, ref):
                assert o.shape == r.shape
                torch.testing.assert_close(o.detach().cpu().double(), r.detach(), rtol=1e-4, atol=1e-4 * float(r.detach().abs().max()))
            if grad:
                sum((o * c.to(DEV).float()).sum() for o, c in zip(outs, coef)).backward()
                assert xs[0].grad is None                                                   # start_level = 1
                for x, r in zip(xs[1:], xs64[1:]):
                    torch.testing.assert_close(x.grad.cpu().double(), r.grad, rtol=1e-3, atol=1e-4 * float(r.grad.abs().max()))
    finally:
        del neck.fused_top_down
