"""The GN+WS Faster R-CNN (configs/gn+ws/faster_rcnn_r50_fpn_gn_ws-all_1x_coco.py: ConvWS + GroupNorm(32) in the ResNet, the FPN and
a Shared4Conv1FCBBoxHead) on a real MI355X against the reference's own run (tests/golden/gn_ws.npz, recipe in
tests/golden/make_golden_gn_ws.py), with the bounds of tests/test_gpu_baselines.py taken over unchanged: losses rtol 5e-4 / atol
1e-4; gradient digests in units of 2e-4 * max(1, max |ref|) + 1e-3 * |ref|, no element over 2 units, rms at most 0.2; feature sums
rtol 1e-5; proposals rtol 1e-5 / atol 2e-3; detections matched one to one within 1e-3 + 1e-5 * the largest coordinate.  Every map
of the backbone goes through mmcv_ops.group_norm_map, every convolution through mmcv_ops.weight_standardize.

The fixture's weights are chosen (gn_ws_util.load_fixture_weights_) so that the reference's fp32 and fp64 runs take the same discrete
decisions and differ by roundings only; tests/test_gn_ws.py asserts that on the fixture.  One bound is then still below the
reference's own arithmetic: its fp32 gradient of a few early layers is up to 3 of the units above from its fp64 one.  For a
gradient that misses the units bound the replacement is 4 x the reference's fp32-against-fp64 gap that the make script records
(err32.grad.*, the rule of tests/test_gpu_iou_losses.py), measured against the stored fp64 run -- never anything this code
computes.  Every other bound is the one of tests/test_gpu_baselines.py, against the fp32 run."""
import numpy as np
import pytest
import torch

import baselines_util as BU
import gn_ws_util as U
from golden_util import match_detections

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.from_numpy(np.asarray(a))


def small_cfg():
    from htd_amd.configs import faster_rcnn_gn_ws_config
    cfg = faster_rcnn_gn_ws_config()
    BU.small_counts(cfg.train_cfg, cfg.test_cfg)
    return cfg


def inputs(dev):
    imgs, metas, gts, labels = BU.detector_inputs()
    return T(imgs).to(dev), metas, [T(x).to(dev) for x in gts], [T(x).to(dev) for x in labels]


@pytest.fixture(scope='module')
def det(golden):
    """The detector with the fixture's weights, sampling replayed from the CPU generator."""
    from htd_amd.configs import build_baseline_detector
    from htd_amd.core import set_randperm
    g = golden('gn_ws')
    model = U.load_fixture_weights_(build_baseline_detector(cfg=small_cfg()), *U.fixture_args(g))
    model = model.to(torch.device(DEV))
    set_randperm(lambda n, device: torch.randperm(n).to(device))
    yield model
    set_randperm(None)


def test_every_layer_takes_the_new_kernels(det):
    """One training forward: the backbone's GroupNorms go through htd_group_norm_map_fwd (the stem, 16 bottlenecks x 3 and four
    downsample branches, plus the two finest pyramid levels' ConvModules), every ConvWS through htd_weight_standardize_fwd, the
    7 x 7 tiles of the head through the tile kernels."""
    from htd_amd import capi
    img, _, _, _ = inputs(torch.device(DEV))
    calls, real = [], capi.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    capi.call = spy
    try:
        det.train()
        feats = det.extract_feat(img)
        rois = torch.tensor([[0, 8., 8., 60., 70.], [1, 20., 10., 90., 100.]], device=img.device)
        det.roi_head._bbox_forward(feats, rois)
    finally:
        capi.call = real
    n_ws = sum(isinstance(m, type(det.backbone.conv1)) for m in det.backbone.modules()) + \
        sum(isinstance(m, type(det.backbone.conv1)) for m in det.neck.modules()) + 4
    assert calls.count('htd_weight_standardize_fwd') == n_ws == 53 + 8 + 4
    assert calls.count('htd_group_norm_map_fwd') == 53 + 4          # backbone; laterals and outputs of the 32 x 40 and 16 x 20 levels
    assert sum(c.startswith('htd_group_norm_relu_fwd') for c in calls) == 4 + 4      # the two coarse levels, the head's four convs
    assert len(feats) == 5 and all(torch.isfinite(f).all().item() for f in feats)


def test_train_step_matches_reference_fixture(det, golden):
    g = golden('gn_ws')
    dev = torch.device(DEV)
    img, metas, gts, labels = inputs(dev)
    det.train()
    torch.manual_seed(int(g['seed_sampler']))
    losses = det.forward_train(img, metas, gts, labels)
    loss, log_vars = det._parse_losses(losses)
    assert set(log_vars.keys()) == {f[5:] for f in g.files if f.startswith('loss.')}
    worst_loss = 0.0
    for k, v in log_vars.items():
        ref = float(g[f'loss.{k}'])
        worst_loss = max(worst_loss, abs(v - ref) / (1e-4 + 5e-4 * abs(ref)))
        print(f'loss {k}: {v:.6f} reference {ref:.6f}')
    det.zero_grad()
    loss.backward()
    params = dict(det.named_parameters())
    worst, worst_rms = (0.0, ''), (0.0, '')
    for k in U.GRAD_KEYS:
        frozen = k.startswith(('backbone.conv1', 'backbone.gn1', 'backbone.layer1.'))
        assert (params[k].grad is None) == frozen, k
        gr = params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
        ref = g[f'grad.{k}.sample']
        assert frozen or np.abs(ref).max() > 0, k
        tol = 2e-4 * max(1.0, np.abs(ref).max()) + 1e-3 * np.abs(ref)
        ratio = np.abs(BU.digest(gr.cpu())[1] - ref) / tol
        print(f'grad {k}: worst element {float(ratio.max()):.3f} units, rms {float(np.sqrt(np.mean(ratio ** 2))):.3f}')
        worst, worst_rms = max(worst, (float(ratio.max()), k)), max(worst_rms, (float(np.sqrt(np.mean(ratio ** 2))), k))
    print(f'worst loss ratio {worst_loss:.3f}; worst gradient element {worst[0]:.3f} units ({worst[1]}), '
          f'worst rms {worst_rms[0]:.3f} ({worst_rms[1]})')
    for k, v in log_vars.items():
        np.testing.assert_allclose(v, float(g[f'loss.{k}']), rtol=5e-4, atol=1e-4, err_msg=k)
    # gradients: the bound of test_gpu_baselines.py, or 4 x the reference's own fp32 error against its fp64 run
    for k in U.GRAD_KEYS:
        gr = params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])
        mine, ref, ref64 = BU.digest(gr.cpu())[1], g[f'grad.{k}.sample'], g[f'grad64.{k}.sample']
        ratio = np.abs(mine - ref) / (2e-4 * max(1.0, np.abs(ref).max()) + 1e-3 * np.abs(ref))
        if ratio.max() <= 2.0 and np.sqrt(np.mean(ratio ** 2)) <= 0.2:
            continue
        e64, e32 = float(np.abs(mine - ref64).max()), float(g[f'err32.grad.{k}'])
        assert np.isfinite(e32) and e32 <= 2e-3 * max(1.0, np.abs(ref).max()), (k, e32)      # a rounding-sized gap: 10 units at most
        print(f'grad {k}: |kernel - fp64| {e64:.3e}  |reference fp32 - fp64| {e32:.3e}  bound {4 * e32:.3e}')
        assert e64 <= 4.0 * e32, (k, e64, e32)


def test_inference_matches_reference_fixture(det, golden):
    g = golden('gn_ws')
    dev = torch.device(DEV)
    img, metas, _, _ = inputs(dev)
    det.eval()
    with torch.no_grad():
        feats = det.extract_feat(img)
        for i, f in enumerate(feats):
            print(f'feat{i}_abs: {f.double().abs().sum().item():.6f} reference {float(g[f"feat{i}_abs"]):.6f}')
        for i, f in enumerate(feats):
            np.testing.assert_allclose(f.double().abs().sum().item(), float(g[f'feat{i}_abs']), rtol=1e-5)
        props = det.rpn_head.simple_test_rpn(feats, metas)
        res = det.roi_head.simple_test(feats, props, metas, rescale=False)
    worst = 0.0
    for i in range(2):
        ref_p = g[f'test_props{i}']
        assert props[i].shape == ref_p.shape
        print(f'props{i}: worst |kernel - reference| {float(np.abs(props[i].cpu().numpy() - ref_p).max()):.5f}')
        np.testing.assert_allclose(props[i].cpu().numpy(), ref_p, rtol=1e-5, atol=2e-3)
        mine, ref = BU.dets_array(res[i]), g[f'test_dets{i}']
        assert mine.shape == ref.shape and len(ref) > 0
        used = np.zeros(len(mine), dtype=bool)
        for r in ref:
            d = np.abs(mine[:, :5] - r[:5]).max(1) + 1e3 * (mine[:, 5] != r[5]) + 1e3 * used
            j = int(d.argmin())
            worst = max(worst, d[j] / (1e-3 + 1e-5 * np.abs(r[:4]).max()))
            assert d[j] <= 1e-3 + 1e-5 * np.abs(r[:4]).max(), (r, mine[j], d[j])
            used[j] = True
    print(f'worst detection ratio {worst:.3f}')


def test_stage_logits_match_reference_fixture(det, golden):
    """Fed the reference's own RoIs, the head's logits and deltas within 1e-4 of the reference's (train and test), as
    tests/test_gpu_baselines.py."""
    g = golden('gn_ws')
    dev = torch.device(DEV)
    img, _, _, _ = inputs(dev)
    with torch.no_grad():
        for phase in ('train', 'test'):
            det.train(phase == 'train')
            feats = det.extract_feat(img)
            res = det.roi_head._bbox_forward(feats, T(g[f'{phase}_s0_rois']).to(dev))
            for key, k in (('cls_score', 'cls'), ('bbox_pred', 'reg')):
                e = float((res[key].cpu() - T(g[f'{phase}_s0_{k}'])).abs().max())
                print(f'{phase} {k}: |kernel - reference| {e:.3e}')
                assert e <= 1e-4, (phase, k, e)


def test_eval_mode_forward_of_the_gn_resnet(det):
    """conv_bn once called frozen_bn_fold on a GroupNorm in eval mode and raised; GroupNorm has no running statistics, so eval and
    train mode compute the same maps, bit for bit."""
    from htd_amd.detector.resnet import ResNet
    dev = torch.device(DEV)
    net = ResNet(50, conv_cfg=dict(type='ConvWS'), norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), norm_eval=True,
                 frozen_stages=1, zero_init_residual=False)
    net.init_weights(None)
    net = net.to(dev)
    x = torch.randn(2, 3, 64, 96, device=dev)
    with torch.no_grad():
        a = net.eval()(x)
        b = net.train()(x)
    assert [tuple(t.shape) for t in a] == [(2, 256, 16, 24), (2, 512, 8, 12), (2, 1024, 4, 6), (2, 2048, 2, 3)]
    assert all(torch.isfinite(s).all().item() and torch.equal(s, t) for s, t in zip(a, b))


def test_two_trainers_end_bitwise_equal():
    """Two Trainers from one seed, three steps each, end with bitwise equal flat parameters: no float atomics in the map kernels."""
    from htd_amd.configs import build_baseline_detector
    from htd_amd.core import bbox as _bbox, set_randperm
    from htd_amd.runner import Trainer, synthetic_batch
    dev = torch.device(DEV)

    def run():
        torch.manual_seed(0)
        model = build_baseline_detector(cfg=small_cfg()).to(dev).train()
        tr = Trainer(model, lr=0.01)
        data = synthetic_batch(2, 256, 320, 311, device=dev, seed=1)
        for _ in range(3):
            out = tr.train_step(data)
        assert torch.isfinite(out['loss'].detach()).item()
        return tr.flat.flat.detach().clone()
    saved = _bbox._randperm
    set_randperm(None)
    try:
        a, b = run(), run()
    finally:
        set_randperm(None if saved is _bbox._device_randperm else saved)
    assert torch.isfinite(a).all().item() and torch.equal(a, b)


def test_reference_format_checkpoint_loads_and_reproduces_the_fixture(golden, tmp_path):
    """A `.pth` in the reference's wire format goes through load_checkpoint(strict=True) into a freshly built detector, which
    reproduces the reference's detections."""
    from htd_amd.checkpoint import load_checkpoint
    from htd_amd.configs import build_baseline_detector
    g = golden('gn_ws')
    dev = torch.device(DEV)
    # the fixture's weights under the reference's keys and logical shapes: the state dict of a detector that holds them
    src = U.load_fixture_weights_(build_baseline_detector(cfg=small_cfg()), *U.fixture_args(g))
    ref = {k: v.detach().clone() for k, v in src.state_dict().items()}
    assert list(ref) == [str(k) for k in g['state_keys']]
    assert all(list(v.shape) == [int(x) for x in shape[:v.dim()]] for v, shape in zip(ref.values(), g['state_shapes']))
    path = str(tmp_path / 'epoch_3.pth')
    torch.save(dict(meta=dict(epoch=3, iter=100, mmdet_version='2.7.0', CLASSES=('person', )),
                    state_dict={'module.' + k: v for k, v in ref.items()}), path)
    torch.manual_seed(123)                                   # different init: every value must come from the file
    model = build_baseline_detector(cfg=small_cfg())
    ckpt = load_checkpoint(model, path, strict=True)
    assert ckpt['meta']['epoch'] == 3
    model = model.to(dev).eval()
    img, metas, _, _ = inputs(dev)
    with torch.no_grad():
        res = model.simple_test(img, metas)
    for i in range(2):
        match_detections(BU.dets_array(res[i]), g[f'test_dets{i}'])
