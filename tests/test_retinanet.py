"""RetinaNet without a GPU: the configuration against the reference's merged config, the state dict, FocalLoss in fp64 against the
reference's own run (tests/golden/retinanet.npz), FPN with extra convolutions, PseudoSampler, the tensor-path RetinaHead.loss and
the new entry points of the C ABI."""
import json
import os

import numpy as np
import pytest
import torch

import baselines_util as BU
from dense_fixture_util import T
import retina_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_retinanet_config_equals_the_reference_merged_config():
    from htd_amd.configs import retinanet_config
    ref = json.load(open(os.path.join(GOLDEN, 'retinanet_r50_fpn_1x_coco_cfg.json')))
    cfg = retinanet_config()
    mine = json.loads(json.dumps({k: (cfg[k].to_dict() if hasattr(cfg[k], 'to_dict') else cfg[k]) for k in U.CFG_KEYS}))
    assert mine == ref
    with pytest.raises(ValueError):
        retinanet_config(34)


def test_state_dict_keys_and_shapes_equal_the_fixture(golden):
    from htd_amd.configs import build_retinanet_detector
    g = golden('retinanet')
    det = build_retinanet_detector()
    sd = det.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_keys']]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == g['state_shapes'].tolist()
    assert type(det).__name__ == 'RetinaNet' and det.bbox_head.sampling is False
    assert type(det.bbox_head.sampler).__name__ == 'PseudoSampler'
    b = det.bbox_head.retina_cls.bias
    assert torch.allclose(b.sigmoid(), torch.full_like(b, 0.01))             # bias_init_with_prob(0.01)
    with pytest.raises(NotImplementedError):
        det.aug_test([], [])
    from htd_amd.apis import _num_classes
    assert _num_classes(det) == 80
    from htd_amd.configs import build_baseline_detector, retinanet_config
    assert type(build_baseline_detector(cfg=retinanet_config())).__name__ == 'RetinaNet'
    with pytest.raises(ValueError, match='kind'):          # the kinds of that builder stay the two-stage ones
        build_baseline_detector('retinanet')


@pytest.mark.parametrize('i', range(len(U.FOCAL_PARAMS)))
def test_focal_loss_fp64_equals_the_reference(golden, i):
    """Every reduction and weight shape of FocalLoss.forward in fp64 against the reference's run, to 1e-12 relative; the fp32
    module stays within the reference's own fp32 error (x 4) of it."""
    from htd_amd.registry import build_loss
    g = golden('retinanet')
    gamma, alpha = U.FOCAL_PARAMS[i]
    mod = build_loss(dict(type='FocalLoss', use_sigmoid=True, gamma=gamma, alpha=alpha, loss_weight=1.0))
    pred0, labels, weight0 = U.focal_rows()
    C = pred0.size(1)
    pred, w = pred0.double().requires_grad_(), weight0.double()
    wnc = w.view(-1, 1) * torch.linspace(0.5, 1.5, C, dtype=torch.float64).view(1, -1)
    red = torch.stack([mod(pred, labels, w), mod(pred, labels, w, avg_factor=U.AVG), mod(pred, labels, w, reduction_override='sum'),
                       mod(pred, labels), mod(pred, labels, reduction_override='sum'), mod(pred, labels, wnc, avg_factor=U.AVG),
                       mod(pred, labels, wnc.reshape(-1), avg_factor=U.AVG)])
    none = mod(pred, labels, w, reduction_override='none')
    none.sum().backward()
    p = f'focal.{i}.'
    assert torch.isfinite(none).all() and torch.isfinite(pred.grad).all()
    np.testing.assert_allclose(red.detach().numpy(), g[p + 'red64'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(none.detach().numpy(), g[p + 'none64'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(pred.grad.numpy(), g[p + 'gnone64'], rtol=1e-12, atol=1e-300)
    none32 = mod(pred0.clone(), labels, weight0, reduction_override='none')
    assert float((none32.double() - T(g[p + 'none64'])).abs().max()) <= 4 * max(float(g[p + 'err32'][0]), 2.0 ** -23 * float(g[p + 'none64'].max()))
    with pytest.raises(ValueError):
        mod(pred, labels, w, avg_factor=3.0, reduction_override='sum')
    with pytest.raises(AssertionError):
        build_loss(dict(type='FocalLoss', use_sigmoid=False))


def test_mmcv_ops_focal_surface_on_the_cpu():
    """The CPU fallback of mmcv_ops.sigmoid_focal_loss is the tensor formula (stable form): values and gradient against the
    reference arithmetic in fp64, finite at +-90."""
    from htd_amd import mmcv_ops as M
    pred, labels, weight = U.focal_rows(16, 5)
    l64, g64 = U.focal_ref(pred, labels, weight, 2.0, 0.25)
    x = pred.double().requires_grad_()
    out = M.sigmoid_focal_loss(x, labels, 2.0, 0.25, weight.double(), 'none')
    out.sum().backward()
    torch.testing.assert_close(out.detach(), l64, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(x.grad, g64, rtol=1e-9, atol=1e-12)
    m = M.SigmoidFocalLoss(2.0, 0.25)
    torch.testing.assert_close(m(pred.double(), labels), U.focal_ref(pred, labels, None, 2.0, 0.25)[0].mean(), rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        M.sigmoid_focal_loss(x, labels.float(), 2.0, 0.25, None, 'none')


@pytest.mark.parametrize('source', ['on_input', 'on_lateral', 'on_output', True])
def test_fpn_extra_convs_layout(source):
    """Module layout of FPN with extra levels against the closed form of necks/fpn.py:137-155, and the source rule of :200-215:
    every stand-in convolution fills its output with a value of its own, so what the first extra convolution was fed names its
    producer -- the last backbone input, the top lateral or the last output."""
    from htd_amd.detector.fpn import FPN
    ins = [8, 16, 32, 64]
    plain = FPN(ins, 12, 5, start_level=1)
    assert len(plain.fpn_convs) == 3 and plain.add_extra_convs is False              # the default keeps the subsampled levels
    neck = FPN(ins, 12, 5, start_level=1, add_extra_convs=source, relu_before_extra_convs=True)
    mode = 'on_input' if source is True else source
    assert len(neck.lateral_convs) == 3 and [m.conv.in_channels for m in neck.lateral_convs] == ins[1:]
    assert neck.add_extra_convs == mode and len(neck.fpn_convs) == 5
    extra = neck.fpn_convs[3:]
    assert [m.conv.in_channels for m in extra] == [64 if mode == 'on_input' else 12, 12]
    assert all(m.conv.stride == (2, 2) and m.conv.kernel_size == (3, 3) and m.conv.padding == (1, 1) for m in extra)
    assert all(m.conv.stride == (1, 1) for m in neck.fpn_convs[:3])
    assert FPN(ins, 12, 5, add_extra_convs=True, extra_convs_on_inputs=False).add_extra_convs == 'on_output'
    seen = {}

    class Fake(torch.nn.Module):
        def __init__(self, name, cout, stride, value):
            super().__init__()
            self.name, self.cout, self.stride, self.value = name, cout, stride, value
            self.with_norm = self.with_activation = False

        def forward(self, x):
            seen[self.name] = (tuple(x.shape), sorted(set(x.reshape(-1).tolist())))
            h, w = (x.size(2) - 1) // self.stride + 1, (x.size(3) - 1) // self.stride + 1
            return torch.full((x.size(0), self.cout, h, w), self.value)
    LAT, OUT, INPUT = [-10., -20., -40.], [-100., -200., -300., -400., 500.], [-1., -2., -3., -4.]
    neck.lateral_convs = torch.nn.ModuleList(Fake(f'l{i}', 12, 1, LAT[i]) for i in range(3))
    neck.fpn_convs = torch.nn.ModuleList(Fake(f'f{i}', 12, 2 if i >= 3 else 1, OUT[i]) for i in range(5))
    feats = [torch.full((2, c, 64 // 2 ** i, 48 // 2 ** i), INPUT[i]) for i, c in enumerate(ins)]
    outs = neck(feats)
    assert [tuple(o.shape) for o in outs] == [(2, 12, 32, 24), (2, 12, 16, 12), (2, 12, 8, 6), (2, 12, 4, 3), (2, 12, 2, 2)]
    assert [float(o.flatten()[0]) for o in outs] == OUT
    # laterals: the top one is the plain 1x1 output, the others carry the top-down sum; output convolution i reads lateral i
    assert seen['l2'] == ((2, 64, 8, 6), [INPUT[3]]) and seen['l0'] == ((2, 16, 32, 24), [INPUT[1]])
    assert seen['f2'] == ((2, 12, 8, 6), [LAT[2]]) and seen['f1'][1] == [LAT[1] + LAT[2]] and seen['f0'][1] == [sum(LAT)]
    want = dict(on_input=((2, 64, 8, 6), [INPUT[3]]), on_lateral=((2, 12, 8, 6), [LAT[2]]), on_output=((2, 12, 8, 6), [OUT[2]]))
    assert seen['f3'] == want[mode], (mode, seen['f3'])
    # relu_before_extra_convs: from the second extra convolution on (the first output is negative, so its ReLU is 0)
    assert seen['f4'] == ((2, 12, 4, 3), [0.0])
    neck.relu_before_extra_convs = False
    neck(feats)
    assert seen['f4'] == ((2, 12, 4, 3), [OUT[3]])


def test_pseudo_sampler():
    from htd_amd.core.bbox import AssignResult
    from htd_amd.registry import build_sampler
    s = build_sampler(dict(type='PseudoSampler'))
    boxes = torch.arange(24.).view(6, 4)
    gts = torch.tensor([[0., 0., 4., 4.], [1., 1., 9., 9.]])
    res = AssignResult(2, torch.tensor([0, 2, -1, 1, 0, 2]), torch.zeros(6), labels=torch.tensor([-1, 5, -1, 3, -1, 5]))
    sr = s.sample(res, boxes, gts)
    assert sr.pos_inds.tolist() == [1, 3, 5] and sr.neg_inds.tolist() == [0, 4]
    assert sr.pos_assigned_gt_inds.tolist() == [1, 0, 1] and torch.equal(sr.pos_gt_bboxes, gts[[1, 0, 1]])
    assert torch.equal(sr.pos_bboxes, boxes[[1, 3, 5]]) and int(sr.pos_is_gt.sum()) == 0


def test_tensor_path_head_loss_on_the_cpu_matches_the_reference(golden):
    """RetinaHead.loss (tensor path) on the seeded maps of retina_util.head_maps against the reference head's own result: fp64 to
    1e-10, fp32 to 1e-5 relative."""
    from htd_amd.configs import retinanet_config
    from htd_amd.registry import build_head
    import htd_amd.detector  # noqa: F401
    g = golden('retinanet')
    cfg = retinanet_config()
    spec = cfg.model.bbox_head.to_dict()
    spec.update(train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    head = build_head(spec)
    _, metas, gts, labels = BU.detector_inputs()
    for dt, tag, rtol in ((torch.float64, '64', 1e-10), (torch.float32, '32', 1e-5)):
        cls, reg = U.head_maps()
        cls, reg = [c.to(dt).requires_grad_() for c in cls], [r.to(dt) for r in reg]
        losses = head.loss(cls, reg, [T(x).to(dt) for x in gts], [T(x) for x in labels], metas)
        assert set(losses) == {'loss_cls', 'loss_bbox'} and len(losses['loss_cls']) == 5
        mine = torch.stack([sum(losses['loss_cls']), sum(losses['loss_bbox'])])
        np.testing.assert_allclose(mine.detach().numpy(), g['head.loss' + tag], rtol=rtol)
    sum(losses['loss_cls']).backward()
    assert all(torch.isfinite(c.grad).all() for c in cls)


def test_new_abi_symbols_are_declared_and_exported():
    from htd_amd import capi
    names = {n for n, _, _ in capi.declared_functions()}
    want = {'htd_focal_loss_partial_rows', 'htd_sigmoid_focal_loss', 'htd_retina_avg_factor_workspace_bytes',
            'htd_retina_avg_factor', 'htd_retina_loss', 'htd_retina_grad_scale', 'htd_retina_keys'}
    assert want <= names
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in want)
    assert lib.htd_focal_loss_partial_rows() > 0 and lib.htd_retina_avg_factor_workspace_bytes(4) >= 4 * 4
