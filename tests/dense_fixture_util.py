"""Shared by the seven dense detectors' fixtures (RetinaNet, GHM, FCOS, ATSS, GFL, VFNet, FoveaBox): their *_util.py, their
tests/test_*.py and tests/test_gpu_*.py.  One text each of the small helpers, of the allocator fixture, of the seeded fixture
weights (one table of edits per head, walked by the loader and by the state builder) and of the three detector checks with
their bounds.  What is particular to a head -- its cases, reference formulas, head_cfg, head_maps -- stays in its util."""
import numpy as np
import pytest
import torch

from golden_util import load_seeded_, match_detections, seeded_array, seeded_state_value

EPS32 = float(np.finfo(np.float32).eps)
CFG_KEYS = ('model', 'train_cfg', 'test_cfg', 'evaluation', 'optimizer', 'optimizer_config', 'lr_config', 'total_epochs')
STRIDES = (8, 16, 32, 64, 128)
LEVEL_SIZES = ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))                  # of a 128 x 160 batch at strides 8 .. 128

# ---- the bounds of the detector checks, stated here once
LOSS_RTOL, LOSS_ATOL = 5e-4, 1e-4                   # every logged loss against the fixture's
GRAD_UNIT_ABS, GRAD_UNIT_REL = 2e-4, 1e-3           # one unit of a gradient digest: 2e-4 * max(1, max |ref|) + 1e-3 * |ref|
GRAD_MAX_UNITS, GRAD_MAX_RMS = 2.0, 0.2             # no element over 2 units, rms at most 0.2
OUTPUT_TOL = 2.5e-4                                 # head outputs: 2.5e-4 * max(1, |ref|) (distances are exponentials)
DET_TOL, DET_COORD_RTOL = 1e-3, 1e-5                # matched detections: 1e-3 + 1e-5 * the largest coordinate, same class
CKPT_META = dict(epoch=3, iter=100, mmdet_version='2.7.0', CLASSES=('person', ))


# ---------------------------------------------------------------------------------------------------- small helpers
def T(a):
    return torch.from_numpy(np.asarray(a))


def err(a, ref):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(ref).double()).abs().max())


def bound(e32, ref):
    """The project's rule for every value a kernel computes: 4 x max(the reference's own fp32 error on that case, one fp32 ulp of
    the largest entry).  The fp32 error comes from the fixture or from the fp32 run of the formula, never from the code under test."""
    return 4.0 * max(float(e32), EPS32 * float(torch.as_tensor(ref).abs().max()))


def spied(fn):
    """fn() with capi.call recorded -> (result, list of entry points)."""
    from htd_amd import capi
    calls, real = [], capi.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    capi.call = spy
    try:
        return fn(), calls
    finally:
        capi.call = real


def inputs(dev, source):
    """source() = (images, metas, boxes, labels) as numpy -> the same with tensors on dev."""
    imgs, metas, gts, labels = source()
    return T(imgs).to(dev), metas, [T(x).to(dev) for x in gts], [T(x).to(dev) for x in labels]


def pad_gts(gts_list, labels_list=None, K=None):
    """-> (B, K, 4) boxes, (B, K) validity, (B, K) labels, zero-padded like core.bbox.pad_gt_batch (K = max(1, longest list))."""
    B = len(gts_list)
    K = max(1, max(len(g) for g in gts_list)) if K is None else K
    gts, valid, labels = torch.zeros(B, K, 4), torch.zeros(B, K, dtype=torch.bool), torch.zeros(B, K, dtype=torch.long)
    for b, g in enumerate(gts_list):
        gts[b, :len(g)], valid[b, :len(g)] = g, True
        if labels_list is not None:
            labels[b, :len(g)] = labels_list[b]
    return gts, valid, labels


def levels_to_images(per_level, B):
    """The reference's per-level tensors (rows: image after image) -> (B, P, ...) level-major per image."""
    return torch.cat([t.reshape(B, t.size(0) // B, *t.shape[1:]) for t in per_level], 1)


def maps_to_rows(maps):
    """(B, c, h, w) per level -> (B, P, c)."""
    B = maps[0].size(0)
    return torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, m.size(1)) for m in maps], 1)


# ---------------------------------------------------------------------------------------------------- the allocator fixture
@pytest.fixture(scope='module', autouse=True)
def leave_the_allocator_as_found():
    """(Imported by a test module into its own namespace.)  The cached blocks of the module go back to the driver when it ends, and
    so do the small device tensors that its new shapes added to the package's content-keyed caches (top-k plans, descriptor
    tables, constants, the last padded gts), which would otherwise stay for the rest of the session and pin their segments of the
    small pool: later modules that look at the allocator's layout (test_gpu_wgrad_stream.py) find it as they would without this
    one.  A dropped entry is rebuilt on a miss."""
    import gc
    from htd_amd import capi, mmcv_ops as M
    from htd_amd.core import bbox, misc
    caches = (capi._TABLES, M._TOPK_PLANS, misc._CONSTS, misc._ARANGES, bbox._SAMPLE_PLANS)
    before = [set(c) for c in caches]
    yield
    for c, keys in zip(caches, before):
        for k in [k for k in c if k not in keys]:
            del c[k]
    bbox._PAD_GT_LAST.clear()
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- seeded weights from one table
# A head's fixture weights are load_seeded_(det, 'det.') and then
#   edits      ((state-dict key, 'mul' | 'add' | 'sub', a float or the name of a figure the fixture records), ...), in order;
#   scales     the ModuleLists of bbox_head whose zero-dimensional level scales are seeded by hand: 1 + 0.25 * seeded_array(...);
#   constants  {state-dict key: shape -> tensor} of buffers that keep the value the module gives them.
_OPS = dict(mul=(torch.Tensor.mul_, torch.Tensor.mul), add=(torch.Tensor.add_, torch.Tensor.add), sub=(torch.Tensor.sub_, torch.Tensor.sub))


def _hand_seeded(key, scales):
    part = key.split('.')
    return part[0] == 'bbox_head' and part[1] in scales


def _scale_value(key):
    return 1.0 + 0.25 * float(seeded_array('det.' + key, (1, ))[0])


def load_fixture_weights(det, edits, scales=(), constants=None, **figures):
    """Edit a built detector in place: fp32 mul_ / add_ / sub_ by a Python float, in the order of `edits`.  One rule for the
    children of the head: a child is seeded unless it is hand-seeded, holds a constant, or has an empty state dict."""
    kept = set(scales) | {k.split('.')[1] for k in (constants or {})}
    load_seeded_(det.backbone, 'det.backbone.')
    load_seeded_(det.neck, 'det.neck.')
    for name, child in det.bbox_head.named_children():
        if name not in kept and len(child.state_dict()) > 0:
            load_seeded_(child, f'det.bbox_head.{name}.')
    state = det.state_dict()                # (shares storage with the parameters and buffers)
    with torch.no_grad():
        for k, t in state.items():
            if _hand_seeded(k, scales):
                t.fill_(_scale_value(k))
        for key, op, value in edits:
            _OPS[op][0](state[key], float(figures[value] if isinstance(value, str) else value))
    return det


def fixture_state(keys, shapes, edits, scales=(), constants=None, **figures):
    """The state dict load_fixture_weights leaves, from a fixture's key and shape lists (shapes padded to 4 dims with 0): the same
    table, each operation out of place."""
    out = {}
    for k, shape in zip(keys, shapes):
        k, shape = str(k), [int(s) for s in shape if s]
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros((), dtype=torch.int64)
        elif _hand_seeded(k, scales):
            out[k] = torch.tensor(_scale_value(k))
        elif k in (constants or {}):
            out[k] = constants[k](shape)
        else:
            out[k] = torch.from_numpy(np.asarray(seeded_state_value('det.' + k, shape)))
    for key, op, value in edits:
        out[key] = _OPS[op][1](out[key], float(figures[value] if isinstance(value, str) else value))
    return out


def grad_keys(det, extra):
    from baselines_util import GRAD_KEYS
    names = dict(det.named_parameters())
    return [k for k in GRAD_KEYS + tuple(extra) if k in names and names[k].requires_grad]


# ---------------------------------------------------------------------------------------------------- the detector checks
def check_train_step(det, g, prefix, tag, losses, loss_names, grad_keys, min_keys, zero_grad_ok=(), backward=None):
    """`losses` of det.forward_train on the fixture's batch: the logged losses are the fixture's set and lie within LOSS_RTOL /
    LOSS_ATOL of it; after the backward pass (backward(loss), or loss.backward()) the gradient digests of `grad_keys` lie within
    GRAD_MAX_UNITS units and GRAD_MAX_RMS rms.  zero_grad_ok: parts of the names of parameters whose reference gradient may be
    all zero (a level without positives gives its scale exactly 0)."""
    import baselines_util as BU
    loss, log_vars = det._parse_losses(losses)
    n = len(prefix) + 5
    assert set(log_vars.keys()) == {f[n:] for f in g.files if f.startswith(prefix + 'loss.')} == set(loss_names) | {'loss'}
    det.zero_grad()
    loss.backward() if backward is None else backward(loss)
    params = dict(det.named_parameters())
    assert len(grad_keys) >= min_keys, grad_keys
    worst, worst_rms, worst_loss = (0.0, ''), (0.0, ''), 0.0
    for k, v in log_vars.items():
        ref = float(g[f'{prefix}loss.{k}'])
        worst_loss = max(worst_loss, abs(v - ref) / (LOSS_ATOL + LOSS_RTOL * abs(ref)))
    for k in grad_keys:
        ref = g[f'{prefix}grad.{k}.sample']
        assert float(g[f'{prefix}grad.{k}.sums'][1]) > 0 or any(s in k for s in zero_grad_ok), k
        tol = GRAD_UNIT_ABS * max(1.0, np.abs(ref).max()) + GRAD_UNIT_REL * np.abs(ref)
        ratio = np.abs(BU.digest(params[k].grad.cpu())[1] - ref) / tol
        worst, worst_rms = max(worst, (float(ratio.max()), k)), max(worst_rms, (float(np.sqrt(np.mean(ratio ** 2))), k))
    print(f'{tag}: worst loss ratio {worst_loss:.3f}; worst gradient element {worst[0]:.3f} units ({worst[1]}), '
          f'worst rms {worst_rms[0]:.3f} ({worst_rms[1]})')
    for k, v in log_vars.items():
        np.testing.assert_allclose(v, float(g[f'{prefix}loss.{k}']), rtol=LOSS_RTOL, atol=LOSS_ATOL, err_msg=k)
    assert worst[0] <= GRAD_MAX_UNITS and worst_rms[0] <= GRAD_MAX_RMS, (worst, worst_rms)


def check_outputs(det, g, prefix, kinds, level_sizes, img):
    """The per-level outputs of the training forward (one list of maps per kind, e.g. ('cls', 'reg', 'ctr')) within OUTPUT_TOL *
    max(1, |ref|) of the fixture's strided samples -> the worst ratio."""
    import baselines_util as BU
    det.train()
    with torch.no_grad():
        outs = det.bbox_head(det.extract_feat(img))
    assert tuple(tuple(c.shape[-2:]) for c in outs[0]) == tuple(level_sizes)
    worst = 0.0
    for name, maps in zip(kinds, outs):
        for l, t in enumerate(maps):
            ref = g[f'{prefix}{name}{l}.sample']
            mine = BU.digest(t.cpu())[1]
            tol = OUTPUT_TOL * np.maximum(1.0, np.abs(ref))
            worst = max(worst, float((np.abs(mine - ref) / tol).max()))
            assert (np.abs(mine - ref) <= tol).all(), f'{name}{l}'
    return worst


def check_detections(res, g, prefix, min_dets=10):
    """The results of simple_test on the fixture's two images matched one to one with the fixture's, within DET_TOL +
    DET_COORD_RTOL * the largest coordinate and of the same class -> the worst ratio."""
    import baselines_util as BU
    worst = 0.0
    for i in range(2):
        mine, ref = BU.dets_array(res[i]), g[f'{prefix}test_dets{i}']
        assert mine.shape == ref.shape and len(ref) >= min_dets
        worst = max(worst, match_detections(mine, ref, tol=DET_TOL, coord_rtol=DET_COORD_RTOL))
    return worst


def save_reference_checkpoint(state, tmp_path):
    """`state` as a `.pth` in the reference's wire format (DataParallel's `module.` prefix, its meta) -> the path."""
    path = str(tmp_path / 'epoch_3.pth')
    torch.save(dict(meta=dict(CKPT_META), state_dict={'module.' + k: v for k, v in state.items()}), path)
    return path


def check_checkpoint_round_trip(build, state, g, prefix, img, metas, tmp_path, tol):
    """A `.pth` in the reference's wire format goes through load_checkpoint(strict=True) into a detector freshly made by build(),
    which reproduces the fixture's detections within match_detections(tol) -> the loaded checkpoint."""
    import baselines_util as BU
    from htd_amd.checkpoint import load_checkpoint
    path = save_reference_checkpoint(state, tmp_path)
    torch.manual_seed(123)
    model = build()
    ckpt = load_checkpoint(model, path, strict=True)
    model = model.to(img.device).eval()
    with torch.no_grad():
        res = model.simple_test(img, metas)
    for i in range(2):
        match_detections(BU.dets_array(res[i]), g[f'{prefix}test_dets{i}'], tol=tol)
    return ckpt
