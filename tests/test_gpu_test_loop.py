"""The test loop end to end on the GPU: CocoDataset on a tiny on-disk PNG set (PNG so that decoded pixels are exact)
-> build_dataloader -> pipelines.collate -> the seeded small detector -> results, evaluation and the test CLI."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_datasets import Probe, write_png_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w): both orientations, padded sizes (after Pad size_divisor=32) transposes of each other at 0/1 and 2/3
SHAPES = [(64, 96), (96, 64), (96, 128), (128, 96), (80, 80), (70, 100), (100, 70)]


def _cfg():
    from htd_amd.configs import htd_config
    cfg = htd_config(50)
    cfg.test_cfg.rcnn.score_thr = 0.0                 # a seeded (untrained) model: keep every detection
    cfg.train_cfg.rpn_proposal.update(nms_pre=200, nms_post=100, max_num=100)
    for r in cfg.train_cfg.rcnn:
        r.sampler.num = 48
    test_pipe = cfg.data.test.pipeline
    test_pipe[1]['img_scale'] = (128, 128)
    train_pipe = cfg.data.train.pipeline
    train_pipe[2]['img_scale'] = (128, 128)
    return cfg


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('tiny_coco'))
    return root, write_png_set(root, SHAPES, seed=4)


@pytest.fixture(scope='module')
def det():
    from golden_util import load_seeded_
    from htd_amd.configs import build_htd_detector
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    return load_seeded_(build_htd_detector(cfg=_cfg()), 'det.').cuda().eval()


def _dataset(tiny, test_mode=True, samples_per_gpu=1):
    from htd_amd.datasets import build_dataset, replace_ImageToTensor
    root, ann = tiny
    cfg = _cfg().data.test.to_dict() if test_mode else _cfg().data.train.to_dict()
    if samples_per_gpu > 1:
        cfg['pipeline'] = replace_ImageToTensor(cfg['pipeline'])
    cfg.update(ann_file=ann, img_prefix=os.path.join(root, 'imgs'), test_mode=test_mode)
    return build_dataset(cfg)


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb) == 80
        for x, y in zip(ra, rb):
            assert x.shape == y.shape and np.array_equal(x, y)


def test_loop_equals_direct_calls_and_workers(tiny, det):
    from htd_amd.apis import single_gpu_test
    from htd_amd.datasets import build_dataloader
    from htd_amd.pipelines import collate
    ds = _dataset(tiny, samples_per_gpu=2)
    loop = single_gpu_test(det, build_dataloader(ds, 2, 0, dist=False, shuffle=False))
    assert len(loop) == len(SHAPES) and sum(b.shape[0] for r in loop for b in r) > 0
    direct = []
    for batch in build_dataloader(ds, 2, 0, dist=False, shuffle=False):
        with torch.no_grad():
            direct.extend(det(return_loss=False, rescale=True, **collate(batch, 'cuda:0')))
    _same(loop, direct)
    ds.pipeline.transforms.append(Probe())            # the workers of a process that holds a HIP context
    probes = []
    loader = build_dataloader(ds, 2, 2, dist=False, shuffle=False)
    _same(single_gpu_test(det, loader), loop)
    for batch in loader:
        probes += [s.pop('probe') for s in batch]
    assert torch.cuda.is_initialized() and all(p['pid'] != os.getpid() for p in probes)
    assert not any(p['cuda_init'] or p['lib_mapped'] for p in probes)


def test_transposed_orientations_get_their_own_anchors(tiny, det):
    """Image 1 (96 x 64) follows image 0 (64 x 96): equal element counts per level, transposed maps.  Its results and
    its proposals equal those of a run with the proposal cache emptied first."""
    from htd_amd.apis import single_gpu_test
    from htd_amd.datasets import build_dataloader
    from htd_amd.pipelines import collate
    ds = _dataset(tiny)
    loop = single_gpu_test(det, build_dataloader(ds, 1, 0, dist=False, shuffle=False))
    samples = [ds[i] for i in range(2)]
    shapes = [tuple(s['img_metas'][0]['pad_shape'][:2]) for s in samples]
    assert shapes[1] == shapes[0][::-1] and shapes[0][0] != shapes[0][1]
    det.rpn_head.__dict__.pop('_prop_cache', None)
    with torch.no_grad():
        fresh = det(return_loss=False, rescale=True, **collate([samples[1]], 'cuda:0'))
    _same(loop[1:2], fresh)

    def proposals(sample):
        data = collate([sample], 'cuda:0')
        with torch.no_grad():
            x = det.extract_feat(data['img'][0])
            return det.rpn_head.simple_test_rpn(x, data['img_metas'][0])[0]
    det.rpn_head.__dict__.pop('_prop_cache', None)
    alone = proposals(samples[1])
    det.rpn_head.__dict__.pop('_prop_cache', None)
    proposals(samples[0])
    after = proposals(samples[1])
    assert alone.shape[0] > 0 and torch.equal(alone, after)


def test_dataset_evaluate_and_multi_gpu_world_of_one(tiny, det):
    from htd_amd.apis import multi_gpu_test, single_gpu_test
    from htd_amd.coco import CocoEvaluator
    from htd_amd.datasets import build_dataloader
    ds = _dataset(tiny)
    res = single_gpu_test(det, build_dataloader(ds, 1, 0, dist=False, shuffle=False))
    out = ds.evaluate(res)
    assert out == CocoEvaluator(tiny[1]).evaluate(res) and 'bbox_mAP' in out
    dl = build_dataloader(ds, 1, 0, dist=True, shuffle=False)
    _same(multi_gpu_test(det, dl), res)
    triple = multi_gpu_test(det, dl, return_tensors=True)
    assert ds.evaluate(triple) == out
    assert ds.evaluate(single_gpu_test(det, dl, return_tensors=True)) == out


def test_train_loader_batch_drives_a_train_step(tiny):
    from golden_util import load_seeded_
    from htd_amd.configs import build_htd_detector
    from htd_amd.datasets import build_dataloader
    from htd_amd.pipelines import collate
    from htd_amd.runner import Trainer
    ds = _dataset(tiny, test_mode=False)
    np.random.seed(0)
    batch = next(iter(build_dataloader(ds, 2, 0, dist=False, shuffle=True, seed=0)))
    data = collate(batch, 'cuda:0')
    assert data['img'].shape[0] == 2 and len(data['gt_bboxes']) == 2
    model = load_seeded_(build_htd_detector(cfg=_cfg()), 'det.').cuda().train()
    out = Trainer(model, lr=0.001).train_step(data)
    assert torch.isfinite(out['loss']).item()
    assert all(np.isfinite(float(v)) for v in out['log_vars'].values())


def test_cli(tiny, det, tmp_path):
    from htd_amd.apis import single_gpu_test
    from htd_amd.checkpoint import save_checkpoint
    from htd_amd.datasets import build_dataloader
    root, ann = tiny
    cfg = _cfg()
    cfg_file = tmp_path / 'cfg.py'
    cfg_file.write_text(''.join(f'{k} = {cfg[k].to_dict()!r}\n' for k in ('model', 'test_cfg', 'data', 'evaluation')))
    ckpt = str(tmp_path / 'm.pth')
    save_checkpoint(det, ckpt, meta=dict(CLASSES=list(_dataset(tiny).CLASSES)))
    ds = _dataset(tiny, samples_per_gpu=2)
    want = single_gpu_test(det, build_dataloader(ds, 2, 0, dist=False, shuffle=False))
    paths = [f'data.test.ann_file={ann}', f'data.test.img_prefix={os.path.join(root, "imgs")}',
             'data.test.samples_per_gpu=2', 'data.workers_per_gpu=2']
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = [sys.executable, '-m', 'htd_amd.test', str(cfg_file), ckpt, '--cfg-options'] + paths
    p = subprocess.run(run + ['--eval', 'bbox', '--out', str(tmp_path / 'r.pkl')], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "'bbox_mAP'" in p.stdout and 'Average Precision' in p.stdout
    with open(tmp_path / 'r.pkl', 'rb') as f:
        got = pickle.load(f)
    _same(got, want)
    prefix = str(tmp_path / 'fmt')
    p = subprocess.run(run + ['--format-only', '--eval-options', f'jsonfile_prefix={prefix}'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    ds.results2json(got, str(tmp_path / 'direct'))
    with open(prefix + '.bbox.json') as f, open(str(tmp_path / 'direct.bbox.json')) as g:
        assert json.load(f) == json.load(g)
