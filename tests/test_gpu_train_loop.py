"""The epoch runner on the GPU over the tiny on-disk PNG set of test_gpu_test_loop (128 x 128 scale, seeded R50, whose
step is bitwise reproducible): htd_log_accumulate, the runner against a hand-written loop, evaluation that leaves
training alone, exact resume, the train CLI end to end, and no synchronisation added to a step."""
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from test_datasets import write_png_set
from test_gpu_test_loop import SHAPES, _cfg
from test_train_loop import _load_json_logs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_KEYS = ('time', 'data_time', 'memory')


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('tiny_train'))
    return root, write_png_set(root, SHAPES, seed=4)


def _train_cfg(tiny, work_dir, epochs=1):
    root, ann = tiny
    cfg = _cfg()
    for split in (cfg.data.train, cfg.data.val, cfg.data.test):
        split.ann_file, split.img_prefix = ann, os.path.join(root, 'imgs')
    cfg.model.pretrained = None
    cfg.data.workers_per_gpu = 0
    cfg.total_epochs = epochs
    cfg.log_config = dict(interval=2, hooks=[dict(type='TextLoggerHook')])
    cfg.work_dir = str(work_dir)
    cfg.seed = 1
    return cfg


def _model():
    from golden_util import load_seeded_
    from htd_amd.configs import build_htd_detector
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    return load_seeded_(build_htd_detector(cfg=_cfg()), 'det.').cuda().train()


def _train_set(cfg):
    from htd_amd.datasets import build_dataset
    return build_dataset(cfg.data.train.to_dict())


def test_log_accumulate_matches_numpy_fp64():
    from htd_amd import mmcv_ops as M
    rs = np.random.RandomState(1)
    for n, steps in ((23, 50), (1, 7), (130, 9)):
        vals = (rs.randn(steps, n) * 10 ** rs.uniform(-3, 3, (steps, n))).astype(np.float32)
        weights = rs.randint(1, 9, steps)
        if n > 3:
            vals[2, 1], vals[4, 2] = np.inf, -np.inf
        vals[5 % steps, n - 1] = np.nan
        acc = M.log_accumulator(n, 'cuda')
        cpu = M.log_accumulator(n, 'cpu')
        for i in range(steps):
            M.log_accumulate_(acc, torch.from_numpy(vals[i]).cuda(), int(weights[i]), 7 + i)
            M.log_accumulate_(cpu, torch.from_numpy(vals[i]), int(weights[i]), 7 + i)
        want = np.cumsum(vals.astype(np.float64) * weights[:, None], axis=0)[-1]
        got = acc.cpu().numpy()
        np.testing.assert_array_equal(got[:n], want)
        assert got[n] == weights.sum() and got[n + 1] == 7 + 5 % steps
        np.testing.assert_array_equal(got, cpu.numpy())
    with pytest.raises(ValueError):
        M.log_accumulate_(torch.zeros(3, dtype=torch.float64, device='cuda'), torch.zeros(4, device='cuda'), 1, 0)


def test_runner_equals_hand_loop(tiny, tmp_path):
    from htd_amd.apis import set_random_seed, train_detector
    from htd_amd.datasets import build_dataloader
    from htd_amd.pipelines import collate
    from htd_amd.runner import Trainer
    cfg = _train_cfg(tiny, tmp_path / 'w')
    model, ds = _model(), _train_set(cfg)
    set_random_seed(1)
    loader = build_dataloader(ds, 2, 0, dist=False, shuffle=True, seed=1)
    tr = Trainer(model, cfg=cfg, iters_per_epoch=len(loader))
    seen = []
    for samples in loader:
        out = tr.train_step(collate(samples, 'cuda:0'))
        seen.append((dict(out['log_vars'].items()), out['num_samples']))
    assert len(seen) == 4
    model2, ds2 = _model(), _train_set(cfg)
    set_random_seed(1)
    runner = train_detector(model2, ds2, cfg, validate=False, timestamp='t')
    assert runner.trainer.iter == 4
    assert torch.equal(runner.trainer.flat.flat, tr.flat.flat)
    assert torch.equal(runner.trainer.flat.momentum, tr.flat.momentum)
    hist = runner.log_history
    assert [(h['mode'], h['epoch'], h['iter']) for h in hist] == [('train', 1, 2), ('train', 1, 4)]
    logs = _load_json_logs(tmp_path / 'w' / 't.log.json')[1]
    for j, h in enumerate(hist):
        assert h['lr'] == tr.schedule.lr(2 * j + 1)
        part = seen[2 * j:2 * j + 2]
        for k in part[0][0]:
            s = 0.0
            for lv, n in part:
                s += float(n) * lv[k]
            assert h[k] == s / sum(n for _, n in part), k
            assert logs[k][j] == round(h[k], 5)
        assert h['memory'] > 0 and logs['memory'][j] == h['memory']


def test_evaluation_leaves_training_alone(tiny, tmp_path):
    from htd_amd.apis import set_random_seed, train_detector
    flats = []
    for validate in (True, False):
        cfg = _train_cfg(tiny, tmp_path / f'v{int(validate)}', epochs=2)
        model, ds = _model(), _train_set(cfg)
        set_random_seed(1)
        runner = train_detector(model, ds, cfg, validate=validate, timestamp='t')
        flats.append((runner.trainer.flat.flat.clone(), runner.trainer.flat.momentum.clone()))
        vals = [h for h in runner.log_history if h['mode'] == 'val']
        assert len(vals) == (2 if validate else 0)
        assert all('bbox_mAP' in v and v['epoch'] == e + 1 for e, v in enumerate(vals))
        assert model.training
    assert torch.equal(flats[0][0], flats[1][0]) and torch.equal(flats[0][1], flats[1][1])


def test_runner_iteration_adds_no_synchronisation(tiny, tmp_path):
    from htd_amd.apis import EpochRunner
    from htd_amd.datasets import build_dataloader
    from htd_amd.pipelines import collate
    from htd_amd.runner import Trainer
    cfg = _train_cfg(tiny, tmp_path / 'w')
    model, ds = _model(), _train_set(cfg)
    batches = list(build_dataloader(ds, 2, 0, dist=False, shuffle=False))
    tr = Trainer(model, cfg=cfg, iters_per_epoch=4)
    runner = EpochRunner(tr, batches, str(tmp_path / 'w'), 1, log_interval=1000, checkpoint_interval=0)

    def count(fn):
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode('default')
        torch.cuda.synchronize()
        return sum('synchroniz' in str(x.message) for x in w)

    b = batches[0]
    for _ in range(2):                                        # warm-up: the log interval's accumulator exists
        runner.run_iter(b)
    bare = count(lambda: tr.train_step(collate(b, 'cuda:0')))
    in_runner = count(lambda: runner.run_iter(b))
    assert in_runner <= bare, (in_runner, bare)


@pytest.fixture(scope='module')
def cli_run(tiny, tmp_path_factory):
    """`python -m htd_amd.train CFG` for two epochs with evaluation, from a seeded checkpoint (cfg.load_from)."""
    from htd_amd.checkpoint import save_checkpoint
    base = tmp_path_factory.mktemp('cli_train')
    seeded = str(base / 'seeded.pth')
    save_checkpoint(_model(), seeded)
    cfg = _train_cfg(tiny, base / 'unused', epochs=2)
    cfg.load_from = seeded
    cfg_file = base / 'htd_tiny.py'
    cfg_file.write_text(''.join(f'{k} = {v!r}\n' for k, v in cfg.to_dict().items() if k != 'work_dir'))
    work = base / 'a'
    p = _cli(['-m', 'htd_amd.train', str(cfg_file), '--work-dir', str(work)])
    assert p.returncode == 0, p.stderr[-4000:]
    return cfg_file, work


def _cli(args, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _json_lines(work):
    (name, ) = [f for f in os.listdir(work) if f.endswith('.log.json')]
    with open(os.path.join(work, name)) as f:
        return [json.loads(l) for l in f], os.path.join(work, name)


def test_cli_end_to_end(cli_run):
    cfg_file, work = cli_run
    files = os.listdir(work)
    for f in ('htd_tiny.py', 'epoch_1.pth', 'epoch_2.pth', 'latest.pth'):
        assert f in files
    assert any(f.endswith('.log') for f in files) and any(f.endswith('.log.json') for f in files)
    lines, path = _json_lines(work)
    assert 'epoch' not in lines[0] and lines[0]['seed'] == 1 and 'env_info' in lines[0]
    train = [l for l in lines if l.get('mode') == 'train']
    assert [(l['epoch'], l['iter']) for l in train] == [(1, 2), (1, 4), (2, 2), (2, 4)]
    keys = ['mode', 'epoch', 'iter', 'lr', 'memory', 'time', 'data_time', 'loss_rpn_cls', 'loss_rpn_bbox', 'loss_global',
            's0.loss_cls', 's0.acc']
    for l in train:
        assert list(l)[:len(keys)] == keys and list(l)[-1] == 'loss'
    val = [l for l in lines if l.get('mode') == 'val']
    assert [l['epoch'] for l in val] == [1, 2] and all('bbox_mAP' in l for l in val)
    logs = _load_json_logs(path)
    assert sorted(logs) == [1, 2] and logs[2]['mode'] == ['train', 'train', 'val']
    ck = torch.load(os.path.join(work, 'epoch_2.pth'), weights_only=True)
    assert ck['meta']['epoch'] == 2 and ck['meta']['iter'] == 8 and ck['meta']['CLASSES'][0] == 'person'
    assert 'hip' in ck['meta']['rng'] and 'HIP' in ck['meta']['env_info']
    p = _cli(['-m', 'htd_amd.test', str(cfg_file), os.path.join(work, 'epoch_2.pth'), '--eval', 'bbox'])
    assert p.returncode == 0, p.stderr[-3000:]
    m = re.search(r"'bbox_mAP'(?::|,) ([^,)}]+)", p.stdout)         # a dict or an OrderedDict repr
    assert m is not None, (p.stdout[-3000:], p.stderr[-3000:])
    assert float(m.group(1)) == val[-1]['bbox_mAP'], (m.group(1), val[-1])


def test_cli_resume_is_exact(cli_run, tmp_path):
    cfg_file, work = cli_run
    p = _cli(['-m', 'htd_amd.train', str(cfg_file), '--work-dir', str(tmp_path / 'b'), '--no-validate',
              '--resume-from', os.path.join(work, 'epoch_1.pth')])
    assert p.returncode == 0, p.stderr[-4000:]
    assert not os.path.exists(tmp_path / 'b' / 'epoch_1.pth')
    a = torch.load(os.path.join(work, 'epoch_2.pth'), weights_only=True)
    b = torch.load(str(tmp_path / 'b' / 'epoch_2.pth'), weights_only=True)
    assert a['state_dict'].keys() == b['state_dict'].keys()
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k]['momentum_buffer'], sb[k]['momentum_buffer']) for k in sa)
    assert a['meta']['iter'] == b['meta']['iter'] == 8

    def epoch2(w):
        return [{k: v for k, v in l.items() if k not in TIME_KEYS} for l in _json_lines(w)[0]
                if l.get('epoch') == 2 and l.get('mode') == 'train']
    assert epoch2(work) == epoch2(tmp_path / 'b') and len(epoch2(work)) == 2
