"""The train CLI and the epoch runner on the CPU: argument set, work_dir priority, refused settings, the log buffer's
fallback arithmetic, and a gloo world-2 run of train_detector with a toy model on Trainer's CPU path."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _write_cfg(path, **extra):
    text = "optimizer = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001)\n"
    text += "lr_config = dict(policy='step', warmup='linear', warmup_iters=2, warmup_ratio=0.1, step=[2])\n"
    text += 'total_epochs = 3\n'
    for k, v in extra.items():
        text += f'{k} = {v!r}\n'
    path.write_text(text)
    return str(path)


def test_cli_accepts_the_reference_arguments(tmp_path):
    from htd_amd.train import parse_args
    a = parse_args(['cfg.py', '--work-dir', 'w', '--resume-from', 'r.pth', '--no-validate', '--gpus', '1', '--seed', '7',
                    '--deterministic', '--cfg-options', 'a.b=1', 'c=x,y', '--launcher', 'pytorch', '--local_rank', '3'])
    assert (a.config, a.work_dir, a.resume_from, a.no_validate, a.gpus, a.seed, a.deterministic) == \
        ('cfg.py', 'w', 'r.pth', True, 1, 7, True)
    assert a.cfg_options == {'a.b': 1, 'c': ['x', 'y']} and a.launcher == 'pytorch' and a.local_rank == 3
    a = parse_args(['cfg.py'])
    assert a.seed == 1 and a.launcher == 'none' and not a.no_validate and a.gpus is None and a.gpu_ids is None
    with pytest.warns(UserWarning):
        assert parse_args(['cfg.py', '--options', 'k=2']).cfg_options == {'k': 2}
    with pytest.raises(ValueError):
        parse_args(['cfg.py', '--options', 'k=2', '--cfg-options', 'k=3'])
    assert parse_args(['cfg.py', '--gpu-ids', '2']).gpu_ids == [2]
    assert parse_args(['cfg.py', '--gpus', '4', '--launcher', 'pytorch']).gpus == 4


def test_cli_gpus_and_gpu_ids_exclude_each_other_and_one_gpu_without_launcher(capsys):
    from htd_amd.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(['cfg.py', '--gpus', '1', '--gpu-ids', '0'])
    assert 'not allowed with' in capsys.readouterr().err
    for extra in (['--gpus', '2'], ['--gpu-ids', '0', '1']):
        with pytest.raises(SystemExit):
            parse_args(['cfg.py'] + extra)
        err = capsys.readouterr().err
        assert 'exactly one GPU' in err and 'torch.distributed.run' in err and '--launcher pytorch' in err


def test_work_dir_priority(tmp_path):
    from htd_amd.train import load_config, parse_args
    plain = _write_cfg(tmp_path / 'my_exp.py')
    with_dir = _write_cfg(tmp_path / 'other.py', work_dir='from_file')
    assert load_config(parse_args([with_dir, '--work-dir', 'cli'])).work_dir == 'cli'
    assert load_config(parse_args([with_dir])).work_dir == 'from_file'
    assert load_config(parse_args([plain])).work_dir == os.path.join('./work_dirs', 'my_exp')
    assert load_config(parse_args([plain, '--resume-from', 'x.pth'])).resume_from == 'x.pth'


def test_runtime_defaults_and_config_round_trip(tmp_path):
    from htd_amd.registry import Config
    from htd_amd.train import dump_config, load_config, parse_args
    cfg = load_config(parse_args([_write_cfg(tmp_path / 'c.py')]))
    assert cfg.checkpoint_config == dict(interval=1) and cfg.log_config.interval == 50
    assert cfg.log_config.hooks == [dict(type='TextLoggerHook')] and cfg.workflow == [('train', 1)]
    assert cfg.load_from is None and cfg.resume_from is None
    kept = load_config(parse_args([_write_cfg(tmp_path / 'k.py', checkpoint_config=dict(interval=3),
                                              log_config=dict(interval=5, hooks=[dict(type='TextLoggerHook')]))]))
    assert kept.checkpoint_config.interval == 3 and kept.log_config.interval == 5
    dump_config(cfg, str(tmp_path / 'dumped.py'))
    assert Config.fromfile(str(tmp_path / 'dumped.py'))._cfg_dict.to_dict() == cfg._cfg_dict.to_dict()


@pytest.mark.parametrize('key,value', [
    ('workflow', [('train', 1), ('val', 1)]),
    ('custom_hooks', [dict(type='NumClassCheckHook')]),
    ('optimizer_config', dict(grad_clip=dict(max_norm=35, norm_type=2))),
    ('log_config', dict(interval=50, hooks=[dict(type='TextLoggerHook'), dict(type='TensorboardLoggerHook')])),
])
def test_unsupported_settings_are_refused(tmp_path, key, value):
    from htd_amd.train import main
    path = _write_cfg(tmp_path / 'c.py', **{key: value})
    with pytest.raises(NotImplementedError, match=key.split('_')[0]):
        main([path, '--work-dir', str(tmp_path / 'w')])
    assert not (tmp_path / 'w').exists()


def test_log_accumulate_fallback_matches_numpy_fp64():
    from htd_amd import mmcv_ops as M
    rs = np.random.RandomState(0)
    n, steps = 9, 40
    vals = rs.randn(steps, n).astype(np.float32) * 10
    weights = rs.randint(1, 5, steps)
    vals[17, 3] = np.inf
    vals[23, n - 1] = np.nan                         # the total loss (last entry) turns NaN at step 23
    vals[31, n - 1] = np.inf
    acc = M.log_accumulator(n, 'cpu')
    for i in range(steps):
        M.log_accumulate_(acc, torch.from_numpy(vals[i]), int(weights[i]), 100 + i)
    want = np.cumsum(vals.astype(np.float64) * weights[:, None].astype(np.float64), axis=0)[-1]
    got = acc.numpy()
    np.testing.assert_array_equal(got[:n], want)
    assert got[n] == weights.sum() and got[n + 1] == 123
    clean = M.log_accumulator(n, 'cpu')
    M.log_accumulate_(clean, torch.from_numpy(vals[17]), 2, 5)      # non-finite, but not the total loss
    assert clean[n + 1] == -1 and clean[n] == 2
    M.log_accumulate_(clean, torch.from_numpy(vals[17]), 2, 6, loss_index=3)
    assert clean[n + 1] == 6


# ------------------------------------------------------------------------------------------------ gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class ToyDataset:
    CLASSES = ('a', 'b')

    def __init__(self, n):
        self.flag = np.zeros(n, dtype=np.uint8)

    def __len__(self):
        return len(self.flag)

    def __getitem__(self, i):
        return dict(x=torch.full((3,), float(i) / 10))


def _toy_model(nan_at):
    from htd_amd.detector.two_stage import BaseDetector

    class Toy(BaseDetector):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 1)
            self.calls, self.seen = 0, []

        def train_step(self, data, optimizer):
            x = torch.stack([s['x'] for s in data])
            loss_a = (self.lin(x) - 1).pow(2).mean()
            if nan_at is not None and self.calls >= nan_at and dist.get_rank() == 0:
                loss_a = loss_a * float('nan')
            self.calls += 1
            loss, log_vars = self._parse_losses(dict(loss_a=loss_a, acc=torch.tensor(50.0 + self.calls)))
            self.seen.append((log_vars._packed.clone(), len(data)))
            return dict(loss=loss, log_vars=log_vars, num_samples=len(data))
    return Toy()


def _train_worker(rank, world, port, base, nan_at, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from htd_amd import datasets
    from htd_amd.apis import NonFiniteLossError, train_detector
    from htd_amd.registry import Config
    epochs = []
    orig = datasets.DistributedGroupSampler.set_epoch

    def spy(self, epoch):
        epochs.append(epoch)
        orig(self, epoch)
    datasets.DistributedGroupSampler.set_epoch = spy
    torch.manual_seed(0)
    model = _toy_model(nan_at)
    cfg = Config(dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=1e-4),
                      optimizer_config=dict(grad_clip=None), total_epochs=3, seed=0,
                      lr_config=dict(policy='step', warmup='linear', warmup_iters=2, warmup_ratio=0.1, step=[2]),
                      data=dict(samples_per_gpu=2, workers_per_gpu=0),
                      log_config=dict(interval=2, hooks=[dict(type='TextLoggerHook')]),
                      work_dir=os.path.join(base, f'rank{rank}')))
    out = dict(rank=rank, error=None)
    try:
        runner = train_detector(model, ToyDataset(12), cfg, distributed=True, validate=False, timestamp='ts',
                                batch_fn=lambda samples, device: samples)
        out['history'] = runner.log_history
    except NonFiniteLossError as e:
        out['error'] = (e.iter, str(e))
    except Exception:                                  # report instead of leaving the parent waiting
        import traceback
        out['crash'] = traceback.format_exc()
        q.put(out)
        raise
    out['epochs'] = epochs
    out['seen'] = [(p.tolist(), n) for p, n in model.seen]
    q.put(out)
    dist.destroy_process_group()


def _run_world2(base, nan_at):
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_train_worker, args=(r, world, port, str(base), nan_at, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda r: r['rank'])
    for p in procs:
        p.join(timeout=60)
    assert not any('crash' in r for r in res), [r.get('crash') for r in res]
    return res


def _load_json_logs(path):
    """tools/analyze_logs.py:load_json_logs: lines without `epoch` are skipped, `epoch` is popped, every other value is
    appended per epoch."""
    log_dict = {}
    with open(path) as f:
        for line in f:
            log = json.loads(line.strip())
            if 'epoch' not in log:
                continue
            epoch = log.pop('epoch')
            log_dict.setdefault(epoch, {})
            for k, v in log.items():
                log_dict[epoch].setdefault(k, []).append(v)
    return log_dict


def test_train_detector_world2_gloo(tmp_path):
    res = _run_world2(tmp_path, None)
    for r in res:
        assert r['error'] is None and r['epochs'] == [0, 1, 2]          # DistSamplerSeedHook: set_epoch every epoch
    assert not (tmp_path / 'rank1').exists()                             # rank 1 writes nothing
    d0 = tmp_path / 'rank0'
    assert sorted(os.listdir(d0)) == ['epoch_1.pth', 'epoch_2.pth', 'epoch_3.pth', 'latest.pth', 'ts.log', 'ts.log.json']
    assert os.path.realpath(d0 / 'latest.pth') == os.path.realpath(d0 / 'epoch_3.pth')
    ck = torch.load(str(d0 / 'epoch_2.pth'), weights_only=True)
    assert ck['meta']['epoch'] == 2 and ck['meta']['iter'] == 6 and ck['meta']['CLASSES'] == ['a', 'b']
    assert set(ck['meta']['rng']) >= {'python', 'numpy', 'torch'}
    logs = _load_json_logs(d0 / 'ts.log.json')
    assert sorted(logs) == [1, 2, 3]
    for ep in (1, 2, 3):
        assert logs[ep]['mode'] == ['train'] and logs[ep]['iter'] == [2]      # iteration 3 of 3 is a tail: not logged
    hist = res[0]['history']
    assert [list(h)[:6] for h in hist] == [['mode', 'epoch', 'iter', 'lr', 'time', 'data_time']] * 3
    assert [list(h)[6:] for h in hist] == [['loss_a', 'acc', 'loss']] * 3
    seen = res[0]['seen']                                                 # rank-averaged packed scalars, per iteration
    for e, h in enumerate(hist):
        part = seen[3 * e:3 * e + 2]
        for j, k in enumerate(('loss_a', 'acc', 'loss')):
            s = 0.0
            for vals, n in part:
                s += float(n) * float(np.float32(vals[j]))
            assert h[k] == s / sum(n for _, n in part), (e, k)
            assert logs[e + 1][k] == [round(h[k], 5)]
    text = (d0 / 'ts.log').read_text()
    assert 'Epoch [3][2/3]\tlr: ' in text and 'loss_a: ' in text


@pytest.mark.parametrize('nan_at,epochs_kept', [(4, 1), (5, 1), (1, 0)], ids=['log_point', 'epoch_tail', 'first_epoch'])
def test_non_finite_loss_stops_the_run(tmp_path, nan_at, epochs_kept):
    res = _run_world2(tmp_path, nan_at)
    for r in res:
        assert r['error'] is not None and r['error'][0] == nan_at + 1, r['error']
        assert f'iteration {nan_at + 1} ' in r['error'][1]
    files = sorted(os.listdir(tmp_path / 'rank0'))
    assert [f for f in files if f.startswith('epoch_')] == [f'epoch_{e}.pth' for e in range(1, epochs_kept + 1)]
    assert not (tmp_path / 'rank1').exists()
