"""bench.py's plain run on the MI355X: the result line times exactly --steps steps and carries nothing of --full, and
--dump-outputs writes what the last timed step returned, from the same inputs in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '2',
           '--height', '256', '--width', '320', '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    assert '# timed region: ' in r.stderr and ' for 2 steps' in r.stderr
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dumped_outputs(tmp_path):
    out = _bench(tmp_path / 'a')
    assert out['steps'] == 2 and out['warmup'] == 1 and out['ms_per_step'] > 0 and out['value'] > 0
    assert out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert 'roofline' not in out and 'cpu_baseline' not in out and 'trained_like' not in out['config']
    files = sorted(os.listdir(tmp_path / 'a'))
    assert {'loss.npy', 'weights_sample.npy', 'grads_sample.npy'} <= set(files), files
    total = 0
    for f in files:
        a = np.load(tmp_path / 'a' / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.abs(np.load(tmp_path / 'a' / 'grads_sample.npy')).max() > 0
    # same arguments, same inputs: a second run's losses agree to within the summation order of the kernels
    _bench(tmp_path / 'b')
    assert sorted(os.listdir(tmp_path / 'b')) == files
    for f in files:
        if f not in ('weights_sample.npy', 'grads_sample.npy'):
            np.testing.assert_allclose(np.load(tmp_path / 'b' / f), np.load(tmp_path / 'a' / f), rtol=1e-3, atol=1e-5, err_msg=f)
