"""bench.py's plain run (headline leg only) and --dump-outputs: the last timed step's arrays, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--preroll', '3',
           '--envs-per-gpu', '256', '--dump-outputs', str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'FB_BENCH_DEVICE', 'FB_BENCH_BACKEND')}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    a = _bench(tmp_path / 'a', 3)
    assert a['steps'] == 3 and a['ms_per_step'] > 0 and a['dtype'] == 'f64' and a['config']['state_finite']
    assert abs(a['value'] - 256*3/(a['ms_per_step']*3/1e3)) < 1e-6*a['value']
    # the secondary legs are --full only
    assert a['parity_sample'] is None and not {'f32_mode', 'two_stream_mode', 'pipelined_dense_mode', 'flight_mode', 'dmpo_mode', 'cpu_baseline'} & set(a)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(k + '.npy' for k in ('action', 'qpos', 'qvel', 'act', 'obs', 'reward', 'discount', 'step_type'))
    b = _bench(tmp_path / 'b', 3)
    assert b['steps'] == 3
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype in (np.float32, np.float64) and x.shape[0] == 256 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n                   # same arguments, same inputs: the same outputs
    assert np.load(tmp_path / 'a' / 'qpos.npy').shape == (256, 109) and np.load(tmp_path / 'a' / 'obs.npy').shape == (256, 741)
    # --steps sets the number of timed steps: one more step, another last action
    c = _bench(tmp_path / 'c', 4)
    assert not np.array_equal(np.load(tmp_path / 'a' / 'action.npy'), np.load(tmp_path / 'c' / 'action.npy'))
