"""bench.py --steps / --dump-outputs: the timed steps are exactly --steps, and the last timed step's results land as
float32 .npy files under the size cap (a fixed sample of trajectory rows above it).  The CPU test drives the dump routine
on host tensors; the GPU test (-m gpu) runs the script."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import common

NAMES = ('states', 'actions', 'rewards', 'loss', 'policy_grad', 'policy_params', 'adam_exp_avg', 'adam_exp_avg_sq')


def _fake_leg(H, B, D, U, n_par, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return types.SimpleNamespace(last=(r(H + 1, B, D), r(H, B, U), r(H, B, 1), r(n_par)), loss_buf=r(1),
                                 params=r(n_par), m=r(n_par), v=r(n_par))


def _load(d):
    return {n: np.load(os.path.join(d, n + '.npy')) for n in NAMES}


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    leg = _fake_leg(H=5, B=300, D=4, U=2, n_par=50)
    info = bench.dump_outputs(leg, str(tmp_path / 'whole'))
    got = _load(str(tmp_path / 'whole'))
    assert info['rows_sampled'] is None and set(info['arrays']) == set(NAMES)
    assert all(v.dtype == np.float32 for v in got.values())
    S, A, R, g = leg.last
    assert np.array_equal(got['states'], S.numpy()) and np.array_equal(got['rewards'], R.numpy())
    assert np.array_equal(got['policy_grad'], g.numpy()) and np.array_equal(got['adam_exp_avg_sq'], leg.v.numpy())
    assert info['bytes'] == sum(v.nbytes for v in got.values())

    # over the cap: the trajectory keeps the same fixed rows on every call, the flat arrays stay whole
    cap = 20000
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', cap)
    info = bench.dump_outputs(leg, str(tmp_path / 's1'))
    bench.dump_outputs(leg, str(tmp_path / 's2'))
    s1, s2 = _load(str(tmp_path / 's1')), _load(str(tmp_path / 's2'))
    k = info['rows_sampled']
    assert 0 < k < 300 and info['bytes'] <= cap and sum(v.nbytes for v in s1.values()) <= cap
    assert s1['states'].shape == (6, k, 4) and s1['actions'].shape == (5, k, 2) and s1['rewards'].shape == (5, k, 1)
    assert all(np.array_equal(s1[n], s2[n]) for n in NAMES)
    rows = np.sort(np.random.default_rng(0).choice(300, size=k, replace=False))
    assert np.array_equal(s1['states'], S.numpy()[:, rows]) and np.array_equal(s1['policy_params'], leg.params.numpy())


@pytest.mark.gpu
def test_bench_steps_and_dump_outputs(tmp_path):
    out_dir = str(tmp_path / 'dump')
    cmd = [sys.executable, os.path.join(common.ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2',
           '--timing-steps', '1', '--no-cpu-baseline', '--no-f32-twin', '--no-other-configs', '--no-sclk',
           '--dump-outputs', out_dir]
    r = subprocess.run(cmd, cwd=common.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['steps'] == 7 and out['timed_steps'] == 7 and out['timed_blocks'] == 1
    assert out['ms_per_step'] > 0 and out['value'] > 0
    got = _load(out_dir)
    assert out['dumped_outputs']['bytes'] == sum(v.nbytes for v in got.values()) <= 64 << 20
    H, B = out['config']['horizon'], out['config']['rows_per_gpu']
    assert got['states'].shape[:2] == (H + 1, B) and got['rewards'].shape == (H, B, 1)
    assert got['policy_grad'].shape == got['policy_params'].shape == got['adam_exp_avg'].shape
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert np.abs(got['policy_grad']).max() > 0 and np.abs(got['adam_exp_avg_sq']).max() > 0
