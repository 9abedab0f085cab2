"""bench.py end to end on the GPU at a reduced stream count: one JSON line with the contract fields, a positive
throughput, the roofline and (with --full) CPU-baseline objects, and the queued / threaded pipeline shutting down cleanly;
a plain run's line and the outputs it writes with --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_runs_and_prints_one_contract_line():
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--streams', '64', '--steps', '4', '--warmup', '24', '--full'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 4 and d['warmup'] == 24 and d['value'] > 0
    assert d['config']['streams_per_gpu'] == 64 and d['msckf_in_step'] is True
    assert d['roofline']['bound'] == 'hbm' and 0 < d['roofline']['frac'] < 1 and d['roofline']['traffic'] > 0
    assert d['cpu_baseline']['kind'] == 'port' and d['cpu_baseline']['cores'] == 1 and d['cpu_baseline']['value'] > 0
    assert abs(d['value'] - 64 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6


def _plain_run(dump_dir, steps=6, extra=()):
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--streams', '64', '--steps', str(steps), '--warmup', '2',
                        '--dump-outputs', str(dump_dir)] + list(extra), cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(dump_dir, f)) for f in sorted(os.listdir(dump_dir))}


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline only (no CPU baseline, no regimes, no front-end-only loop), --steps timed steps, and the last
    step's features and filter output as float64 arrays -- the same on a second run of the same command."""
    d, a = _plain_run(tmp_path / 'a')
    assert d['steps'] == 6 and d['warmup'] == 2 and d['full'] is False and d['value'] > 0
    assert d['dtype'] and d['unit'] == 'stereo frames/s' and d['higher_is_better'] is True
    assert abs(d['value'] - 64 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    assert 'cpu_baseline' not in d and 'regimes' not in d and d['frontend_only_frames_per_s'] is None
    assert sorted(a) == ['feature_counts', 'feature_ids', 'feature_uv', 'filter_output', 'stream_index']
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a['stream_index'], np.arange(64))
    assert a['feature_counts'].min() > 20 and a['feature_counts'].sum() == len(a['feature_ids']) == len(a['feature_uv'])
    assert a['feature_uv'].shape[1] == 4 and a['filter_output'].shape == (64, 12) and (a['filter_output'][:, 0] > 0.5).all()
    _, b = _plain_run(tmp_path / 'b')
    for k in ('stream_index', 'feature_counts', 'feature_ids', 'feature_uv'):
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(a['filter_output'] - b['filter_output']).max() <= 1e-9


def test_run_longer_than_the_resident_frames_plays_them_forward_and_back(tmp_path):
    """100 steps through 48 resident frames (turns at frames 47 and 24, four of them in the timed region, all at speed): the
    filters follow the mirrored motion -- every stream still publishes, with a finite pose near the synthetic trajectory's range, and the front-end keeps
    its tracks."""
    d, a = _plain_run(tmp_path / 'long', steps=100, extra=['--max-resident-frames', '48'])
    assert d['steps'] == 100 and d['config']['resident_frames'] == 48 and d['config']['frames_stepped'] == 25 + 2 + 100
    assert abs(d['value'] - 64 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    out = a['filter_output']
    assert (out[:, 0] > 0.5).all() and np.isfinite(out).all()
    assert np.abs(out[:, 2:5]).max() < 2.0                      # positions: the trajectories span well under a metre
    assert np.abs(np.linalg.norm(out[:, 5:9], axis=1) - 1).max() < 1e-6 and np.abs(out[:, 9:12]).max() < 1.5
    assert a['feature_counts'].min() > 20
    assert d['steady_state']['cam_states_at_t0'][0] >= 18
