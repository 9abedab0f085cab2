"""The odometry-covariance record of the batched filter (include/airvision.h, "Odometry covariance"; BatchedMSCKF(odom_cov=True)):
C = J P J^T of every stream at the moment it publishes, 120 doubles per stream and step riding the step's read-back.

What is compared with what:
 * against the library's own state (get_cov / get_state right after a synchronous step that does not reset): rows and columns 0:9 bit
   for bit, the rest within 64 eps (|J| |P| |J^T|) entrywise -- sums of at most 21 + 21 products in two stages with operands rounded
   once, and a J whose entries are themselves a few roundings away from NumPy's;
 * against OracleMSCKF, whose covariance and IMU state are snapshotted inside publish (before its online_reset): 1e-6 max|P|, the bar
   the project uses for P itself;
 * two runs of the library against each other (queue, stream groups, hand-over, feature off, a stopped neighbour): bit for bit.
"""
import os

import numpy as np
import pytest

import filter_harness as H
import odom_cov_ref as R
from filter_harness import bits as _bits, same as _same

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_FRAMES = 30                      # past the first camera-state prune (20 states)
CAP = 128


def _snap_oracle(cfg):
    from oracle.msckf_np import OracleMSCKF

    class SnapOracle(OracleMSCKF):
        """OracleMSCKF that keeps what publish saw: state_cov and the IMU state BEFORE online_reset takes effect."""
        snap = None

        def publish(self, time):
            s = self.imu_state
            self.snap = dict(P=self.state_cov.copy(), q=np.array(s.orientation), R_ic=np.array(s.R_imu_cam0), t_ci=np.array(s.t_cam0_imu))
            return OracleMSCKF.publish(self, time)

        def feature_callback(self, msg):
            self.snap = None
            return OracleMSCKF.feature_callback(self, msg)
    return SnapOracle(cfg)


def _run(cfg, streams, n_frames, odom_cov=True, oracle=False, check=None, **kw):
    """filter_harness.run with the covariance on.  oracle: a SnapOracle per stream alongside; check(k, bat, out, cov, results) runs after
    every step, results[i] = dict(pub, reset, snap) of stream i's oracle (None without)."""
    return H.run(cfg, streams, n_frames, odom_cov=odom_cov, oracle=_snap_oracle if oracle else None,
                 oracle_step=lambda ora, r, reset: dict(pub=r is not None, reset=reset, snap=ora.snap),
                 check=check and (lambda k, bat, out, cur: check(k, bat, out, cur['cov'], cur['ref'])), **kw)


def _streams3(cfg):
    from uav_airvision_amd.synth import SyntheticFeatureStream
    return [SyntheticFeatureStream(cfg, seed=100 + i, n_frames=N_FRAMES, n_features=80, motion_scale=1.0 + 0.25 * i) for i in range(3)]


def _against_oracle(C, snap, where):
    """A record against the oracle's snapshot at publish: 1e-6 max|P|."""
    ref = R.odom_cov(snap['P'], snap['q'], snap['R_ic'], snap['t_ci'])
    err, bar = np.abs(C - ref).max(), 1e-6 * np.abs(snap['P']).max()
    assert err <= bar, (where, err, bar)


_SYNC = {}


def _sync3(cfg, wg):
    """The three streams stepped synchronously with the feature on, checked on every step against the library's own state and
    against the oracle; computed once per launch shape and shared (the other tests compare their records with it bit for bit)."""
    from uav_airvision_amd.msckf_ops import unpack_odom_cov
    if wg in _SYNC:
        return _SYNC[wg]
    seen = dict(pub=0, worst=0.0)

    def check(k, bat, out, cov, results):
        assert cov.shape == (3, 120)
        Cs = unpack_odom_cov(cov)
        for i in range(3):
            assert (out[i, 0] == 1.0) == results[i]['pub'], (k, i)
            if out[i, 0] != 1.0:
                assert np.isnan(cov[i]).all(), (k, i)
                continue
            seen['pub'] += 1
            C = Cs[i]
            assert np.isfinite(C).all() and np.array_equal(C, C.T), (k, i)
            P, gs = bat.get_cov(i), bat.get_state(i)                 # (no reset in this run: the state after the step is the published one)
            assert np.array_equal(_bits(C[:9, :9]), _bits(P[np.ix_(R.SEL9, R.SEL9)])), (k, i)
            ref = R.odom_cov(P, gs['q'], gs['R_ic'], gs['t_ci'])
            bnd = 64 * EPS * R.odom_cov_bound(P, gs['q'], gs['R_ic'], gs['t_ci'])
            ratio = float((np.abs(C - ref) / np.where(bnd > 0, bnd, 1.0)).max())
            seen['worst'] = max(seen['worst'], ratio)
            assert (np.abs(C - ref) <= bnd).all(), (k, i, ratio)
            assert (np.diag(C) >= 0).all() and (k == 0 or (np.diag(C) > 0).all()), (k, i)      # (the first frame publishes the initial covariance: p and theta are exact)
            _against_oracle(C, results[i]['snap'], (k, i))
    env = {'AV_DK_WG': '64'} if wg == 64 else {}
    run = _run(cfg, _streams3(cfg), N_FRAMES, oracle=True, check=check, env=env)
    assert run['counters']['prune_stream_steps'] > 0, run['counters']
    assert run['shape'] == [(3, wg)], run['shape']
    assert seen['pub'] > 60, seen
    print('records checked: %d, worst error / bound(64 eps) = %.3f' % (seen['pub'], seen['worst']))
    _SYNC[wg] = run
    return run


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wg', [256, 64])
def test_record_matches_state_and_oracle_in_both_launch_shapes(cfg, wg):
    run = _sync3(cfg, wg)
    assert len(run['covs']) == N_FRAMES


def test_both_launch_shapes_publish_the_same_bits(cfg):
    a, b = _sync3(cfg, 256), _sync3(cfg, 64)
    for k in range(N_FRAMES):
        assert _same(a['covs'][k], b['covs'][k]), k


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def test_reset_step_publishes_the_pre_reset_covariance_and_idle_streams_nan():
    """Seeds 31 / 32, 60 frames, position_std_threshold = 0.012, stream 1's IMU withheld for 8 frames: on a reset step the record is the
    covariance the pose was published with (the oracle's snapshot inside publish), not what get_cov returns afterwards."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import unpack_odom_cov
    from uav_airvision_amd.synth import SyntheticFeatureStream
    cfg = ConfigEuRoC()
    cfg.position_std_threshold = 0.012
    streams = [SyntheticFeatureStream(cfg, seed=31, n_frames=60, n_features=80), SyntheticFeatureStream(cfg, seed=32, n_frames=60, n_features=80)]
    seen = dict(resets=0, idle=0)

    def check(k, bat, out, cov, results):
        Cs = unpack_odom_cov(cov)
        for i in range(2):
            assert (out[i, 0] == 1.0) == results[i]['pub'], (k, i)
            if not results[i]['pub']:
                seen['idle'] += 1
                assert np.isnan(cov[i]).all(), (k, i)
                continue
            _against_oracle(Cs[i], results[i]['snap'], (k, i))
            if results[i]['reset']:
                seen['resets'] += 1
                after = bat.get_cov(i)
                assert after.shape == (21, 21)
                sel = after[np.ix_(R.SEL9, R.SEL9)]
                assert not np.any(sel[:3, :3]) and np.abs(Cs[i][:3, :3]).max() >= 0.012 ** 2 * 0.99, (k, i)
                assert not np.array_equal(Cs[i][:9, :9], sel), (k, i)
    _run(cfg, streams, 60, cap=512, withhold={1: 8}, oracle=True, check=check)
    assert seen['resets'] >= 1 and seen['idle'] >= 5, seen


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_queued_steps_fill_their_own_arrays(cfg):
    """Three submits (the ring's depth), then wait(0): each array holds its own step's records, bit for bit the synchronous run's."""
    sync = _sync3(cfg, 256)
    run = _run(cfg, _streams3(cfg), N_FRAMES, mode='queue3')
    assert len({id(c) for c in run['covs']}) == N_FRAMES
    for k in range(N_FRAMES):
        assert _same(run['outs'][k], sync['outs'][k]), k
        assert _same(run['covs'][k], sync['covs'][k]), k


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def test_two_stream_groups_fill_their_parts(cfg):
    """Streams {0, 1} and {2} as two groups (AV_MSCKF_GROUPS=2, one wavefront per stream): records bit-identical to the single-group run."""
    sync = _sync3(cfg, 64)
    for mode in ('ahead', 'step'):
        run = _run(cfg, _streams3(cfg), N_FRAMES, mode=mode, env={'AV_MSCKF_GROUPS': '2', 'AV_DK_WG': '64'})
        assert run['shape'] == [(2, 64), (1, 64)], run['shape']
        for k in range(N_FRAMES):
            assert _same(run['outs'][k], sync['outs'][k]), (mode, k)
            assert _same(run['covs'][k], sync['covs'][k]), (mode, k)


# ---- (e) -------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(cfg, monkeypatch):
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    on = _sync3(cfg, 256)
    seen = {}

    def check(k, bat, out, cov, results):
        if k == 3:
            with pytest.raises(ValueError, match='odom_cov'):
                bat.step(np.zeros((3, CAP), np.int64), np.zeros((3, CAP, 4)), np.zeros(3, np.int32), np.full(3, -1.0), cov=True)
            with pytest.raises(AirvisionError, match='first step'):
                bat.set_odom_cov(True)
            seen['raised'] = True
    off = _run(cfg, _streams3(cfg), N_FRAMES, odom_cov=False, check=check)
    assert seen.get('raised')
    for k in range(N_FRAMES):
        assert _same(off['outs'][k], on['outs'][k]), k
    for s in range(3):
        assert len(off['final'][s]) == len(on['final'][s])
        for x, y in zip(off['final'][s], on['final'][s]):
            assert _same(x, y), s
    # the C entry refuses a destination while the feature is off
    for name in ('AV_DK_WG', 'AV_MSCKF_GROUPS'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.delenv('AV_MSCKF_STORE', raising=False)
    bat = BatchedMSCKF(cfg, 1)
    try:
        from uav_airvision_amd import _native as N
        buf = np.zeros(120)
        assert N.lib().av_msckf_batch_next_odom_cov(bat._h, buf.ctypes.data) == N.AV_E_INVALID
        assert b'av_msckf_batch_set_odom_cov' in N.lib().av_last_error()
    finally:
        bat.close()


# ---- (f) -------------------------------------------------------------------------------------------------------------------------
_HANDOVER = {}


def _handover_run(cfg):
    """2 streams, 12 rendered frames through FrontendEngine + submit_dev(cov=True), once: (IMU schedule, the messages read back from the
    engine, the step outputs, the records)."""
    if not _HANDOVER:
        h = H.handover_run(cfg, odom_cov=True)
        assert sum(bool(o[0, 0] == 1.0) for o in h['outs']) >= 5
        _HANDOVER.update(h)
    return _HANDOVER


def test_device_handover_matches_a_step_run_of_the_same_messages(cfg):
    """2 streams, 12 rendered frames through FrontendEngine + submit_dev; then a `step` run fed the messages read back from the engine."""
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    h = _handover_run(cfg)
    rows, msgs, outs, covs = h['rows'], h['msgs'], h['outs'], h['covs']
    ref = BatchedMSCKF(cfg, 2, max_features=msgs[0][0].shape[1], odom_cov=True)
    try:
        for k in range(len(msgs)):
            if rows[k]:
                ref.push_imu([i for i, _ in rows[k]], [m.timestamp for _, m in rows[k]], [m.angular_velocity for _, m in rows[k]],
                             [m.linear_acceleration for _, m in rows[k]])
            out = ref.step(*msgs[k], cov=True)
            assert _same(out, outs[k]), k
            assert _same(ref.last_cov, covs[k]), k
            assert np.isnan(covs[k][out[:, 0] != 1.0]).all() and np.isfinite(covs[k][out[:, 0] == 1.0]).all(), k
    finally:
        ref.close()


def test_filter_set_joins_the_parts_records(cfg):
    """The same two streams as two pipelines (EngineSet + FilterSet(odom_cov=True)): last_cov joins the parts' records as the returned
    view joins their poses, and a stream's record is what it is in one batch."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.pipelines import EngineSet, FilterSet
    h = _handover_run(cfg)
    eng = EngineSet(cfg, 2, 2)
    flt = None
    try:
        flt = FilterSet(cfg, eng, max_features=eng.max_features, odom_cov=True)
        with pytest.raises(ValueError):
            flt.submit_dev(eng, h['cams'][0][2], cov=np.zeros((2, 120)))
        outs, covs = [], []
        for k, (c0, c1, ts) in enumerate(h['cams']):
            i = np.array([i for i, _ in h['rows'][k]], np.int32)
            t = np.array([m.timestamp for _, m in h['rows'][k]])
            w = np.array([m.angular_velocity for _, m in h['rows'][k]]).reshape(-1, 3)
            a = np.array([m.linear_acceleration for _, m in h['rows'][k]]).reshape(-1, 3)
            eng.push_imu_batch(i, t, w)
            eng.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            flt.push_imu(i, t, w, a)
            outs.append(flt.submit_dev(eng, ts, msg_stream=N.current_stream(), cov=True))
            covs.append(flt.last_cov)
        flt.wait(0)
        for k in range(len(outs)):
            assert _same(outs[k].array(), h['outs'][k]), k
            assert covs[k].array().shape == (2, 120) and _same(covs[k].array(), h['covs'][k]), k
    finally:
        if flt is not None:
            flt.close()
        eng.close()
    plain = FilterSet.__new__(FilterSet)
    plain.odom_cov, plain.es = False, eng
    with pytest.raises(ValueError, match='odom_cov'):
        plain.submit_dev(eng, np.zeros(2), cov=True)


# ---- (g) -------------------------------------------------------------------------------------------------------------------------
def test_stopped_stream_reads_nan_and_leaves_its_neighbour_alone(cfg):
    """Stream 0 is stopped by a capacity limit (the overflow pool shrunk to 64 rows, a blank frame at 17, as in
    test_overflow_pool_exhaustion_stops_the_stream_with_a_capacity_error): from then on its records are NaN, and stream 1's records are
    those of stream 1 run alone."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    n = 24
    mk = lambda: [SyntheticFeatureStream(cfg, seed=91, n_frames=n, n_features=150), SyntheticFeatureStream(cfg, seed=92, n_frames=n, n_features=40)]
    env = {'AV_MSCKF_POOL_ROWS': '64'}
    both = _run(cfg, mk(), n, cap=192, blank={0: (17,)}, env=env, rows_cap=2048)
    solo = _run(cfg, mk()[1:], n, cap=192, env=env, rows_cap=2048)
    stopped = [k for k in range(n) if both['outs'][k][0, 0] < 0]
    assert stopped == list(range(17, n)), stopped
    for k in range(n):
        if k >= 17:
            assert np.isnan(both['covs'][k][0]).all(), k
        elif both['outs'][k][0, 0] == 1.0:
            assert np.isfinite(both['covs'][k][0]).all(), k
        assert _same(both['outs'][k][1:], solo['outs'][k]), k
        assert _same(both['covs'][k][1:], solo['covs'][k]), k
    assert sum(bool(o[0, 0] == 1.0) for o in solo['outs']) > 15


# ---- (h) -------------------------------------------------------------------------------------------------------------------------
def test_dropin_last_covariance_is_the_stream_s_record(cfg):
    """The drop-in MSCKF with config.publish_covariance: last_covariance after every published frame is stream 0's record of the
    three-stream run, bit for bit (a stream's arithmetic does not depend on its neighbours); vio_result is what it was."""
    import sys
    from conftest import ROOT
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import unpack_odom_cov
    from uav_airvision_amd.synth import replay_features
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import msckf as dmsckf
    sync = _sync3(cfg, 256)
    c = ConfigEuRoC()
    assert c.publish_covariance is False
    off = dmsckf.MSCKF(c, write_trajectory=False)
    assert off.last_covariance is None
    off.close()
    c.publish_covariance = True
    c.T_imu_body = np.identity(4)
    c.T_imu_body[0, 3] = 0.1
    with pytest.raises(ValueError, match='T_imu_body'):
        dmsckf.MSCKF(c, write_trajectory=False)
    c.T_imu_body = np.identity(4)
    flt = dmsckf.MSCKF(c, write_trajectory=False)
    got = []

    def on(m):
        r = flt.feature_callback(m)
        assert r is None or r._fields == ('timestamp', 'pose', 'velocity', 'cam0_pose')
        got.append(None if r is None else flt.last_covariance.copy())
    try:
        replay_features(_streams3(cfg)[0], [flt.imu_callback], on)
    finally:
        flt.close()
    assert len(got) == N_FRAMES and sum(g is not None for g in got) > 20
    for k, g in enumerate(got):
        if g is None:
            assert sync['outs'][k][0, 0] != 1.0, k
        else:
            assert g.shape == (15, 15) and _same(g, unpack_odom_cov(sync['covs'][k][0])), k


def test_sweep_covariance_files_and_anees(tmp_path, monkeypatch, capsys):
    """sweep --covariance on a short EuRoC-layout sequence: next to the trajectory file a _cov file with one row per pose, t + 120 numbers
    that parse to the records of the run (%.9e keeps ten digits); the report carries a finite anees_pos (no bar: nobody has measured it)."""
    import json
    from fe_harness import make_cfg
    from uav_airvision_amd import sweep
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    # (the sequence's IMU starts with its first frame: 20 frames at rest pass before gravity is initialised, and the report wants more than 20 poses)
    st = SyntheticStream(make_cfg(), seed=13, n_frames=44, motion_scale=3.0, t0=1403636580.0, rest=1.0)
    write_euroc_layout(str(tmp_path / 'SEQ'), st, compress_level=1)
    kept = []
    inner = sweep.run_batched

    def run_batched(*a, **kw):
        kept.append(kw['cov_rows'])
        return inner(*a, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    out = tmp_path / 'txts'
    sweep.main(['--root', str(tmp_path), '--sequences', 'SEQ', '--covariance', '--out', str(out)])
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    traj = np.loadtxt(str(out / 'output_SEQ_offset0.txt')).reshape(-1, 8)
    rows = np.loadtxt(str(out / 'output_SEQ_offset0_cov.txt')).reshape(-1, 121)
    (rec,), = kept
    assert len(traj) > 20 and rows.shape == rec.shape == (len(traj), 121)
    assert np.abs(rows[:, 0] - traj[:, 0]).max() < 1e-6 and np.abs(rows[:, 0] - rec[:, 0]).max() < 1e-6
    assert np.isfinite(rec).all()
    assert (np.abs(rows[:, 1:] - rec[:, 1:]) <= 1e-9 * np.abs(rec[:, 1:])).all()
    r0 = rep['report'][0]
    assert r0['frames'] == len(traj) and np.isfinite(r0['ate_rmse'])
    assert np.isfinite(r0['anees_pos']) and r0['anees_pos'] > 0
    print('anees_pos of the synthetic sequence: %.3e (ate %.4f m)' % (r0['anees_pos'], r0['ate_rmse']))
