"""The landmark map of the batched filter (include/airvision.h, "Landmark map"; BatchedMSCKF(landmarks=True)): per stream and step a
count pair and up to landmark_cap records of 40 bytes, riding the step's read-back.

What is compared with what:
 * against tests/landmark_ref.py (the NumPy oracle restated with the records written down), in both launch shapes: counts, ids in order,
   flags and n_obs exactly; positions within 1e-6 * max(1, z^2 / b) metres -- the project's 1e-6 end-to-end state bar times the
   first-order sensitivity of a triangulated depth to pose error (z = distance to the first observing camera, b = the widest baseline
   between observing camera centres, both of the triangulation that fixed the position);
 * two runs of the library against each other (launch shapes, queue, stream groups, hand-over, cap, covariance on, feature off): bit for bit.

Streams: seeds 7 (3 % outliers, so that the gate rejects), 100 and 101, 50 features per frame, 40 frames.  The smallest distance of a
gating value to its chi-square threshold along these runs is 2.9 % (seed 7) and above 78 % (the others), against the 1e-7 at which the
per-call gate comparisons of tests/test_gpu_msckf.py agree: no flag rests on a marginal decision.

Largest position error / bar measured on an MI355X: 4.9e-04 over 593 records, the same at both launch shapes (profiles/landmarks/README.md)."""
import os

import numpy as np
import pytest

import filter_harness as H
import landmark_ref as L
from filter_harness import push as _push, same as _same, same_lm as _same_lm

pytestmark = pytest.mark.gpu

N_FRAMES = 40
CAP = 128
LM_CAP = 64


def _run(cfg, streams, n_frames, landmarks=True, oracle=False, check=None, **kw):
    """filter_harness.run with the map on.  oracle: a LandmarkOracle per stream runs alongside; refs[k][i] is its record list, resets[k][i]
    whether its step ended in online_reset.  check(k, bat, out) runs after every step."""
    run = H.run(cfg, streams, n_frames, landmarks=landmarks, oracle=L.LandmarkOracle if oracle else None,
                oracle_step=lambda ora, r, reset: (list(ora.landmarks), reset), check=check and (lambda k, bat, out, cur: check(k, bat, out)), **kw)
    run['refs'], run['resets'] = [[x[0] for x in ref] for ref in run['refs']], [[x[1] for x in ref] for ref in run['refs']]
    return run


def _against_ref(rec, n, s, ref, lm_cap, where):
    """Stream s's records of one step against the reference's list; returns the largest position error / bar."""
    from uav_airvision_amd.msckf_ops import unpack_landmarks
    assert int(n[s, 0]) == len(ref) and int(n[s, 1]) == min(len(ref), lm_cap), (where, n[s].tolist(), len(ref))
    got = unpack_landmarks(rec, n, s)
    ref = ref[:lm_cap]
    assert got['id'].tolist() == [r['id'] for r in ref], where
    assert got['flags'].tolist() == [r['flags'] for r in ref], (where, got['flags'].tolist(), [r['flags'] for r in ref])
    assert got['n_obs'].tolist() == [r['n_obs'] for r in ref], where
    worst = 0.0
    for g, r in zip(got, ref):
        err, bar = float(np.linalg.norm(g['p'] - r['p'])), 1e-6 * max(1.0, r['z'] ** 2 / r['b'])
        assert err <= bar, (where, r['id'], err, bar)
        worst = max(worst, err / bar)
    return worst


def _streams3(cfg):
    from uav_airvision_amd.synth import SyntheticFeatureStream
    return [SyntheticFeatureStream(cfg, seed=7, n_frames=N_FRAMES, n_features=50, outlier_rate=0.03),
            SyntheticFeatureStream(cfg, seed=100, n_frames=N_FRAMES, n_features=50),
            SyntheticFeatureStream(cfg, seed=101, n_frames=N_FRAMES, n_features=50, motion_scale=1.25)]


_SYNC = {}


def _sync3(cfg, wg):
    """The three streams stepped synchronously with the map on and the reference alongside, checked on every step; computed once per
    launch shape and shared (the other tests compare their records with it bit for bit)."""
    if wg in _SYNC:
        return _SYNC[wg]
    run = _run(cfg, _streams3(cfg), N_FRAMES, oracle=True, env={'AV_DK_WG': '64'} if wg == 64 else {})
    assert run['shape'] == [(3, wg)], run['shape']
    worst, seen = 0.0, set()
    for k in range(N_FRAMES):
        rec, n = run['lms'][k]
        for s in range(3):
            worst = max(worst, _against_ref(rec, n, s, run['refs'][k][s], LM_CAP, 'wg %d frame %d stream %d' % (wg, k, s)))
            seen.update(r['flags'] for r in run['refs'][k][s])
    assert run['counters']['prune_stream_steps'] >= 9, run['counters']
    total = sum(len(r) for ref in run['refs'] for r in ref)
    assert total > 500 and {L.LM_USED | L.LM_NEW, L.LM_REJECTED | L.LM_NEW, L.LM_TRACKED | L.LM_NEW | L.LM_USED, L.LM_USED} <= seen, (total, seen)
    print('wg %d: %d records checked, largest position error / bar = %.3e' % (wg, total, worst))
    _SYNC[wg] = run
    return run


# ---- parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wg', [256, 64])
def test_records_match_the_reference_in_both_launch_shapes(cfg, wg):
    run = _sync3(cfg, wg)
    assert len(run['lms']) == N_FRAMES


def test_both_launch_shapes_publish_the_same_bytes(cfg):
    a, b = _sync3(cfg, 256), _sync3(cfg, 64)
    for k in range(N_FRAMES):
        assert _same(a['outs'][k], b['outs'][k]) and _same_lm(a['lms'][k], b['lms'][k]), k


def test_a_feature_fixed_while_pruning_comes_back_final_with_the_same_bits(cfg):
    """TRACKED | NEW when a pruning step first fixes it; when it is lost later, a final record with identical position bits, without NEW."""
    from uav_airvision_amd.msckf_ops import unpack_landmarks
    run = _sync3(cfg, 256)
    again = 0
    for s in range(3):
        tracked, final = {}, set()
        for k in range(N_FRAMES):
            for r in unpack_landmarks(*run['lms'][k], s):
                fid = int(r['id'])
                if r['flags'] & L.LM_TRACKED:
                    assert r['flags'] & L.LM_NEW and fid not in tracked and fid not in final, (s, k, fid)
                    tracked[fid] = r['p'].tobytes()
                else:
                    assert fid not in final, (s, k, fid)
                    final.add(fid)
                    if fid in tracked:
                        assert not r['flags'] & L.LM_NEW and r['p'].tobytes() == tracked[fid], (s, k, fid)
                        again += 1
                    else:
                        assert r['flags'] & L.LM_NEW, (s, k, fid)
    assert again > 30, again


# ---- the 1,500-row cut and the cap ---------------------------------------------------------------------------------------------------
def test_row_cut_and_cap_on_a_frame_that_loses_every_track(cfg):
    """One stream, 120 features tracked over 10 frames, then an empty message: all are lost at once with 37 rows each, so the cut falls
    inside the list (the 41st feature takes the sum over 1,500).  landmark_cap=256: USED up to and including the crossing feature, no
    bit after it, as the reference has them.  landmark_cap=16: n = {120, 16} and the 16 are the first 16 of the other run, bit for bit."""
    from uav_airvision_amd.msckf_ops import unpack_landmarks
    from uav_airvision_amd.synth import SyntheticFeatureStream

    class Long(SyntheticFeatureStream):
        def _spawn(self, R_c0_w, c0_w):
            tr = SyntheticFeatureStream._spawn(self, R_c0_w, c0_w)
            tr[2] = 10 ** 6
            return tr
    st = Long(cfg, seed=7, n_frames=11, n_features=120, motion_scale=0.3)
    big = _run(cfg, [st], 11, lm_cap=256, blank={0: (10,)}, oracle=True)
    ref = big['refs'][10][0]
    rec, n = big['lms'][10]
    assert len(ref) == 120 and all(r['n_obs'] == 10 for r in ref)
    flags = unpack_landmarks(rec, n, 0)['flags'].tolist()
    assert flags == [L.LM_USED | L.LM_NEW] * 41 + [L.LM_NEW] * 79, flags
    _against_ref(rec, n, 0, ref, 256, 'cut')
    for k in range(10):
        assert big['lms'][k][1].tolist() == [[0, 0]], k
    small = _run(cfg, [st], 11, lm_cap=16, blank={0: (10,)})
    rec16, n16 = small['lms'][10]
    assert n16.tolist() == [[120, 16]] and rec16.shape == (1, 16)
    assert rec16[0].tobytes() == rec[0, :16].tobytes()
    for k in range(11):
        assert _same(small['outs'][k], big['outs'][k]), k


# ---- further behaviours --------------------------------------------------------------------------------------------------------------
def test_idle_and_stopped_streams_read_zero_and_leave_their_neighbour_alone(cfg):
    """Stream 0 is stopped by a capacity limit (the overflow pool shrunk to 64 rows, a blank frame at 17), stream 2 has no frame
    (timestamp < 0) in three steps: both read {0, 0} there, and stream 1's records are those of stream 1 run alone."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    n = 24
    mk = lambda: [SyntheticFeatureStream(cfg, seed=91, n_frames=n, n_features=150), SyntheticFeatureStream(cfg, seed=92, n_frames=n, n_features=40),
                  SyntheticFeatureStream(cfg, seed=100, n_frames=n, n_features=50)]
    env = {'AV_MSCKF_POOL_ROWS': '64'}
    idle = (5, 6, 20)
    both = _run(cfg, mk(), n, cap=192, blank={0: (17,)}, idle={2: idle}, env=env, rows_cap=2048)
    solo = _run(cfg, mk()[1:2], n, cap=192, env=env, rows_cap=2048)
    assert [k for k in range(n) if both['outs'][k][0, 0] < 0] == list(range(17, n))
    had = np.zeros(3, np.int64)
    for k in range(n):
        rec, cnt = both['lms'][k]
        if k >= 17:
            assert cnt[0].tolist() == [0, 0], k
        if k in idle:
            assert both['outs'][k][2, 0] == 0.0 and cnt[2].tolist() == [0, 0], k
        had += cnt[:, 0]
        assert _same(both['outs'][k][1:2], solo['outs'][k]), k
        assert _same_lm((rec[1:2], cnt[1:2]), solo['lms'][k]), k
    assert (had > 20).all(), had


def test_a_step_that_ends_in_online_reset_still_carries_its_records():
    """Seed 31, position_std_threshold = 0.1: the position deviation passes 0.1 m (0.105) in the sixth frame, whose two updates used two
    lost features; the step publishes them although the map is empty afterwards."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticFeatureStream
    cfg = ConfigEuRoC()
    cfg.position_std_threshold = 0.1
    st = SyntheticFeatureStream(cfg, seed=31, n_frames=24, n_features=50)
    run = _run(cfg, [st], 24, oracle=True)
    on_reset = 0
    for k in range(24):
        _against_ref(*run['lms'][k], 0, run['refs'][k][0], LM_CAP, 'reset run frame %d' % k)
        if run['resets'][k][0]:
            on_reset += len(run['refs'][k][0])
    assert run['counters']['max_cam_states'] > 0 and sum(r[0] for r in run['resets']) >= 1 and on_reset >= 2, (run['resets'], on_reset)


def test_queued_steps_fill_their_own_arrays(cfg):
    """Three submits (the ring's depth), then wait(0): each pair holds its own step's records, bit for bit the synchronous run's."""
    sync = _sync3(cfg, 256)
    run = _run(cfg, _streams3(cfg), N_FRAMES, mode='queue3')
    assert len({id(p[0]) for p in run['lms']}) == N_FRAMES
    for k in range(N_FRAMES):
        assert _same(run['outs'][k], sync['outs'][k]) and _same_lm(run['lms'][k], sync['lms'][k]), k


def test_two_stream_groups_fill_their_parts(cfg):
    """Streams {0, 1} and {2} as two groups (AV_MSCKF_GROUPS=2, one wavefront per stream): bit-identical to the single-group run."""
    sync = _sync3(cfg, 64)
    for mode in ('ahead', 'step'):
        run = _run(cfg, _streams3(cfg), N_FRAMES, mode=mode, env={'AV_MSCKF_GROUPS': '2', 'AV_DK_WG': '64'})
        assert run['shape'] == [(2, 64), (1, 64)], run['shape']
        for k in range(N_FRAMES):
            assert _same(run['outs'][k], sync['outs'][k]) and _same_lm(run['lms'][k], sync['lms'][k]), (mode, k)


def test_map_and_covariance_together_equal_their_single_feature_runs(cfg):
    lm_only = _sync3(cfg, 256)
    cov_only = _run(cfg, _streams3(cfg), N_FRAMES, landmarks=False, odom_cov=True)
    for env in ({}, {'AV_DK_WG': '64'}):
        both = _run(cfg, _streams3(cfg), N_FRAMES, odom_cov=True, env=env)
        for k in range(N_FRAMES):
            assert _same(both['outs'][k], lm_only['outs'][k]), k
            assert _same_lm(both['lms'][k], lm_only['lms'][k]), k
            assert _same(both['covs'][k], cov_only['covs'][k]), k


def _live():
    import ctypes
    from uav_airvision_amd import _native as N
    out = (ctypes.c_int64 * 4)()
    N.check(N.lib().av_debug_live_resources(ctypes.byref(out)))
    return [int(v) for v in out]


def test_off_means_off(cfg, monkeypatch):
    """Off: the poses are bit-identical to a run with the map on, no byte of device or pinned memory more than without the feature (the
    run with the map on holds exactly its record and count buffers more: one device pair, one pinned pair per ring slot), landmarks=
    raises; the switch is refused after the first step."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.msckf_ops import LANDMARK_DTYPE, BatchedMSCKF
    on = _sync3(cfg, 256)
    seen = {}

    def check_off(k, bat, out):
        if k == 3:
            seen['off'] = _live()
            with pytest.raises(ValueError, match='landmarks'):
                bat.step(np.zeros((3, CAP), np.int64), np.zeros((3, CAP, 4)), np.zeros(3, np.int32), np.full(3, -1.0), landmarks=True)
            with pytest.raises(AirvisionError, match='first step'):
                bat.set_landmarks(64)
            assert bat.landmark_cap == 0 and bat.last_landmarks is None

    def check_on(k, bat, out):
        if k == 3:
            seen['on'] = _live()
    base = _live()
    off = _run(cfg, _streams3(cfg), N_FRAMES, landmarks=False, check=check_off)
    _run(cfg, _streams3(cfg), 4, check=check_on)
    assert _live() == base
    for k in range(N_FRAMES):
        assert _same(off['outs'][k], on['outs'][k]), k
    S, ring = 3, 3
    assert seen['on'][0] - seen['off'][0] == (S * LM_CAP * 40 + 256) + (S * 2 * 4 + 256), (seen, base)
    assert seen['on'][1] - seen['off'][1] == ring * ((S * LM_CAP * 40 + 64) + (S * 2 * 4 + 64)), (seen, base)
    assert seen['on'][2:] == seen['off'][2:]
    for name in ('AV_DK_WG', 'AV_MSCKF_GROUPS', 'AV_MSCKF_STORE'):
        monkeypatch.delenv(name, raising=False)
    bat = BatchedMSCKF(cfg, 1)
    try:
        rec, n = np.zeros((1, 64), LANDMARK_DTYPE), np.zeros((1, 2), np.int32)
        assert N.lib().av_msckf_batch_next_landmarks(bat._h, rec.ctypes.data, n.ctypes.data) == N.AV_E_INVALID
        assert b'av_msckf_batch_set_landmarks' in N.lib().av_last_error()
    finally:
        bat.close()


def test_abi_record_layout():
    """Header, ctypes mirror and NumPy dtype agree on the 40-byte record (the header's struct is checked against the compiler on the CPU
    side by tests/test_landmark_abi.py)."""
    import ctypes
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.msckf_ops import LANDMARK_DTYPE
    assert ctypes.sizeof(N.Landmark) == LANDMARK_DTYPE.itemsize == 40
    assert [LANDMARK_DTYPE.fields[f][1] for f in ('id', 'p', 'flags', 'n_obs')] == [N.Landmark.id.offset, N.Landmark.p.offset, N.Landmark.flags.offset, N.Landmark.n_obs.offset]


# ---- hand-over, FilterSet -----------------------------------------------------------------------------------------------------------
_HANDOVER = {}


def _handover_run(cfg):
    """2 streams, 12 rendered frames through FrontendEngine + submit_dev(landmarks=True), once."""
    if not _HANDOVER:
        h = H.handover_run(cfg, landmarks=True)
        assert sum(bool(o[0, 0] == 1.0) for o in h['outs']) >= 5 and sum(int(p[1][:, 1].sum()) for p in h['lms']) > 0
        _HANDOVER.update(h)
    return _HANDOVER


def test_device_handover_matches_a_step_run_of_the_same_messages(cfg):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    h = _handover_run(cfg)
    ref = BatchedMSCKF(cfg, 2, max_features=h['msgs'][0][0].shape[1], landmarks=True)
    try:
        for k in range(len(h['msgs'])):
            _push(ref, h['rows'][k])
            out = ref.step(*h['msgs'][k], landmarks=True)
            assert _same(out, h['outs'][k]) and _same_lm(ref.last_landmarks, h['lms'][k]), k
    finally:
        ref.close()


def test_filter_set_joins_the_parts_records(cfg):
    """The same two streams as two pipelines (EngineSet + FilterSet(landmarks=True)): last_landmarks joins the parts' arrays."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.pipelines import EngineSet, FilterSet
    h = _handover_run(cfg)
    eng = EngineSet(cfg, 2, 2)
    flt = None
    try:
        flt = FilterSet(cfg, eng, max_features=eng.max_features, landmarks=True)
        with pytest.raises(ValueError):
            flt.submit_dev(eng, h['cams'][0][2], landmarks=(1, 2))
        outs, lms = [], []
        for k, (c0, c1, ts) in enumerate(h['cams']):
            i = np.array([i for i, _ in h['rows'][k]], np.int32)
            t = np.array([m.timestamp for _, m in h['rows'][k]])
            w = np.array([m.angular_velocity for _, m in h['rows'][k]]).reshape(-1, 3)
            a = np.array([m.linear_acceleration for _, m in h['rows'][k]]).reshape(-1, 3)
            eng.push_imu_batch(i, t, w)
            eng.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            flt.push_imu(i, t, w, a)
            outs.append(flt.submit_dev(eng, ts, msg_stream=N.current_stream(), landmarks=True))
            lms.append(flt.last_landmarks)
        flt.wait(0)
        for k in range(len(outs)):
            rec, n = lms[k][0].array(), lms[k][1].array()
            assert rec.shape == (2, LM_CAP) and n.shape == (2, 2)
            assert _same(outs[k].array(), h['outs'][k]) and _same_lm((rec, n), h['lms'][k]), k
    finally:
        if flt is not None:
            flt.close()
        eng.close()
    plain = FilterSet.__new__(FilterSet)
    plain.odom_cov, plain.landmarks, plain.es = False, False, eng
    with pytest.raises(ValueError, match='landmarks'):
        plain.submit_dev(eng, np.zeros(2), landmarks=True)


# ---- drop-in, sweep -------------------------------------------------------------------------------------------------------------------
def test_dropin_last_landmarks_are_stream_0s_records_in_the_published_frame(cfg):
    """The drop-in MSCKF with config.publish_landmarks and a T_imu_body that rotates and shifts: last_landmarks after every
    feature_callback holds stream 0's records of the three-stream run (a stream's arithmetic does not depend on its neighbours) with
    p mapped by T_imu_body, within the bar of the reference's records mapped the same way; vio_result is what it was."""
    import sys
    from conftest import ROOT
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import unpack_landmarks
    from uav_airvision_amd.synth import replay_features
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import msckf as dmsckf
    sync = _sync3(cfg, 256)
    c = ConfigEuRoC()
    assert c.publish_landmarks is False
    off = dmsckf.MSCKF(c, write_trajectory=False)
    assert off.last_landmarks is None
    off.close()
    ang = 0.3
    T = np.identity(4)
    T[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.1, -0.2, 0.05]
    c.publish_landmarks, c.landmark_cap, c.T_imu_body = True, LM_CAP, T
    flt = dmsckf.MSCKF(c, write_trajectory=False)
    got = []

    def on(m):
        r = flt.feature_callback(m)
        assert r is None or r._fields == ('timestamp', 'pose', 'velocity', 'cam0_pose')
        got.append(flt.last_landmarks.copy())
    try:
        replay_features(_streams3(cfg)[0], [flt.imu_callback], on)
    finally:
        flt.close()
    assert len(got) == N_FRAMES and sum(len(g) for g in got) > 150
    for k, g in enumerate(got):
        want = unpack_landmarks(*sync['lms'][k], 0)
        ref = sync['refs'][k][0]
        assert len(g) == len(want) == len(ref), k
        assert g['id'].tolist() == want['id'].tolist() and g['flags'].tolist() == want['flags'].tolist() and g['n_obs'].tolist() == want['n_obs'].tolist(), k
        if len(g):
            assert np.abs(g['p'] - (want['p'] @ T[:3, :3].T + T[:3, 3])).max() <= 1e-12, k
        for a, r in zip(g, ref):
            err, bar = float(np.linalg.norm(a['p'] - (T[:3, :3] @ r['p'] + T[:3, 3]))), 1e-6 * max(1.0, r['z'] ** 2 / r['b'])
            assert err <= bar, (k, r['id'], err, bar)


def test_sweep_writes_the_map_file(tmp_path, monkeypatch, capsys):
    """sweep --landmarks on a short EuRoC-layout sequence: next to the trajectory file a _map file, one line `t id x y z flags n_obs` per
    record of the run (%.9f keeps the nanometre); the report states the records dropped to the cap."""
    import json
    from fe_harness import make_cfg
    from uav_airvision_amd import sweep
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(make_cfg(), seed=13, n_frames=44, motion_scale=3.0, t0=1403636580.0, rest=1.0)
    write_euroc_layout(str(tmp_path / 'SEQ'), st, compress_level=1)
    kept = []
    inner = sweep.run_batched

    def run_batched(*a, **kw):
        kept.append(kw['lm_rows'])
        return inner(*a, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    out = tmp_path / 'txts'
    sweep.main(['--root', str(tmp_path), '--sequences', 'SEQ', '--landmarks', '--landmark-cap', '32', '--out', str(out)])
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    traj = np.loadtxt(str(out / 'output_SEQ_offset0.txt')).reshape(-1, 8)
    rows = np.loadtxt(str(out / 'output_SEQ_offset0_map.txt')).reshape(-1, 7)
    ((ts, rec, dropped),), = kept
    assert len(traj) > 20 and len(rows) == len(rec) == len(ts) > 20
    assert np.abs(rows[:, 0] - ts).max() < 1e-6 and np.isin(np.round(rows[:, 0], 6), np.round(traj[:, 0], 6)).all()
    assert rows[:, 1].astype(np.int64).tolist() == rec['id'].tolist()
    assert np.abs(rows[:, 2:5] - rec['p']).max() <= 1e-9
    assert rows[:, 5].astype(np.int32).tolist() == rec['flags'].tolist() and rows[:, 6].astype(np.int32).tolist() == rec['n_obs'].tolist()
    assert rep['landmarks'] == dict(cap=32, records=[len(rec)], dropped_to_cap=[int(dropped)])
