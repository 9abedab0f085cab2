"""The IMU-rate odometry of the batched filter (include/airvision.h, "IMU-rate odometry"; BatchedMSCKF(imu_rate=True)): per stream and
step a count pair and the state after every IMU sample the step's prediction integrated, records of 112 bytes riding the step's
read-back.

What is compared with what:
 * against tests/imu_rate_ref.py (OracleMSCKF with the records written down): counts and t exactly; p, q, v, w within 1e-6, the bar the
   project uses for the filter's state against OracleMSCKF (the records are that state between two frames);
 * against the step's own published pose, for a stream that never updates: bit for bit;
 * two runs of the library against each other (launch shapes, queue, stream groups, hand-over, FilterSet, the other outputs on, the
   feature off, a stopped neighbour, a restart, the drop-in class): bit for bit.

Streams: the three of tests/test_gpu_odom_cov.py (seeds 100 .. 102, 80 features per frame), 30 frames, about 10 IMU samples per frame:
cap = 32 does not overflow, cap = 4 does (tests/test_imu_rate_ref.py confirms both on the CPU).

Largest difference to the reference measured on an MI355X: 1.2e-10 over 870 records, the same at both launch shapes."""
import os

import numpy as np
import pytest

import filter_harness as H
import imu_rate_harness as Ih
import imu_rate_ref as Ir
from filter_harness import same as _same
from imu_rate_harness import IR_CAP, N_FRAMES, same_ir as _same_ir

pytestmark = pytest.mark.gpu

CAP = Ih.CAP
BAR = 1e-6


def _against_ref(rec, n, s, ref, cap, where):
    """Stream s's records of one step against the reference's list; -> the largest difference."""
    from uav_airvision_amd.msckf_ops import unpack_imu_states
    had, wr, want = Ir.capped(ref, cap)
    assert n[s].tolist() == [had, wr], (where, n[s].tolist(), had, wr)
    got = unpack_imu_states(rec, n, s)
    worst = 0.0
    for g, r in zip(got, want):
        assert g['t'] == r['t'], (where, g['t'], r['t'])
        for f in ('p', 'q', 'v', 'w'):
            e = float(np.abs(g[f] - r[f]).max())
            assert e <= BAR, (where, f, e)
            worst = max(worst, e)
    return worst


_SYNC = {}


def _sync3(cfg, wg):
    """The three streams stepped synchronously with the records on and the reference alongside, checked on every step; once per launch
    shape, shared (the other tests compare with it bit for bit)."""
    if wg in _SYNC:
        return _SYNC[wg]
    run = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, oracle=Ir.ImuRateOracle, env={'AV_DK_WG': '64'} if wg == 64 else {})
    assert run['shape'] == [(3, wg)], run['shape']
    worst, total, most = 0.0, 0, 0
    for k in range(N_FRAMES):
        rec, n = run['irs'][k]
        assert rec.shape == (3, IR_CAP) and n.shape == (3, 2)
        for s in range(3):
            worst = max(worst, _against_ref(rec, n, s, run['refs'][k][s], IR_CAP, 'wg %d frame %d stream %d' % (wg, k, s)))
            total += int(n[s, 1]); most = max(most, int(n[s, 0]))
    assert run['counters']['prune_stream_steps'] > 0 and total > 500 and 4 < most <= IR_CAP, (run['counters'], total, most)
    print('wg %d: %d records checked, largest difference to the reference %.3e (bar %.0e), most samples in a frame %d' % (wg, total, worst, BAR, most))
    _SYNC[wg] = run
    return run


# ---- (i), (iii) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wg', [256, 64])
def test_records_match_the_reference_in_both_launch_shapes(cfg, wg):
    assert len(_sync3(cfg, wg)['irs']) == N_FRAMES


def test_both_launch_shapes_publish_the_same_bytes(cfg):
    a, b = _sync3(cfg, 256), _sync3(cfg, 64)
    for k in range(N_FRAMES):
        assert _same(a['outs'][k], b['outs'][k]) and _same_ir(a['irs'][k], b['irs'][k]), k


# ---- (ii) ----------------------------------------------------------------------------------------------------------------------------
def test_without_an_update_the_last_record_is_the_published_pose(cfg):
    """Stream 1 is fed blank feature messages: no update ever corrects it, so the last record of every step -- t, p, q, v, the record's
    first eleven doubles -- is bit for bit what the step publishes (out[1:12]).  Its neighbours, which do update, are those of the
    ordinary run."""
    sync = _sync3(cfg, 256)
    run = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, blank={1: range(N_FRAMES)})
    seen = 0
    for k in range(N_FRAMES):
        rec, n = run['irs'][k]
        if n[1, 1] > 0:
            assert run['outs'][k][1, 0] == 1.0, k
            last = rec[1, n[1, 1] - 1:n[1, 1]].view(np.float64).reshape(14)
            assert _same(last[:11], run['outs'][k][1, 1:12]), k
            seen += 1
        for s in (0, 2):
            assert _same(run['outs'][k][s], sync['outs'][k][s]) and _same_ir(run['irs'][k], sync['irs'][k], s, s), (k, s)
    assert seen >= 20, seen
    differs = sum(not _same(sync['irs'][k][0][0, sync['irs'][k][1][0, 1] - 1:sync['irs'][k][1][0, 1]].view(np.float64).reshape(14)[:11], sync['outs'][k][0, 1:12])
                  for k in range(N_FRAMES) if sync['irs'][k][1][0, 1] > 0)
    assert differs >= 10, differs                                # (a stream that updates: the correction shows between the two)


# ---- the cap -------------------------------------------------------------------------------------------------------------------------
def test_cap_4_keeps_the_last_four_of_every_step(cfg):
    sync = _sync3(cfg, 256)
    run = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, ir_cap=4)
    over = 0
    for k in range(N_FRAMES):
        (rec, n), (rec32, n32) = run['irs'][k], sync['irs'][k]
        assert rec.shape == (3, 4) and _same(run['outs'][k], sync['outs'][k]), k
        for s in range(3):
            had = int(n32[s, 0])
            assert n[s].tolist() == [had, min(had, 4)], (k, s)
            assert rec[s, :n[s, 1]].tobytes() == rec32[s, had - n[s, 1]:had].tobytes(), (k, s)
            over += had > 4
    assert over > 60, over


# ---- (iv) ----------------------------------------------------------------------------------------------------------------------------
def test_queued_steps_fill_their_own_arrays(cfg):
    sync = _sync3(cfg, 256)
    run = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, mode='queue3')
    assert len({id(p[0]) for p in run['irs']}) == N_FRAMES
    for k in range(N_FRAMES):
        assert _same(run['outs'][k], sync['outs'][k]) and _same_ir(run['irs'][k], sync['irs'][k]), k


def test_two_stream_groups_fill_their_parts(cfg):
    sync = _sync3(cfg, 64)
    for mode in ('ahead', 'step'):
        run = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, mode=mode, env={'AV_MSCKF_GROUPS': '2', 'AV_DK_WG': '64'})
        assert run['shape'] == [(2, 64), (1, 64)], run['shape']
        for k in range(N_FRAMES):
            assert _same(run['outs'][k], sync['outs'][k]) and _same_ir(run['irs'][k], sync['irs'][k]), (mode, k)


_HANDOVER = {}


def _handover(cfg):
    if not _HANDOVER:
        h = Ih.handover_run(cfg)
        assert sum(bool(o[0, 0] == 1.0) for o in h['outs']) >= 5 and sum(int(p[1][:, 1].sum()) for p in h['irs']) > 50
        _HANDOVER.update(h)
    return _HANDOVER


def test_device_handover_matches_a_step_run_of_the_same_messages(cfg):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    h = _handover(cfg)
    ref = BatchedMSCKF(cfg, 2, max_features=h['msgs'][0][0].shape[1], imu_rate=True, imu_rate_cap=IR_CAP)
    try:
        for k in range(len(h['msgs'])):
            H.push(ref, h['rows'][k])
            out = ref.step(*h['msgs'][k], imu_states=True)
            assert _same(out, h['outs'][k]) and _same_ir(ref.last_imu_states, h['irs'][k]), k
    finally:
        ref.close()


def test_filter_set_joins_the_parts_records(cfg):
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.pipelines import EngineSet, FilterSet
    h = _handover(cfg)
    eng = EngineSet(cfg, 2, 2)
    flt = None
    try:
        flt = FilterSet(cfg, eng, max_features=eng.max_features, imu_rate=True, imu_rate_cap=IR_CAP)
        with pytest.raises(ValueError):
            flt.submit_dev(eng, h['cams'][0][2], imu_states=(1, 2))
        outs, irs = [], []
        for k, (c0, c1, ts) in enumerate(h['cams']):
            i = np.array([i for i, _ in h['rows'][k]], np.int32)
            t = np.array([m.timestamp for _, m in h['rows'][k]])
            w = np.array([m.angular_velocity for _, m in h['rows'][k]]).reshape(-1, 3)
            a = np.array([m.linear_acceleration for _, m in h['rows'][k]]).reshape(-1, 3)
            eng.push_imu_batch(i, t, w)
            eng.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            flt.push_imu(i, t, w, a)
            outs.append(flt.submit_dev(eng, ts, msg_stream=N.current_stream(), imu_states=True))
            irs.append(flt.last_imu_states)
        flt.wait(0)
        for k in range(len(outs)):
            rec, n = irs[k][0].array(), irs[k][1].array()
            assert rec.shape == (2, IR_CAP) and n.shape == (2, 2)
            assert _same(outs[k].array(), h['outs'][k]) and _same_ir((rec, n), h['irs'][k]), k
    finally:
        if flt is not None:
            flt.close()
        eng.close()
    plain = FilterSet.__new__(FilterSet)
    plain.odom_cov, plain.landmarks, plain.stats, plain.imu_rate, plain.es = False, False, False, False, eng
    with pytest.raises(ValueError, match='imu_rate'):
        plain.submit_dev(eng, np.zeros(2), imu_states=True)


# ---- (v), refusals -------------------------------------------------------------------------------------------------------------------
def _live():
    import ctypes
    from uav_airvision_amd import _native as N
    out = (ctypes.c_int64 * 4)()
    N.check(N.lib().av_debug_live_resources(ctypes.byref(out)))
    return [int(v) for v in out]


def test_off_means_off(cfg, monkeypatch):
    """Off: the twelve doubles, get_state and get_cov of every step are bit-identical to the run with the records on and the launch shape
    is the same; not a byte of device or pinned memory more than the records' own buffers; imu_states= raises.  The switch is refused
    after the first step and with a cap outside 0 .. 4096; next without set is refused."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.msckf_ops import IMU_STATE_DTYPE, BatchedMSCKF
    on = _sync3(cfg, 256)
    seen = {}

    def check_off(k, bat, out, cur):
        if k == 3:
            seen['off'] = _live()
            with pytest.raises(ValueError, match='imu_states'):
                bat.step(np.zeros((3, CAP), np.int64), np.zeros((3, CAP, 4)), np.zeros(3, np.int32), np.full(3, -1.0), imu_states=True)
            with pytest.raises(AirvisionError, match='first step'):
                bat.set_imu_rate(32)
            assert bat.imu_rate_cap == 0 and bat.last_imu_states is None

    def check_on(k, bat, out, cur):
        if k == 3:
            seen['on'] = _live()
    base = _live()
    off = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, imu_rate=False, check=check_off)
    Ih.run(cfg, Ih.streams3(cfg), 4, check=check_on)
    assert _live() == base
    assert off['shape'] == on['shape'] and off['irs'] == [None] * N_FRAMES
    for k in range(N_FRAMES):
        assert _same(off['outs'][k], on['outs'][k]), k
        for s in range(3):
            assert all(_same(a, b) for a, b in zip(off['states'][k][s], on['states'][k][s])), (k, s)
    S, ring = 3, 3
    assert seen['on'][0] - seen['off'][0] == (S * IR_CAP * 112 + 256) + (S * 2 * 4 + 256), (seen, base)
    assert seen['on'][1] - seen['off'][1] == ring * ((S * IR_CAP * 112 + 64) + (S * 2 * 4 + 64)), (seen, base)
    assert seen['on'][2:] == seen['off'][2:]
    for name in ('AV_DK_WG', 'AV_MSCKF_GROUPS', 'AV_MSCKF_STORE'):
        monkeypatch.delenv(name, raising=False)
    bat = BatchedMSCKF(cfg, 1)
    try:
        rec, n = np.zeros((1, 32), IMU_STATE_DTYPE), np.zeros((1, 2), np.int32)
        assert N.lib().av_msckf_batch_next_imu_rate(bat._h, rec.ctypes.data, n.ctypes.data) == N.AV_E_INVALID
        assert b'av_msckf_batch_set_imu_rate' in N.lib().av_last_error()
        for cap in (-1, 4097):
            with pytest.raises(AirvisionError, match='bad arguments'):
                bat.set_imu_rate(cap)
        bat.set_imu_rate(4096); bat.set_imu_rate(0); bat.set_imu_rate(8)
        assert bat.imu_rate_cap == 8
    finally:
        bat.close()
    for cap in (0, 4097):
        with pytest.raises(ValueError, match='imu_rate_cap'):
            BatchedMSCKF(cfg, 1, imu_rate=True, imu_rate_cap=cap)
    assert _live() == base


# ---- (vi) ----------------------------------------------------------------------------------------------------------------------------
def test_all_four_outputs_together_equal_their_single_runs(cfg):
    ir_only = _sync3(cfg, 256)
    rest = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, imu_rate=False, others=('odom_cov', 'landmarks', 'stats'))
    for env in ({}, {'AV_DK_WG': '64'}):
        both = Ih.run(cfg, Ih.streams3(cfg), N_FRAMES, others=('odom_cov', 'landmarks', 'stats'), env=env)
        for k in range(N_FRAMES):
            assert _same(both['outs'][k], ir_only['outs'][k]) and _same_ir(both['irs'][k], ir_only['irs'][k]), k
            assert _same(both['covs'][k], rest['covs'][k]) and H.same_lm(both['lms'][k], rest['lms'][k]) and H.same_bytes(both['sts'][k], rest['sts'][k]), k


# ---- (vii) ---------------------------------------------------------------------------------------------------------------------------
def test_idle_and_stopped_streams_read_zero_and_leave_their_neighbour_alone(cfg):
    """Stream 0 is stopped by a capacity limit (the overflow pool shrunk to 64 rows, a blank frame at 17), stream 2 has no frame in three
    steps.  Stream 0's records of step 17 are there -- the prediction ran before the update met the limit -- and from step 18 on it reads
    (0, 0); stream 2 reads (0, 0) where it has no frame and integrates the samples it missed with its next one; stream 1's records are those
    of stream 1 run alone."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    n = 24
    mk = lambda: [SyntheticFeatureStream(cfg, seed=91, n_frames=n, n_features=150), SyntheticFeatureStream(cfg, seed=92, n_frames=n, n_features=40),
                  SyntheticFeatureStream(cfg, seed=100, n_frames=n, n_features=50)]
    env = {'AV_MSCKF_POOL_ROWS': '64'}
    idle = (5, 6, 20)
    both = Ih.run(cfg, mk(), n, cap=192, ir_cap=64, blank={0: (17,)}, idle={2: idle}, env=env, rows_cap=2048)
    solo = Ih.run(cfg, mk()[1:2], n, cap=192, ir_cap=64, env=env, rows_cap=2048)
    assert [k for k in range(n) if both['outs'][k][0, 0] < 0] == list(range(17, n))
    had = np.zeros(3, np.int64)
    for k in range(n):
        rec, cnt = both['irs'][k]
        if k == 17:
            assert cnt[0, 0] > 0, cnt[0]
        if k >= 18:
            assert cnt[0].tolist() == [0, 0], k
        if k in idle:
            assert both['outs'][k][2, 0] == 0.0 and cnt[2].tolist() == [0, 0], k
        had += cnt[:, 0]
        assert _same(both['outs'][k][1:2], solo['outs'][k]), k
        assert _same_ir((rec[1:2], cnt[1:2]), solo['irs'][k]), k
    assert both['irs'][7][1][2, 0] > both['irs'][8][1][2, 0] > 0 and (had > 100).all(), had      # (frame 7 catches up on frames 5 and 6)


# ---- (viii) --------------------------------------------------------------------------------------------------------------------------
def test_restart_clears_the_rows_and_the_new_life_is_a_fresh_stream(cfg):
    """Stream 1 is restarted ahead of step 14 and fed its own stream again from the first sample and frame.  Its counts read (0, 0) until
    the new life is live, every step of the new life has the bytes of the same step of a fresh batch (the ordinary run's stream 1, 14
    steps earlier), and streams 0 and 2 are the ordinary run's throughout."""
    sync = _sync3(cfg, 256)
    k0 = 14
    streams = Ih.streams3(cfg)
    rows, msgs = H.schedule(streams, N_FRAMES), H.messages(streams, N_FRAMES)
    life2 = H.schedule(Ih.streams3(cfg)[1:2], N_FRAMES - k0)
    for k in range(k0, N_FRAMES):
        rows[k] = [(i, m) for i, m in rows[k] if i != 1] + [(1, m) for _, m in life2[k - k0]]
        msgs[k] = [msgs[k][0], streams[1].frame(k - k0), msgs[k][2]]
    run = Ih.run(cfg, streams, N_FRAMES, restart={k0: [1]}, rows=rows, msgs=msgs)
    quiet = 0
    for k in range(N_FRAMES):
        for s in (0, 2):
            assert _same(run['outs'][k][s], sync['outs'][k][s]) and _same_ir(run['irs'][k], sync['irs'][k], s, s), (k, s)
        j = k if k < k0 else k - k0
        assert _same(run['outs'][k][1], sync['outs'][j][1]) and _same_ir(run['irs'][k], sync['irs'][j], 1, 1), (k, j)
        if k >= k0 and run['outs'][k][1, 0] == 0.0:
            assert run['irs'][k][1][1].tolist() == [0, 0], k
            quiet += 1
    assert run['irs'][k0 - 1][1][1, 0] > 0 and sum(int(run['irs'][k][1][1, 1]) for k in range(k0, N_FRAMES)) > 50
    assert quiet == sum(sync['outs'][j][1, 0] == 0.0 for j in range(N_FRAMES - k0))


# ---- (ix), (x) -----------------------------------------------------------------------------------------------------------------------
def _dropin():
    import sys
    from conftest import ROOT
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import msckf as dmsckf
    return dmsckf


def test_dropin_last_imu_states_are_stream_0s_records(cfg):
    """The drop-in MSCKF with config.publish_imu_rate: last_imu_states after every feature_callback holds stream 0's written records of
    the three-stream run, bit for bit (T_imu_body = identity); with a T_imu_body that rotates and shifts, p, q, v are mapped the way
    publish maps the pose and the velocity, and t and w keep their bits.  vio_result is what it was."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import unpack_imu_states
    from uav_airvision_amd.synth import replay_features
    dmsckf = _dropin()
    from utils import Isometry3d, to_rotation
    sync = _sync3(cfg, 256)
    c = ConfigEuRoC()
    assert c.publish_imu_rate is False
    off = dmsckf.MSCKF(c, write_trajectory=False)
    assert off.last_imu_states is None
    off.close()
    ang = 0.3
    T = np.identity(4)
    T[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.1, -0.2, 0.05]
    for body in (None, T):
        c = ConfigEuRoC()
        c.publish_imu_rate, c.imu_rate_cap = True, IR_CAP
        if body is not None:
            c.T_imu_body = body
        flt = dmsckf.MSCKF(c, write_trajectory=False)
        got = []

        def on(m):
            r = flt.feature_callback(m)
            assert r is None or r._fields == ('timestamp', 'pose', 'velocity', 'cam0_pose')
            got.append((flt.last_imu_states.copy(), flt.last_imu_states_dropped, r))
        try:
            replay_features(Ih.streams3(cfg)[0], [flt.imu_callback], on)
        finally:
            flt.close()
        assert len(got) == N_FRAMES and sum(len(g[0]) for g in got) > 150
        for k, (g, dropped, r) in enumerate(got):
            want = unpack_imu_states(*sync['irs'][k], 0)
            assert dropped == 0 and len(g) == len(want), k
            if body is None:
                assert g.tobytes() == want.tobytes(), k
                continue
            assert g['t'].tobytes() == want['t'].tobytes() and g['w'].tobytes() == want['w'].tobytes(), k
            B = Isometry3d(T[:3, :3], T[:3, 3])
            for a, b in zip(g, want):
                P = B * Isometry3d(to_rotation(b['q']).T, b['p']) * B.inverse()
                assert np.abs(a['p'] - P.t).max() <= 1e-12 and np.abs(to_rotation(a['q']).T - P.R).max() <= 1e-12 and np.abs(a['v'] - T[:3, :3] @ b['v']).max() <= 1e-12, k


def test_sweep_writes_the_imu_file(tmp_path, monkeypatch, capsys):
    """sweep --imu-rate on a short EuRoC-layout sequence: next to the trajectory file an _imu file, one line `t p q v w` per record and,
    behind the records of every step, the step's published pose as one more line; the report states the records and those dropped to
    the cap, and --imu-rate-cap 4 drops some."""
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
        kept.append(kw['ir_rows'])
        return inner(*a, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    reps = {}
    for cap in (32, 4):
        out = tmp_path / ('txts%d' % cap)
        sweep.main(['--root', str(tmp_path), '--sequences', 'SEQ', '--imu-rate', '--imu-rate-cap', str(cap), '--out', str(out)])
        rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
        traj = np.loadtxt(str(out / 'output_SEQ_offset0.txt')).reshape(-1, 8)
        lines = np.loadtxt(str(out / 'output_SEQ_offset0_imu.txt')).reshape(-1, 14)
        ((rows, n_rec, dropped),), = kept[-1:]
        assert len(traj) > 20 and len(lines) == len(rows) == n_rec + len(traj), (cap, len(lines), n_rec, len(traj))
        assert np.abs(lines[:, 0] - rows[:, 0]).max() < 1e-6 and np.nanmax(np.abs(lines[:, 1:] - rows[:, 1:])) <= 1e-9
        assert (np.diff(rows[:, 0]) >= 0).all()
        assert rep['imu_rate'] == dict(cap=cap, records=[n_rec], dropped_to_cap=[dropped], lines=[len(rows)])
        reps[cap] = (rep, rows, traj)
    assert reps[32][0]['imu_rate']['dropped_to_cap'] == [0] and reps[4][0]['imu_rate']['dropped_to_cap'][0] > 0
    assert reps[32][0]['imu_rate']['records'][0] == reps[4][0]['imu_rate']['records'][0] + reps[4][0]['imu_rate']['dropped_to_cap'][0]
    assert np.array_equal(reps[32][2], reps[4][2])
