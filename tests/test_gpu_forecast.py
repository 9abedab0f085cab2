"""The forecast of the batched filter (include/airvision.h, "Forecast"; BatchedMSCKF(forecast=True)): per stream and step a count pair,
the state after every pending IMU sample (the samples pushed beyond the frame's time, the first `cap`), and the odometry covariance
at the last of them, riding the step's read-back.

What is compared with what:
 * against tests/forecast_ref.py (the oracle carried through its own pending messages): counts and t exactly; p, q, v, w within 1e-6,
   the covariance within 1e-6 max|C| -- the project's bars for the filter's state and for the odometry covariance against the oracle;
 * the chain: the records of step k against the leading IMU-rate records of step k + 1, two GPU evaluations of the same function from
   the same state, each within the operator bar of the reference: twice the `samples` family's bar;
 * with nothing pending, against the step's own odometry-covariance record and against the map of the state the step leaves (a reset
   step: of the re-initialised block), 64 EPS odom_cov_bound;
 * two runs of the library against each other (the forecast off, launch shapes, queue, stream groups, caller-owned arrays, hand-over, a
   stopped neighbour, a restart): bit for bit.

Streams: the three of tests/test_gpu_odom_cov.py, 30 frames, 80 features, the IMU pushed one frame ahead (tests/forecast_harness.py).

Measured on an MI355X: 870 records, largest difference to the oracle 1.2e-10, covariance 8.9e-10 of max|C|; the chain's 870 record pairs
are bit-equal."""
import numpy as np
import pytest

import filter_harness as H
import forecast_harness as Fh
import forecast_ref as Fr
import imu_rate_harness as Ih
import msckf_predict_cases as Pc
import odom_cov_ref as R
from filter_harness import same as _same
from forecast_harness import FC_CAP, N_FRAMES, same_fc as _same_fc

pytestmark = pytest.mark.gpu

CAP = Fh.CAP
BAR = 1e-6
EPS = Pc.EPS
OTHERS = ('odom_cov', 'landmarks', 'stats', 'imu_rate')


def _against_ref(fc, s, ref, where):
    """Stream s's forecast of one step against the oracle's; -> (largest state difference, largest covariance difference / max|C|)."""
    from uav_airvision_amd.msckf_ops import unpack_forecast
    rec, n, cov = fc
    want, (had, wr), C = ref
    assert n[s].tolist() == [had, wr], (where, n[s].tolist(), had, wr)
    got, C15, reached = unpack_forecast(rec, n, cov, s)
    worst = 0.0
    for g, r in zip(got, want):
        assert g['t'] == r['t'], (where, g['t'], r['t'])
        for f in ('p', 'q', 'v', 'w'):
            e = float(np.abs(g[f] - r[f]).max())
            assert e <= BAR, (where, f, e)
            worst = max(worst, e)
    assert reached == (want[-1]['t'] if want else None)
    if np.isnan(C).all():
        assert np.isnan(C15).all(), where
        return worst, 0.0
    ec = float(np.abs(C15 - C).max() / np.abs(C).max())
    assert ec <= BAR, (where, ec)
    return worst, ec


_RUN = {}


def _sync(cfg):
    """The three streams stepped synchronously, the IMU one frame ahead, every output on and the oracle alongside, checked on every step;
    once, shared (the other tests compare with it bit for bit)."""
    if 'sync' not in _RUN:
        run = Fh.run(cfg, Fh.streams3(cfg), N_FRAMES, oracle=Fr.ForecastOracle, others=OTHERS)
        assert run['shape'] == [(3, 256)], run['shape']
        worst, worst_c, total, most = 0.0, 0.0, 0, 0
        for k in range(N_FRAMES):
            rec, n, cov = run['fcs'][k]
            assert rec.shape == (3, FC_CAP) and n.shape == (3, 2) and cov.shape == (3, 120)
            for s in range(3):
                e, ec = _against_ref(run['fcs'][k], s, run['refs'][k][s], 'frame %d stream %d' % (k, s))
                worst, worst_c = max(worst, e), max(worst_c, ec)
                total += int(n[s, 1]); most = max(most, int(n[s, 0]))
        assert run['counters']['prune_stream_steps'] > 0 and total > 500 and 4 < most <= FC_CAP, (run['counters'], total, most)
        print('FORECAST e2e: %d records, largest difference to the oracle %.3e, covariance %.3e of max|C| (bars %.0e), most pending %d' % (total, worst, worst_c, BAR, most))
        _RUN['sync'] = run
    return _RUN['sync']


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_step_matches_the_oracle(cfg):
    run = _sync(cfg)
    assert len(run['fcs']) == N_FRAMES
    assert all(run['fcs'][N_FRAMES - 1][1][s].tolist() == [0, 0] for s in range(3))          # nothing is pushed beyond the last frame
    assert np.isfinite(run['fcs'][N_FRAMES - 1][2]).all()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_chain_forecast_records_are_the_next_steps_imu_rate_records(cfg):
    """Both are GPU evaluations of predict_new_state from the state step k leaves over the same samples, each within FACTOR e_fam of the
    50-digit reference: they agree within twice that, the `samples` family's bar."""
    from uav_airvision_amd.msckf_ops import unpack_forecast, unpack_imu_states
    run, bars = _sync(cfg), Pc.bars('samples', cfg)
    pairs, equal, worst = 0, 0, dict(q=0.0, p=0.0, v=0.0)
    for k in range(N_FRAMES - 1):
        for s in range(3):
            a = unpack_forecast(*run['fcs'][k], s)[0]
            if not len(a):
                continue
            b = unpack_imu_states(*run['irs'][k + 1], s)[:len(a)]
            assert len(b) == len(a) and a['t'].tobytes() == b['t'].tobytes() and a['w'].tobytes() == b['w'].tobytes(), (k, s)
            for x, y in zip(a, b):
                pairs += 1
                equal += x.tobytes() == y.tobytes()
                for f in worst:
                    y_ = y[f] if (f != 'q' or np.dot(x[f], y[f]) >= 0) else -y[f]
                    e = float(np.linalg.norm(x[f] - y_) / np.linalg.norm(y_))
                    worst[f] = max(worst[f], e)
                    assert e <= 2 * Pc.FACTOR * bars[f], (k, s, f, e)
    print('FORECAST chain: %d record pairs, %d bit-equal, worst relative difference q %.2e p %.2e v %.2e' % (pairs, equal, worst['q'], worst['p'], worst['v']))
    assert pairs > 500


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_read_only_every_other_output_and_the_state_are_those_of_the_run_without(cfg):
    on = _sync(cfg)
    off = Fh.run(cfg, Fh.streams3(cfg), N_FRAMES, forecast=False, others=OTHERS)
    assert off['shape'] == on['shape'] and off['fcs'] == [None] * N_FRAMES
    for k in range(N_FRAMES):
        assert _same(off['outs'][k], on['outs'][k]) and _same(off['covs'][k], on['covs'][k]), k
        assert H.same_lm(off['lms'][k], on['lms'][k]) and H.same_bytes(off['sts'][k], on['sts'][k]) and Ih.same_ir(off['irs'][k], on['irs'][k]), k
        for s in range(3):
            assert all(_same(a, b) for a, b in zip(off['states'][k][s], on['states'][k][s])), (k, s)
    for s in range(3):
        assert all(_same(a, b) for a, b in zip(off['final'][s], on['final'][s])), s


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_nothing_pending_is_the_steps_covariance_and_on_a_reset_the_new_blocks(cfg):
    """lead = 0: no step has pending samples.  Without a reset the record is the step's odometry-covariance record; always it is the map
    of the state and block the step leaves -- on a reset step (position_std_threshold = 0.012, seeds 31 / 32, as tests/test_gpu_odom_cov.py
    provokes them: most steps of that run reset) of the re-initialised block, which the step's odometry-covariance record is not.  The
    three ordinary streams, which never reset, give the steps without one."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import unpack_odom_cov
    from uav_airvision_amd.synth import SyntheticFeatureStream
    low = ConfigEuRoC()
    low.position_std_threshold = 0.012
    streams = [SyntheticFeatureStream(low, seed=31, n_frames=60, n_features=80), SyntheticFeatureStream(low, seed=32, n_frames=60, n_features=80)]
    seen = dict(resets=0, plain=0, idle=0)

    def check(k, bat, out, cur):
        rec, n, cov = cur['fc']
        for i in range(len(out)):
            if out[i, 0] != 1.0:
                assert n[i].tolist() == [0, 0] and np.isnan(cov[i]).all(), (k, i)
                seen['idle'] += 1
                continue
            assert n[i].tolist() == [0, 0], (k, i)
            C, Cs = unpack_odom_cov(cov[i]), unpack_odom_cov(cur['cov'][i])
            P, gs = bat.get_cov(i), bat.get_state(i)
            left = R.odom_cov(P, gs['q'], gs['R_ic'], gs['t_ci'])
            bnd = 64 * EPS * R.odom_cov_bound(P, gs['q'], gs['R_ic'], gs['t_ci'])
            assert (np.abs(C - left) <= bnd).all(), (k, i)
            if P.shape == (21, 21):                              # a step that publishes adds a camera state: none left = online_reset ran
                seen['resets'] += 1
                assert not np.any(C[:3, :3]) and np.abs(Cs[:3, :3]).max() >= 0.012 ** 2 * 0.99, (k, i)
            else:
                seen['plain'] += 1
                assert (np.abs(C - Cs) <= bnd).all(), (k, i)
    Fh.run(low, streams, 60, lead=0, cap=512, withhold={1: 8}, others=('odom_cov',), check=check)
    assert seen['resets'] >= 1 and seen['idle'] >= 5, seen
    resets = seen['resets']
    Fh.run(cfg, Fh.streams3(cfg), N_FRAMES, lead=0, others=('odom_cov',), check=check)
    assert seen['resets'] == resets and seen['plain'] >= 80, seen


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode, env, own', [('queue3', {}, False), ('ahead', {}, False), ('step', {'AV_DK_WG': '64'}, False),
                                            ('step', {'AV_MSCKF_GROUPS': '2'}, False), ('step', {}, True)])
def test_the_same_bytes_in_every_mode(cfg, mode, env, own):
    sync = _sync(cfg)
    run = Fh.run(cfg, Fh.streams3(cfg), N_FRAMES, mode=mode, env=env, own=own)
    if env.get('AV_DK_WG'):
        assert run['shape'] == [(3, 64)]
    if env.get('AV_MSCKF_GROUPS'):
        assert [g[0] for g in run['shape']] == [2, 1], run['shape']
    assert len({id(p[0]) for p in run['fcs']}) == N_FRAMES
    for k in range(N_FRAMES):
        assert _same(run['outs'][k], sync['outs'][k]) and _same_fc(run['fcs'][k], sync['fcs'][k]), (mode, env, k)
        if own:                                                   # the caller's arrays took the step's: counts and covariance rows are all rewritten
            rec, n, cov = run['fcs'][k]                           # (the whole record buffer is copied: rows past `written` are unspecified)
            assert not (cov == 7.0).any() and (n >= 0).all(), k


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_blank_idle_and_withheld_streams(cfg):
    """Stream 0 gets blank frames in 10 .. 12 (it still publishes: a forecast), stream 1 has no frame in 5, 6 and 20 ({0, 0}, NaN), stream 2's
    IMU is withheld until frame 8 (no gravity before: {0, 0}, NaN).  The oracle, fed the same, agrees on every step."""
    idle, hold = (5, 6, 20), 8
    run = Fh.run(cfg, Fh.streams3(cfg), N_FRAMES, blank={0: (10, 11, 12)}, idle={1: idle}, withhold={2: hold}, oracle=Fr.ForecastOracle)
    quiet = 0
    for k in range(N_FRAMES):
        rec, n, cov = run['fcs'][k]
        for s in range(3):
            _against_ref(run['fcs'][k], s, run['refs'][k][s], (k, s))
        if k in idle:
            assert run['outs'][k][1, 0] == 0.0 and n[1].tolist() == [0, 0] and np.isnan(cov[1]).all(), k
        if run['outs'][k][2, 0] == 0.0:
            assert n[2].tolist() == [0, 0] and np.isnan(cov[2]).all(), k
            quiet += 1
        if k in (10, 11, 12):
            assert run['outs'][k][0, 0] == 1.0 and n[0, 1] > 0 and np.isfinite(cov[0]).all(), k
    assert quiet >= hold - 1 and run['fcs'][N_FRAMES - 2][1][2, 1] > 0, quiet
    assert run['fcs'][7][1][1, 0] > 0                              # (the idle stream's pending samples are still there for its next frame)


def test_a_stream_stopped_by_a_capacity_limit_reads_zero_from_the_stopping_step_on(cfg):
    """Stream 0 is stopped by a capacity limit (the overflow pool shrunk to 64 rows, a blank frame at 17): {0, 0} and NaN in the stopping
    step and afterwards; stream 1's forecast is that of stream 1 run alone."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    n = 22
    mk = lambda: [SyntheticFeatureStream(cfg, seed=91, n_frames=n, n_features=150), SyntheticFeatureStream(cfg, seed=92, n_frames=n, n_features=40)]
    env = {'AV_MSCKF_POOL_ROWS': '64'}
    both = Fh.run(cfg, mk(), n, cap=192, blank={0: (17,)}, env=env, rows_cap=2048)
    solo = Fh.run(cfg, mk()[1:2], n, cap=192, env=env, rows_cap=2048)
    assert [k for k in range(n) if both['outs'][k][0, 0] < 0] == list(range(17, n))
    for k in range(n):
        rec, cnt, cov = both['fcs'][k]
        if k >= 17:
            assert cnt[0].tolist() == [0, 0] and np.isnan(cov[0]).all(), k
        elif both['outs'][k][0, 0] == 1.0:
            assert cnt[0, 1] > 0 and np.isfinite(cov[0]).all(), k
        assert _same(both['outs'][k][1:2], solo['outs'][k]) and _same_fc(both['fcs'][k], solo['fcs'][k], 1, 0), k
    assert both['fcs'][16][1][0, 1] > 0


def test_restart_clears_the_rows_and_leaves_the_neighbours_alone(cfg):
    """Stream 1 is restarted ahead of step 14 and fed its own stream again from the first sample and frame (its pending samples of the old
    life go with the restart).  Its rows read {0, 0} and NaN until the new life is live, every step of the new life has the bytes of the
    same step of a fresh stream, and streams 0 and 2 are the ordinary run's throughout."""
    sync = _sync(cfg)
    k0 = 14
    streams = Fh.streams3(cfg)
    ahead = Fh.lead_rows(H.schedule(streams, N_FRAMES), 1)
    life2 = Fh.lead_rows(H.schedule(Fh.streams3(cfg)[1:2], N_FRAMES), 1)
    msgs = H.messages(streams, N_FRAMES)
    for k in range(k0, N_FRAMES):
        ahead[k] = [(i, m) for i, m in ahead[k] if i != 1] + [(1, m) for _, m in life2[k - k0]]
        msgs[k] = [msgs[k][0], streams[1].frame(k - k0), msgs[k][2]]
    # rows are handed over as they are pushed: lead = 0 on rows that already run ahead
    run = Fh.run(cfg, streams, N_FRAMES, lead=0, restart={k0: [1]}, rows=ahead, msgs=msgs)
    quiet = 0
    for k in range(N_FRAMES):
        for s in (0, 2):
            assert _same(run['outs'][k][s], sync['outs'][k][s]) and _same_fc(run['fcs'][k], sync['fcs'][k], s, s), (k, s)
        j = k if k < k0 else k - k0
        if k != k0 - 1:                                            # (step 13's forecast ran through the old life's frame-14 samples: the ordinary run's)
            assert _same(run['outs'][k][1], sync['outs'][j][1]) and _same_fc(run['fcs'][k], sync['fcs'][j], 1, 1), (k, j)
        if k >= k0 and run['outs'][k][1, 0] == 0.0:
            assert run['fcs'][k][1][1].tolist() == [0, 0] and np.isnan(run['fcs'][k][2][1]).all(), k
            quiet += 1
    assert _same_fc(run['fcs'][k0 - 1], sync['fcs'][k0 - 1], 1, 1)
    assert quiet == sum(sync['outs'][j][1, 0] == 0.0 for j in range(N_FRAMES - k0))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_switch_and_destination_are_refused_where_the_contract_says(cfg, monkeypatch):
    from uav_airvision_amd import _native as N
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.msckf_ops import IMU_STATE_DTYPE, BatchedMSCKF
    for name in H.ENV_KEYS:
        monkeypatch.delenv(name, raising=False)
    bat = BatchedMSCKF(cfg, 3)
    try:
        z = (np.zeros((3, CAP), np.int64), np.zeros((3, CAP, 4)), np.zeros(3, np.int32), np.full(3, -1.0))
        with pytest.raises(ValueError, match='forecast'):
            bat.step(*z, forecast=True)
        rec, n, cov = np.zeros((3, 32), IMU_STATE_DTYPE), np.zeros((3, 2), np.int32), np.zeros((3, 120))
        assert N.lib().av_msckf_batch_next_forecast(bat._h, rec.ctypes.data, n.ctypes.data, cov.ctypes.data) == N.AV_E_INVALID
        assert b'av_msckf_batch_set_forecast' in N.lib().av_last_error()
        for cap in (-1, 4097):
            with pytest.raises(AirvisionError, match='bad arguments'):
                bat.set_forecast(cap)
        bat.set_forecast(4096); bat.set_forecast(0); bat.set_forecast(8)
        assert bat.forecast_cap == 8
        with pytest.raises(ValueError, match='triple'):
            bat.step(*z, forecast=(rec, n, cov))                   # 32 records per stream, the cap is 8
        bat.step(*z, forecast=True)
        assert bat.last_forecast[0].shape == (3, 8) and (bat.last_forecast[1] == 0).all() and np.isnan(bat.last_forecast[2]).all()
        with pytest.raises(AirvisionError, match='first step'):
            bat.set_forecast(16)
    finally:
        bat.close()
    for cap in (0, 4097):
        with pytest.raises(ValueError, match='forecast_cap'):
            BatchedMSCKF(cfg, 1, forecast=True, forecast_cap=cap)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_device_handover_matches_a_step_run_of_the_same_messages(cfg):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    h = Fh.handover_run(cfg)
    assert sum(bool(o[0, 0] == 1.0) for o in h['outs']) >= 5 and sum(int(p[1][:, 1].sum()) for p in h['fcs']) > 50
    ref = BatchedMSCKF(cfg, 2, max_features=h['msgs'][0][0].shape[1], forecast=True, forecast_cap=FC_CAP)
    try:
        for k in range(len(h['msgs'])):
            H.push(ref, h['ahead'][k])
            out = ref.step(*h['msgs'][k], forecast=True)
            assert _same(out, h['outs'][k]) and _same_fc(ref.last_forecast, h['fcs'][k]), k
    finally:
        ref.close()
