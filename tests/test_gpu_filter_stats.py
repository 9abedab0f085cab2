"""The innovation statistics of the batched filter (include/airvision.h, "Innovation statistics"; BatchedMSCKF(stats=True)): per stream
and step two blocks of 64 bytes -- the lost-feature update's and the pruning update's gate counts, dof and gamma sums, rows and the
size of the correction -- riding the step's read-back.

What is compared with what:
 * against tests/filter_stats_ref.py (the NumPy oracle restated with the record written down), in both launch shapes: every integer
   field exactly; gamma_eval and gamma_pass within 1e-6 relative (+ 1e-12), the per-call gamma bar of tests/test_gpu_msckf.py
   (compare_calls, tol_gamma); dx_pos and dx_rot within that file's per-call delta_x bar taken over as it is,
   1e-6 * max(largest |component| of the reference's delta_x, 1e-3);
 * against the library's own debug_capture / debug_read of a second, synchronous run: gamma_eval against math.fsum of the captured
   per-feature values within n * 2^-52 * sum -- n non-negative terms added in ANY order by n - 1 roundings of at most 2^-53 relative
   to a partial sum that never exceeds the total stay within (n - 1) * 2^-53 * sum of the exact sum; fsum's own rounding is another
   2^-53 * sum.  The bar is derived, not measured;
 * two runs of the library against each other (launch shapes, queue, stream groups, hand-over, the other two outputs beside it,
   feature off): bit for bit.

Streams: those of tests/test_gpu_landmarks.py -- seeds 7 (3 % outliers), 100 and 101, 50 features per frame, 40 frames -- whose gates
tests/test_filter_stats_ref.py shows to decide with a margin of 2.9 % at worst; and filter_stats_ref.cut_stream, whose blank seventh
frame loses 150 features of 21 rows each, so that the 1,500-row cut falls into the second trip of 64 candidates; and one stream with
check_motion switched on, so that candidates stay without a position (n_pos < n_cand).

Largest deviations from the reference measured on an MI355X: profiles/filter_stats/README.md."""
import math
import os

import numpy as np
import pytest

import filter_harness as H
import filter_stats_ref as R
from filter_harness import messages as _messages, push as _push, same as _same, same_bytes as _same_st, same_lm as _same_lm, schedule as _schedule, zero as _zero

pytestmark = pytest.mark.gpu

N_FRAMES = R.N_FRAMES
CAP = 128
LM_CAP = 64


def _reference(cfg, streams, n_frames, blank=None):
    """A StatsOracle per stream over the same messages and IMU schedule: recs[k] = STATS_DTYPE[S, 2], dx_inf[k][s] = the largest
    |component| of the delta_x each of the step's two updates applied, gammas[k][s] = the values its two gates evaluated."""
    rows, msgs = _schedule(streams, n_frames), _messages(streams, n_frames, blank)
    oras = [R.StatsOracle(cfg) for _ in streams]
    recs, dx_inf, gammas = [], [], []
    for k in range(n_frames):
        for i, m in rows[k]:
            oras[i].imu_callback(m)
        for i, m in enumerate(msgs[k]):
            oras[i].feature_callback(m)
        recs.append(np.array([o.stats for o in oras])); dx_inf.append([list(o.dx_inf) for o in oras]); gammas.append([[list(g) for g in o.gammas] for o in oras])
    return dict(recs=recs, dx_inf=dx_inf, gammas=gammas)


def _run(cfg, streams, n_frames, stats=True, check=None, **kw):
    """filter_harness.run with the statistics on; check(k, bat, out) runs after every step."""
    return H.run(cfg, streams, n_frames, stats=stats, check=check and (lambda k, bat, out, cur: check(k, bat, out)), **kw)


def _against_ref(got, ref, dx_inf, where, worst):
    """One stream's [2] record of one step against the reference's; worst collects the largest deviation / bar per field."""
    for b in range(2):
        for n in R.INTS:
            assert int(got[b][n]) == int(ref[b][n]), (where, b, n, got[b], ref[b])
        for n in ('gamma_eval', 'gamma_pass'):
            err, bar = abs(float(got[b][n]) - float(ref[b][n])), 1e-12 + 1e-6 * abs(float(ref[b][n]))
            worst[n] = max(worst[n], err / bar)
            assert err <= bar, (where, b, n, float(got[b][n]), float(ref[b][n]))
        for n in ('dx_pos', 'dx_rot'):
            err, bar = abs(float(got[b][n]) - float(ref[b][n])), 1e-6 * max(dx_inf[b], 1e-3)
            worst[n] = max(worst[n], err / bar)
            assert err <= bar, (where, b, n, float(got[b][n]), float(ref[b][n]), dx_inf[b])


_CACHE = {}


def _ref3(cfg):
    if 'ref3' not in _CACHE:
        _CACHE['ref3'] = _reference(cfg, R.streams3(cfg), N_FRAMES)
    return _CACHE['ref3']


def _sync3(cfg, wg):
    """The three streams stepped synchronously with the statistics on, checked against the reference on every step; computed once per
    launch shape and shared (the other tests compare their records with it bit for bit)."""
    if ('sync', wg) in _CACHE:
        return _CACHE['sync', wg]
    ref = _ref3(cfg)
    run = _run(cfg, R.streams3(cfg), N_FRAMES, env={'AV_DK_WG': '64'} if wg == 64 else {})
    assert run['shape'] == [(3, wg)], run['shape']
    worst = dict(gamma_eval=0.0, gamma_pass=0.0, dx_pos=0.0, dx_rot=0.0)
    for k in range(N_FRAMES):
        assert run['sts'][k].shape == (3, 2)
        for s in range(3):
            _against_ref(run['sts'][k][s], ref['recs'][k][s], ref['dx_inf'][k][s], 'wg %d frame %d stream %d' % (wg, k, s), worst)
    allr = np.array(run['sts'])
    assert run['counters']['prune_stream_steps'] >= 9, run['counters']
    assert allr['n_eval'][:, :, 0].sum() > 200 and allr['n_eval'][:, :, 1].sum() > 1000 and (allr['n_pass'] < allr['n_eval']).any()
    assert (allr['flags'][:, :, 1] & R.FS_RAN).sum() >= 27 and not np.isnan(allr['gamma_eval']).any()
    print('wg %d: %d blocks with candidates checked; largest deviation / bar: %s'
          % (wg, int((allr['n_cand'] > 0).sum()), ', '.join('%s %.3e' % kv for kv in sorted(worst.items()))))
    _CACHE['sync', wg] = run
    return run


def _cut(cfg, wg):
    if ('cut', wg) not in _CACHE:
        _CACHE['cut', wg] = _run(cfg, [R.cut_stream(cfg)], R.CUT_FRAMES, cap=192, blank={0: (R.CUT_FRAMES - 1,)}, env={'AV_DK_WG': '64'} if wg == 64 else {})
    return _CACHE['cut', wg]


# ---- parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wg', [256, 64])
def test_records_match_the_reference_in_both_launch_shapes(cfg, wg):
    run = _sync3(cfg, wg)
    assert len(run['sts']) == N_FRAMES


def test_both_launch_shapes_publish_the_same_bytes(cfg):
    a, b = _sync3(cfg, 256), _sync3(cfg, 64)
    for k in range(N_FRAMES):
        assert _same(a['outs'][k], b['outs'][k]) and _same_st(a['sts'][k], b['sts'][k]), k
    assert all(_same_st(x, y) for x, y in zip(_cut(cfg, 256)['sts'], _cut(cfg, 64)['sts']))


@pytest.mark.parametrize('wg', [256, 64])
def test_row_cut_on_a_frame_that_loses_every_track(cfg, wg):
    """150 features of 21 rows lost at once: 72 evaluated (the 72nd takes the sum over 1,500, in the second trip of 64 candidates), 78
    behind the cut in the second and third trip: AV_FS_CUT, n_eval < n_pos, everything as the reference has it."""
    if 'refcut' not in _CACHE:
        _CACHE['refcut'] = _reference(cfg, [R.cut_stream(cfg)], R.CUT_FRAMES, blank={0: (R.CUT_FRAMES - 1,)})
    ref, run = _CACHE['refcut'], _cut(cfg, wg)
    assert run['shape'] == [(1, wg)]
    worst = dict(gamma_eval=0.0, gamma_pass=0.0, dx_pos=0.0, dx_rot=0.0)
    for k in range(R.CUT_FRAMES):
        _against_ref(run['sts'][k][0], ref['recs'][k][0], ref['dx_inf'][k][0], 'cut wg %d frame %d' % (wg, k), worst)
        assert k == R.CUT_FRAMES - 1 or _zero(run['sts'][k])
    last = run['sts'][-1][0, 0]
    assert [int(last[n]) for n in R.INTS] == [150, 150, 72, 72, 360, 360, 1512, R.FS_RAN | R.FS_CUT], last
    assert last['n_eval'] < last['n_pos'] and _zero(run['sts'][-1][0, 1])
    print('cut, wg %d: largest deviation / bar: %s' % (wg, ', '.join('%s %.3e' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('wg', [256, 64])
def test_candidates_without_a_position_are_counted_and_not_evaluated(wg):
    """translation_threshold = 0.04 (check_motion on; the stream and the threshold of tests/test_gpu_msckf.py's check_motion test, whose
    every frame follows the oracle): most candidates of both updates are held back without a position, so n_pos < n_cand, in steps
    where others are evaluated; every field as the reference has it."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticFeatureStream
    c = ConfigEuRoC()
    c.optimization_config.translation_threshold = 0.04
    n = 50
    mk = lambda: [SyntheticFeatureStream(c, seed=62, n_frames=n, n_features=60, motion_scale=0.5)]
    if 'refmotion' not in _CACHE:
        _CACHE['refmotion'] = _reference(c, mk(), n)
    ref = _CACHE['refmotion']
    run = _run(c, mk(), n, cap=192, env={'AV_DK_WG': '64'} if wg == 64 else {})
    assert run['shape'] == [(1, wg)]
    worst = dict(gamma_eval=0.0, gamma_pass=0.0, dx_pos=0.0, dx_rot=0.0)
    for k in range(n):
        _against_ref(run['sts'][k][0], ref['recs'][k][0], ref['dx_inf'][k][0], 'check_motion wg %d frame %d' % (wg, k), worst)
    allr = np.array(run['sts'])[:, 0]
    mixed = ((allr['n_pos'] < allr['n_cand']) & (allr['n_pos'] > 0)).sum(axis=0)
    assert (mixed >= 5).all() and (allr['n_eval'] == allr['n_pos']).all(), mixed


def test_gamma_sums_equal_the_captured_values_summed_exactly(cfg):
    """A second, synchronous run with debug_capture on: the same bytes, and gamma_eval against math.fsum of the per-feature values the
    library's own tap returns, within n * 2^-52 * sum (module docstring); the tap returns exactly n_eval values."""
    checked = 0
    for name, streams, n, kw, plain in (('three', R.streams3(cfg), N_FRAMES, {}, _sync3(cfg, 256)),
                                        ('cut', [R.cut_stream(cfg)], R.CUT_FRAMES, dict(cap=192, blank={0: (R.CUT_FRAMES - 1,)}), _cut(cfg, 256))):
        run = _run(cfg, streams, n, debug=True, **kw)
        for k in range(n):
            assert _same(run['outs'][k], plain['outs'][k]) and _same_st(run['sts'][k], plain['sts'][k]), (name, k)
            for s in range(len(streams)):
                for ph in range(2):
                    g, rec = run['dbg'][k][s][ph], run['sts'][k][s, ph]
                    assert len(g) == rec['n_eval'] and (g >= 0).all(), (name, k, s, ph)
                    exact = math.fsum(g.tolist())
                    assert abs(float(rec['gamma_eval']) - exact) <= len(g) * 2.0 ** -52 * exact, (name, k, s, ph, float(rec['gamma_eval']), exact)
                    checked += len(g) > 1
    assert checked > 60, checked


# ---- two runs of the library ---------------------------------------------------------------------------------------------------------
def test_queued_steps_fill_their_own_arrays(cfg):
    """Three submits (the ring's depth), then wait(0): each array holds its own step's records, bit for bit the synchronous run's."""
    sync = _sync3(cfg, 256)
    run = _run(cfg, R.streams3(cfg), N_FRAMES, mode='queue3')
    assert len({id(p) for p in run['sts']}) == N_FRAMES
    for k in range(N_FRAMES):
        assert _same(run['outs'][k], sync['outs'][k]) and _same_st(run['sts'][k], sync['sts'][k]), k


def test_two_stream_groups_fill_their_parts(cfg):
    """Streams {0, 1} and {2} as two groups (AV_MSCKF_GROUPS=2, one wavefront per stream): bit-identical to the single-group run."""
    sync = _sync3(cfg, 64)
    for mode in ('ahead', 'step'):
        run = _run(cfg, R.streams3(cfg), N_FRAMES, mode=mode, env={'AV_MSCKF_GROUPS': '2', 'AV_DK_WG': '64'})
        assert run['shape'] == [(2, 64), (1, 64)], run['shape']
        for k in range(N_FRAMES):
            assert _same(run['outs'][k], sync['outs'][k]) and _same_st(run['sts'][k], sync['sts'][k]), (mode, k)


def test_beside_the_map_and_the_covariance_and_off(cfg):
    """All three outputs on, in both launch shapes: the statistics are those of the run that has only them; and with the statistics off
    the twelve published doubles, the covariance and the landmark bytes are those of the run with them on."""
    only = _sync3(cfg, 256)
    off = _run(cfg, R.streams3(cfg), N_FRAMES, stats=False, landmarks=True, odom_cov=True)
    assert all(s is None for s in off['sts'])
    for env in ({}, {'AV_DK_WG': '64'}):
        allon = _run(cfg, R.streams3(cfg), N_FRAMES, landmarks=True, odom_cov=True, env=env)
        for k in range(N_FRAMES):
            assert _same_st(allon['sts'][k], only['sts'][k]), k
            assert _same(allon['outs'][k], only['outs'][k]) and _same(allon['outs'][k], off['outs'][k]), k
            assert _same(allon['covs'][k], off['covs'][k]) and _same_lm(allon['lms'][k], off['lms'][k]), k
    for pair in (dict(landmarks=True), dict(odom_cov=True)):
        one = _run(cfg, R.streams3(cfg), N_FRAMES, **pair)
        for k in range(N_FRAMES):
            assert _same_st(one['sts'][k], only['sts'][k]) and _same(one['outs'][k], only['outs'][k]), (pair, k)


def _allon3(cfg):
    """The three streams stepped synchronously with all three outputs on, once."""
    if 'allon' not in _CACHE:
        _CACHE['allon'] = _run(cfg, R.streams3(cfg), N_FRAMES, landmarks=True, odom_cov=True)
    return _CACHE['allon']


def test_every_subset_of_the_outputs_publishes_the_all_on_bits(cfg):
    """Every subset of {covariance, landmarks, statistics}, stepped synchronously -- every dk_mid and dk_finish instance the step can
    launch: each output that is on is bit for bit the all-on run's, the poses of all eight runs are the same bits, and an output that
    is off has no array."""
    allon = _allon3(cfg)
    for cov in (False, True):
        for lm in (False, True):
            for st in (False, True):
                if cov and lm and st:
                    continue
                run = _sync3(cfg, 256) if (cov, lm, st) == (False, False, True) else _run(cfg, R.streams3(cfg), N_FRAMES, stats=st, landmarks=lm, odom_cov=cov)
                for k in range(N_FRAMES):
                    assert _same(run['outs'][k], allon['outs'][k]), (cov, lm, st, k)
                    assert _same(run['covs'][k], allon['covs'][k]) if cov else run['covs'][k] is None, (cov, lm, st, k)
                    assert _same_lm(run['lms'][k], allon['lms'][k]) if lm else run['lms'][k] is None, (cov, lm, st, k)
                    assert _same_st(run['sts'][k], allon['sts'][k]) if st else run['sts'][k] is None, (cov, lm, st, k)


def test_two_stream_groups_offset_every_output_of_a_queued_step(cfg):
    """All three outputs on, streams {0, 1} and {2} as two groups (AV_MSCKF_GROUPS=2), three submits then wait(0): stream 2 lies in the
    second group, so each of the four arrays is written at its own offset; bit for bit the synchronous single-group run."""
    allon = _allon3(cfg)
    run = _run(cfg, R.streams3(cfg), N_FRAMES, landmarks=True, odom_cov=True, mode='queue3', env={'AV_MSCKF_GROUPS': '2'})
    assert run['shape'] == [(2, 256), (1, 256)], run['shape']
    for k in range(N_FRAMES):
        assert _same(run['outs'][k], allon['outs'][k]) and _same(run['covs'][k], allon['covs'][k]), k
        assert _same_lm(run['lms'][k], allon['lms'][k]) and _same_st(run['sts'][k], allon['sts'][k]), k
    assert sum(int(p[1][2, 1]) for p in run['lms']) > 0 and sum(int(s['n_eval'][2].sum()) for s in run['sts']) > 0


def test_idle_blank_and_stopped_streams(cfg):
    """Stream 0 is stopped by a capacity limit (the overflow pool shrunk to 64 rows, a blank frame at 17): 128 zero bytes from that step
    on.  Stream 2 has no frame (timestamp < 0) in three steps: zero there.  Stream 1 has a blank frame at 12, which loses every track:
    a lost-feature block of 32 candidates, as the reference has it.  Stream 1's records are those of stream 1 run alone; nothing in the buffer is NaN."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    n = 24
    mk = lambda: [SyntheticFeatureStream(cfg, seed=91, n_frames=n, n_features=150), SyntheticFeatureStream(cfg, seed=92, n_frames=n, n_features=40),
                  SyntheticFeatureStream(cfg, seed=100, n_frames=n, n_features=50)]
    env = {'AV_MSCKF_POOL_ROWS': '64'}
    idle = (5, 6, 20)
    both = _run(cfg, mk(), n, cap=192, blank={0: (17,), 1: (12,)}, idle={2: idle}, env=env, rows_cap=2048)
    solo = _run(cfg, mk()[1:2], n, cap=192, blank={0: (12,)}, env=env, rows_cap=2048)
    assert [k for k in range(n) if both['outs'][k][0, 0] < 0] == list(range(17, n))
    had = np.zeros(3, np.int64)
    for k in range(n):
        st = both['sts'][k]
        for f in R.DOUBLES:
            assert np.isfinite(st[f]).all(), (k, f)
        if k >= 17:
            assert _zero(st[0]), k
        if k in idle:
            assert both['outs'][k][2, 0] == 0.0 and _zero(st[2]), k
        had += st['n_cand'].sum(axis=1)
        assert _same(both['outs'][k][1:2], solo['outs'][k]) and _same_st(st[1:2], solo['sts'][k]), k
    assert (had > 20).all(), had
    # the blank frame of stream 1 against the reference: 32 features of 1,152 rows lost at once, under the cut
    ref = _reference(cfg, mk()[1:2], n, blank={0: (12,)})
    worst = dict(gamma_eval=0.0, gamma_pass=0.0, dx_pos=0.0, dx_rot=0.0)
    for k in range(n):
        _against_ref(both['sts'][k][1], ref['recs'][k][0], ref['dx_inf'][k][0], 'blank-frame stream, frame %d' % k, worst)
    st12 = both['sts'][12][1]
    assert st12['n_cand'][0] == 32 and st12['rows'][0] == 1152 and st12['flags'][0] == R.FS_RAN, st12


def _live():
    import ctypes
    from uav_airvision_amd import _native as N
    out = (ctypes.c_int64 * 4)()
    N.check(N.lib().av_debug_live_resources(ctypes.byref(out)))
    return [int(v) for v in out]


def test_lifecycle_and_switch(cfg, monkeypatch):
    """On: exactly one device buffer of S * 128 bytes and one pinned buffer of S * 128 bytes per ring slot more than off, nothing left
    after close().  Off: stats= raises, next_stats is refused; the switch is refused after the first step."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.msckf_ops import FILTER_STATS_DTYPE, BatchedMSCKF
    seen = {}

    def check_off(k, bat, out):
        if k == 3:
            seen['off'] = _live()
            with pytest.raises(ValueError, match='stats'):
                bat.step(np.zeros((3, CAP), np.int64), np.zeros((3, CAP, 4)), np.zeros(3, np.int32), np.full(3, -1.0), stats=True)
            with pytest.raises(AirvisionError, match='first step'):
                bat.set_stats(True)
            assert bat.stats is False and bat.last_stats is None

    def check_on(k, bat, out):
        if k == 3:
            seen['on'] = _live()
            with pytest.raises(ValueError, match='FILTER_STATS_DTYPE'):
                bat.step(np.zeros((3, CAP), np.int64), np.zeros((3, CAP, 4)), np.zeros(3, np.int32), np.full(3, -1.0), stats=np.zeros((3, 2)))
    base = _live()
    _run(cfg, R.streams3(cfg), 4, stats=False, check=check_off)
    _run(cfg, R.streams3(cfg), 4, check=check_on)
    assert _live() == base
    S, ring = 3, 3
    assert seen['on'][0] - seen['off'][0] == S * 128 + 256, (seen, base)
    assert seen['on'][1] - seen['off'][1] == ring * (S * 128 + 64), (seen, base)
    assert seen['on'][2:] == seen['off'][2:]
    for name in ('AV_DK_WG', 'AV_MSCKF_GROUPS', 'AV_MSCKF_STORE'):
        monkeypatch.delenv(name, raising=False)
    bat = BatchedMSCKF(cfg, 1)
    try:
        rec = np.zeros((1, 2), FILTER_STATS_DTYPE)
        assert N.lib().av_msckf_batch_next_stats(bat._h, rec.ctypes.data) == N.AV_E_INVALID
        assert b'av_msckf_batch_set_stats' in N.lib().av_last_error()
    finally:
        bat.close()
    assert _live() == base


# ---- hand-over, FilterSet -----------------------------------------------------------------------------------------------------------
def test_device_handover_and_filter_set_match_a_step_run_of_the_same_messages(cfg):
    """2 streams, 12 rendered frames through FrontendEngine + submit_dev(stats=True); the same messages through step(); the same two
    streams as two pipelines (EngineSet + FilterSet(stats=True)), whose last_stats joins the parts' arrays."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.pipelines import EngineSet, FilterSet
    F, S = 12, 2
    h = H.handover_run(cfg, F, S, stats=True)
    rows, cams, msgs, outs, sts = h['rows'], h['cams'], h['msgs'], h['outs'], h['sts']
    assert sum(bool(o[0, 0] == 1.0) for o in outs) >= 5 and sum(int(p['n_eval'].sum()) for p in sts) > 0
    ref = BatchedMSCKF(cfg, S, max_features=msgs[0][0].shape[1], stats=True)
    try:
        for k in range(F):
            _push(ref, rows[k])
            out = ref.step(*msgs[k], stats=True)
            assert _same(out, outs[k]) and _same_st(ref.last_stats, sts[k]), k
    finally:
        ref.close()
    es = EngineSet(cfg, 2, 2)
    fs = None
    try:
        fs = FilterSet(cfg, es, max_features=es.max_features, stats=True)
        with pytest.raises(ValueError):
            fs.submit_dev(es, cams[0][2], stats=np.zeros(2))
        o2, s2 = [], []
        for k, (c0, c1, ts) in enumerate(cams):
            i = np.array([i for i, _ in rows[k]], np.int32)
            t = np.array([m.timestamp for _, m in rows[k]])
            w = np.array([m.angular_velocity for _, m in rows[k]]).reshape(-1, 3)
            a = np.array([m.linear_acceleration for _, m in rows[k]]).reshape(-1, 3)
            es.push_imu_batch(i, t, w)
            es.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            fs.push_imu(i, t, w, a)
            o2.append(fs.submit_dev(es, ts, msg_stream=N.current_stream(), stats=True))
            s2.append(fs.last_stats)
        fs.wait(0)
        for k in range(F):
            assert _same(o2[k].array(), outs[k]) and _same_st(s2[k].array(), sts[k]), k
    finally:
        if fs is not None:
            fs.close()
        es.close()
    plain = FilterSet.__new__(FilterSet)
    plain.odom_cov, plain.landmarks, plain.stats, plain.es = False, False, False, es
    with pytest.raises(ValueError, match='stats'):
        plain.submit_dev(es, np.zeros(2), stats=True)


# ---- drop-in, sweep -------------------------------------------------------------------------------------------------------------------
def test_dropin_last_innovation_is_stream_0s_record(cfg):
    """The drop-in MSCKF with config.publish_innovation: last_innovation after every feature_callback holds, bit for bit, stream 0's
    record of the three-stream run (a stream's arithmetic does not depend on its neighbours); vio_result is what it was."""
    import sys
    from conftest import ROOT
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import FILTER_STATS_DTYPE
    from uav_airvision_amd.synth import replay_features
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import msckf as dmsckf
    sync = _sync3(cfg, 256)
    c = ConfigEuRoC()
    assert c.publish_innovation is False
    off = dmsckf.MSCKF(c, write_trajectory=False)
    assert off.last_innovation is None
    off.close()
    c.publish_innovation = True
    flt = dmsckf.MSCKF(c, write_trajectory=False)
    got = []

    def on(m):
        r = flt.feature_callback(m)
        assert r is None or r._fields == ('timestamp', 'pose', 'velocity', 'cam0_pose')
        got.append(flt.last_innovation)
    try:
        replay_features(R.streams3(cfg)[0], [flt.imu_callback], on)
    finally:
        flt.close()
    assert len(got) == N_FRAMES and len({id(g) for g in got}) == N_FRAMES
    for k, g in enumerate(got):
        assert g.shape == (2,) and g.dtype == FILTER_STATS_DTYPE and g.tobytes() == sync['sts'][k][0].tobytes(), k


def test_sweep_writes_the_nis_file(tmp_path, monkeypatch, capsys):
    """sweep --innovation on a short EuRoC-layout sequence: next to the trajectory file a _nis file with one line per pose, `t` + sixteen
    integers + eight doubles, and in the stream's report the run-wide nis_rows and reject_rate of exactly those records."""
    import json
    from fe_harness import make_cfg
    from uav_airvision_amd import sweep
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.msckf_ops import filter_stats_rows
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(make_cfg(), seed=13, n_frames=44, motion_scale=3.0, t0=1403636580.0, rest=1.0)
    write_euroc_layout(str(tmp_path / 'SEQ'), st, compress_level=1)
    kept = []
    inner = sweep.run_batched

    def run_batched(*a, **kw):
        kept.append(kw['nis_rows'])
        return inner(*a, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    out = tmp_path / 'txts'
    sweep.main(['--root', str(tmp_path), '--sequences', 'SEQ', '--innovation', '--out', str(out)])
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    traj = np.loadtxt(str(out / 'output_SEQ_offset0.txt')).reshape(-1, 8)
    rows = np.loadtxt(str(out / 'output_SEQ_offset0_nis.txt')).reshape(-1, 25)
    ((ts, rec),), = kept
    assert len(traj) > 20 and len(rows) == len(traj) == len(rec) == len(ts)
    assert np.abs(rows[:, 0] - traj[:, 0]).max() < 1e-6
    ints = np.stack([rec[n][:, b] for b in range(2) for n in R.INTS], axis=1)
    dbls = np.stack([rec[n][:, b] for b in range(2) for n in R.DOUBLES], axis=1)
    assert np.array_equal(rows[:, 1:17].astype(np.int64), ints) and np.array_equal(rows[:, 17:], dbls)
    assert rec['n_eval'].sum() > 50
    r0 = rep['report'][0]
    assert r0['sequence'] == 'SEQ' and r0['frames'] == len(traj)
    assert r0['nis_rows'] == float(rec['gamma_eval'].sum()) / int(filter_stats_rows(rec)[0].sum())
    assert r0['reject_rate'] == 1.0 - int(rec['n_pass'].sum()) / int(rec['n_eval'].sum())
