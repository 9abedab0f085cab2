"""The zero-velocity update end to end (include/airvision.h, "Zero-velocity update"): the batched filter with the update on against
OracleMSCKF with tests/zupt_ref.py applied after every feature_callback (the tolerances of tests/test_gpu_msckf.py's end-to-end parity,
no new ones), and what must hold bit for bit: an unreachable min_tracks is the feature off, streams are independent, step = submit,
a restarted stream is a fresh one, nothing stays allocated, the drop-in is a one-stream batch."""
import ctypes

import numpy as np
import pytest

import filter_harness as H
import zupt_ref as Z

pytestmark = pytest.mark.gpu

N_FRAMES = 40
CAP = 128


def _streams(cfg):
    """At rest, moving, and at rest for a second and then moving."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    kw = dict(n_frames=N_FRAMES, n_features=40, pixel_sigma=0.05)
    return [SyntheticFeatureStream(cfg, seed=0, motion_scale=0.0, **kw), SyntheticFeatureStream(cfg, seed=1, **kw),
            SyntheticFeatureStream(cfg, seed=2, rest=1.0, **kw)]


_CACHE = {}


def _run(cfg, key, streams, **kw):
    if key not in _CACHE:
        _CACHE[key] = H.run(cfg, streams, N_FRAMES, cap=CAP, **kw)
    return _CACHE[key]


def _same_run(a, b, sa=None, sb=None):
    """Two runs publish the same bits in every step and end in the same state (sa, sb: stream sa of a against stream sb of b)."""
    if sa is None:
        return all(H.same(x, y) for x, y in zip(a['outs'], b['outs'])) and all(H.same(p, q) for fa, fb in zip(a['final'], b['final']) for p, q in zip(fa, fb))
    return all(H.same(x[sa], y[sb]) for x, y in zip(a['outs'], b['outs'])) and all(H.same(p, q) for p, q in zip(a['final'][sa], b['final'][sb]))


@pytest.mark.parametrize('wg', (256, 64))
def test_three_streams_follow_the_oracle_with_the_update_applied(cfg, wg):
    streams = _streams(cfg)
    recs = []

    def check(k, bat, out, cur):
        rec = bat.read_zupt()
        recs.append(rec)
        for i in range(3):
            o = cur['ref'][i]
            assert bool(out[i, 0]) and o.published is not None, (k, i)
            for f in ('flags', 'n_imu', 'n_tracked', 'n_still', 'detected_total', 'applied_total'):
                assert int(rec[i][f]) == int(o.record[f]), (k, i, f, rec[i], o.record)
            for f in ('w_max', 'a_dev_max', 'v_norm', 'gamma', 'dx_pos'):
                assert abs(rec[i][f] - o.record[f]) <= 1e-6 * max(1.0, abs(o.record[f])), (k, i, f, rec[i], o.record)
            # the step's published pose is the pre-update one
            p, q, v = o.published
            assert max(np.abs(out[i, 2:5] - p).max(), np.abs(out[i, 5:9] - q).max(), np.abs(out[i, 9:12] - v).max()) < 1e-6, (k, i)
            # get_state sees the corrected state: every target of the injection
            s, gs = o.imu_state, bat.get_state(i)
            assert max(np.abs(gs['p'] - s.position).max(), np.abs(gs['q'] - s.orientation).max(), np.abs(gs['v'] - s.velocity).max()) < 1e-6, (k, i)
            assert np.abs(gs['bg'] - s.gyro_bias).max() < 1e-7 and np.abs(gs['ba'] - s.acc_bias).max() < 1e-6, (k, i)
            assert np.abs(gs['R_ic'] - s.R_imu_cam0).max() < 1e-6 and np.abs(gs['t_ci'] - s.t_cam0_imu).max() < 1e-6, (k, i)
            assert list(gs['cam_ids']) == list(o.cam_states.keys()), (k, i)
            if len(gs['cam_ids']):
                assert np.abs(gs['cam_q'] - np.array([c.orientation for c in o.cam_states.values()])).max() < 1e-6
                assert np.abs(gs['cam_p'] - np.array([c.position for c in o.cam_states.values()])).max() < 1e-6
            if rec[i]['flags'] & Z.APPLIED:
                assert not np.array_equal(gs['v'], out[i, 9:12]), (k, i)
            P, Po = bat.get_cov(i), o.state_cov
            assert P.shape == Po.shape and np.abs(P - Po).max() <= 1e-6 * np.abs(Po).max(), (k, i)
            assert np.array_equal(P, P.T), (k, i)

    run = H.run(cfg, streams, N_FRAMES, cap=CAP, oracle=Z.ZuptOracle, oracle_step=lambda o, r, reset: o, check=check,
                env={'AV_DK_WG': '64'} if wg == 64 else {}, zupt=True)
    assert run['shape'] == [(3, wg)]
    last = recs[-1]
    # at rest: every frame from the second on; moving: none after its start; rest then motion: the first second only
    assert last[0]['detected_total'] == N_FRAMES - 1 and last[0]['applied_total'] >= N_FRAMES - 5
    assert last[1]['detected_total'] <= 2 and 15 <= last[2]['detected_total'] <= 25 and last[2]['applied_total'] >= 10
    assert not any(r[2]['flags'] & Z.DETECTED for r in recs[30:])
    print('ZUPT e2e wg=%d totals (detected, applied): %s' % (wg, [(int(r['detected_total']), int(r['applied_total'])) for r in last]))


def test_an_unreachable_min_tracks_is_the_feature_off_bit_for_bit(cfg):
    from uav_airvision_amd.msckf_ops import zupt_params
    streams = _streams(cfg)
    off = _run(cfg, 'off', streams)
    on = H.run(cfg, streams, N_FRAMES, cap=CAP, zupt=dict(zupt_params(cfg), min_tracks=1 << 20))
    assert _same_run(on, off) and on['counters'] == off['counters']
    live = _run(cfg, 'on', streams, zupt=True)
    assert not _same_run(live, off)                      # ... and the feature itself is not a no-op


def test_a_stream_alone_is_the_stream_beside_a_resting_neighbour(cfg):
    streams = _streams(cfg)
    three = _run(cfg, 'on', streams, zupt=True)
    for s in (0, 1, 2):
        alone = H.run(cfg, [streams[s]], N_FRAMES, cap=CAP, zupt=True)
        assert _same_run(alone, three, 0, s), s


@pytest.mark.parametrize('mode', ('queue3', 'ahead'))
def test_step_and_submit_are_the_same_bits(cfg, mode):
    streams = _streams(cfg)
    assert _same_run(H.run(cfg, streams, N_FRAMES, cap=CAP, mode=mode, zupt=True), _run(cfg, 'on', streams, zupt=True))


def test_two_stream_groups_read_their_records_side_by_side(cfg):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    streams = _streams(cfg)
    got = {}
    for env in ({}, {'AV_MSCKF_GROUPS': '2'}):
        def check(k, bat, out, cur):
            got.setdefault(len(env), []).append(bat.read_zupt())
        run = H.run(cfg, streams, 12, cap=CAP, env=env, check=check, zupt=True)
        assert len(run['shape']) == 1 + len(env)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], got[1])) and got[0][-1]['applied_total'][0] > 0


def test_restart_clears_record_and_totals_and_the_stream_is_a_fresh_one(cfg):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    streams = _streams(cfg)[:2]
    fresh = H.run(cfg, [streams[0]], 15, cap=CAP, zupt=True)
    with H.clean_env():
        bat = BatchedMSCKF(cfg, 2, zupt=True)
        try:
            rows, msgs = H.schedule(streams, 15), H.messages(streams, 15)
            for k in range(10):
                H.push(bat, rows[k])
                bat.step(*H.arrays(msgs[k], CAP))
            before = bat.read_zupt()
            assert before[0]['applied_total'] > 0 and before[0]['detected_total'] == 9
            bat.restart([0])
            after = bat.read_zupt()
            assert H.zero(after[0]) and after[1].tobytes() == before[1].tobytes()
            # the new life: the same inputs from the start, beside a neighbour that goes on
            outs = []
            for k in range(15):
                H.push(bat, [(i, m) for i, m in rows[k] if i == 0])
                if 10 + k < 15:
                    H.push(bat, [(i, m) for i, m in rows[10 + k] if i == 1])
                m1 = msgs[10 + k][1] if 10 + k < 15 else None
                outs.append(bat.step(*H.arrays([msgs[k][0], m1], CAP)))
            assert all(H.same(o[0], f[0]) for o, f in zip(outs, fresh['outs']))
            assert all(H.same(p, q) for p, q in zip(H.state_bits(bat, 0), fresh['final'][0]))
        finally:
            bat.close()


def test_refusals_that_need_a_batch(cfg):
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.msckf_ops import BatchedMSCKF, zupt_params
    streams = _streams(cfg)[:1]
    bat = BatchedMSCKF(cfg, 1)
    try:
        assert bat.zupt is None and H.zero(bat.read_zupt())
        for bad in (dict(velocity_sigma=0.0), dict(gate=-1.0), dict(still_percent=101), dict(min_tracks=-1), dict(acc_dev_max=float('inf'))):
            with pytest.raises(N.AirvisionError) as e:
                bat.set_zupt(dict(zupt_params(cfg), **bad))
            assert e.value.code == N.AV_E_INVALID and 'av_msckf_batch_set_zupt' in str(e.value)
        bat.set_zupt(zupt_params(cfg))
        bat.set_zupt(None)
        bat.set_zupt(zupt_params(cfg))
        rows, msgs = H.schedule(streams, 2), H.messages(streams, 2)
        H.push(bat, rows[0])
        bat.step(*H.arrays(msgs[0], CAP))
        for p in (None, zupt_params(cfg)):
            with pytest.raises(N.AirvisionError) as e:
                bat.set_zupt(p)
            assert e.value.code == N.AV_E_INVALID and 'has stepped' in str(e.value)
    finally:
        bat.close()


def test_nothing_stays_allocated_after_close(cfg):
    """av_debug_live_resources: four zeros before, something alive while the batch steps with the update on, four zeros after close().
    In a process of its own: the counts are the process's, and in a suite's process objects of earlier modules may still await their
    collection (2.2 MB of device memory did when this test first ran behind the whole suite)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = ('import ctypes, sys\n'
            'sys.path[:0] = [%r, %r]\n'
            'import filter_harness as H, test_gpu_zupt as T\n'
            'from uav_airvision_amd import _native as N\n'
            'from uav_airvision_amd.config import ConfigEuRoC\n'
            'def live():\n'
            '    o = (ctypes.c_int64 * 4)()\n'
            '    N.check(N.lib().av_debug_live_resources(ctypes.byref(o)))\n'
            '    return [int(v) for v in o]\n'
            'cfg = ConfigEuRoC()\n'
            'assert live() == [0, 0, 0, 0], live()\n'
            'peak = []\n'
            'H.run(cfg, T._streams(cfg), 6, cap=T.CAP, zupt=True, check=lambda k, bat, out, cur: peak.append(live()))\n'
            'assert all(p[0] > 0 and p[1] > 0 for p in peak), peak\n'
            'assert live() == [0, 0, 0, 0], live()\n'
            'print("ZUPT_LIFECYCLE_OK", max(p[0] for p in peak))\n') % (ROOT, os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'ZUPT_LIFECYCLE_OK' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])


def test_the_dropin_with_use_zupt_is_a_one_stream_batch(cfg):
    import copy
    import os
    import sys
    from conftest import ROOT
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')      # the drop-in is used from the module search path, as the reference's src/ is
    if d not in sys.path:
        sys.path.insert(0, d)
    import msckf as dmsckf
    from uav_airvision_amd.synth import replay_features
    c = copy.copy(cfg)
    c.use_zupt = True
    fs = _streams(c)[2]
    batch = H.run(c, [fs], N_FRAMES, cap=64, zupt=True)
    flt = dmsckf.MSCKF(c, write_trajectory=False)
    try:
        totals = []
        replay_features(fs, [flt.imu_callback], lambda m: totals.append((flt.feature_callback(m) is not None, int(flt.last_zupt['applied_total']))))
        assert all(t[0] for t in totals) and totals[-1][1] >= 10
        assert all(H.same(p, q) for p, q in zip(H.state_bits(flt._flt, 0), batch['final'][0]))
    finally:
        flt.close()


def test_sweep_with_the_switch_reports_the_totals_of_every_stream(tmp_path, capsys):
    """`sweep --zupt` on one short EuRoC-layout sequence whose rig stands still for its first two seconds, from two offsets: the report
    gains "zupt" with one (detected_total, applied_total) per stream, applied <= detected <= frames, and the stream that is live while
    the rig still stands is detected there.  (That the report has no such entry without the switch, and that every other switch
    still lands, is tests/test_zupt_ref.py's, without a card.)"""
    import json
    from uav_airvision_amd import sweep
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    # (a swept stream goes live with its 200th IMU sample, one second after its start: the rig stands for two, so frames 20 .. 23 of
    #  the first stream are live frames of a rig at rest; the second stream starts three frames later and is live from frame 23)
    n = 24
    write_euroc_layout(str(tmp_path / 'SEQ'), SyntheticStream(ConfigEuRoC(), seed=17, n_frames=n, motion_scale=3.0, t0=1403636580.0, rest=2.0), compress_level=1)
    sweep.main(['--root', str(tmp_path), '--sequences', 'SEQ', '--offsets', '0.0', '0.12', '--zupt', '--out', str(tmp_path / 'txts')])
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert rep['stream_frames'] == 2 * n - 3
    z = rep['zupt']
    print('ZUPT sweep totals', z, [r.get('frames') for r in rep['report']])
    assert sorted(z) == ['applied_total', 'detected_total'] and len(z['detected_total']) == len(z['applied_total']) == 2
    assert all(0 <= a <= d <= n for d, a in zip(z['detected_total'], z['applied_total']))
    assert z['detected_total'][0] >= 1 and z['applied_total'][0] >= 1
