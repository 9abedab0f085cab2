"""The NumPy statement of the forecast's contract (tests/forecast_ref.py) on the CPU: forecast() leaves its oracle untouched; its records
are the records the same oracle writes for the same samples in its NEXT feature_callback (the same NumPy code on the same inputs: bit
for bit); pushing the IMU a frame ahead changes no published pose; and the fp64 oracle against the 50-digit version over the families
of tests/msckf_predict_cases.py, which gives the e_fam the GPU kernels' bars are taken from (tests/test_gpu_forecast_ops.py)."""
import pickle

import numpy as np
import pytest

import forecast_harness as Fh
import forecast_ref as Fr
import msckf_predict_cases as Pc

N_FRAMES = 12


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _snapshot(o):
    """Everything the oracle's run depends on, as bytes."""
    s = o.imu_state
    return pickle.dumps((s.timestamp, s.orientation, s.position, s.velocity, s.gyro_bias, s.acc_bias, s.orientation_null, s.position_null, s.velocity_null,
                         s.R_imu_cam0, s.t_cam0_imu, o.state_cov, o.gravity, [(m.timestamp, m.angular_velocity, m.linear_acceleration) for m in o.imu_msg_buffer],
                         sorted(o.cam_states), len(o.map_server), o.next_imu_id, [sorted(r.items(), key=lambda kv: kv[0]) for r in o.imu_states]))


@pytest.fixture(scope='module')
def runs(cfg):
    streams = Fh.streams3(cfg, N_FRAMES)
    return {lead: Fh.oracle_run(cfg, streams, N_FRAMES, lead) for lead in (0, 1)}


def test_forecast_leaves_the_oracle_untouched_and_meets_its_next_frame(cfg):
    """Frame by frame with the IMU a frame ahead: forecast() changes nothing of the oracle, and its records are bit for bit the leading
    imu_states the oracle records in its next feature_callback; a cap of 4 keeps the FIRST four."""
    streams = Fh.streams3(cfg, N_FRAMES)
    rows = Fh.lead_rows(Fh.H.schedule(streams, N_FRAMES), 1)
    oras = [Fr.ForecastOracle(cfg) for _ in streams]
    prev, live = [None] * len(streams), 0
    for k in range(N_FRAMES):
        for i, m in rows[k]:
            oras[i].imu_callback(m)
        for i, st in enumerate(streams):
            oras[i].feature_callback(st.frame(k))
            if prev[i] is not None and prev[i][1][1] > 0:
                recs, (had, wr), _ = prev[i]
                nxt = oras[i].imu_states
                assert wr == had <= len(nxt), (k, i)
                for a, b in zip(recs, nxt):
                    assert a['t'] == b['t'] and all(_bits(a[f], b[f]) for f in ('p', 'q', 'v', 'w')), (k, i)
                live += 1
            before = _snapshot(oras[i])
            fc = oras[i].forecast(Fh.FC_CAP)
            assert _snapshot(oras[i]) == before, (k, i)
            few = oras[i].forecast(4)
            assert few[1] == (fc[1][0], min(fc[1][0], 4)) and len(few[0]) == few[1][1]
            for a, b in zip(few[0], fc[0]):
                assert a['t'] == b['t'] and all(_bits(a[f], b[f]) for f in ('p', 'q', 'v', 'w'))
            prev[i] = fc if oras[i].published else None
    assert live >= 2 * (N_FRAMES - 2)


def test_a_frame_of_lead_changes_no_published_pose(runs):
    (p0, f0, _), (p1, f1, _) = runs[0], runs[1]
    n = 0
    for k in range(N_FRAMES):
        for a, b in zip(p0[k], p1[k]):
            assert (a is None) == (b is None), k
            if a is not None:
                assert a.timestamp == b.timestamp and _bits(a.pose.R, b.pose.R) and _bits(a.pose.t, b.pose.t) and _bits(a.velocity, b.velocity), k
                n += 1
    assert n > N_FRAMES
    # nothing pending without the lead, about a frame's worth with it, except behind the last frame
    assert all(fc[1] == (0, 0) for row in f0 for fc in row)
    assert any(fc[1][0] > 4 for row in f1[:-1] for fc in row) and all(fc[1] == (0, 0) for fc in f1[-1])


def test_nothing_pending_is_the_map_of_the_state_the_frame_leaves(cfg, runs):
    from odom_cov_ref import odom_cov
    _, f0, oras = runs[0]
    for o, (recs, n, C) in zip(oras, f0[-1]):
        s = o.imu_state
        assert recs == [] and n == (0, 0) and _bits(C, odom_cov(o.state_cov, s.orientation, s.R_imu_cam0, s.t_cam0_imu))


@pytest.mark.parametrize('name', Fr.FAMILIES)
def test_oracle_against_the_50_digit_forecast(cfg, name):
    """e_fam: the fp64 oracle's forecast of every case of the family against the 50-digit one.  q, p, v of every record within the bar
    the kernels get (16 e_fam of msckf_predict_cases.bars); the record's e_fam is what this measures, floored at 4 ulp, and it is small:
    the map adds a few roundings to the propagated block's."""
    bars = Fr.bars(name, cfg)
    errs = Fr.oracle_errors(name, cfg)
    assert not any(e['left_out'] for e in errs)
    for case, e in zip(Pc.family(name, cfg), errs):
        recs, (had, wr), _ = Fr.predict_case(case, cfg, Fh.FC_CAP)
        assert had == wr == len(case['imu']) == len(recs)
        for g, m in zip(recs, case['imu']):
            assert g['t'] == m[0] and _bits(g['w'], m[1:4] - case['state']['bg']), case['name']
        assert all(e[f] <= Pc.FACTOR * bars[f] for f in ('q', 'p', 'v')), (case['name'], e, bars)
    print('FORECAST ref %s: e_fam q %.2e p %.2e v %.2e C %.2e' % (name, bars['q'], bars['p'], bars['v'], bars['C']))
    assert Pc.FLOOR <= bars['C'] < 1e-9, bars


def test_the_cap_keeps_the_first_samples_in_50_digits_too(cfg):
    """cap 4 against 10 pending: the reference of the first four is that of the case cut to four samples."""
    case = Pc.family('samples', cfg)[0]
    recs, n, C = Fr.predict_case(case, cfg, 4)
    assert n == (10, 4) and [r['t'] for r in recs] == case['imu'][:4, 0].tolist()
    ref = Fr.mp_forecast(case, 4)
    assert len(ref['states']) == 4
    b = Fr.bars('samples', cfg)
    assert Fr.rec_err(C, ref['C']) <= Pc.FACTOR * b['C']
    for g, want in zip(recs, ref['states']):
        assert all(Pc.vec_err(g[f], want[f], quaternion=f == 'q') <= Pc.FACTOR * b[f] for f in ('q', 'p', 'v'))
