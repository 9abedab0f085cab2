"""tests/forecast_harness.py -- TEST INFRASTRUCTURE ONLY.

The driver of tests/test_gpu_forecast.py: imu_rate_harness.run with the forecast on and the IMU samples pushed `lead` frames AHEAD of
the frame that consumes them -- rows[k + 1] ahead of step k with lead = 1 -- so that every step has pending samples.  The oracles are
fed in the same order."""
import numpy as np

import filter_harness as H
from imu_rate_harness import CAP, N_FRAMES, streams3      # noqa: F401

FC_CAP = 32


def lead_rows(rows, lead):
    """rows (filter_harness.schedule) -> what is pushed ahead of every step: step 0 gets rows[0 .. lead], step k > 0 rows[k + lead]."""
    out = []
    for k in range(len(rows)):
        if k == 0:
            out.append([x for r in rows[:lead + 1] for x in r])
        else:
            out.append(list(rows[k + lead]) if k + lead < len(rows) else [])
    return out


def same_fc(a, b, sa=None, sb=None):
    """Two (records, counts, covariance) triples publish the same bytes: counts, the records up to `written`, the covariance rows
    (NaN rows compare by their bytes).  With sa, sb: stream sa of a against stream sb of b only."""
    (ra, na, ca), (rb, nb, cb) = a, b
    pairs = [(sa, sb)] if sa is not None else [(s, s) for s in range(len(na))]
    if sa is None and na.shape != nb.shape:
        return False
    return all(np.array_equal(na[x], nb[y]) and ra[x, :na[x, 1]].tobytes() == rb[y, :nb[y, 1]].tobytes() and ca[x].tobytes() == cb[y].tobytes()
               for x, y in pairs)


def run(cfg, streams, n_frames, forecast=True, fc_cap=FC_CAP, lead=1, mode='step', cap=CAP, blank=None, idle=None, withhold=None, env=None,
        oracle=None, check=None, others=(), restart=None, rows=None, msgs=None, own=False, **kw):
    """Drives a BatchedMSCKF over the streams with the forecast on (forecast) and, named in `others`, any of 'odom_cov', 'landmarks',
    'stats', 'imu_rate'.  lead: frames the IMU pushes run ahead.  mode: 'step', 'queue3', 'ahead' as filter_harness.run.  oracle(cfg): one
    per stream, fed the same samples and messages in the same order after every step; refs[k][i] = its forecast(fc_cap) after that frame.
    own: caller-owned arrays for the forecast instead of True.  restart = {frame: [streams]}.  check(k, bat, out, cur) after every step.
    Returns outs, fcs ((records, counts, covariance) per frame; None when off), covs, lms, sts, irs, refs, states (mode 'step'), final,
    counters, shape."""
    from uav_airvision_amd.msckf_ops import BatchedMSCKF, IMU_STATE_DTYPE
    with H.clean_env(env):
        bat = None
        try:
            S = len(streams)
            rows = H.schedule(streams, n_frames, withhold) if rows is None else rows
            ahead = lead_rows(rows, lead)
            msgs = H.messages(streams, n_frames, blank) if msgs is None else msgs
            on = {o: o in others for o in ('odom_cov', 'landmarks', 'stats', 'imu_rate')}
            bat = BatchedMSCKF(cfg, S, forecast=forecast, forecast_cap=fc_cap, **dict(on, **kw))
            assert bat.device_resident()
            oras = [oracle(cfg) for _ in streams] if oracle else None
            res = dict(outs=[], fcs=[], covs=[], lms=[], sts=[], irs=[], refs=[], states=[])
            args = dict(cov=True if on['odom_cov'] else None, landmarks=True if on['landmarks'] else None, stats=True if on['stats'] else None,
                        imu_states=True if on['imu_rate'] else None)
            for k in range(n_frames):
                if restart and k in restart:
                    bat.restart(restart[k])
                H.push(bat, ahead[k])
                ids, uv, nf, ts = H.arrays(msgs[k], cap, idle=[i for i in range(S) if idle and k in idle.get(i, ())])
                fc = None
                if forecast:
                    fc = (np.full((S, fc_cap, 14), 7.0).view(IMU_STATE_DTYPE).reshape(S, fc_cap), np.full((S, 2), -7, np.int32),
                          np.full((S, 120), 7.0)) if own else True
                if mode == 'step':
                    out = bat.step(ids, uv, nf, ts, forecast=fc, **args)
                    res['states'].append([H.state_bits(bat, s) for s in range(S)])
                else:
                    out = bat.submit(ids, uv, nf, ts, forecast=fc, **args)
                    if mode == 'ahead':
                        bat.wait(1)
                    elif k % 3 == 2:
                        bat.wait(0)
                cur = dict(fc=bat.last_forecast if forecast else None, cov=bat.last_cov if on['odom_cov'] else None,
                           lm=bat.last_landmarks if on['landmarks'] else None, st=bat.last_stats if on['stats'] else None,
                           ir=bat.last_imu_states if on['imu_rate'] else None, ref=None)
                res['outs'].append(out); res['fcs'].append(cur['fc']); res['covs'].append(cur['cov']); res['lms'].append(cur['lm'])
                res['sts'].append(cur['st']); res['irs'].append(cur['ir'])
                if oras is not None:
                    for i, m in ahead[k]:
                        oras[i].imu_callback(m)
                    cur['ref'] = []
                    for i, m in enumerate(msgs[k]):
                        if idle and k in idle.get(i, ()):
                            cur['ref'].append(([], (0, 0), np.full((15, 15), np.nan)))
                            continue
                        oras[i].feature_callback(m)
                        cur['ref'].append(oras[i].forecast(fc_cap))
                    res['refs'].append(cur['ref'])
                if check is not None:
                    check(k, bat, out, cur)
            bat.wait(0)
            res.update(final=[H.state_bits(bat, s) for s in range(S)], counters=bat.counters(), shape=bat.launch_shape())
            return res
        finally:
            if bat is not None:
                bat.close()


def oracle_run(cfg, streams, n_frames, lead, fc_cap=FC_CAP, oracle=None):
    """The oracles alone (no GPU), fed as `run` feeds them: -> (published poses per frame and stream: what feature_callback returned,
    forecasts per frame and stream, the oracles)."""
    import forecast_ref as Fr
    oracle = oracle or Fr.ForecastOracle
    rows = H.schedule(streams, n_frames)
    ahead = lead_rows(rows, lead)
    msgs = H.messages(streams, n_frames)
    oras = [oracle(cfg) for _ in streams]
    pubs, fcs = [], []
    for k in range(n_frames):
        for i, m in ahead[k]:
            oras[i].imu_callback(m)
        pubs.append([oras[i].feature_callback(m) for i, m in enumerate(msgs[k])])
        fcs.append([o.forecast(fc_cap) for o in oras])
    return pubs, fcs, oras


def handover_run(cfg, F=12, S=2, fc_cap=FC_CAP, lead=1):
    """filter_harness.handover_run with the forecast on and the IMU pushed `lead` frames ahead: S streams, F rendered frames through
    FrontendEngine + submit_dev(..., forecast=True): rows as pushed (ahead), the messages read back from the engine (msgs), the step
    outputs (outs) and the forecast triples (fcs)."""
    import torch
    from fe_harness import Frames
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    streams = [Frames.cached(SyntheticStream(cfg, seed=900 + u, n_frames=F)) for u in range(S)]
    rows = H.schedule(streams, F)
    ahead = lead_rows(rows, lead)
    cams = []
    for k in range(F):
        fr = [st.frame(k) for st in streams]
        cams.append((np.stack([m.cam0_image for m in fr]), np.stack([m.cam1_image for m in fr]), np.array([m.timestamp for m in fr])))
    eng = FrontendEngine(cfg, n_streams=S)
    flt = BatchedMSCKF(cfg, S, max_features=eng.max_features, forecast=True, forecast_cap=fc_cap)
    h = dict(ahead=ahead, msgs=[], outs=[], fcs=[])
    try:
        for k in range(F):
            c0, c1, ts = cams[k]
            for i, m in rows[k]:
                eng.push_imu(i, m.timestamp, m.angular_velocity)
            eng.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            H.push(flt, ahead[k])
            h['outs'].append(flt.submit_dev(eng, ts, msg_stream=N.current_stream(), forecast=True))
            h['fcs'].append(flt.last_forecast)
            ids, uv, n = eng.read_features_raw()
            h['msgs'].append((ids.copy(), uv.copy(), n.copy(), ts))
        flt.wait(0)
    finally:
        flt.close()
        eng.close()
    return h
