"""tests/imu_rate_harness.py -- TEST INFRASTRUCTURE ONLY.

The driver of tests/test_gpu_imu_rate.py: filter_harness.run with the keyword its signature cannot carry (imu_states=), over the
pieces filter_harness already has -- the IMU schedule, the messages, the four arrays of a step, the environment."""
import numpy as np

import filter_harness as H

N_FRAMES = 30                      # past the first camera-state prune (20 states)
CAP = 128
IR_CAP = 32


def streams3(cfg, n_frames=N_FRAMES):
    """The three streams of tests/test_gpu_odom_cov.py."""
    from uav_airvision_amd.synth import SyntheticFeatureStream
    return [SyntheticFeatureStream(cfg, seed=100 + i, n_frames=n_frames, n_features=80, motion_scale=1.0 + 0.25 * i) for i in range(3)]


def same_ir(a, b, sa=None, sb=None):
    """Two (records, counts) pairs publish the same bytes: the counts, and the records up to `written`.  With sa, sb: stream sa of a
    against stream sb of b only."""
    (ra, na), (rb, nb) = a, b
    if sa is not None:
        return np.array_equal(na[sa], nb[sb]) and ra[sa, :na[sa, 1]].tobytes() == rb[sb, :nb[sb, 1]].tobytes()
    if not (na.shape == nb.shape and np.array_equal(na, nb)):
        return False
    return all(ra[s, :na[s, 1]].tobytes() == rb[s, :nb[s, 1]].tobytes() for s in range(len(na)))


def run(cfg, streams, n_frames, imu_rate=True, ir_cap=IR_CAP, mode='step', cap=CAP, blank=None, idle=None, withhold=None, env=None, oracle=None,
        check=None, others=(), restart=None, rows=None, msgs=None, **kw):
    """Drives a BatchedMSCKF over the streams with the IMU-rate odometry on (imu_rate) and, named in `others`, any of 'odom_cov',
    'landmarks', 'stats'.  mode, blank, idle, withhold, env: as filter_harness.run.  oracle(cfg): one per stream, fed the same samples and
    messages after every step; refs[k][i] = its imu_states list of that frame.  restart = {frame: [streams]}: BatchedMSCKF.restart ahead of
    that frame's IMU samples.  rows, msgs: the IMU schedule and the messages, where they are not those of `streams` (a slot fed two lives).
    check(k, bat, out, cur) after every step.
    Returns outs, irs ((records, counts) per frame; None when off), covs, lms, sts, refs, states (per frame and stream, mode 'step'
    only), final, counters, shape."""
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    with H.clean_env(env):
        bat = None
        try:
            S = len(streams)
            rows = H.schedule(streams, n_frames, withhold) if rows is None else rows
            msgs = H.messages(streams, n_frames, blank) if msgs is None else msgs
            on = {o: o in others for o in ('odom_cov', 'landmarks', 'stats')}
            bat = BatchedMSCKF(cfg, S, imu_rate=imu_rate, imu_rate_cap=ir_cap, **dict(on, **kw))
            assert bat.device_resident()
            oras = [oracle(cfg) for _ in streams] if oracle else None
            res = dict(outs=[], irs=[], covs=[], lms=[], sts=[], refs=[], states=[])
            args = dict(imu_states=True if imu_rate else None, cov=True if on['odom_cov'] else None, landmarks=True if on['landmarks'] else None,
                        stats=True if on['stats'] else None)
            for k in range(n_frames):
                if restart and k in restart:
                    bat.restart(restart[k])
                H.push(bat, rows[k])
                ids, uv, nf, ts = H.arrays(msgs[k], cap, idle=[i for i in range(S) if idle and k in idle.get(i, ())])
                if mode == 'step':
                    out = bat.step(ids, uv, nf, ts, **args)
                    res['states'].append([H.state_bits(bat, s) for s in range(S)])
                else:
                    out = bat.submit(ids, uv, nf, ts, **args)
                    if mode == 'ahead':
                        bat.wait(1)
                    elif k % 3 == 2:
                        bat.wait(0)
                cur = dict(ir=bat.last_imu_states if imu_rate else None, cov=bat.last_cov if on['odom_cov'] else None,
                           lm=bat.last_landmarks if on['landmarks'] else None, st=bat.last_stats if on['stats'] else None, ref=None)
                res['outs'].append(out); res['irs'].append(cur['ir']); res['covs'].append(cur['cov']); res['lms'].append(cur['lm']); res['sts'].append(cur['st'])
                if oras is not None:
                    for i, m in rows[k]:
                        oras[i].imu_callback(m)
                    cur['ref'] = []
                    for i, m in enumerate(msgs[k]):
                        oras[i].feature_callback(m)
                        cur['ref'].append(list(oras[i].imu_states))
                    res['refs'].append(cur['ref'])
                if check is not None:
                    check(k, bat, out, cur)
            bat.wait(0)
            res.update(final=[H.state_bits(bat, s) for s in range(S)], counters=bat.counters(), shape=bat.launch_shape())
            return res
        finally:
            if bat is not None:
                bat.close()


def handover_run(cfg, F=12, S=2, ir_cap=IR_CAP):
    """filter_harness.handover_run with the IMU-rate odometry on: S streams, F rendered frames through FrontendEngine + submit_dev(...,
    imu_states=True): the IMU schedule (rows), the images (cams), the messages read back from the engine (msgs), the step outputs (outs)
    and the (records, counts) pairs (irs)."""
    import torch
    from fe_harness import Frames
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    streams = [Frames.cached(SyntheticStream(cfg, seed=900 + u, n_frames=F)) for u in range(S)]
    rows = H.schedule(streams, F)
    cams = []
    for k in range(F):
        fr = [st.frame(k) for st in streams]
        cams.append((np.stack([m.cam0_image for m in fr]), np.stack([m.cam1_image for m in fr]), np.array([m.timestamp for m in fr])))
    eng = FrontendEngine(cfg, n_streams=S)
    flt = BatchedMSCKF(cfg, S, max_features=eng.max_features, imu_rate=True, imu_rate_cap=ir_cap)
    h = dict(rows=rows, cams=cams, msgs=[], outs=[], irs=[])
    try:
        for k in range(F):
            c0, c1, ts = cams[k]
            for i, m in rows[k]:
                eng.push_imu(i, m.timestamp, m.angular_velocity)
            eng.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            H.push(flt, rows[k])
            h['outs'].append(flt.submit_dev(eng, ts, msg_stream=N.current_stream(), imu_states=True))
            h['irs'].append(flt.last_imu_states)
            ids, uv, n = eng.read_features_raw()
            h['msgs'].append((ids.copy(), uv.copy(), n.copy(), ts))
        flt.wait(0)
    finally:
        flt.close()
        eng.close()
    return h
