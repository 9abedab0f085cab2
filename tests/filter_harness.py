"""One driver for the suites of the batched filter's optional outputs (tests/test_gpu_odom_cov.py, test_gpu_landmarks.py,
test_gpu_filter_stats.py) and for tests/restart_helpers.py: bit comparisons, the IMU schedule and the messages of a set of synthetic
streams, and `run`, which steps a BatchedMSCKF over them in one of three modes with any of the outputs on."""
import contextlib
import os

import numpy as np

CAP = 128
LM_CAP = 64
ENV_KEYS = ('AV_DK_WG', 'AV_MSCKF_GROUPS', 'AV_MSCKF_STORE', 'AV_MSCKF_POOL_ROWS')      # what `run` clears and puts back


# ---- bit comparisons ------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Two float64 arrays, bit for bit."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_bytes(a, b):
    """Two record arrays (statistics), byte for byte."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_lm(a, b, sa=None, sb=None):
    """Two (records, counts) pairs publish the same bytes: the counts, and the records up to the count.  With sa, sb: stream sa of a
    against stream sb of b only."""
    (ra, na), (rb, nb) = a, b
    if sa is not None:
        return np.array_equal(na[sa], nb[sb]) and ra[sa, :na[sa, 1]].tobytes() == rb[sb, :nb[sb, 1]].tobytes()
    if not (na.shape == nb.shape and np.array_equal(na, nb)):
        return False
    return all(ra[s, :na[s, 1]].tobytes() == rb[s, :nb[s, 1]].tobytes() for s in range(len(na)))


def zero(rec):
    return not rec.tobytes().strip(b'\0')


# ---- streams -> what a step is fed ----------------------------------------------------------------------------------------------------
def schedule(streams, n_frames, withhold=None):
    """Per frame the IMU samples [(stream, msg)] that arrive before it (synth.replay's rule: each sample once, in the first frame that
    is not older than it); withhold = {stream: k0} keeps a stream's samples back until frame k0."""
    withhold = withhold or {}
    its = [iter(s.imu) for s in streams]
    pend = [next(it, None) for it in its]
    held = [[] for _ in streams]
    rows = []
    for k in range(n_frames):
        row = []
        for i, st in enumerate(streams):
            t = st.frame(k).timestamp
            while pend[i] is not None and pend[i].timestamp <= t:
                held[i].append(pend[i])
                pend[i] = next(its[i], None)
            if k >= withhold.get(i, 0):
                row += [(i, m) for m in held[i]]
                held[i] = []
        rows.append(row)
    return rows


def messages(streams, n_frames, blank=None):
    """msgs[k][i] = frame k of stream i; blank = {stream: frames} replaces those messages by empty ones of the same time."""
    from uav_airvision_amd.synth import feature_msg_t
    out = []
    for k in range(n_frames):
        msgs = [st.frame(k) for st in streams]
        if blank:
            msgs = [feature_msg_t(m.timestamp, []) if k in blank.get(i, ()) else m for i, m in enumerate(msgs)]
        out.append(msgs)
    return out


def arrays(msgs, cap, idle=()):
    """The four arrays of a step.  A stream listed in idle, or whose message is None, has no frame: timestamp -1, no features."""
    S = len(msgs)
    ids = np.zeros((S, cap), np.int64); uv = np.zeros((S, cap, 4)); nf = np.zeros(S, np.int32)
    ts = np.full(S, -1.0)
    for i, m in enumerate(msgs):
        if m is None or i in idle:
            continue
        ts[i] = m.timestamp
        nf[i] = len(m.features)
        ids[i, :nf[i]] = [f.id for f in m.features]
        uv[i, :nf[i]] = np.array([(f.u0, f.v0, f.u1, f.v1) for f in m.features]).reshape(-1, 4)
    return ids, uv, nf, ts


def push(bat, row):
    if row:
        bat.push_imu([i for i, _ in row], [m.timestamp for _, m in row], [m.angular_velocity for _, m in row], [m.linear_acceleration for _, m in row])


@contextlib.contextmanager
def clean_env(env=None):
    """The filter's switches (ENV_KEYS) cleared, then `env` set; what was there before comes back."""
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def state_bits(bat, s):
    gs = bat.get_state(s)
    return [np.atleast_1d(np.asarray(gs[key], dtype=np.float64)) for key in sorted(gs) if key != 'cam_ids'] + [bat.get_cov(s)]


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def run(cfg, streams, n_frames, odom_cov=False, landmarks=False, stats=False, mode='step', cap=CAP, lm_cap=LM_CAP, blank=None, idle=None,
        withhold=None, env=None, debug=False, oracle=None, oracle_step=None, check=None, **kw):
    """Drives a BatchedMSCKF over the streams.  mode: 'step' (synchronous), 'queue3' (three submits -- the ring's depth -- then wait(0)),
    'ahead' (submit + wait(1)).  blank = {stream: frames} replaces messages by empty ones, idle = {stream: frames} gives the stream no
    frame (timestamp -1), withhold: as in `schedule`.  debug: debug_capture on, dbg[k][s][ph] = the gammas debug_read returns after the
    step.  oracle(cfg): an oracle per stream that is fed the same IMU samples and messages after every step; refs[k][i] =
    oracle_step(oracle i, what its feature_callback returned, whether that step ended in its online_reset).  check(k, bat, out, cur)
    runs after every step and its oracles, cur = dict(cov, lm, st, ref) of the step.  kw goes to BatchedMSCKF.
    Returns per-frame outputs (outs), covariance arrays (covs), (records, counts) pairs (lms) and statistics arrays (sts) -- None where
    the output is off --, dbg, refs, the final state bits of every stream, the counters and the launch shape."""
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    with clean_env(env):
        bat = None
        try:
            S = len(streams)
            rows, msgs = schedule(streams, n_frames, withhold), messages(streams, n_frames, blank)
            bat = BatchedMSCKF(cfg, S, odom_cov=odom_cov, landmarks=landmarks, landmark_cap=lm_cap, stats=stats, **kw)
            assert bat.device_resident()
            if debug:
                bat.debug_capture(True)
            oras = [oracle(cfg) for _ in streams] if oracle else None
            res = dict(outs=[], covs=[], lms=[], sts=[], dbg=[], refs=[])
            args = dict(cov=True if odom_cov else None, landmarks=True if landmarks else None, stats=True if stats else None)
            for k in range(n_frames):
                push(bat, rows[k])
                ids, uv, nf, ts = arrays(msgs[k], cap, idle=[i for i in range(S) if idle and k in idle.get(i, ())])
                if mode == 'step':
                    out = bat.step(ids, uv, nf, ts, **args)
                else:
                    out = bat.submit(ids, uv, nf, ts, **args)
                    if mode == 'ahead':
                        bat.wait(1)
                    elif k % 3 == 2:
                        bat.wait(0)
                cur = dict(cov=bat.last_cov if odom_cov else None, lm=bat.last_landmarks if landmarks else None, st=bat.last_stats if stats else None, ref=None)
                res['outs'].append(out); res['covs'].append(cur['cov']); res['lms'].append(cur['lm']); res['sts'].append(cur['st'])
                if debug:
                    res['dbg'].append([[bat.debug_read(s, ph)[0] for ph in range(2)] for s in range(S)])
                if oras is not None:
                    for i, m in rows[k]:
                        oras[i].imu_callback(m)
                    cur['ref'] = []
                    for i, m in enumerate(msgs[k]):
                        ncam = len(oras[i].cam_states)
                        r = oras[i].feature_callback(m)
                        cur['ref'].append(oracle_step(oras[i], r, r is not None and ncam > 0 and len(oras[i].cam_states) == 0))
                    res['refs'].append(cur['ref'])
                if check is not None:
                    check(k, bat, out, cur)
            bat.wait(0)
            res.update(final=[state_bits(bat, s) for s in range(S)], counters=bat.counters(), shape=bat.launch_shape())
            return res
        finally:
            if bat is not None:
                bat.close()


def handover_run(cfg, F=12, S=2, **features):
    """S streams, F rendered frames through FrontendEngine + submit_dev with the outputs named in features (odom_cov / landmarks / stats
    = True) on: the IMU schedule (rows), the images (cams), the messages read back from the engine (msgs), the step outputs and the
    outputs' arrays (outs, covs, lms, sts)."""
    import torch
    from fe_harness import Frames
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    streams = [Frames.cached(SyntheticStream(cfg, seed=900 + u, n_frames=F)) for u in range(S)]
    rows = schedule(streams, F)
    cams = []
    for k in range(F):
        fr = [st.frame(k) for st in streams]
        cams.append((np.stack([m.cam0_image for m in fr]), np.stack([m.cam1_image for m in fr]), np.array([m.timestamp for m in fr])))
    args = dict(cov=features.get('odom_cov') or None, landmarks=features.get('landmarks') or None, stats=features.get('stats') or None)
    eng = FrontendEngine(cfg, n_streams=S)
    flt = BatchedMSCKF(cfg, S, max_features=eng.max_features, **features)
    h = dict(rows=rows, cams=cams, msgs=[], outs=[], covs=[], lms=[], sts=[])
    try:
        for k in range(F):
            c0, c1, ts = cams[k]
            for i, m in rows[k]:
                eng.push_imu(i, m.timestamp, m.angular_velocity)
            eng.step(torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda(), ts)
            push(flt, rows[k])
            h['outs'].append(flt.submit_dev(eng, ts, msg_stream=N.current_stream(), **args))
            h['covs'].append(flt.last_cov); h['lms'].append(flt.last_landmarks); h['sts'].append(flt.last_stats)
            ids, uv, n = eng.read_features_raw()
            h['msgs'].append((ids.copy(), uv.copy(), n.copy(), ts))
        flt.wait(0)
    finally:
        flt.close()
        eng.close()
    return h
