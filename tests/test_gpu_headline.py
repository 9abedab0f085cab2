"""Parity of the configuration bench.py's headline number is produced with, and of the launch shapes the library picks by itself.

The headline is 2,048 streams on one GPU: the batched filter split into two stream groups (own worker thread and HIP stream each), the
per-stream filter kernels (dk_begin4 / dk_cov<64> / dk_mid / dk_finish) launched as ONE wavefront per stream, the feature message
handed over on the device (av_msckf_batch_submit_dev), av_frontend_prestage for frame k + 1 enqueued before frame k's hand-over, no
host wait inside the loop.  The shapes are chosen per GROUP (include/airvision.h, av_msckf_batch_launch_shape), so 2,048 is the smallest
stream count at which the library takes them by itself; (a) pins that table, (b) the two-group branch of the hand-over at its
smallest shape, (c) the filter alone and (d) the complete path at 2,048 streams with no AV_* override.

Tolerances: features bit for bit against OracleFrontend; filter against OracleMSCKF as in test_gpu_msckf.py (1e-6 on p / q / v and the
camera states, 1e-7 on the gyro bias, 1e-6 relative on the covariance); everything that compares two runs of the library with each
other, or two replicas within one run, bit for bit.

Measured on one MI355X (wall time of each test, fixtures included; two runs):
  (a) test_launch_shape_table                 2.4 - 2.7 s for the five cases (2.2 - 2.5 s of them the first one, which initialises the GPU)
  (b) test_two_group_device_handover          4.9 - 5.7 s (4.7 - 5.3 s the `rendered` fixture: three streams rendered and run through both CPU oracles)
  (c) test_filter_alone_at_2048_streams       3.1 - 3.2 s
  (d) test_complete_path_at_2048_streams      0.6 s (the fixture is shared with (b))

Seen to fail (each by breaking what it guards, once): (d) with replica 2,047 shown the other original's frames -- filter outputs of
stream 2,047 differ from frame 5 on; (d) with stream 0 and all its replicas shown original 1's frames -- the replicas agree, stream 0
is 2.8e-3 off the 2-stream run at frame 5; (c) with one coordinate of replica 2,047's message one ulp off at frame 31 -- that frame, that
stream; (c) with one pixel added to u0 of every replica of original 1 from frame 31 on -- 3.3e-3 against the oracle's 1e-6; (b) with a
64 x 64 patch of stream 1's frame 5 inverted for the engine only -- 290 features against the oracle's 300; (a) with AV_MSCKF_GROUPS=1
or AV_DK_WG=256 left in place.  Two did NOT fail: the 2-stream run of (d) with four wavefronts per stream publishes the same bits as
with one (the per-stream kernels' arithmetic does not depend on the workgroup size), and (b) without msg_stream passes at three streams
(the copy still finds the finished message there).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = dict(grid_row=4, grid_col=5, grid_min_feature_num=3, grid_max_feature_num=15)      # bench.py's grid: 300 features per frame
N_FRAMES = 26                                                                              # past the first camera-state prune (20 states)
OVERRIDES = ('AV_DK_WG', 'AV_MSCKF_GROUPS', 'AV_MSCKF_STORE')


def _no_override(monkeypatch):
    for name in OVERRIDES:
        monkeypatch.delenv(name, raising=False)


# ---- references ------------------------------------------------------------------------------------------------------------------
def _snapshot(flt, res):
    """What the filter checks below read of an OracleMSCKF right after its feature_callback returned `res`."""
    s = flt.imu_state
    cams = list(flt.cam_states.values())
    return dict(pub=res is not None, p=s.position.copy(), q=s.orientation.copy(), v=s.velocity.copy(), bg=s.gyro_bias.copy(),
                ba=s.acc_bias.copy(), R_ic=np.array(s.R_imu_cam0), t_ci=np.array(s.t_cam0_imu), cam_ids=list(flt.cam_states.keys()),
                cam_q=np.array([c.orientation for c in cams]).reshape(-1, 4), cam_p=np.array([c.position for c in cams]).reshape(-1, 3),
                sizes=(flt.state_cov.shape[0], len(flt.cam_states), len(flt.map_server)))


@pytest.fixture(scope='module')
def rendered():
    """Three rendered 752 x 480 streams of 26 frames and, computed once and never changed, what the CPU oracles make of each:
    per frame the feature message (ids, uv) of OracleFrontend and the snapshot of an OracleMSCKF fed that message, and the
    covariance after the last frame."""
    from fe_harness import Frames
    from oracle.frontend import OracleFrontend
    from oracle.msckf_np import OracleMSCKF
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream, replay
    from concurrent.futures import ThreadPoolExecutor
    cfg = ConfigEuRoC(**GRID)

    def one(u):
        st = Frames.cached(SyntheticStream(cfg, seed=900 + u, n_frames=N_FRAMES))
        fe, flt, rows = OracleFrontend(cfg), OracleMSCKF(cfg), []

        def on_frame(m):
            msg = fe.stereo_callback(m)
            ids = np.array([f.id for f in msg.features], np.int64)
            uv = np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features], np.float64).reshape(-1, 4)
            rows.append(dict(_snapshot(flt, flt.feature_callback(msg)), ids=ids, uv=uv))
        replay(st, [fe.imu_callback, flt.imu_callback], on_frame)
        return st, dict(frames=rows, cov=flt.state_cov.copy())
    with ThreadPoolExecutor(3) as pool:          # the streams are independent; the renderer and both oracles spend their time in NumPy and C
        done = list(pool.map(one, range(3)))
    return cfg, [st for st, _ref in done], [ref for _st, ref in done]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _imu_rows(streams, n_frames, S):
    """Per frame (stream index int32[n], t[n], gyro[n,3], acc[n,3]) for S streams, stream s being a replica of streams[s % U]: every
    sample newer than the previous frame and not newer than this one (synth.replay's rule), built per original and tiled."""
    U = len(streams)
    tab = [(np.array([m.timestamp for m in st.imu]), np.array([m.angular_velocity for m in st.imu]).reshape(-1, 3),
            np.array([m.linear_acceleration for m in st.imu]).reshape(-1, 3)) for st in streams]
    rows = []
    for k in range(n_frames):
        idx, t, w, a = [], [], [], []
        for u, st in enumerate(streams):
            T, W, A = tab[u]
            sel = (T <= st.frame(k).timestamp) & ((T > st.frame(k - 1).timestamp) if k else True)
            reps = np.arange(u, S, U, dtype=np.int32)
            idx.append(np.repeat(reps, int(sel.sum()))); t.append(np.tile(T[sel], len(reps)))
            w.append(np.tile(W[sel], (len(reps), 1))); a.append(np.tile(A[sel], (len(reps), 1)))
        rows.append((np.concatenate(idx), np.concatenate(t), np.concatenate(w), np.concatenate(a)))
    return rows


def _frame_times(streams, n_frames, S):
    U = len(streams)
    return [np.array([st.frame(k).timestamp for st in streams], np.float64)[np.arange(S) % U] for k in range(n_frames)]


def _resident(streams, n_frames):
    """frames(k) -> (cam0, cam1) cuda tensors [U,h,w] with every frame of the few streams resident."""
    import torch
    dev = [tuple(torch.from_numpy(np.stack([getattr(st.frame(k), name) for st in streams])).cuda() for name in ('cam0_image', 'cam1_image'))
           for k in range(n_frames)]
    return lambda k: dev[k]


class _Ring(object):
    """frames(k) for S replicas with at most three frames of the batch resident: a ring of three [S,h,w] tensors per camera, slot
    k % 3 filled on the current stream from the uploaded originals (orig[cam]: [F,U,h,w]; source[s] = the original replica s shows)
    when frame k is first asked for -- which the loop below does right before the prestage that first names it.  With
    AV_FE_INPUTS_PERSIST a frame stays alive until the next step's kernels are done and the fill is stream-ordered behind them, so
    frames k - 1, k and k + 1 are the ones in use."""

    def __init__(self, orig, source):
        import torch
        S = len(source)
        self.orig, self.source = orig, torch.from_numpy(np.asarray(source, np.int64)).cuda()
        self.slots = [tuple(torch.empty((S,) + tuple(o.shape[2:]), dtype=torch.uint8, device='cuda') for o in orig) for _ in range(3)]
        self.holds = [None, None, None]

    def __call__(self, k):
        import torch
        if self.holds[k % 3] != k:
            for o, slot in zip(self.orig, self.slots[k % 3]):
                torch.index_select(o[k], 0, self.source, out=slot)
            self.holds[k % 3] = k
        return self.slots[k % 3]


# ---- the two loops ---------------------------------------------------------------------------------------------------------------
def _handover(cfg, S, frames, imu, ts, n_frames, read, msg_stream=True):
    """bench.py's run_device_handover, per frame k: eng.push_imu_batch, eng.step(frame k), eng.prestage(frame k + 1) if there is one,
    flt.push_imu, flt.submit_dev(msg_stream = the step's stream) issued under a second torch stream; no wait and no read-back inside
    the loop, one wait(0) after the last frame.  Returns (outputs [n_frames][S,12], read(eng, flt))."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    eng = FrontendEngine(cfg, n_streams=S, inputs_persist=True)
    flt = None
    try:
        flt = BatchedMSCKF(cfg, S, max_features=eng.max_features)
        assert flt.device_resident()
        side = torch.cuda.Stream()
        outs = []
        for k in range(n_frames):
            i, t, w, a = imu[k]
            eng.push_imu_batch(i, t, w)
            eng.step(*frames(k), ts[k])
            if k + 1 < n_frames:
                eng.prestage(*frames(k + 1))
            flt.push_imu(i, t, w, a)
            ms = N.current_stream()
            with torch.cuda.stream(side):
                outs.append(flt.submit_dev(eng, ts[k], msg_stream=ms if msg_stream else None))
        flt.wait(0)
        return outs, read(eng, flt)
    finally:
        if flt is not None:
            flt.close()
        eng.close()


def _last_features(eng):
    ids, uv, n = eng.read_features_raw()
    return ids.copy(), uv.copy(), n.copy()


def _state_bits(flt, s):
    """get_state and get_cov of stream s as one list of arrays, for bit-for-bit comparisons."""
    gs = flt.get_state(s)
    return [np.atleast_1d(np.asarray(gs[key])) for key in sorted(gs)] + [flt.get_cov(s)]


def _same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check_filter(out_row, sizes, gs, ref, where):
    """One stream's step output, sizes and get_state against the oracle's snapshot of the same frame: the tolerances of
    test_batched_filters_match_reference_golden_and_oracle."""
    assert bool(out_row[0] > 0.5) == ref['pub'] and out_row[0] >= 0, (where, out_row[0])
    assert tuple(sizes) == ref['sizes'], (where, sizes, ref['sizes'])
    err = max(np.abs(out_row[2:5] - ref['p']).max(), np.abs(out_row[5:9] - ref['q']).max(), np.abs(out_row[9:12] - ref['v']).max())
    assert err < 1e-6, (where, err)
    err = max(np.abs(gs['p'] - ref['p']).max(), np.abs(gs['q'] - ref['q']).max(), np.abs(gs['v'] - ref['v']).max())
    assert err < 1e-6, (where, err)
    assert np.abs(gs['bg'] - ref['bg']).max() < 1e-7 and np.abs(gs['ba'] - ref['ba']).max() < 1e-6, where
    assert np.abs(gs['R_ic'] - ref['R_ic']).max() < 1e-6 and np.abs(gs['t_ci'] - ref['t_ci']).max() < 1e-6, where
    assert list(gs['cam_ids']) == ref['cam_ids'], (where, list(gs['cam_ids']), ref['cam_ids'])
    if ref['cam_ids']:
        assert np.abs(gs['cam_q'] - ref['cam_q']).max() < 1e-6 and np.abs(gs['cam_p'] - ref['cam_p']).max() < 1e-6, where


def _check_cov(P, Po, where):
    assert P.shape == Po.shape and np.abs(P - Po).max() <= 1e-6 * np.abs(Po).max(), (where, np.abs(P - Po).max(), np.abs(Po).max())


def _synchronous(cfg, streams, refs, imu, ts, frames, shape):
    """The few streams one frame at a time -- step, read_features_raw, flt.step -- with every frame's features bit for bit against
    OracleFrontend and every frame's filter output, sizes and get_state (and the covariance at the end) against OracleMSCKF.
    Returns the filter outputs."""
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    U = len(streams)
    eng = FrontendEngine(cfg, n_streams=U, inputs_persist=True)
    flt = None
    try:
        flt = BatchedMSCKF(cfg, U, max_features=eng.max_features)
        outs = []
        for k in range(N_FRAMES):
            i, t, w, a = imu[k]
            eng.push_imu_batch(i, t, w)
            eng.step(*frames(k), ts[k])
            ids, uv, n = eng.read_features_raw()
            for u in range(U):
                r, m = refs[u]['frames'][k], int(n[u])
                assert m == len(r['ids']) and m > 20, (k, u, m, len(r['ids']))
                assert np.array_equal(ids[u, :m], r['ids']), (k, u)
                assert np.array_equal(uv[u, :m].view(np.uint64), r['uv'].view(np.uint64)), (k, u)
            flt.push_imu(i, t, w, a)
            out = flt.step(ids, uv, n, ts[k])
            for u in range(U):
                _check_filter(out[u], flt.sizes(u), flt.get_state(u), refs[u]['frames'][k], ('synchronous', k, u))
            outs.append(out)
        for u in range(U):
            _check_cov(flt.get_cov(u), refs[u]['cov'], ('synchronous', u))
        assert flt.launch_shape() == shape
        assert flt.counters()['prune_stream_steps'] > 0, 'no stream reached its first camera-state prune'
        return outs
    finally:
        if flt is not None:
            flt.close()
        eng.close()


def _small_run(cfg, streams, refs, shape):
    """The hand-over loop over the few streams under the environment of the caller, held to the oracles through the synchronous run of
    the same streams: that one is compared with OracleFrontend and OracleMSCKF on every frame, and the hand-over's filter outputs,
    final states and covariances must equal its outputs bit for bit (states and covariances are additionally within the oracle's
    tolerances by themselves).  Returns (outputs, last frame's features, [state bits per stream])."""
    U = len(streams)
    imu, ts, frames = _imu_rows(streams, N_FRAMES, U), _frame_times(streams, N_FRAMES, U), _resident(streams, N_FRAMES)
    sync = _synchronous(cfg, streams, refs, imu, ts, frames, shape)

    def read(eng, flt):
        assert flt.launch_shape() == shape, flt.launch_shape()
        assert all(flt.stream_status(u) == (0, '') for u in range(U))
        for u in range(U):
            _check_cov(flt.get_cov(u), refs[u]['cov'], ('hand-over', u))
        return _last_features(eng), [_state_bits(flt, u) for u in range(U)]
    outs, (feats, states) = _handover(cfg, U, frames, imu, ts, N_FRAMES, read)
    for k in range(N_FRAMES):
        assert np.array_equal(outs[k].view(np.uint64), sync[k].view(np.uint64)), (k, np.abs(outs[k] - sync[k]).max())
    ids, uv, n = feats
    for u in range(U):
        r = refs[u]['frames'][-1]
        assert int(n[u]) == len(r['ids']) and np.array_equal(ids[u, :n[u]], r['ids']) and np.array_equal(uv[u, :n[u]].view(np.uint64), r['uv'].view(np.uint64)), u
    assert sum(bool(o[0, 0] > 0.5) for o in outs) > 5, 'the filters must have published'
    return outs, feats, states


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,wg,shape', [(1023, None, [(1023, 256)]), (1024, None, [(512, 256), (512, 256)]),
                                        (2047, None, [(1024, 64), (1023, 256)]), (2048, None, [(1024, 64), (1024, 64)]),
                                        (3, '64', [(3, 64)])])
def test_launch_shape_table(cfg, monkeypatch, S, wg, shape):
    """The groups and the workgroup size of the per-stream kernels are chosen per group: two groups from 1,024 streams of the batch up,
    one wavefront per stream from 1,024 streams of the GROUP up.  av_msckf_batch_launch_shape reports what dev_enqueue launched (0
    before the first step), after one step with an empty message."""
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    _no_override(monkeypatch)
    if wg:
        monkeypatch.setenv('AV_DK_WG', wg)
    flt = BatchedMSCKF(cfg, S, max_features=8)
    try:
        assert flt.device_resident()
        assert flt.launch_shape() == [(n, 0) for n, _wg in shape]
        idx = np.arange(S, dtype=np.int32)
        flt.push_imu(idx, np.full(S, 99.9), np.zeros((S, 3)), np.tile([0.0, 0.0, 9.81], (S, 1)))
        out = flt.submit(np.zeros((S, 8), np.int64), np.zeros((S, 8, 4)), np.zeros(S, np.int32), np.full(S, 100.0))
        flt.wait(0)
        assert flt.launch_shape() == shape
        assert not out[:, 0].any()                          # one IMU sample: no stream is initialised, none publishes, none failed
    finally:
        flt.close()


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def test_two_group_device_handover(rendered, monkeypatch):
    """The group branch of av_msckf_batch_submit_dev at its smallest shape: three rendered streams in two groups of 2 + 1 (the
    message split at an uneven, non-zero stream offset, one event shared by both groups, jobs handed to the group workers),
    one wavefront per stream, in bench.py's order with no read-back inside the loop."""
    cfg, streams, refs = rendered
    _no_override(monkeypatch)
    monkeypatch.setenv('AV_MSCKF_GROUPS', '2')
    monkeypatch.setenv('AV_DK_WG', '64')
    _small_run(cfg, streams, refs, [(2, 64), (1, 64)])


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_filter_alone_at_2048_streams(cfg, monkeypatch):
    """The batched filter by itself at the headline's stream count, no override: replicas s % 3 of three feature streams of different
    loads, so both groups hold all three.  Stepped with submit + wait(1) as bench.py's queued path does; the state accessors need a
    drained queue, so every frame is drained before they are read."""
    from oracle.msckf_np import OracleMSCKF
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticFeatureStream
    _no_override(monkeypatch)
    S, F, cap = 2048, 60, 160
    streams = [SyntheticFeatureStream(cfg, seed=0, n_frames=F, n_features=100),
               SyntheticFeatureStream(cfg, seed=21, n_frames=F, n_features=60, motion_scale=1.5),
               SyntheticFeatureStream(cfg, seed=22, n_frames=F, n_features=140)]
    U = len(streams)
    rep = np.arange(S) % U
    watch = [0, 1, 2, 1023, 1024, 2045, 2046, 2047]
    imu = _imu_rows(streams, F, S)
    oras = [OracleMSCKF(cfg) for _ in streams]
    its = [iter(st.imu) for st in streams]
    pend = [next(it, None) for it in its]
    flt = BatchedMSCKF(cfg, S, max_features=cap)
    try:
        published = 0
        for k in range(F):
            msgs = [st.frame(k) for st in streams]
            ids3 = np.zeros((U, cap), np.int64); uv3 = np.zeros((U, cap, 4)); n3 = np.zeros(U, np.int32)
            for u, m in enumerate(msgs):
                n3[u] = len(m.features)
                ids3[u, :n3[u]] = [f.id for f in m.features]
                uv3[u, :n3[u]] = [(f.u0, f.v0, f.u1, f.v1) for f in m.features]
            t3 = np.array([m.timestamp for m in msgs])
            flt.push_imu(*imu[k])
            out = flt.submit(ids3[rep], uv3[rep], n3[rep], t3[rep])
            flt.wait(1)
            snaps = []
            for u, m in enumerate(msgs):
                while pend[u] is not None and pend[u].timestamp <= m.timestamp:
                    oras[u].imu_callback(pend[u]); pend[u] = next(its[u], None)
                snaps.append(_snapshot(oras[u], oras[u].feature_callback(m)))
            flt.wait(0)
            assert np.array_equal(out.view(np.uint64), out[:U][rep].view(np.uint64)), (k, np.nonzero((out != out[:U][rep]).any(axis=1))[0][:8])
            for s in watch:
                _check_filter(out[s], flt.sizes(s), flt.get_state(s), snaps[s % U], (k, s))
            published += int(out[0, 0] > 0.5)
        assert published > 40
        assert flt.launch_shape() == [(1024, 64), (1024, 64)]
        bad = [(s, st) for s, st in ((s, flt.stream_status(s)) for s in range(S)) if st != (0, '')]
        assert not bad, bad[:4]
        for s in watch:
            _check_cov(flt.get_cov(s), oras[s % U].state_cov, s)
        c = flt.counters()
        assert c['prune_stream_steps'] > 0, c          # (two_pass_streams in c: > 0 means the groups' shared overflow pools were in play)
        print('filter alone at %d streams: %s' % (S, c))
    finally:
        flt.close()


# ---- (d) -------------------------------------------------------------------------------------------------------------------------
def test_complete_path_at_2048_streams(rendered, monkeypatch):
    """bench.py's default configuration end to end, no override: 2,048 replicas s % 2 of two rendered streams through
    FrontendEngine(inputs_persist) + prestage + submit_dev in run_device_handover's order.  Every replica must publish bit for bit
    what its original publishes, streams 0 and 1 what a 2-stream run of the same loop publishes (AV_DK_WG=64: the same kernels), and
    that run is held to OracleFrontend and OracleMSCKF by _small_run."""
    import torch
    cfg, streams, refs = rendered
    U, S = 2, 2048
    streams, refs = streams[:U], refs[:U]
    _no_override(monkeypatch)
    monkeypatch.setenv('AV_DK_WG', '64')
    small, small_feats, small_states = _small_run(cfg, streams, refs, [(2, 64)])
    monkeypatch.delenv('AV_DK_WG')

    rep = np.arange(S) % U
    watch = [0, 1, 1023, 1024, 2046, 2047]
    orig = [torch.from_numpy(np.stack([np.stack([getattr(st.frame(k), name) for st in streams]) for k in range(N_FRAMES)])).cuda()
            for name in ('cam0_image', 'cam1_image')]

    def read(eng, flt):
        assert flt.launch_shape() == [(1024, 64), (1024, 64)], flt.launch_shape()
        bad = [(s, st) for s, st in ((s, flt.stream_status(s)) for s in range(S)) if st != (0, '')]
        assert not bad, bad[:4]
        return _last_features(eng), {s: _state_bits(flt, s) for s in watch}, flt.counters()
    outs, (feats, states, counters) = _handover(cfg, S, _Ring(orig, rep), _imu_rows(streams, N_FRAMES, S), _frame_times(streams, N_FRAMES, S),
                                                N_FRAMES, read)
    for k in range(N_FRAMES):
        o = outs[k]
        assert np.array_equal(o.view(np.uint64), o[:U][rep].view(np.uint64)), (k, np.nonzero((o != o[:U][rep]).any(axis=1))[0][:8])
        assert np.array_equal(o[:U].view(np.uint64), small[k].view(np.uint64)), (k, np.abs(o[:U] - small[k]).max())
    ids, uv, n = feats
    assert np.array_equal(n, n[:U][rep]), np.nonzero(n != n[:U][rep])[0][:8]
    for u in range(U):
        m = int(n[u])
        assert np.array_equal(ids[u::U, :m], np.broadcast_to(ids[u, :m], ids[u::U, :m].shape)), u
        assert np.array_equal(uv[u::U, :m].view(np.uint64), np.broadcast_to(uv[u, :m].view(np.uint64), uv[u::U, :m].shape)), u
        assert m == int(small_feats[2][u]) and np.array_equal(ids[u, :m], small_feats[0][u, :m]), u
        assert np.array_equal(uv[u, :m].view(np.uint64), small_feats[1][u, :m].view(np.uint64)), u
    for s in watch:
        assert _same_bits(states[s], states[s % U]), s
    for u in range(U):
        assert _same_bits(states[u], small_states[u]), u
    assert counters['prune_stream_steps'] > 0, counters
    print('complete path at %d streams: %s' % (S, counters))
