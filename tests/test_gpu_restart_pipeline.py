"""Stream restart through the complete path (include/airvision.h, "Stream restart"): a front-end engine whose feature message goes to
the batched filter on the device (`submit_dev`), two rendered streams, and a restart of BOTH halves of stream 1 in the middle of the run,
after which it is fed another rendered stream from its first IMU sample.
  * stream 0 -- features and published poses -- equals the uninterrupted run bit for bit;
  * stream 1's second life equals that of a fresh engine + filter pair fed the same life from step 0 beside the same stream 0;
as one FrontendEngine + BatchedMSCKF, as EngineSet + FilterSet with two parts (stream 1 is the second part's), and through the drop-in
pair ImageProcessor + MSCKF.  The second life is long enough to fill the window and prune."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from fe_harness import Frames

pytestmark = pytest.mark.gpu

N1, N2 = 10, 24             # frames before the restart, frames of the second life (the window holds 20 camera states)

_STREAMS = {}


def _streams(cfg):
    if 'all' not in _STREAMS:
        from uav_airvision_amd.synth import SyntheticStream
        _STREAMS['all'] = (Frames.cached(SyntheticStream(cfg, seed=21, n_frames=N1 + N2)), Frames.cached(SyntheticStream(cfg, seed=22, n_frames=N1 + N2)),
                           Frames.cached(SyntheticStream(cfg, seed=23, n_frames=N2)))
    return _STREAMS['all']


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(cfg, plan, n_steps, parts):
    """plan: per slot [(first step, Frames, frames)], a frame for every slot in every step.  parts = 1: FrontendEngine + BatchedMSCKF;
    2: EngineSet + FilterSet.  A life that begins at a step > 0 is preceded by the restart of both halves of its slot.  Returns per step
    the features of every stream and the [S, 12] pose array, and the generation counts of both halves at the end."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.pipelines import EngineSet, FilterSet
    S = len(plan)
    eng = flt = None
    try:
        if parts > 1:
            eng = EngineSet(cfg, S, parts)
            flt = FilterSet(cfg, eng, max_features=eng.max_features)
        else:
            eng = FrontendEngine(cfg, n_streams=S)
            flt = BatchedMSCKF(cfg, S, max_features=eng.max_features)
        assert flt.device_resident()

        def life(i, k):
            for first, fr, n in plan[i]:
                if first <= k < first + n:
                    return first, fr
            raise AssertionError((i, k))
        imu, feats, outs = {}, [], []
        for k in range(n_steps):
            begin = [i for i in range(S) if life(i, k)[0] == k and k > 0]
            if begin:
                eng.restart(begin)
                flt.restart(begin)
            ms = [life(i, k)[1].frame(k - life(i, k)[0]) for i in range(S)]
            ts = np.array([m.timestamp for m in ms])
            idx, t, w, a = [], [], [], []
            for i in range(S):
                first, fr = life(i, k)
                if (i, first) not in imu:
                    it = iter(fr.imu)
                    imu[i, first] = [it, next(it, None)]
                st = imu[i, first]
                while st[1] is not None and st[1].timestamp <= ts[i]:
                    idx.append(i); t.append(st[1].timestamp); w.append(st[1].angular_velocity); a.append(st[1].linear_acceleration)
                    st[1] = next(st[0], None)
            if idx:
                eng.push_imu_batch(np.array(idx, np.int32), np.array(t), np.array(w).reshape(-1, 3))
                flt.push_imu(np.array(idx, np.int32), np.array(t), np.array(w).reshape(-1, 3), np.array(a).reshape(-1, 3))
            eng.step(torch.from_numpy(np.stack([m.cam0_image for m in ms])).cuda(), torch.from_numpy(np.stack([m.cam1_image for m in ms])).cuda(), list(ts))
            outs.append(flt.submit_dev(eng, ts, msg_stream=N.current_stream()))
            feats.append(eng.read_features())
        flt.wait(0)
        poses = [o.array() if hasattr(o, 'array') else np.array(o) for o in outs]
        gen = (np.asarray(eng.generation).tolist(), np.asarray(flt.generation).tolist())
        return dict(feats=feats, poses=poses, generation=gen)
    finally:
        if flt is not None:
            flt.close()
        if eng is not None:
            eng.close()


def _same_stream(x, kx, sx, y, ky, sy):
    (ia, ua), (ib, ub) = x['feats'][kx][sx], y['feats'][ky][sy]
    return np.array_equal(ia, ib) and np.array_equal(ua.view(np.uint64), ub.view(np.uint64)) and _bits(x['poses'][kx][sx], y['poses'][ky][sy])


@pytest.mark.parametrize('parts', [1, 2])
def test_both_halves_of_a_stream_restart_mid_run(cfg, parts):
    s0, s1, s2 = _streams(cfg)
    n = N1 + N2
    a = _run(cfg, [[(0, s0, n)], [(0, s1, n)]], n, parts)
    b = _run(cfg, [[(0, s0, n)], [(0, s1, N1), (N1, s2, N2)]], n, parts)
    c = _run(cfg, [[(0, s0, N2)], [(0, s2, N2)]], N2, parts)
    assert b['generation'] == ([0, 1], [0, 1]) and a['generation'] == ([0, 0], [0, 0])
    for k in range(n):
        assert _same_stream(b, k, 0, a, k, 0), 'stream 0 differs from the uninterrupted run at step %d' % k
        if k < N1:
            assert _same_stream(b, k, 1, a, k, 1), 'stream 1 differs before the restart at step %d' % k
    for j in range(N2):
        assert _same_stream(b, N1 + j, 1, c, j, 1), "stream 1's second life differs from a fresh pair's at frame %d" % j
    pub = [j for j in range(N2) if b['poses'][N1 + j][1, 0] == 1.0]
    assert len(pub) >= 15 and b['poses'][N1][1, 0] >= 0.0, pub
    assert sorted(b['feats'][N1][1][0].tolist()) == list(range(len(b['feats'][N1][1][0])))      # ids begin again at 0


def test_the_drop_in_pair_restarts(cfg):
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    from msckf import MSCKF
    from uav_airvision_amd.synth import replay
    _, s1, s2 = _streams(cfg)

    def feed(proc, flt, stream, n):
        got = []

        def on_frame(m):
            fm = proc.stereo_callback(m)
            r = flt.feature_callback(fm)
            ids = np.array([f.id for f in fm.features], np.int64)
            uv = np.array([[f.u0, f.v0, f.u1, f.v1] for f in fm.features], np.float64).reshape(-1, 4)
            pose = None if r is None else np.concatenate([[r.timestamp], r.pose.t, r.pose.R.reshape(-1), r.velocity, r.cam0_pose.t, r.cam0_pose.R.reshape(-1)])
            got.append((ids, uv, pose))

        class Head(object):
            imu, frame, n_frames = stream.imu, staticmethod(stream.frame), n
        replay(Head, [proc.imu_callback, flt.imu_callback], on_frame)
        return got

    def pair():
        return ip.ImageProcessor(cfg), MSCKF(cfg, write_trajectory=False)
    proc, flt = pair()
    try:
        feed(proc, flt, s1, N1)
        assert flt.is_gravity_set and not proc.first_frame and (proc.generation, flt.generation) == (0, 0)
        proc.restart(); flt.restart()
        assert not flt.is_gravity_set and proc.first_frame and (proc.generation, flt.generation) == (1, 1)
        assert len(flt.map_server) == 0 and len(flt.state_server.cam_states) == 0 and proc.next_feature_id == 0
        second = feed(proc, flt, s2, N2)
    finally:
        proc.close(); flt.close()
    proc, flt = pair()
    try:
        fresh = feed(proc, flt, s2, N2)
    finally:
        proc.close(); flt.close()
    n_pub = 0
    for j, ((ia, ua, pa), (ib, ub, pb)) in enumerate(zip(second, fresh)):
        assert np.array_equal(ia, ib) and np.array_equal(ua.view(np.uint64), ub.view(np.uint64)), j
        assert (pa is None) == (pb is None) and (pa is None or _bits(pa, pb)), j
        n_pub += pa is not None
    assert n_pub >= 15, n_pub
