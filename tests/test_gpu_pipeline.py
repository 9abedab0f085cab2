"""Whole hot path on the GPU: images -> HIP front-end -> HIP MSCKF, through the drop-in classes and
with the reference's three-thread call pattern (modules/vio.py:17-53), against the all-CPU oracle
pipeline (oracle front-end + numpy MSCKF) on the same seeded stream."""
import os
import sys
from queue import Queue
from threading import Thread

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dropin_path():
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    return d


def _oracle_run(cfg, st):
    from oracle.frontend import OracleFrontend
    from oracle.msckf_np import OracleMSCKF
    from uav_airvision_amd.synth import replay
    fe, flt = OracleFrontend(cfg), OracleMSCKF(cfg)
    out = []

    def on_frame(m):
        feat = fe.stereo_callback(m)
        res = flt.feature_callback(feat)
        out.append(None if res is None else (res.timestamp, res.pose.t.copy(), res.pose.R.copy(), res.cam0_pose.t.copy()))
    replay(st, [fe.imu_callback, flt.imu_callback], on_frame)
    return out


def test_sequential_replay_matches_oracle_pipeline(cfg, dropin_path):
    from image_processing import ImageProcessor
    from msckf import MSCKF
    from uav_airvision_amd.synth import SyntheticStream, replay
    st = SyntheticStream(cfg, seed=4, n_frames=30, motion_scale=1.5)
    ref = _oracle_run(cfg, st)
    ip, flt = ImageProcessor(cfg), MSCKF(cfg, write_trajectory=False)
    got = []

    def on_frame(m):
        feat = ip.stereo_callback(m)
        res = flt.feature_callback(feat)
        got.append(None if res is None else (res.timestamp, res.pose.t.copy(), res.pose.R.copy(), res.cam0_pose.t.copy()))
    replay(st, [ip.imu_callback, flt.imu_callback], on_frame)
    assert len(got) == len(ref) == 30 and all(g is not None for g in got)
    for g, r in zip(got, ref):
        assert g[0] == r[0]
        assert np.abs(g[1] - r[1]).max() < 1e-7 and np.abs(g[2] - r[2]).max() < 1e-7 and np.abs(g[3] - r[3]).max() < 1e-7
    assert np.linalg.norm(ref[-1][1]) > 0.05            # the platform really moved
    ip.close(); flt.close()


def test_threaded_vio_call_pattern(cfg, dropin_path):
    """The reference's orchestration (three daemon threads, three queues, None sentinels) around the
    drop-in classes; with the IMU thread never starved the result equals the sequential replay."""
    from image_processing import ImageProcessor
    from msckf import MSCKF
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(cfg, seed=4, n_frames=12, motion_scale=1.5)
    ip, flt = ImageProcessor(cfg), MSCKF(cfg, write_trajectory=False)
    img_q, imu_q, feat_q, results = Queue(), Queue(), Queue(), []
    imu_done = []

    def t_img():
        while True:
            m = img_q.get()
            if m is None:
                feat_q.put(None); break
            feat = ip.stereo_callback(m)
            if feat:
                feat_q.put(feat)

    def t_imu():
        while True:
            m = imu_q.get()
            if m is None:
                break
            ip.imu_callback(m); flt.imu_callback(m)
            imu_done.append(m.timestamp)

    def t_vio():
        while True:
            f = feat_q.get()
            if f is None:
                break
            r = flt.feature_callback(f)
            if r:
                results.append(r)
    threads = [Thread(target=f, daemon=True) for f in (t_img, t_imu, t_vio)]
    for t in threads:
        t.start()
    it = iter(st.imu); pend = next(it, None)
    import time
    for k in range(st.n_frames):
        m = st.frame(k)
        last = None
        while pend is not None and pend.timestamp <= m.timestamp:
            imu_q.put(pend); last = pend.timestamp
            pend = next(it, None)
        while last is not None and (not imu_done or imu_done[-1] < last):
            time.sleep(0.001)                         # deterministic limit: IMU delivered before the frame
        img_q.put(m)
        while len(results) < k + 1:
            time.sleep(0.001)
    img_q.put(None); imu_q.put(None)
    for t in threads:
        t.join(timeout=30)
    ref = _oracle_run(cfg, st)
    assert len(results) == 12
    for r, o in zip(results, ref):
        assert np.abs(r.pose.t - o[1]).max() < 1e-7
    ip.close(); flt.close()


def test_euroc_directory_through_sweep_runner(cfg, tmp_path):
    """EuRoC-layout directory (PNG + CSV, written from the synthetic stream) -> reader ->
    deterministic replay -> GPU front-end + GPU filter -> trajectory -> ATE against the stream's truth."""
    from PIL import Image
    from uav_airvision_amd import evaluate
    from uav_airvision_amd.sweep import run_stream
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(cfg, seed=8, n_frames=60, motion_scale=1.5, t0=1403636580.0)
    root = str(tmp_path / 'SYN_01')
    for cam in ('cam0', 'cam1'):
        os.makedirs(os.path.join(root, 'mav0', cam, 'data'))
    for k in range(st.n_frames):
        m = st.frame(k)
        name = '%d.png' % int(round(m.timestamp * 1e9))
        Image.fromarray(m.cam0_image).save(os.path.join(root, 'mav0', 'cam0', 'data', name))
        Image.fromarray(m.cam1_image).save(os.path.join(root, 'mav0', 'cam1', 'data', name))
    os.makedirs(os.path.join(root, 'mav0', 'imu0'))
    with open(os.path.join(root, 'mav0', 'imu0', 'data.csv'), 'w') as f:
        f.write('#timestamp [ns],w_RS_S_x,w_RS_S_y,w_RS_S_z,a_RS_S_x,a_RS_S_y,a_RS_S_z\n')
        for m in st.imu:
            f.write('%d,%.12f,%.12f,%.12f,%.12f,%.12f,%.12f\n' % (int(round(m.timestamp * 1e9)), *m.angular_velocity, *m.linear_acceleration))
    os.makedirs(os.path.join(root, 'mav0', 'state_groundtruth_estimate0'))
    with open(os.path.join(root, 'mav0', 'state_groundtruth_estimate0', 'data.csv'), 'w') as f:
        f.write('#timestamp,p_RS_R,q_RS,v,bw,ba\n')
        for m in st.imu:
            p = st.position(m.timestamp)
            f.write(','.join(['%d' % int(round(m.timestamp * 1e9))] + ['%.9f' % v for v in p] + ['1', '0', '0', '0'] + ['0'] * 9) + '\n')
    traj, ds = run_stream(cfg, root, offset=0.0)
    assert len(traj) >= 40                                   # the first second of IMU is consumed by gravity initialisation
    a = evaluate.ate(traj, ds.groundtruth_array())
    assert a['rmse'] < 0.05, a
    assert np.linalg.norm(traj[-1, 1:4] - traj[0, 1:4]) > 0.2


def test_bench_scale_batch_is_stream_independent(dropin_path):
    """Size-independent property at the bench's shape (752x480, grid 4x5x15 = 300 features per frame, hundreds of streams
    per launch, filter in concurrent stream groups): every stream's result depends on that stream's inputs only.
    256 streams are replicas of 2 rendered streams; all replicas of one stream must publish bit-identical features and
    filter states, equal to those of a 2-stream batch, and the first frames must equal the CPU oracle."""
    import torch
    from oracle.frontend import OracleFrontend
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    cfg = ConfigEuRoC(grid_row=4, grid_col=5, grid_min_feature_num=3, grid_max_feature_num=15)
    U, n_frames = 2, 26                                  # 26 frames: past the first camera-state prune (20 states)
    streams = [SyntheticStream(cfg, seed=900 + u, n_frames=n_frames) for u in range(U)]
    frames = [[st.frame(k) for k in range(n_frames)] for st in streams]

    def run(S):
        dev = torch.device('cuda', 0)
        eng = FrontendEngine(cfg, n_streams=S, device=0)
        flt = BatchedMSCKF(cfg, S, device=0, rows_cap=4096)
        its = [iter(st.imu) for st in streams]
        pend = [next(it, None) for it in its]
        feats, poses = [], []
        for k in range(n_frames):
            idx, ts, gy, ac = [], [], [], []
            for u in range(U):
                tf = frames[u][k].timestamp
                batch = []
                while pend[u] is not None and pend[u].timestamp <= tf:
                    batch.append(pend[u]); pend[u] = next(its[u], None)
                for s in range(u, S, U):
                    for m in batch:
                        idx.append(s); ts.append(m.timestamp); gy.append(m.angular_velocity); ac.append(m.linear_acceleration)
            if idx:
                eng.push_imu_batch(np.array(idx, np.int32), np.array(ts), np.array(gy).reshape(-1, 3))
                flt.push_imu(idx, ts, gy, ac)
            img0 = torch.from_numpy(np.stack([frames[s % U][k].cam0_image for s in range(S)])).to(dev)
            img1 = torch.from_numpy(np.stack([frames[s % U][k].cam1_image for s in range(S)])).to(dev)
            eng.step(img0, img1, [frames[s % U][k].timestamp for s in range(S)])
            eng.read_features_begin(k & 1)
            ids, uv, n = eng.read_features_end(k & 1)
            feats.append((ids, uv, n))
            poses.append(flt.step(ids, uv, n, [frames[s % U][k].timestamp for s in range(S)]))
        eng.close(); flt.close()
        return feats, poses

    big_f, big_p = run(256)                                 # one stream group (device store: two groups only from 1,024 streams up), 256-wide kernels
    small_f, small_p = run(2)
    for k in range(n_frames):
        ids, uv, n = big_f[k]
        for s in range(256):
            u = s % U
            m = int(n[u])
            assert int(n[s]) == m, (k, s)
            assert np.array_equal(ids[s, :m], ids[u, :m]) and np.array_equal(uv[s, :m].view(np.uint64), uv[u, :m].view(np.uint64)), (k, s)
            assert np.array_equal(big_p[k][s].view(np.uint64), big_p[k][u].view(np.uint64)), (k, s)
        for u in range(U):
            m = int(n[u])
            assert int(small_f[k][2][u]) == m
            assert np.array_equal(small_f[k][0][u, :m], ids[u, :m]) and np.array_equal(small_f[k][1][u, :m].view(np.uint64), uv[u, :m].view(np.uint64))
            assert np.array_equal(small_p[k][u].view(np.uint64), big_p[k][u].view(np.uint64)), (k, u)
    assert any(p[0, 0] for p in big_p), 'the filters must have started publishing'
    # spot check against the CPU oracle front-end on the first frames of stream 0
    ora = OracleFrontend(cfg)
    it = iter(streams[0].imu); pend0 = next(it, None)
    for k in range(3):
        while pend0 is not None and pend0.timestamp <= frames[0][k].timestamp:
            ora.imu_callback(pend0); pend0 = next(it, None)
        ref = ora.stereo_callback(frames[0][k])
        m = int(big_f[k][2][0])
        assert m == len(ref.features)
        assert np.array_equal(big_f[k][0][0, :m], np.array([f.id for f in ref.features], np.int64))
        refuv = np.array([[f.u0, f.v0, f.u1, f.v1] for f in ref.features], np.float64).reshape(-1, 4)
        assert np.array_equal(big_f[k][1][0, :m].view(np.uint64), refuv.view(np.uint64))
