"""config.use_ransac through the drop-in stage classes and through the filter."""
import os
import sys
from collections import defaultdict

import numpy as np
import pytest

from conftest import ROOT
from fe_harness import Frames, make_cfg as _cfg, read_ransac_counts, run_engine
from ransac_helpers import STREAM

pytestmark = pytest.mark.gpu


def _dropin():
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    return ip


def _stage_pipeline(cfg, stream):
    """The reference's stage classes wired as src/image_processing/pipeline.py:46-150 wires them (tests/test_gpu_stages.py), the
    tracker built with the switch's arguments.  Returns per frame (ids, after_matching, after_ransac)."""
    ip = _dropin()
    imu = ip.IMUProcessor(cfg.T_imu_cam0, cfg.T_imu_cam1)
    detector = ip.FastFeatureDetector_create(cfg.fast_threshold)
    cam = ip.CameraModel(cfg.cam0_intrinsics, cfg.cam0_distortion_model, cfg.cam0_distortion_coeffs)
    state = dict(next_id=0, prev=[[] for _ in range(cfg.grid_num)], first=True, prev_msg=None, prev_pyr=None, frame=0)
    out = []

    def on_frame(msg):
        imu.cam0_prev_img_msg, imu.cam0_curr_img_msg = state['prev_msg'], msg.cam0_msg
        curr = [[] for _ in range(cfg.grid_num)]
        num = defaultdict(int)
        pb = ip.PyramidBuilder(cfg.win_size, cfg.pyramid_levels, msg.cam0_msg, msg.cam1_msg)
        pyr0, _pyr1 = pb.create_image_pyramids()
        sm = ip.StereoMatcher(cfg.lk_params, imu, pb, cam, cfg.stereo_threshold)
        if state['first']:
            init = ip.FeatureInitializer(detector=detector, stereo_matcher=sm, config=cfg, cam0_curr_img_msg=msg.cam0_msg,
                                         curr_features=curr, next_feature_id=state['next_id'], grid_row=cfg.grid_row,
                                         grid_col=cfg.grid_col, grid_min_feature_num=cfg.grid_min_feature_num)
            init.initialize_first_frame()
            state['next_id'], state['first'] = init.next_feature_id, False
        else:
            tr = ip.FeatureTracker(lk_params=cfg.lk_params, imu_processor=imu, stereo_matcher=sm,
                                   cam0_intrinsics=cfg.cam0_intrinsics, cam0_distortion_model=cfg.cam0_distortion_model,
                                   cam0_distortion_coeffs=cfg.cam0_distortion_coeffs, cam1_intrinsics=cfg.cam1_intrinsics,
                                   cam1_distortion_model=cfg.cam1_distortion_model, cam1_distortion_coeffs=cfg.cam1_distortion_coeffs,
                                   prev_cam0_pyramid=state['prev_pyr'], curr_cam0_pyramid=pyr0, prev_features=state['prev'],
                                   curr_features=curr, num_features=num, grid_row=cfg.grid_row, grid_col=cfg.grid_col,
                                   ransac_threshold=cfg.ransac_threshold, use_ransac=cfg.use_ransac,
                                   ransac_success_probability=cfg.ransac_success_probability, ransac_seed=cfg.ransac_seed,
                                   frame_number=state['frame'])
            tr.track_features()
            ad = ip.FeatureAdder(detector=detector, stereo_matcher=sm, config=cfg, cam0_curr_img_msg=msg.cam0_msg, curr_features=curr,
                                 next_feature_id=state['next_id'], grid_row=cfg.grid_row, grid_col=cfg.grid_col,
                                 grid_max_feature_num=cfg.grid_max_feature_num, grid_min_feature_num=cfg.grid_min_feature_num)
            ad.add_new_features()
            state['next_id'] = ad.next_feature_id
            pr = ip.FeaturePruner(cfg.grid_max_feature_num)
            pr.curr_features, pr.config = curr, cfg
            pr.prune_features()
            curr = pr.curr_features
        pub = ip.FeaturePublisher(cfg.cam0_intrinsics, cfg.cam0_distortion_model, cfg.cam0_distortion_coeffs,
                                  cfg.cam1_intrinsics, cfg.cam1_distortion_model, cfg.cam1_distortion_coeffs)
        pub.cam0_curr_img_msg, pub.cam1_curr_img_msg, pub.curr_features = msg.cam0_msg, msg.cam1_msg, curr
        fm = pub.publish()
        state['prev_msg'], state['prev'], state['prev_pyr'] = msg.cam0_msg, curr, pyr0
        state['frame'] += 1
        out.append((np.array([f.id for f in fm.features], np.int64), num['after_matching'], num['after_ransac']))
    from uav_airvision_amd.synth import replay
    replay(stream, [imu.imu_callback], on_frame)
    return out


def test_stage_tracker_with_ransac_gives_the_engines_ids_and_counts():
    from uav_airvision_amd.synth import SyntheticStream
    cfg = _cfg(use_ransac=True)
    st = Frames.cached(SyntheticStream(cfg, **dict(STREAM, n_frames=10)))
    eng = run_engine(cfg, [st], read=read_ransac_counts)[0]
    got = _stage_pipeline(cfg, st)
    assert any(g[2] < g[1] for g in got)
    for k, ((ids, am, ar), (ids_e, _uv, cnt, rc)) in enumerate(zip(got, eng)):
        assert np.array_equal(ids, ids_e), k
        if k > 0:
            assert am == cnt['after_matching'] and ar == rc['after_ransac'], (k, am, ar, cnt, rc)
    # the engine-backed drop-in reports the engine's count where it used to copy after_matching
    ip = _dropin()
    proc = ip.ImageProcessor(cfg)
    from uav_airvision_amd.synth import replay
    seen = []
    replay(st, [proc.imu_callback], lambda m: (proc.stereo_callback(m), seen.append(dict(proc.num_features))))
    proc.close()
    assert [s['after_ransac'] for s in seen[1:]] == [g[2] for g in got[1:]]


def test_front_end_with_ransac_feeds_the_filter():
    """Front-end + BatchedMSCKF on the moving-region stream, RANSAC on: the stream stays active and its poses finite.  The ATE
    against the synthetic truth, switch on and off, is printed (recorded in DESIGN.md), not asserted."""
    from uav_airvision_amd.evaluate import ate
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    st = Frames.cached(SyntheticStream(_cfg(), **dict(STREAM, n_frames=60)))
    res = {}
    for on in (True, False):
        cfg = _cfg(use_ransac=on)
        eng = FrontendEngine(cfg, n_streams=1)
        flt = BatchedMSCKF(cfg, 1, max_features=eng.max_features)
        it = iter(st.imu)
        pend = next(it, None)
        traj = []
        for k in range(st.n_frames):
            m = st.frame(k)
            while pend is not None and pend.timestamp <= m.timestamp:
                eng.push_imu(0, pend.timestamp, pend.angular_velocity)
                flt.push_imu([0], [pend.timestamp], [pend.angular_velocity], [pend.linear_acceleration])
                pend = next(it, None)
            eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
            ids, uv, n = eng.read_features_raw()
            out = flt.step(ids, uv, n, [m.timestamp])
            assert out[0, 0] >= 0, 'the filter stopped the stream at frame %d' % k
            assert np.isfinite(out[0]).all(), k
            if out[0, 0] > 0.5:
                traj.append(out[0, 1:5].copy())
        eng.close(); flt.close()
        assert len(traj) >= 40
        traj = np.array(traj)
        gt = np.array([[t] + list(st.position(t)) for t in traj[:, 0]])
        res[on] = ate(traj, gt)['rmse']
    print('ATE rmse over %d frames: RANSAC on %.4f m, off %.4f m' % (st.n_frames, res[True], res[False]))
