"""tests/ransac_helpers.py -- TEST INFRASTRUCTURE ONLY: what the RANSAC GPU tests share: the synthetic stream with an independently
moving region, and the CPU oracle front-end with the NumPy reference of tests/ransac_ref.py inserted where the engine runs its stage
(streams, runners and comparisons are those of tests/fe_harness.py)."""
import numpy as np

import ransac_ref as rr
from fe_harness import run_oracle
from oracle.frontend import (Feat, OracleFrontend, cell_of, cvops, grid_size, integrate_imu, predict_feature_tracking,
                             tracking_homography)

REGION = (250, 150, 500, 330)          # the independently moving rectangle of the synthetic stream (x0, y0, x1, y1)
STREAM = dict(seed=13, n_frames=26, motion_scale=3.0, moving_region=REGION, moving_amplitude=0.3)


class RansacOracle(OracleFrontend):
    """OracleFrontend with the reference RANSAC between the stereo match and the re-binning of FeatureTracker.track_features
    (feature_tracker.py:135-136 is the empty step), cam1_R_p_c kept, the stream's own frame number counted."""

    def __init__(self, config):
        OracleFrontend.__init__(self, config)
        self.frame_no = 0
        self.ransac_counts = [0, 0, 0, 0]
        self.margin = np.inf
        self.rejected = []                 # cam0 points (current frame) of the features the stage rejected in the last frame

    def stereo_callback(self, stereo_msg):
        self.ransac_counts, self.margin, self.rejected = [0, 0, 0, 0], np.inf, []
        msg = OracleFrontend.stereo_callback(self, stereo_msg)
        self.frame_no += 1
        return msg

    def _track(self, prev_img0, img0, img1, t_prev, t_curr):
        cfg = self.config
        gh, gw = grid_size(img0, cfg)
        R0, R1, self.imu_buffer = integrate_imu(self.imu_buffer, t_prev, t_curr, self.geom)
        prev = [f for cell in self.prev_features for f in cell]
        self.num_features['before_tracking'] = len(prev)
        if not prev:
            return
        prev_pts = np.array([f.cam0_point for f in prev], dtype=np.float32)
        H = tracking_homography(R0, cfg.cam0_intrinsics)
        pred = predict_feature_tracking(prev_pts, H)
        curr_pts, mask, _ = cvops.calc_optical_flow_pyr_lk(prev_img0, img0, prev_pts, pred, cache_pyramids=self.cache_pyramids, **cfg.lk_params)
        h, w = img0.shape[:2]
        keep = [i for i, p in enumerate(curr_pts) if mask[i] and not (p[0] < 0 or p[0] > w - 1 or p[1] < 0 or p[1] > h - 1)]
        self.num_features['after_tracking'] = len(keep)
        tracked = [curr_pts[i] for i in keep]
        cam1_pts, match, _ = self._stereo(img0, img1, tracked)
        sel = [(k, i) for k, i in enumerate(keep) if match[k]]
        self.num_features['after_matching'] = len(sel)
        survive = np.ones(len(sel), bool)
        if sel:
            common = dict(inlier_error=cfg.ransac_threshold, success_probability=cfg.ransac_success_probability, seed=cfg.ransac_seed,
                          frame=self.frame_no)
            m0, i0 = rr.two_point_ransac(np.array([prev[i].cam0_point for _k, i in sel], np.float32), np.array([tracked[k] for k, _i in sel], np.float32),
                                         R0, cfg.cam0_intrinsics, cfg.cam0_distortion_model, cfg.cam0_distortion_coeffs, camera=0, **common)
            m1, i1 = rr.two_point_ransac(np.array([prev[i].cam1_point for _k, i in sel], np.float32), np.array([cam1_pts[k] for k, _i in sel], np.float32),
                                         R1, cfg.cam1_intrinsics, cfg.cam1_distortion_model, cfg.cam1_distortion_coeffs, camera=1, **common)
            survive = (m0 == 1) & (m1 == 1)
            self.ransac_counts = [int(survive.sum()), i0['n_set'], i1['n_set'], i0['path'] | i1['path'] << 4]
            self.margin = min(i0['margin'], i1['margin'])
        for ok, (k, i) in zip(survive, sel):
            if not ok:
                self.rejected.append(tracked[k])
                continue
            f = Feat()
            f.id = prev[i].id
            f.lifetime = prev[i].lifetime + 1
            f.cam0_point = tracked[k]
            f.cam1_point = cam1_pts[k]
            self.curr_features[cell_of(f.cam0_point, gh, gw, cfg)].append(f)
        self.num_features['after_ransac'] = int(survive.sum())


def run_ransac_oracle(cfg, stream):
    """run_oracle with the RANSAC oracle; per frame also its counts (as read_ransac_counts orders them), margin and rejected points."""
    return run_oracle(cfg, stream, oracle=RansacOracle(cfg),
                      extra=lambda fe, _msg: dict(counts=list(fe.ransac_counts), margin=fe.margin, rejected=list(fe.rejected)))


def check_ransac_counts(ref, got, tag):
    """read_ransac_counts (the fourth element of run_engine's frames with read=read_ransac_counts) equal to the oracle's, per frame."""
    for k, (r, g) in enumerate(zip(ref, got)):
        rc = g[3]
        assert [rc['after_ransac'], rc['cam0_set'], rc['cam1_set'], rc['path']] == r['counts'], (tag, k, rc, r['counts'])
