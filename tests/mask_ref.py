"""tests/mask_ref.py -- TEST INFRASTRUCTURE ONLY: the static per-camera masks of the front-end ("Static masks" in include/airvision.h)
stated in NumPy: how a mask is binned, the two mask shapes the tests use, and the CPU oracle front-end with the three gates added.

A mask is uint8 [h, w]: non-zero = scene, 0 = never scene.  A pixel coordinate is mapped to a mask pixel by truncation,
m[int(y)][int(x)] (the reference's rule for its 7 x 7 mask, feature_adder.py:59-62).
  1. detection: a FAST keypoint on a masked cam0 pixel is dropped after the non-max suppression (first frame and add_new_features)
  2. temporal tracking: a tracked point that passed LK status and the bounds test but sits on a masked cam0 pixel is dropped there
  3. stereo: a match that passed the in-image test but whose cam1 point sits on a masked cam1 pixel is not an inlier
The stage bodies below are those of oracle/frontend.py restated, each with the one line its rule adds (marked `rule n`)."""
import math

import numpy as np

from fe_harness import run_oracle
from oracle.frontend import Feat, OracleFrontend, cell_of, cvops, grid_size, integrate_imu, matvec3, predict_feature_tracking, tracking_homography


def bin_mask(mask, f):
    """The mask of the image binned f x f: pixel (x, y) is valid iff all f x f source pixels are non-zero.  uint8 of 0 / 1."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    assert h % f == 0 and w % f == 0
    return m.reshape(h // f, f, w // f, f).all(axis=(1, 3)).astype(np.uint8)


def circle_mask(w, h, cx, cy, radius):
    """Valid iff (x - cx)^2 + (y - cy)^2 <= radius^2, pixel by pixel."""
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = 1 if (x - cx) * (x - cx) + (y - cy) * (y - cy) <= radius * radius else 0
    return out


def comb_mask(w, h, period, width, phase):
    """Vertical bands: the columns with (x + phase) % period < width are 0, the rest 1."""
    cols = np.array([0 if (x + phase) % period < width else 1 for x in range(w)], np.uint8)
    return np.ascontiguousarray(np.broadcast_to(cols, (h, w)))


class MaskedOracle(OracleFrontend):
    """OracleFrontend with the static masks mask0 / mask1 (uint8 [h, w] at the size of the frames it is fed, or None) and counts of
    what each gate dropped over the run: drops = dict(track=..., stereo=...)."""

    def __init__(self, config, mask0=None, mask1=None):
        OracleFrontend.__init__(self, config)
        self.mask0 = None if mask0 is None else np.ascontiguousarray(np.asarray(mask0) != 0, dtype=np.uint8)
        self.mask1 = None if mask1 is None else np.ascontiguousarray(np.asarray(mask1) != 0, dtype=np.uint8)
        self.drops = dict(track=0, stereo=0)

    def _stereo(self, img0, img1, cam0_points):
        """stereo_match of oracle/frontend.py (stereo_matcher.py:33-115)."""
        config, geom = self.config, self.geom
        if len(cam0_points) == 0:
            return np.array([]), np.array([], dtype=bool), {}
        K0, D0 = config.cam0_intrinsics, config.cam0_distortion_coeffs
        pts0 = np.array(cam0_points, dtype=np.float32)
        M0 = getattr(config, 'cam0_distortion_model', 'radtan')
        und0 = cvops.undistort_points(pts0, K0, D0, geom.R0to1, distortion_model=M0)
        proj1 = cvops.distort_points(und0, K0, D0, distortion_model=M0)
        lk = dict(config.lk_params)
        p1, track_mask, _ = cvops.calc_optical_flow_pyr_lk(img0, img1, pts0, np.array(proj1, dtype=np.float32), cache_pyramids=self.cache_pyramids, **lk)
        p0r, _rev, _ = cvops.calc_optical_flow_pyr_lk(img1, img0, p1, pts0.copy(), cache_pyramids=self.cache_pyramids, **lk)
        d = pts0 - p0r
        err = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        disp = np.abs(proj1[:, 1] - p1[:, 1])
        inlier = track_mask.reshape(-1).astype(bool) & (err < 3) & (disp < 20)
        h, w = img1.shape[:2]
        for i in range(len(p1)):
            if inlier[i]:
                x, y = p1[i]
                if x < 0 or x >= w or y < 0 or y >= h:
                    inlier[i] = False
                elif self.mask1 is not None and self.mask1[int(y), int(x)] == 0:          # rule 3
                    inlier[i] = False
                    self.drops['stereo'] += 1
        undist0 = cvops.undistort_points(pts0, K0, D0, distortion_model=M0)
        undist1 = cvops.undistort_points(p1, K0, D0, distortion_model=M0)
        thr = config.stereo_threshold * geom.norm_unit
        E = geom.E
        for i in range(len(p1)):
            if not inlier[i]:
                continue
            line = matvec3(E, (float(undist0[i, 0]), float(undist0[i, 1]), 1.0))
            err_epi = abs(float(undist1[i, 0]) * line[0]) / math.sqrt(line[0] * line[0] + line[1] * line[1])
            if err_epi > thr:
                inlier[i] = False
        return p1, inlier, dict(proj1=proj1, p0r=p0r, track_mask=track_mask)

    def _initialize_first_frame(self, img0, img1):
        """feature_initializer.py:45-85."""
        cfg = self.config
        gh, gw = grid_size(img0, cfg)
        xs, ys, sc = cvops.fast_detect(img0, cfg.fast_threshold, self.mask0)                     # rule 1 (None: no mask, as the reference)
        cam0_points = [(float(x), float(y)) for x, y in zip(xs, ys)]
        cam1_points, inl, _ = self._stereo(img0, img1, cam0_points)
        cells = [[] for _ in range(cfg.grid_num)]
        for i, ok in enumerate(inl):
            if not ok:
                continue
            f = Feat()
            f.response = float(sc[i]); f.cam0_point = cam0_points[i]; f.cam1_point = cam1_points[i]
            cells[cell_of(f.cam0_point, gh, gw, cfg)].append(f)
        n_new = 0
        for idx, feats in enumerate(cells):
            for f in sorted(feats, key=lambda q: q.response, reverse=True)[:cfg.grid_min_feature_num]:
                f.id = self.next_feature_id
                f.lifetime = 1
                self.curr_features[idx].append(f)
                self.next_feature_id += 1
                n_new += 1
        self.debug['add'] = dict(n_candidates=len(cam0_points), n_new=n_new, n_fast=len(xs))

    def _track(self, prev_img0, img0, img1, t_prev, t_curr):
        """feature_tracker.py:74-157."""
        cfg = self.config
        gh, gw = grid_size(img0, cfg)
        R0, _R1, self.imu_buffer = integrate_imu(self.imu_buffer, t_prev, t_curr, self.geom)
        prev = [f for cell in self.prev_features for f in cell]
        self.num_features['before_tracking'] = len(prev)
        if not prev:
            return
        prev_pts = np.array([f.cam0_point for f in prev], dtype=np.float32)
        H = tracking_homography(R0, cfg.cam0_intrinsics)
        pred = predict_feature_tracking(prev_pts, H)
        curr_pts, mask, _ = cvops.calc_optical_flow_pyr_lk(prev_img0, img0, prev_pts, pred, cache_pyramids=self.cache_pyramids, **cfg.lk_params)
        h, w = img0.shape[:2]
        keep = []
        for i, p in enumerate(curr_pts):
            if not mask[i]:
                continue
            if p[0] < 0 or p[0] > w - 1 or p[1] < 0 or p[1] > h - 1:
                continue
            if self.mask0 is not None and self.mask0[int(p[1]), int(p[0])] == 0:                # rule 2
                self.drops['track'] += 1
                continue
            keep.append(i)
        self.num_features['after_tracking'] = len(keep)
        tracked = [curr_pts[i] for i in keep]
        cam1_pts, match, _ = self._stereo(img0, img1, tracked)
        n = 0
        for k, i in enumerate(keep):
            if not match[k]:
                continue
            f = Feat()
            f.id = prev[i].id
            f.lifetime = prev[i].lifetime + 1
            f.cam0_point = tracked[k]
            f.cam1_point = cam1_pts[k]
            self.curr_features[cell_of(f.cam0_point, gh, gw, cfg)].append(f)
            n += 1
        self.num_features['after_matching'] = n
        self.num_features['after_ransac'] = n

    def _add_new(self, img0, img1):
        """feature_adder.py:52-108."""
        cfg = self.config
        gh, gw = grid_size(img0, cfg)
        mask = np.ones(img0.shape[:2], dtype='uint8') if self.mask0 is None else self.mask0.copy()      # rule 1: static & 7x7
        for cell in self.curr_features:
            for f in cell:
                x, y = int(f.cam0_point[0]), int(f.cam0_point[1])
                mask[y - 3:y + 4, x - 3:x + 4] = 0
        xs, ys, sc = cvops.fast_detect(img0, cfg.fast_threshold, mask)
        sieve = [[] for _ in range(cfg.grid_num)]
        for x, y, s in zip(xs, ys, sc):
            pt = (float(x), float(y))
            sieve[cell_of(pt, gh, gw, cfg)].append((pt, float(s)))
        cand = []
        for cell in sieve:
            if len(cell) > cfg.grid_max_feature_num:
                cell = sorted(cell, key=lambda q: q[1], reverse=True)[:cfg.grid_max_feature_num]
            cand.extend(cell)
        cam0_points = [c[0] for c in cand]
        cam1_points, inl, _ = self._stereo(img0, img1, cam0_points)
        cells = [[] for _ in range(cfg.grid_num)]
        for i, ok in enumerate(inl):
            if not ok:
                continue
            f = Feat()
            f.response = cand[i][1]; f.cam0_point = cam0_points[i]; f.cam1_point = cam1_points[i]
            cells[cell_of(f.cam0_point, gh, gw, cfg)].append(f)
        n_new = 0
        for idx, feats in enumerate(cells):
            for f in sorted(feats, key=lambda q: q.response, reverse=True)[:cfg.grid_min_feature_num]:
                f.id = self.next_feature_id
                f.lifetime = 1
                self.curr_features[idx].append(f)
                self.next_feature_id += 1
                n_new += 1
        self.debug['add'] = dict(n_candidates=len(cand), n_new=n_new, n_fast=len(xs))


def run_masked_oracle(cfg, stream, mask0=None, mask1=None, n_frames=None):
    """fe_harness.run_oracle with the masked oracle: per frame also the pixel coordinates p0, p1 of the grid's points in both cameras;
    and the oracle itself (its .drops)."""
    fe = MaskedOracle(cfg, mask0, mask1)

    def points(fe, _msg):
        return {name: np.array([getattr(f, attr) for cell in fe.prev_features for f in cell], np.float64).reshape(-1, 2)
                for name, attr in (('p0', 'cam0_point'), ('p1', 'cam1_point'))}
    return run_oracle(cfg, stream, n_frames, fe, points), fe
