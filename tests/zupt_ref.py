"""tests/zupt_ref.py -- TEST INFRASTRUCTURE ONLY.

A NumPy statement of the zero-velocity update (include/airvision.h, "Zero-velocity update"): the detector on the IMU samples a step
consumed and on the frame it appended, and the update as the oracle's own measurement_update with H selecting state columns 6..8,
r = -v and velocity_sigma^2 in place of observation_noise.  ZuptOracle is OracleMSCKF with both applied after every feature_callback:
what the batched filter with the update on is held to.  A record is a dict of the fields of av_zupt.
"""
import numpy as np

from oracle.msckf_np import OracleMSCKF

IMU_OK, VIS_OK, DETECTED, APPLIED, GATED, BAD = 1, 2, 4, 8, 16, 32
FIELDS = ('flags', 'n_imu', 'n_tracked', 'n_still', 'detected_total', 'applied_total', 'w_max', 'a_dev_max', 'v_norm', 'gamma', 'dx_pos')


def zero_record(detected_total=0, applied_total=0):
    r = dict.fromkeys(FIELDS, 0)
    r.update(w_max=0.0, a_dev_max=0.0, v_norm=0.0, gamma=0.0, dx_pos=0.0, detected_total=detected_total, applied_total=applied_total)
    return r


def params_of(cfg):
    """The av_zupt_params of a config, restated (uav_airvision_amd.msckf_ops.zupt_params is the code under test)."""
    return dict(gyro_max=cfg.zupt_gyro_threshold, acc_dev_max=cfg.zupt_acc_threshold,
                disparity_max=cfg.zupt_max_disparity * 2.0 / (cfg.cam0_intrinsics[0] + cfg.cam0_intrinsics[1]),
                velocity_sigma=cfg.zupt_velocity_sigma, gate=cfg.zupt_gate, min_tracks=int(cfg.zupt_min_tracks), still_percent=int(cfg.zupt_still_percent))


def detect(gyro, acc, gravity_norm, cur, prev, params):
    """gyro, acc: the bias-corrected samples of the step [k, 3]; cur: [(id, u0, v0)] of the appended frame; prev: {id: (u0, v0)} of the
    features the previous frame observed and the map still holds.  -> dict(flags, n_imu, n_tracked, n_still, w_max, a_dev_max)."""
    gyro, acc = np.asarray(gyro, dtype=np.float64).reshape(-1, 3), np.asarray(acc, dtype=np.float64).reshape(-1, 3)
    n_imu = len(gyro)
    w = np.sqrt((gyro * gyro).sum(axis=1))
    ad = np.abs(np.sqrt((acc * acc).sum(axis=1)) - gravity_norm)
    w_max, a_max = (float(w.max()), float(ad.max())) if n_imu else (0.0, 0.0)
    imu_ok = n_imu >= 1 and bool(w_max <= params['gyro_max']) and bool(a_max <= params['acc_dev_max'])
    n_tracked = n_still = 0
    dm2 = params['disparity_max'] * params['disparity_max']
    for fid, u, v in cur:
        if fid in prev:
            n_tracked += 1
            du, dv = u - prev[fid][0], v - prev[fid][1]
            n_still += bool(du * du + dv * dv <= dm2)
    vis_ok = n_tracked >= params['min_tracks'] and 100 * n_still >= params['still_percent'] * n_tracked
    flags = (IMU_OK if imu_ok else 0) | (VIS_OK if vis_ok else 0) | (DETECTED if imu_ok and vis_ok else 0)
    return dict(flags=flags, n_imu=n_imu, n_tracked=n_tracked, n_still=n_still, w_max=w_max, a_dev_max=a_max)


def decide(P, v, params):
    """The update's decisions on covariance P and velocity v -> (APPLIED | GATED | BAD, gamma, r): gamma = r^T S^-1 r first, then the gate,
    then whether S is finite and positive definite."""
    r = -np.asarray(v, dtype=np.float64)
    S = P[6:9, 6:9] + params['velocity_sigma'] ** 2 * np.identity(3)
    ok = bool(np.isfinite(S).all())
    if ok:
        try:
            np.linalg.cholesky((S + S.T) / 2)
        except np.linalg.LinAlgError:
            ok = False
    gamma = float(r @ np.linalg.solve(S, r)) if ok else float('nan')
    if params['gate'] > 0 and gamma > params['gate']:
        return GATED, gamma, r
    return (APPLIED if ok else BAD), gamma, r


def update_arrays(P, v, sigma):
    """The update written out on arrays: S = P[6:9, 6:9] + sigma^2 I, C = P[:, 6:9], delta_x = C S^-1 r, P+ = P - C S^-1 C^T computed for
    i <= j and mirrored.  -> (delta_x [n], P+ [n, n], gamma)."""
    P = np.asarray(P, dtype=np.float64)
    r = -np.asarray(v, dtype=np.float64)
    S = P[6:9, 6:9] + sigma ** 2 * np.identity(3)
    Si = np.linalg.inv(S)
    Si = (Si + Si.T) / 2
    C = P[:, 6:9]
    U = np.triu(P - C @ Si @ C.T)
    return C @ Si @ r, U + np.triu(U, 1).T, float(r @ Si @ r)


def apply(flt, params):
    """The update on an OracleMSCKF, through its own measurement_update.  -> dict(flag, v_norm, gamma, dx_pos)."""
    v = flt.imu_state.velocity.copy()
    flag, gamma, r = decide(flt.state_cov, v, params)
    out = dict(flag=flag, v_norm=float(np.linalg.norm(v)), gamma=gamma, dx_pos=0.0)
    if flag != APPLIED:
        return out
    n = len(flt.state_cov)
    H = np.zeros((3, n))
    H[:, 6:9] = np.identity(3)
    keep = flt.config.observation_noise
    flt.config.observation_noise = params['velocity_sigma'] ** 2
    try:
        flt.measurement_update(H, r)
    finally:
        flt.config.observation_noise = keep
    out['dx_pos'] = float(np.linalg.norm(flt.debug['delta_x'][12:15]))
    return out


class ZuptOracle(OracleMSCKF):
    """feature_callback(msg), then the zero-velocity update.  `record`: the av_zupt of the last step; `published`: (p, q, v) as the step
    published them, before the update; `records`: one per step."""

    def __init__(self, config, params=None):
        super().__init__(config)
        self.params = params_of(config) if params is None else dict(params)
        self.record = zero_record()
        self.records = []
        self.published = None
        self._prev = {}

    def feature_callback(self, msg):
        tot = (self.record['detected_total'], self.record['applied_total'])
        if not self.is_gravity_set:
            self.record = zero_record(*tot)
            self.records.append(self.record)
            return super().feature_callback(msg)
        s = self.imu_state
        t0 = msg.timestamp if self.is_first_img else s.timestamp
        used = [m for m in self.imu_msg_buffer if t0 <= m.timestamp <= msg.timestamp]
        gyro = np.array([m.angular_velocity - s.gyro_bias for m in used]).reshape(-1, 3)
        acc = np.array([m.linear_acceleration - s.acc_bias for m in used]).reshape(-1, 3)
        prev = {fid: uv for fid, uv in self._prev.items() if fid in self.map_server}
        cur = [(f.id, f.u0, f.v0) for f in msg.features]
        d = detect(gyro, acc, float(np.linalg.norm(self.gravity)), cur, prev, self.params)
        res = super().feature_callback(msg)
        self.published = (s.position.copy(), s.orientation.copy(), s.velocity.copy())
        self._prev = {fid: (u, v) for fid, u, v in cur} if len(self.map_server) else {}      # (an online reset empties the map)
        rec = zero_record(*tot)
        rec.update(d)
        rec['detected_total'] += bool(d['flags'] & DETECTED)
        if d['flags'] & DETECTED:
            u = apply(self, self.params)
            rec['flags'] |= u['flag']
            rec['applied_total'] += u['flag'] == APPLIED
            rec.update(v_norm=u['v_norm'], gamma=u['gamma'], dx_pos=u['dx_pos'])
        self.record = rec
        self.records.append(rec)
        return res
