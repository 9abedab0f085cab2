"""`msckf.MSCKF` of the drop-in (reference: src/msckf.py:95-867): the class `modules/vio.py:15,43,51` constructs and feeds.

A view over the library's batched filter with ONE stream (`av_msckf_batch_*`, include/airvision.h): `imu_callback` hands the
sample to `av_msckf_batch_push_imu`, `feature_callback` runs `av_msckf_batch_step` and wraps the published pose in the
reference's `vio_result`.  The whole of MSCKF.feature_callback -- IMU integration, state augmentation, the observation map,
lost-feature and camera-pruning updates, online reset (msckf.py:177-228 and everything it calls) -- runs inside the library,
C++ bookkeeping and HIP kernels, the same code the throughput path steps for thousands of streams; nothing of it is restated
here.  `state_server`, `map_server` and `debug` are read-only views for callers and parity tests.

Unlike the reference, gravity and the stereo extrinsics belong to the filter instance (several filters can live in one
process); `IMUState.gravity`, `CAMState.R_cam0_cam1` ... are still published as class attributes.
"""
import os
from collections import OrderedDict, namedtuple

import numpy as np

from feature import BaseFeature
from utils import Isometry3d, to_quaternion, to_rotation
from uav_airvision_amd import _native as N
from uav_airvision_amd.msckf_ops import BatchedMSCKF, unpack_forecast, unpack_imu_states, unpack_landmarks, unpack_odom_cov

_vio_result = namedtuple('vio_result', ['timestamp', 'pose', 'velocity', 'cam0_pose'])


def _make_output_filepath():
    """results/txts/output_<DATASET_NAME>_offset<TIME_OFFSET>.txt (reference: msckf.py:10-16)."""
    base = 'results/txts'
    os.makedirs(base, exist_ok=True)
    return os.path.join(base, 'output_%s_offset%s.txt' % (os.getenv('DATASET_NAME', 'unknown'), os.getenv('TIME_OFFSET', '0')))


class IMUState(object):
    """Snapshot of the filter's IMU state (reference: msckf.py:18-58)."""
    next_id = 0
    gravity = np.array([0., 0., -9.81])
    T_imu_body = Isometry3d(np.identity(3), np.zeros(3))

    def __init__(self, st=None):
        self.id = None
        if st is None:
            self.timestamp = None
            self.orientation = np.array([0., 0., 0., 1.]); self.position = np.zeros(3); self.velocity = np.zeros(3)
            self.gyro_bias = np.zeros(3); self.acc_bias = np.zeros(3)
            self.R_imu_cam0 = np.identity(3); self.t_cam0_imu = np.zeros(3)
        else:
            self.timestamp = float(st['t'])
            self.orientation, self.position, self.velocity = st['q'], st['p'], st['v']
            self.gyro_bias, self.acc_bias = st['bg'], st['ba']
            self.R_imu_cam0, self.t_cam0_imu = st['R_ic'], st['t_ci']


class CAMState(object):
    """Snapshot of one camera state of the window (reference: msckf.py:61-77)."""
    R_cam0_cam1 = None
    t_cam0_cam1 = None

    def __init__(self, new_id=None, orientation=None, position=None):
        self.id = new_id
        self.timestamp = None
        self.orientation = np.array([0., 0., 0., 1.]) if orientation is None else orientation
        self.position = np.zeros(3) if position is None else position


class StateServer(object):
    """`state_server` of the reference (msckf.py:80-91), read from the library on every access."""

    def __init__(self, flt):
        self._flt = flt

    @property
    def imu_state(self):
        return IMUState(self._flt.get_state(0))

    @property
    def cam_states(self):
        st = self._flt.get_state(0)
        return OrderedDict((int(i), CAMState(int(i), q, p)) for i, q, p in zip(st['cam_ids'], st['cam_q'], st['cam_p']))

    @property
    def state_cov(self):
        return self._flt.get_cov(0)


class _MapView(object):
    """`map_server`: the observation map lives in the library; its size is what callers and tests look at."""

    def __init__(self, flt):
        self._flt = flt

    def __len__(self):
        return self._flt.sizes(0)[2]


class MSCKF(object):
    def __init__(self, config, device=0, rows_cap=None, write_trajectory=True):
        self.config = config
        self.optimization_config = config.optimization_config
        # config.publish_covariance = True (no reference counterpart; default off): `last_covariance` holds the 15 x 15 odometry
        # covariance (p, theta, v, p_c, theta_c; include/airvision.h) of the last published result.  vio_result is unchanged.
        self._cov_on = bool(getattr(config, 'publish_covariance', False))
        self.last_covariance = None
        if self._cov_on and not np.array_equal(np.asarray(config.T_imu_body, dtype=np.float64), np.identity(4)):
            raise ValueError('config.publish_covariance needs config.T_imu_body = identity: the covariance is not conjugated into a body frame')
        # config.publish_landmarks = True (no reference counterpart; default off): `last_landmarks` holds the landmark records
        # (msckf_ops.LANDMARK_DTYPE, at most config.landmark_cap) of the last feature_callback, positions mapped by T_imu_body into the
        # world frame of the published pose; `last_landmarks_dropped` = records of that frame beyond the cap.  vio_result is unchanged.
        self._lm_on = bool(getattr(config, 'publish_landmarks', False))
        self.last_landmarks = None
        self.last_landmarks_dropped = 0
        # config.publish_innovation = True (no reference counterpart; default off): `last_innovation` holds the two innovation-statistics
        # blocks (msckf_ops.FILTER_STATS_DTYPE[2], see msckf_ops.unpack_filter_stats) of the last feature_callback.  vio_result is unchanged.
        self._stats_on = bool(getattr(config, 'publish_innovation', False))
        self.last_innovation = None
        # config.publish_imu_rate = True (no reference counterpart; default off): `last_imu_states` holds the IMU-rate records
        # (msckf_ops.IMU_STATE_DTYPE, the last config.imu_rate_cap of them) of the last feature_callback -- the state after every IMU sample
        # the frame's prediction integrated -- with p, q, v mapped by T_imu_body the way `publish` maps the pose and the velocity; w stays
        # the bias-corrected gyro in the IMU frame.  `last_imu_states_dropped` = records of that frame beyond the cap.  vio_result is unchanged.
        self._ir_on = bool(getattr(config, 'publish_imu_rate', False))
        self.last_imu_states = None
        self.last_imu_states_dropped = 0
        # config.publish_forecast = True (no reference counterpart; default off): `last_forecast` holds the forecast records
        # (msckf_ops.IMU_STATE_DTYPE, the first config.forecast_cap of them) of the last feature_callback -- the pose the step leaves carried
        # through the IMU messages received beyond the frame's time -- with p, q, v mapped by T_imu_body exactly as `last_imu_states` maps
        # them; `last_forecast_pending` = (had, written).  `last_forecast_covariance` is the 15 x 15 covariance at the last record (at the
        # frame's pose when there is none) for T_imu_body = identity only: it is not conjugated into a body frame, so it is None otherwise,
        # and together with config.publish_covariance a T_imu_body != identity is refused as above.  vio_result is unchanged.
        self._fc_on = bool(getattr(config, 'publish_forecast', False))
        self._fc_cov = self._fc_on and np.array_equal(np.asarray(config.T_imu_body, dtype=np.float64), np.identity(4))
        self.last_forecast = None
        self.last_forecast_pending = (0, 0)
        self.last_forecast_covariance = None
        # config.use_zupt = True (no reference counterpart; default off): the zero-velocity update with the config's zupt_* thresholds
        # (include/airvision.h, "Zero-velocity update").  It acts behind every feature_callback: the vio_result of a frame is the
        # pre-update pose, state_server and the next frame see the corrected state.  `last_zupt` holds the frame's record
        # (msckf_ops.ZUPT_DTYPE, see msckf_ops.unpack_zupt).  vio_result is unchanged.
        self._zupt_on = bool(getattr(config, 'use_zupt', False))
        self.last_zupt = None
        self._flt = BatchedMSCKF(config, 1, device=device, rows_cap=rows_cap, odom_cov=self._cov_on, landmarks=self._lm_on,
                                 landmark_cap=int(getattr(config, 'landmark_cap', 256)), stats=self._stats_on, imu_rate=self._ir_on,
                                 imu_rate_cap=int(getattr(config, 'imu_rate_cap', 32)), forecast=self._fc_on,
                                 forecast_cap=int(getattr(config, 'forecast_cap', 32)), zupt=self._zupt_on)
        self.state_server = StateServer(self._flt)
        self.map_server = _MapView(self._flt)
        # class-level statics the reference sets in its constructor (msckf.py:128-150), kept for code that reads them
        IMUState.gravity = np.array(config.gravity, dtype=np.float64)
        T = np.asarray(config.T_cn_cnm1, dtype=np.float64)
        CAMState.R_cam0_cam1 = BaseFeature.R_cam0_cam1 = T[:3, :3]
        CAMState.t_cam0_cam1 = BaseFeature.t_cam0_cam1 = T[:3, 3]
        self.T_imu_body = Isometry3d(np.asarray(config.T_imu_body)[:3, :3], np.asarray(config.T_imu_body)[:3, 3])
        IMUState.T_imu_body = self.T_imu_body
        self._n_imu = 0
        self.is_gravity_set = False
        self.tracking_rate = None
        self._cap = 64
        self._outfile = _make_output_filepath() if write_trajectory else None
        self.debug = {}
        self._capture = False

    def close(self):
        self._flt.close()

    def restart(self):
        """No counterpart in the reference: the filter back to "as constructed" without rebuilding it (BatchedMSCKF.restart).  IMU
        messages received so far are dropped -- gravity is initialised again from the next 200 -- camera-state ids begin again at 0;
        `generation` counts the restarts.  vio_result is unchanged."""
        self._flt.restart([0])
        self._n_imu = 0
        self.is_gravity_set = False
        self.tracking_rate = None
        self.last_covariance = None
        self.last_landmarks = None
        self.last_landmarks_dropped = 0
        self.last_innovation = None
        self.last_imu_states = None
        self.last_imu_states_dropped = 0
        self.last_forecast = None
        self.last_forecast_pending = (0, 0)
        self.last_forecast_covariance = None
        self.last_zupt = None
        self.debug = {}

    @property
    def generation(self):
        return int(self._flt.generation[0])

    def capture_debug(self, enable=True):
        """Parity tests: after every frame `debug['gamma']` is extended by the gating values of the frame (reference order),
        `debug['updates']` holds [(rows, delta_x, P_after)] of the frame's updates and `debug['delta_x']` the last delta_x."""
        self._capture = bool(enable)
        self._flt.debug_capture(enable)

    # ---- callbacks ---------------------------------------------------------------------------
    def imu_callback(self, imu_msg):
        """msckf.py:162-175 (buffering and, with the 200th sample, initialize_gravity_and_bias happen in the library)."""
        self._flt.push_imu([0], [imu_msg.timestamp], [imu_msg.angular_velocity], [imu_msg.linear_acceleration])
        self._n_imu += 1
        if self._n_imu >= 200:
            self.is_gravity_set = True

    def feature_callback(self, feature_msg):
        """msckf.py:177-228: returns `vio_result` or None (no gravity yet)."""
        feats = feature_msg.features
        n = len(feats)
        if n > self._cap:
            self._cap = (n + 63) // 64 * 64
        ids = np.zeros((1, self._cap), np.int64)
        uv = np.zeros((1, self._cap, 4), np.float64)
        if n:
            ids[0, :n] = [f.id for f in feats]
            uv[0, :n] = [(f.u0, f.v0, f.u1, f.v1) for f in feats]
        out = self._flt.step(ids, uv, [n], [feature_msg.timestamp], cov=True if self._cov_on else None, landmarks=True if self._lm_on else None,
                             stats=True if self._stats_on else None, imu_states=True if self._ir_on else None,
                             forecast=True if self._fc_on else None)
        if self._zupt_on:
            self.last_zupt = self._flt.read_zupt()[0].copy()
        if self._fc_on:
            rec, cnt, cov = self._flt.last_forecast
            got, C15, _ = unpack_forecast(rec, cnt, cov, 0)
            self.last_forecast = self._to_body(got.copy())
            self.last_forecast_pending = (int(cnt[0, 0]), int(cnt[0, 1]))
            self.last_forecast_covariance = C15 if self._fc_cov and out[0, 0] == 1.0 else None
        if self._ir_on:
            rec, cnt = self._flt.last_imu_states
            self.last_imu_states = self._to_body(unpack_imu_states(rec, cnt, 0).copy())
            self.last_imu_states_dropped = int(cnt[0, 0] - cnt[0, 1])
        if self._stats_on:
            self.last_innovation = self._flt.last_stats[0].copy()
        if self._lm_on:
            rec, cnt = self._flt.last_landmarks
            lm = unpack_landmarks(rec, cnt, 0).copy()
            lm['p'] = lm['p'] @ self.T_imu_body.R.T + self.T_imu_body.t
            self.last_landmarks = lm
            self.last_landmarks_dropped = int(cnt[0, 0] - cnt[0, 1])
        if self._cov_on and out[0, 0] == 1.0:
            self.last_covariance = unpack_odom_cov(self._flt.last_cov[0])
        if self._capture:
            ups = []
            for phase in (0, 1):
                g, rows, dx, P = self._flt.debug_read(0, phase)
                self.debug.setdefault('gamma', []).extend(g.tolist())
                if rows:
                    ups.append((rows, dx, P))
                    self.debug['delta_x'] = dx
            self.debug['updates'] = ups
        if out[0, 0] < 0:
            code, msg = self._flt.stream_status(0)
            raise N.AirvisionError(code, msg)
        if out[0, 0] == 0:
            return None
        return self.publish(feature_msg.timestamp, out[0])

    def _to_body(self, rec):
        """IMU-rate records in the filter's frame -> the frame of the published pose: p, q from T_imu_body * T_i_w * T_imu_body^-1, v
        rotated by T_imu_body, as `publish` does; w is left in the IMU frame.  Identity T_imu_body: the records as they are, bit for bit."""
        B = self.T_imu_body
        if np.array_equal(B.R, np.identity(3)) and not np.any(B.t):
            return rec
        Binv = B.inverse()
        for r in rec:
            T_b_w = B * Isometry3d(to_rotation(r['q']).T, r['p'].copy()) * Binv
            r['p'], r['q'], r['v'] = T_b_w.t, to_quaternion(T_b_w.R.T), B.R @ r['v']
        return rec

    def publish(self, time, out):
        """msckf.py:845-867 on the state the step just published: out = [1, t, p(3), q(4), v(3)]."""
        p, q, v = out[2:5].copy(), out[5:9].copy(), out[9:12].copy()
        st = self._flt.get_state(0)                      # extrinsics are part of the estimated state
        T_i_w = Isometry3d(to_rotation(q).T, p)
        T_b_w = self.T_imu_body * T_i_w * self.T_imu_body.inverse()
        body_velocity = self.T_imu_body.R @ v
        R_w_c = st['R_ic'] @ T_i_w.R.T
        t_c_w = p + T_i_w.R @ st['t_ci']
        if self._outfile is not None:                    # msckf.py:152-160
            with open(self._outfile, 'a') as f:
                f.write('%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n' % (out[1], p[0], p[1], p[2], q[0], q[1], q[2], q[3]))
        return _vio_result(time, T_b_w, body_velocity, Isometry3d(R_w_c.T, t_c_w))
