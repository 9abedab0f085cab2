"""tests/imu_rate_ref.py -- TEST INFRASTRUCTURE ONLY.

The contract of the IMU-rate odometry (include/airvision.h, "IMU-rate odometry") written down in NumPy: an OracleMSCKF that keeps, for
the frame it is working on, the state after every IMU sample its prediction integrated, and the rule of the cap.  Shared by
tests/test_imu_rate_ref.py (CPU: this reference against the 50-digit predict_new_state) and the GPU suites.
"""
import numpy as np

from oracle.msckf_np import OracleMSCKF

FIELDS = ('t', 'p', 'q', 'v', 'w')


class ImuRateOracle(OracleMSCKF):
    """OracleMSCKF with `imu_states`: one (t, p, q, v, w) per process_model call of the last feature_callback, in order -- the sample's
    stamp, position, orientation and velocity right after the call, and the bias-corrected gyro the sample was integrated with."""

    def __init__(self, config, next_imu_id=0):
        OracleMSCKF.__init__(self, config, next_imu_id)
        self.imu_states = []

    def process_model(self, time, m_gyro, m_acc):
        OracleMSCKF.process_model(self, time, m_gyro, m_acc)
        s = self.imu_state
        self.imu_states.append(dict(t=float(time), p=np.array(s.position, dtype=np.float64), q=np.array(s.orientation, dtype=np.float64),
                                    v=np.array(s.velocity, dtype=np.float64), w=np.asarray(m_gyro, dtype=np.float64) - s.gyro_bias))

    def feature_callback(self, feature_msg):
        self.imu_states = []
        return OracleMSCKF.feature_callback(self, feature_msg)


def capped(states, cap):
    """(had, written, the records a step publishes): on overflow the LAST cap samples, in time order."""
    had = len(states)
    wr = min(had, int(cap))
    return had, wr, list(states[had - wr:])


def as_arrays(states):
    """A list of records -> dict of arrays t[n], p[n, 3], q[n, 4], v[n, 3], w[n, 3]."""
    dims = dict(t=(), p=(3,), q=(4,), v=(3,), w=(3,))
    return {f: np.array([s[f] for s in states], dtype=np.float64).reshape((len(states),) + dims[f]) for f in FIELDS}


def predict_case(case, cfg):
    """The records of one case of tests/msckf_predict_cases.py (one stream, one frame) by the recording oracle's process_model, from the
    case's state: what av_msckf_predict_ops_dev_rate is to return for it."""
    f = ImuRateOracle(cfg)
    s, st = f.imu_state, case['state']
    s.timestamp = float(st['ts'])
    s.orientation, s.position, s.velocity = st['q'].copy(), st['p'].copy(), st['v'].copy()
    s.gyro_bias, s.acc_bias = st['bg'].copy(), st['ba'].copy()
    s.orientation_null, s.position_null, s.velocity_null = st['qn'].copy(), st['pn'].copy(), st['vn'].copy()
    f.gravity = st['gravity'].copy()
    f.Qc = np.diag(np.repeat(case['noise'], 3))
    f.state_cov = case['P'][:21, :21].copy()                 # (the states do not depend on the covariance: the IMU block is enough)
    for m in case['imu']:
        f.process_model(m[0], m[1:4], m[4:7])
        s.timestamp = m[0]
    return f.imu_states


def mp_states(case):
    """The same in 50 digits (tests/msckf_mp_ref.predict_new_state per sample, state only): a list of dict(q, p, v) of mpf arrays."""
    import msckf_mp_ref as R
    s = R.imu_state(case['state'])
    out = []
    for m in case['imu']:
        dt = R.mpf(float(m[0])) - s['ts']
        R.predict_new_state(s, dt, R.M(m[1:4]) - s['bg'], R.M(m[4:7]) - s['ba'])
        s['ts'] = R.mpf(float(m[0]))
        out.append(dict(q=s['q'], p=s['p'], v=s['v']))
    return out
