"""tests/forecast_ref.py -- TEST INFRASTRUCTURE ONLY.

The contract of the forecast (include/airvision.h, "Forecast") written down in NumPy: an oracle that, after a feature_callback, carries
a deep copy of itself through the IMU messages its buffer still holds -- the pending samples, the first `cap` of them -- by its own
process_model, and maps the copy's IMU block and state to the odometry-covariance record (tests/odom_cov_ref.py).  And the same in 50
digits on a case of tests/msckf_predict_cases.py.  Shared by tests/test_forecast_ref.py (CPU) and the GPU suites.
"""
import collections
import copy

import numpy as np

import imu_rate_ref as Ir
import msckf_mp_ref as R
import msckf_predict_cases as Pc
from odom_cov_ref import odom_cov

FAMILIES = ('samples', 'rate', 'sparsity', 'gap')
ImuMsg = collections.namedtuple('ImuMsg', 'timestamp angular_velocity linear_acceleration')


class ForecastOracle(Ir.ImuRateOracle):
    """ImuRateOracle with `forecast(cap)`, to be called after feature_callback.  `published`: whether that callback published."""

    def __init__(self, config, next_imu_id=0):
        Ir.ImuRateOracle.__init__(self, config, next_imu_id)
        self.published = False

    def feature_callback(self, feature_msg):
        r = Ir.ImuRateOracle.feature_callback(self, feature_msg)
        self.published = r is not None
        return r

    def forecast(self, cap):
        """-> (records: list of dict(t, p, q, v, w), (had, written), C float64[15, 15]).  Works on a deep copy: the oracle is untouched.
        A callback that did not publish: ([], (0, 0), NaN)."""
        if not self.published:
            return [], (0, 0), np.full((15, 15), np.nan)
        keep = (self.config, self.opt, self.map_server, self.cam_states, self.chi2_table, self.trajectory, self.debug)     # process_model reads none of them
        c = copy.deepcopy(self, {id(o): o for o in keep})
        had = len(c.imu_msg_buffer)
        wr = min(had, int(cap))
        c.imu_states = []
        for m in c.imu_msg_buffer[:wr]:
            c.process_model(m.timestamp, m.angular_velocity, m.linear_acceleration)
            c.imu_state.timestamp = m.timestamp
        s = c.imu_state
        return list(c.imu_states), (had, wr), odom_cov(c.state_cov, s.orientation, s.R_imu_cam0, s.t_cam0_imu)


def case_oracle(case, cfg):
    """A ForecastOracle in the state of a case of msckf_predict_cases -- the state a step leaves -- with the case's IMU samples as its
    pending messages."""
    f = ForecastOracle(cfg)
    s, st = f.imu_state, case['state']
    s.timestamp = float(st['ts'])
    s.orientation, s.position, s.velocity = st['q'].copy(), st['p'].copy(), st['v'].copy()
    s.gyro_bias, s.acc_bias = st['bg'].copy(), st['ba'].copy()
    s.orientation_null, s.position_null, s.velocity_null = st['qn'].copy(), st['pn'].copy(), st['vn'].copy()
    s.R_imu_cam0, s.t_cam0_imu = st['R_ic'].copy(), st['t_ci'].copy()
    f.gravity = st['gravity'].copy()
    f.Qc = np.diag(np.repeat(case['noise'], 3))
    f.state_cov = case['P'].copy()
    f.imu_msg_buffer = [ImuMsg(float(m[0]), m[1:4].copy(), m[4:7].copy()) for m in case['imu']]
    f.published = True
    return f


def predict_case(case, cfg, cap):
    """ForecastOracle.forecast on a case: what av_msckf_forecast_ops_dev is to return for it."""
    return case_oracle(case, cfg).forecast(cap)


# ---- 50 digits --------------------------------------------------------------------------------------------------------------------
def mp_odom_cov(P, q, R_ic, t_ci):
    """odom_cov_ref.odom_cov in mpmath: J P[0:21, 0:21] J^T -> object array [15, 15]."""
    R_wb = R.to_rotation(q).T
    J = R.zeros(15, 21)
    J[0:3, 12:15] = R.eye(3)
    J[3:6, 0:3] = R.eye(3)
    J[6:9, 6:9] = R.eye(3)
    J[9:12, 12:15] = R.eye(3)
    J[9:12, 0:3] = -R_wb.dot(R.skew(t_ci))
    J[9:12, 18:21] = R_wb
    J[12:15, 0:3] = R_ic
    J[12:15, 15:18] = R.eye(3)
    return J.dot(np.array(P, dtype=object)[:21, :21]).dot(J.T)


_cache = {}


def mp_forecast(case, cap, cfg=None, full=None):
    """The forecast of a case in 50 digits: states as imu_rate_ref.mp_states, the IMU block as mp_predict's P_prop[:21, :21], J P J^T in
    mpmath at the last state's orientation -> dict(states: list of dict(q, p, v), C: object array [15, 15]).  The first `cap` samples.
    full: mp_predict of the whole case where the caller has it (msckf_predict_cases.reference); cached per (case, written)."""
    wr = min(len(case['imu']), int(cap))
    key = (case['name'], wr)
    if key not in _cache:
        sub = dict(case, imu=case['imu'][:wr], P=case['P'][:21, :21])      # (the IMU block depends on nothing else: the cut case is exact for it)
        states = Ir.mp_states(sub)
        ref = full if (full is not None and wr == len(case['imu'])) else Pc.mp_predict(sub)
        s0 = R.imu_state(case['state'])
        q = states[-1]['q'] if states else s0['q']
        _cache[key] = dict(states=states, C=mp_odom_cov(ref['P_prop'], q, s0['R_ic'], s0['t_ci']))
    return _cache[key]


def rec_err(got, ref):
    """The covariance record entry by entry relative to sqrt(C_ii C_jj) of the reference's record."""
    return Pc.cov_err(np.asarray(got, dtype=np.float64), ref)


def oracle_errors(name, cfg):
    """Per case of the family, the fp64 oracle's forecast (every sample) against the 50-digit one: dict(q, p, v: the largest error of
    any record, C)."""
    key = ('err', name)
    if key not in _cache:
        out = []
        for case, r in zip(Pc.family(name, cfg), Pc.reference(name, cfg)):
            recs, _, C = predict_case(case, cfg, len(case['imu']) + 1)
            ref = mp_forecast(case, len(case['imu']) + 1, full=r['ref'])
            e = dict(q=0.0, p=0.0, v=0.0, C=rec_err(C, ref['C']))
            for g, want in zip(recs, ref['states']):
                for f in ('q', 'p', 'v'):
                    e[f] = max(e[f], Pc.vec_err(g[f], want[f], quaternion=f == 'q'))
            out.append(dict(e, left_out=r['left_out']))
        _cache[key] = out
    return _cache[key]


def bars(name, cfg):
    """e_fam of the family: q, p, v as msckf_predict_cases.bars takes them; C = the oracle's largest record error over the family,
    floored at 4 ulp.  A kernel may be Pc.FACTOR times these."""
    b = Pc.bars(name, cfg)
    errs = [e['C'] for e in oracle_errors(name, cfg) if not e['left_out']]
    return dict(q=b['q'], p=b['p'], v=b['v'], C=max([Pc.FLOOR] + errs))
