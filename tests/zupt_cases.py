"""tests/zupt_cases.py -- TEST INFRASTRUCTURE ONLY.

Seeded inputs for the zero-velocity update's kernel (dk_zupt_update through av_msckf_zupt_ops_dev), with the fp64 oracle
(tests/zupt_ref.py: OracleMSCKF.measurement_update with H selecting columns 6..8) and the 50-digit reference
(tests/msckf_mp_ref.py: measurement_update(I3, r, P, [6, 7, 8], sigma^2), its delta_x injected in 50 digits after the oracle's formulas)
evaluated on them, and the bars the kernel is held to.  Shared by tests/test_zupt_ref.py (CPU) and tests/test_gpu_zupt_ops.py; every
reference value is computed once per process and cached.

A case is one stream: msckf_predict_cases.make_state / make_window / make_cov at a state dimension n, the velocity scaled so that
gamma = r^T S^-1 r takes a chosen value.  Errors: q, cam_q (sign-aligned), p, v, bg, ba, t_ci, cam_p as msckf_predict_cases.vec_err,
R_ic likewise on its nine entries, P entry by entry relative to sqrt(P+_ii P+_jj) of the reference (cov_err).  Bars, by the rule of
msckf_feature_cases (no new constant, none from a kernel): e_fam per quantity is the fp64 oracle's largest error over the cases,
floored at 4 ulp; a kernel may be FACTOR = 16 times that.
"""
import numpy as np

import msckf_mp_ref as R
import msckf_predict_cases as Pc
import zupt_ref as Z
from msckf_feature_cases import EPS, FACTOR      # noqa: F401  (the project's constants, no new one)
from oracle import msckf_np as O

LD = Pc.LD
DIMS = (21, 27, 81, 87, 165)                  # state dimensions at ld = 165: no camera, one, and both sides of 64 and of 128 + 21
SIGMA = 0.05
GATE = 50.0                                   # the launches' gate; a case's gamma is GATE / 2 (applied) or 2 GATE (gated)
FLOOR = 4 * EPS
QUANTITIES = ('q', 'p', 'v', 'bg', 'ba', 'R_ic', 't_ci', 'cam_q', 'cam_p', 'P')
PARAMS = dict(gyro_max=0.1, acc_dev_max=0.5, disparity_max=1e-3, velocity_sigma=SIGMA, gate=GATE, min_tracks=10, still_percent=90)

_cache = {}


def make_case(n, seed=4100, gamma=GATE / 2):
    """-> dict(state, cam_q, cam_p, P, n, ncam): the velocity scaled so that the fp64 gamma is `gamma`."""
    rng = np.random.default_rng(seed + n)
    ncam = (n - 21) // 6
    st = Pc.make_state(rng)
    cam_q, cam_p = Pc.make_window(rng, ncam)
    P = Pc.make_cov(rng, n)
    g0 = Z.update_arrays(P, st['v'], SIGMA)[2]
    st['v'] = st['v'] * np.sqrt(gamma / g0)
    st['vn'] = st['v'] + rng.normal(0, 2e-3, 3)
    return dict(state=st, cam_q=cam_q, cam_p=cam_p, P=P, n=n, ncam=ncam, name='n%d_g%g' % (n, gamma))


def case(n, gamma=GATE / 2):
    key = ('case', n, gamma)
    if key not in _cache:
        _cache[key] = make_case(n, gamma=gamma)
    return _cache[key]


# ---- the 50-digit statement: delta_x and P+ by msckf_mp_ref.measurement_update, the injection after oracle/msckf_np.py ------------------
def _mp_small_angle(d):
    dq = d / R.mpf(2)
    n2 = dq.dot(dq)
    if n2 <= 1:
        return np.array(list(dq) + [R.mp.sqrt(1 - n2)], dtype=object)
    return np.array(list(dq) + [R.ONE], dtype=object) / R.mp.sqrt(1 + n2)


def _mp_qmul(q1, q2):
    q1, q2 = q1 / R.norm(q1), q2 / R.norm(q2)
    L = np.array([[q1[3], q1[2], -q1[1], q1[0]], [-q1[2], q1[3], q1[0], q1[1]], [q1[1], -q1[0], q1[3], q1[2]], [-q1[0], -q1[1], -q1[2], q1[3]]], dtype=object)
    q = L.dot(q2)
    return q / R.norm(q)


def reference(c):
    """dict(QUANTITIES in 50 digits, dx, gamma) of the update on case c; cached."""
    key = ('ref', c['name'])
    if key not in _cache:
        st = c['state']
        r = -R.M(st['v'])
        dx, Pn = R.measurement_update(np.identity(3), -st['v'], c['P'], [6, 7, 8], SIGMA ** 2)
        S = R.M(c['P'])[6:9, 6:9] + R.eye(3) * R.mpf(SIGMA) ** 2
        out = dict(dx=dx, P=Pn, gamma=float(r.dot(R.solve(S, r))))
        out['q'] = _mp_qmul(_mp_small_angle(dx[:3]), R.M(st['q']))
        out['bg'], out['v'], out['ba'], out['p'] = R.M(st['bg']) + dx[3:6], R.M(st['v']) + dx[6:9], R.M(st['ba']) + dx[9:12], R.M(st['p']) + dx[12:15]
        out['R_ic'] = R.to_rotation(_mp_small_angle(dx[15:18])).dot(R.M(st['R_ic']))
        out['t_ci'] = R.M(st['t_ci']) + dx[18:21]
        out['cam_q'] = [_mp_qmul(_mp_small_angle(dx[21 + 6 * k:24 + 6 * k]), R.M(c['cam_q'][k])) for k in range(c['ncam'])]
        out['cam_p'] = [R.M(c['cam_p'][k]) + dx[24 + 6 * k:27 + 6 * k] for k in range(c['ncam'])]
        _cache[key] = out
    return _cache[key]


def errors(got, ref):
    """got: dict(QUANTITIES as fp64 arrays; cam_q [ncam, 4], cam_p [ncam, 3]) -> the error of every quantity against the reference."""
    e = {k: Pc.vec_err(got[k], ref[k], quaternion=k == 'q') for k in ('q', 'p', 'v', 'bg', 'ba', 't_ci')}
    e['R_ic'] = Pc.vec_err(np.asarray(got['R_ic']).reshape(-1), ref['R_ic'].reshape(-1))
    e['cam_q'] = max([0.0] + [Pc.vec_err(g, w, quaternion=True) for g, w in zip(got['cam_q'], ref['cam_q'])])
    e['cam_p'] = max([0.0] + [Pc.vec_err(g, w) for g, w in zip(got['cam_p'], ref['cam_p'])])
    e['P'] = Pc.cov_err(np.asarray(got['P']), ref['P'])
    return e


def oracle_filter(c, cfg):
    """An OracleMSCKF holding the case's state, window and covariance."""
    flt = O.OracleMSCKF(cfg)
    s, st = flt.imu_state, c['state']
    s.orientation, s.position, s.velocity, s.gyro_bias, s.acc_bias = st['q'].copy(), st['p'].copy(), st['v'].copy(), st['bg'].copy(), st['ba'].copy()
    s.R_imu_cam0, s.t_cam0_imu = np.array(st['R_ic'], dtype=np.float64).reshape(3, 3).copy(), st['t_ci'].copy()
    for k in range(c['ncam']):
        cs = O.OCAMState(k)
        cs.orientation, cs.position = c['cam_q'][k].copy(), c['cam_p'][k].copy()
        flt.cam_states[k] = cs
    flt.state_cov = c['P'].copy()
    return flt


def oracle_result(c, cfg, params=PARAMS):
    """The fp64 oracle's update of the case (zupt_ref.apply) -> (dict of QUANTITIES, the record part apply returns)."""
    flt = oracle_filter(c, cfg)
    u = Z.apply(flt, params)
    s = flt.imu_state
    cams = list(flt.cam_states.values())
    return dict(q=s.orientation, p=s.position, v=s.velocity, bg=s.gyro_bias, ba=s.acc_bias, R_ic=s.R_imu_cam0, t_ci=s.t_cam0_imu,
                cam_q=np.array([cs.orientation for cs in cams]).reshape(-1, 4), cam_p=np.array([cs.position for cs in cams]).reshape(-1, 3),
                P=flt.state_cov, dx=flt.debug.get('delta_x')), u


def bars(cfg):
    """e_fam per quantity: the oracle's largest error over the applied cases of DIMS, floored at 4 ulp; cached."""
    key = ('bars',)
    if key not in _cache:
        errs = [errors(oracle_result(case(n), cfg)[0], reference(case(n))) for n in DIMS]
        _cache[key] = {k: max([FLOOR] + [e[k] for e in errs]) for k in QUANTITIES}
    return _cache[key]
