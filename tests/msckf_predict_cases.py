"""tests/msckf_predict_cases.py -- TEST INFRASTRUCTURE ONLY.

Seeded inputs for the part of a filter step that runs before any feature is looked at -- state integration (predict_new_state),
covariance propagation (process_model), state augmentation, removal of camera states, the redundancy rule -- with the fp64 oracle
(oracle/msckf_np.py) and the 50-digit reference (tests/msckf_mp_ref.py) evaluated on them, and the bars the GPU kernels are held to.
Shared by tests/test_msckf_mp_ref.py (CPU: oracle against reference) and tests/test_gpu_msckf_predict.py (kernels against reference);
every reference value is computed once per process and cached.

A case is a full input record of one stream: the IMU state with INDEPENDENT null states (a perturbed copy, as after an update: with
them Phi[:3, :3] = R_new R_null^T is not R_new R_old^T and the observability correction is not nearly zero -- a run without updates
never gets there), a window of camera states, a symmetric positive definite covariance (realistic block scales times 0.5 I + L L^T / 3
with L of rank 3, so that every cross block is dense), the frame's IMU samples at 5 ms and the continuous noise variances.

Bars, by the rule of msckf_feature_cases (none comes from the code under test): e_fam = the largest error of the fp64 ORACLE against
the 50-digit reference over the family, floored at 4 ulp; a kernel may be FACTOR = 16 times that.  Errors: q (sign-aligned), p, v,
cam_q, cam_p as |x - ref| / |ref|; the covariance entry by entry relative to sqrt(P_ii P_jj) of the reference's result.
"""
import numpy as np

import msckf_mp_ref as R
from msckf_feature_cases import EPS, FACTOR, GOLDEN, GRAVITY, MARGIN_MIN      # noqa: F401  (FACTOR, MARGIN_MIN: the project's, not new ones)
from oracle import msckf_np as O

DT = 0.005
CAM_STRIDE = 24                 # capacity of the window in the launches: ld = 21 + 6 * 24 = 165
LD = 21 + 6 * CAM_STRIDE
FLOOR = 4 * EPS
QUANTITIES = ('q', 'p', 'v', 'cam_q', 'cam_p', 'P')

# family -> cases: camera states in the window (n = 21 + 6 ncam), IMU samples, gyro mode, orientation, index of a sample that repeats
# its predecessor's time stamp.  The large windows take at most 3 samples (cost of the reference).
FAMILIES = {
    # 0, 1, 10 and 17 samples per frame (17 = DEV_IMU_BATCH + 1) at n = 21 (no camera state: no cross block) and 27 (a cross block
    # narrower than a chunk)
    'samples': [dict(ncam=0, n_imu=10), dict(ncam=1, n_imu=17), dict(ncam=1, n_imu=0), dict(ncam=0, n_imu=1)],
    # n = 81 (60 columns: just under a chunk of 64), 87 (66: a second chunk of two), 159 -> 165 (the window limit: three chunks, the
    # last of 10 columns)
    'large': [dict(ncam=10, n_imu=3), dict(ncam=11, n_imu=1), dict(ncam=23, n_imu=3)],
    # the `> 1e-5` branch of predict_new_state: gyro exactly 0, |w| = 5e-6, 2e-5, 0.3 rad/s
    'rate': [dict(ncam=1, n_imu=3, gyro='zero'), dict(ncam=1, n_imu=3, gyro=5e-6), dict(ncam=1, n_imu=3, gyro=2e-5), dict(ncam=1, n_imu=3, gyro=0.3)],
    # patterns of exact zeros the kernels' bit masks read off the matrices: identity orientation with the gyro along one axis (zeros in
    # R_w_i and skew(w)), one gyro component exactly 0, a sample with dt = 0 among ordinary ones
    'sparsity': [dict(ncam=1, n_imu=3, gyro='axis_x', q='identity'), dict(ncam=2, n_imu=3, gyro='one_zero'), dict(ncam=1, n_imu=4, dt0=2)],
    # at 5 ms the two branches agree to 1e-20 anywhere near the threshold, so a misplaced threshold cannot show in the cases above: this
    # one can, 5e-5 rad/s across an IMU gap of 20 s (with the branch taken at 1e-4 the 50-digit formulas themselves move q by 4e-11)
    'gap': [dict(ncam=1, n_imu=1, gyro=5e-5, dt=20.0)],
}
SEEDS = {name: 300 + 20 * i for i, name in enumerate(FAMILIES)}

# (K cameras in the window, (i0, i1) to remove): first pair, first and last, last pair, an adjacent and a separated middle pair
REMOVALS = [(2, (0, 1))] + [(K, pr) for K in (11, 24) for pr in ((0, 1), (0, K - 1), (K - 2, K - 1), (K // 2, K // 2 + 1), (2, K - 3))]

# redundancy rule on a window of 6 (key state 2, candidates 3 and 4): (motion of the two candidates, tracking rate) -> what leaves
REDUNDANT = [
    dict(name='both', cand=('near', 'near'), rate=0.9, want=(3, 4)),
    dict(name='neither', cand=('far', 'turned'), rate=0.9, want=(0, 1)),
    dict(name='first_only', cand=('near', 'far'), rate=0.9, want=(0, 3)),            # selected as [3, 0]: the swap to ascending order
    dict(name='second_only', cand=('turned', 'near'), rate=0.9, want=(0, 4)),
    dict(name='rate_exactly_half', cand=('near', 'near'), rate=0.5, want=(0, 1)),    # 0.5 is not > 0.5
    dict(name='rate_low', cand=('near', 'near'), rate=0.3, want=(0, 1)),
    dict(name='full_window', cand=('near', 'far'), rate=0.9, want=(0, 21), ncam=24), # key state 20, candidates 21 and 22
]


def _unit(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def make_cov(rng, n):
    """Symmetric positive definite, block scales of a running filter, every cross block dense."""
    d = np.concatenate([[1e-4] * 3, [1e-6] * 3, [1e-2] * 3, [1e-4] * 3, [1e-2] * 3, [1e-5] * 6] + [[1e-4] * 3 + [1e-2] * 3] * ((n - 21) // 6))
    L = rng.normal(0, 1, (n, 3))
    A = 0.5 * np.eye(n) + L @ L.T / 3
    P = np.sqrt(d)[:, None] * A * np.sqrt(d)
    return (P + P.T) / 2


def make_window(rng, ncam):
    q = np.array([O.small_angle_quaternion(rng.normal(0, 0.03, 3)) for _ in range(ncam)]).reshape(ncam, 4)
    p = np.cumsum(rng.normal(0, 0.15, (ncam, 3)) + np.array([0.15, 0, 0]), axis=0).reshape(ncam, 3)
    return q, p


def make_state(rng, q='random'):
    """The fp64 IMU state of a stream (msckf_ops.MsckfDevice.STATE_FIELDS), null states a perturbed copy."""
    st = dict(ts=100.0 + rng.uniform(0, 1))
    if q == 'identity':
        st['q'] = np.array([0.0, 0.0, 0.0, 1.0])
    else:
        qq = rng.normal(0, 1, 4)
        st['q'] = qq / np.linalg.norm(qq)
    st['p'] = rng.normal(0, 2, 3) + np.array([3.0, -2.0, 1.0])          # |p|, |v| stay away from 0
    st['v'] = rng.normal(0, 0.5, 3) + np.array([1.0, 0.5, -0.3])
    st['bg'], st['ba'] = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
    st['R_ic'] = O.to_rotation(O.small_angle_quaternion(rng.normal(0, 0.5, 3)))
    st['t_ci'] = rng.normal(0, 0.05, 3)
    st['qn'] = O.quaternion_multiplication(O.small_angle_quaternion(rng.normal(0, 2e-3, 3)), st['q'])
    st['pn'], st['vn'] = st['p'] + rng.normal(0, 2e-3, 3), st['v'] + rng.normal(0, 2e-3, 3)
    st['gravity'] = GRAVITY.copy()
    st['tracking_rate'] = 0.9
    return st


def make_case(seed, cfg, ncam, n_imu, gyro=0.3, q='random', dt0=None, dt=DT):
    """-> dict(state: make_state, cam_q, cam_p, P, imu [n_imu, 7], t_frame, noise, n, ncam)."""
    rng = np.random.default_rng(seed)
    st = make_state(rng, q)
    cam_q, cam_p = make_window(rng, ncam)
    n = 21 + 6 * ncam
    axis = _unit(rng)
    imu, t = np.zeros((n_imu, 7)), st['ts']
    for k in range(n_imu):
        if dt0 is None or k != dt0:
            t = t + dt
        if gyro == 'zero':
            w = np.zeros(3)
        elif gyro == 'axis_x':
            w = np.array([0.3 + 0.01 * k, 0.0, 0.0])
        elif gyro == 'one_zero':
            w = np.array([0.2, -0.25 + 0.01 * k, 0.0])
        else:
            w = float(gyro) * (axis + (0.05 * rng.normal(0, 1, 3) if gyro >= 0.1 else 0.0))
            if gyro < 0.1:
                w = float(gyro) * axis                              # the magnitude is the case: |w| = 5e-6 / 2e-5 up to rounding
        f = O.to_rotation(st['q']) @ (-GRAVITY) + rng.normal(0, 0.5, 3)
        imu[k] = np.concatenate([[t], st['bg'] + w, st['ba'] + f])   # (bg + 0) - bg is exactly 0: the zero components survive the bias
    noise = np.array([cfg.gyro_noise, cfg.gyro_bias_noise, cfg.acc_noise, cfg.acc_bias_noise], dtype=np.float64)
    return dict(state=st, cam_q=cam_q, cam_p=cam_p, P=make_cov(rng, n), imu=imu, t_frame=float(t) + 1e-3, noise=noise, n=n, ncam=ncam, seed=seed)


_cache = {}


def family(name, cfg):
    key = ('fam', name)
    if key not in _cache:
        _cache[key] = [dict(make_case(SEEDS[name] + i, cfg, **spec), name='%s[%d]' % (name, i)) for i, spec in enumerate(FAMILIES[name])]
    return _cache[key]


# ---- the oracle on a case -------------------------------------------------------------------------------
def oracle_predict(case, cfg):
    """OracleMSCKF.process_model per sample (with the time stamp batch_imu_processing sets) and state_augmentation on the case.
    -> dict(q, p, v, qn, pn, vn, cam_q, cam_p, P, samples: per IMU sample the arguments of av_msckf_propagate, aug: those of av_msckf_augment)."""
    f = O.OracleMSCKF(cfg)
    s, st = f.imu_state, case['state']
    s.timestamp, s.id = float(st['ts']), case['ncam']
    s.orientation, s.position, s.velocity = st['q'].copy(), st['p'].copy(), st['v'].copy()
    s.gyro_bias, s.acc_bias = st['bg'].copy(), st['ba'].copy()
    s.orientation_null, s.position_null, s.velocity_null = st['qn'].copy(), st['pn'].copy(), st['vn'].copy()
    s.R_imu_cam0, s.t_cam0_imu = st['R_ic'].copy(), st['t_ci'].copy()
    f.gravity = st['gravity'].copy()
    f.Qc = np.diag(np.repeat(case['noise'], 3))
    f.state_cov = case['P'].copy()
    for i in range(case['ncam']):
        c = O.OCAMState(i)
        c.orientation, c.position = case['cam_q'][i].copy(), case['cam_p'][i].copy()
        f.cam_states[i] = c
    samples = []
    for m in case['imu']:
        a = dict(dt=m[0] - s.timestamp, gyro=m[1:4] - s.gyro_bias, acc=m[4:7] - s.acc_bias, q_old=s.orientation.copy(), q_null=s.orientation_null.copy(),
                 v_null=s.velocity_null.copy(), p_null=s.position_null.copy())
        f.process_model(m[0], m[1:4], m[4:7])
        s.timestamp = m[0]
        a.update(q_new=s.orientation.copy(), v_new=s.velocity.copy(), p_new=s.position.copy())
        samples.append(a)
    Rwi = O.to_rotation(s.orientation)
    aug = dict(R_ic=s.R_imu_cam0.copy(), sk=O.skew(Rwi.T @ s.t_cam0_imu))
    f.state_augmentation(case['t_frame'])
    c = f.cam_states[case['ncam']]
    return dict(q=s.orientation.copy(), p=s.position.copy(), v=s.velocity.copy(), qn=s.orientation_null.copy(), pn=s.position_null.copy(),
                vn=s.velocity_null.copy(), cam_q=c.orientation.copy(), cam_p=c.position.copy(), P=f.state_cov.copy(), samples=samples, aug=aug)


# ---- the reference on a case ----------------------------------------------------------------------------
_mp = np.frompyfunc(lambda x: R.mpf(x), 1, 1)


def mp_predict(case):
    """-> dict(q, p, v, cam_q, cam_p, P: objects arrays of mpf; rate_margin; P_prop: the covariance before the augmentation; seconds)."""
    import time
    t0 = time.perf_counter()
    s = R.imu_state(case['state'])
    P = _mp(case['P'])
    P, margin = R.batch_imu_processing(s, P, [(m[0], m[1:4], m[4:7]) for m in case['imu']], case['noise'])
    cam_q, cam_p, Pa = R.state_augmentation(s, P)
    return dict(q=s['q'], p=s['p'], v=s['v'], cam_q=cam_q, cam_p=cam_p, P=Pa, P_prop=P, rate_margin=margin, seconds=time.perf_counter() - t0)


def vec_err(got, ref, quaternion=False):
    got = _mp(np.asarray(got, dtype=np.float64))
    if quaternion and got.dot(ref) < 0:
        got = -got
    return float(R.norm(got - ref) / R.norm(ref))


def cov_err(got, ref):
    """Largest |got_ij - ref_ij| / sqrt(ref_ii ref_jj)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    sd = np.array([R.mp.sqrt(ref[i, i]) for i in range(len(ref))], dtype=object)
    d = np.abs(_mp(got) - ref) / np.outer(sd, sd)
    return float(d.max())


def errors(got, ref):
    """Errors of a launcher's (or the oracle's) result dict against mp_predict's, for the quantities it holds."""
    out = {}
    for k in QUANTITIES:
        if k in got and got[k] is not None:
            out[k] = cov_err(got[k], ref[k]) if k == 'P' else vec_err(got[k], ref[k], quaternion=k in ('q', 'cam_q'))
    return out


def reference(name, cfg):
    """Per case of the family: dict(ref: mp_predict, oracle: oracle_predict, oracle_err, left_out); cached."""
    key = ('ref', name)
    if key not in _cache:
        out = []
        for case in family(name, cfg):
            ref, ora = mp_predict(case), oracle_predict(case, cfg)
            out.append(dict(ref=ref, oracle=ora, oracle_err=errors(ora, ref), left_out=bool(ref['rate_margin'] < MARGIN_MIN)))
        _cache[key] = out
    return _cache[key]


def bars(name, cfg):
    """e_fam per quantity: the oracle's largest error over the family, floored at 4 ulp."""
    refs = reference(name, cfg)
    return {k: max([FLOOR] + [r['oracle_err'][k] for r in refs if not r['left_out']]) for k in QUANTITIES}


# ---- removal and the redundancy rule ----------------------------------------------------------------------
def removal_case(K, seed=700):
    """A window of K camera states and a covariance whose every entry is distinct (the removal is a copy: compared bit for bit)."""
    rng = np.random.default_rng(seed + K)
    return make_cov(rng, 21 + 6 * K)


def redundant_case(spec, seed=800):
    """-> (cam_q, cam_p, tracking rate): key state at ncam - 4, the two candidates behind it moved as spec['cand'] says --
    'near': 0.05 rad, 0.1 m (redundant), 'far': 0.05 rad, 0.8 m, 'turned': 0.5 rad, 0.1 m."""
    ncam = spec.get('ncam', 6)
    rng = np.random.default_rng(seed + sum(map(ord, spec['name'])))
    q, p = make_window(rng, ncam)
    key = ncam - 4
    for j, kind in enumerate(spec['cand']):
        ang, dist = (0.5 if kind == 'turned' else 0.05), (0.8 if kind == 'far' else 0.1)
        q[key + 1 + j] = O.quaternion_multiplication(O.small_angle_quaternion(ang * _unit(rng)), q[key])
        p[key + 1 + j] = p[key] + dist * _unit(rng)
    return q, p, spec['rate']


def redundant_reference(spec):
    key = ('red', spec['name'])
    if key not in _cache:
        q, p, rate = redundant_case(spec)
        pos, info = R.find_redundant_cam_states(q, p, rate)
        _cache[key] = dict(pos=tuple(pos), info=info, margin=min(i['margin'] for i in info), left_out=bool(min(i['margin'] for i in info) < MARGIN_MIN))
    return _cache[key]


def oracle_redundant(spec, cfg):
    q, p, rate = redundant_case(spec)
    f = O.OracleMSCKF(cfg)
    for i in range(len(q)):
        c = O.OCAMState(i)
        c.orientation, c.position = q[i].copy(), p[i].copy()
        f.cam_states[i] = c
    f.tracking_rate = rate
    return tuple(f.find_redundant_cam_states())
