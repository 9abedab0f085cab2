"""tests/msckf_feature_cases.py -- TEST INFRASTRUCTURE ONLY.

Seeded inputs for the per-feature chain of the filter (triangulation, projected Jacobian rows, chi^2 gate), the fp64 oracle and the
50-digit reference evaluated on them, and the bars the GPU kernels are held to.  Shared by tests/test_msckf_mp_ref.py (CPU: oracle
against reference) and tests/test_gpu_msckf_features.py (kernels against reference); every reference value is computed once per
process and cached.

A family is one set of camera states, one covariance and about 12 features with the same number of observations.  Camera states: small
rotations, a random-walk position (the cameras look along +z), null-space states a perturbed copy.  Covariance: random symmetric
positive definite, camera blocks strongly correlated (rank 3 plus diagonal), scaled per family so that the non-zero eigenvalues of
H P H^T of its first feature span 1e-6 .. 1e+3 times the observation noise.  The rows / gate stage of every feature takes the fp64 rounding of the
reference's triangulated position and measurements of its own: the feature's true projections with a noise of 0.002, and of 0.03 --
about the observation noise -- for every other feature, so that the gate rejects some and both outcomes occur.

Bars (none comes from the code under test).  With e_fam the largest error of the fp64 ORACLE against the 50-digit reference over the
family's decided features, floored at 4 ulp of the quantity's scale, a kernel may be 16 e_fam off: four bits for a different but
legitimate summation order (a 64-lane tree against a sequential sum) and for contraction into fused multiply-adds.  Triangulation adds
und * d * max(1, d) for the Levenberg-Marquardt steps fp64 cannot decide (msckf_mp_ref.triangulate): a step delta in (alpha, beta, rho)
moves the point by about d |delta| across and d^2 |delta| along the ray at depth d.  Position errors are relative to the size of the
problem (pos_err).
"""
import os

import numpy as np
from scipy.stats import chi2

import msckf_mp_ref as R
from conftest import ROOT
from oracle import msckf_np as O

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EPS = 2.0 ** -52
FACTOR = 16.0
MARGIN_MIN = 1e-9           # a Huber / stop / gate margin below this leaves the case out of the comparison
GRAVITY = np.array([0.0, 0.0, -9.81])
CHI2 = np.zeros(100)
CHI2[1:] = [chi2.ppf(0.05, i) for i in range(1, 100)]

# name -> observations per feature, depth [m], camera step per frame [m], measurement noise, features, features that get the gate
FAMILIES = {
    'm1_5m': dict(M=1, depth=5.0, step=0.15, noise=0.002, n=12, gate=0),
    'm2_5m': dict(M=2, depth=5.0, step=0.15, noise=0.002, n=12, gate=12),
    'm3_5m': dict(M=3, depth=5.0, step=0.15, noise=0.002, n=12, gate=12),
    'm4_40m_lowpar': dict(M=4, depth=40.0, step=0.02, noise=0.0005, n=12, gate=12),
    'm5_5m': dict(M=5, depth=5.0, step=0.15, noise=0.002, n=12, gate=12),
    'm8_100m': dict(M=8, depth=100.0, step=0.3, noise=0.0005, n=12, gate=6),
    'm9_100m': dict(M=9, depth=100.0, step=0.3, noise=0.0005, n=12, gate=6),
    'm9_huber': dict(M=9, depth=8.0, step=0.15, noise=0.02, n=12, gate=6),
    'm20_10m': dict(M=20, depth=10.0, step=0.1, noise=0.002, n=12, gate=2),
    'm32_10m': dict(M=32, depth=10.0, step=0.08, noise=0.002, n=4, gate=0),
}
SEEDS = {name: 100 + i for i, name in enumerate(FAMILIES)}


def _small_q(rng, sigma):
    return O.small_angle_quaternion(rng.normal(0, sigma, 3))


def _project(q, p, T01, pw):
    """(u0, v0, u1, v1) of world point pw in the stereo pair at camera state (q, p)."""
    Rw0 = O.to_rotation(q)
    p0 = Rw0 @ (pw - p)
    Rw1 = T01[:3, :3] @ Rw0
    p1 = Rw1 @ (pw - (p - Rw1.T @ T01[:3, 3]))
    return np.array([p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]])


def _cameras(rng, n_cam, step):
    q = np.array([_small_q(rng, 0.03) for _ in range(n_cam)])
    p = np.cumsum(rng.normal(0, step, (n_cam, 3)) + np.array([step, 0, 0]), axis=0)
    qn = np.array([O.quaternion_multiplication(_small_q(rng, 2e-3), qq) for qq in q])
    pn = p + rng.normal(0, 2e-3, p.shape)
    return q, p, qn, pn


def make_family(name, cfg, variant=0):
    """-> dict(name, M, T01, opt, cam_q, cam_p, cam_qn, cam_pn, obs: [[(camera, z4), ...] per feature], pts: the true points, n_gate).
    variant > 0: the same family from another seed (a second stream for the launch-shape tests; it has no reference of its own)."""
    spec = FAMILIES[name]
    seed = SEEDS[name] + 500 * variant
    rng = np.random.default_rng(seed)
    M, T01 = spec['M'], np.array(cfg.T_cn_cnm1, dtype=np.float64)
    n_cam = M + 2
    q, p, qn, pn = _cameras(rng, n_cam, spec['step'])
    obs, pts = [], []
    for _ in range(spec['n']):
        cams = np.sort(rng.choice(n_cam, M, replace=False))
        d = spec['depth'] * rng.uniform(0.8, 1.25)
        c0 = int(cams[0])
        pw = p[c0] + O.to_rotation(q[c0]).T @ np.array([rng.uniform(-0.25, 0.25) * d, rng.uniform(-0.2, 0.2) * d, d])
        obs.append([(int(c), _project(q[c], p[c], T01, pw) + rng.normal(0, spec['noise'], 4)) for c in cams])
        pts.append(pw)
    return dict(pts=pts, name=name if variant == 0 else '%s#%d' % (name, variant), M=M, T01=T01, opt=cfg.optimization_config, cam_q=q, cam_p=p, cam_qn=qn, cam_pn=pn,
                obs=obs, n_gate=spec['gate'], seed=seed)


def make_recorded(cfg):
    """The 60 recorded triangulation cases of tests/golden/msckf_units.npz (tracks of 3 .. 24 observations), with the reference's results."""
    u = np.load(os.path.join(GOLDEN, 'msckf_units.npz'))
    obs = []
    for i in range(len(u['t_obs'])):
        obs.append([(k, u['t_obs'][i, k].copy()) for k in range(u['t_obs'].shape[1]) if not np.isnan(u['t_obs'][i, k, 0])])
    return dict(name='recorded', M=max(len(o) for o in obs), T01=np.array(cfg.T_cn_cnm1, dtype=np.float64), opt=cfg.optimization_config,
                cam_q=u['t_cam_q'].copy(), cam_p=u['t_cam_p'].copy(), cam_qn=u['t_cam_q'].copy(), cam_pn=u['t_cam_p'].copy(), obs=obs, n_gate=0,
                ref_pos=u['t_pos'].copy(), ref_ok=u['t_ok'].astype(bool))


def make_special(cfg):
    """Two features that must come out INVALID: one that lies behind its cameras (consistent measurements of a point at negative depth),
    and one with zero parallax -- identity camera, a stereo pair that differs by a pure translation, the same image point in both: the
    two-view guess divides zero by zero, fp64 carries NaN through every comparison, and the depth check fails.  (The 50-digit reference
    reports the division as degenerate and invalid.)  Each comes with the stereo transform it is to be run with."""
    rng = np.random.default_rng(77)
    T01 = np.array(cfg.T_cn_cnm1, dtype=np.float64)
    q, p, qn, pn = _cameras(rng, 4, 0.15)
    pw = p[0] + O.to_rotation(q[0]).T @ np.array([0.4, -0.3, -5.0])
    behind = [(c, _project(q[c], p[c], T01, pw)) for c in range(3)]
    Tt = np.eye(4)
    Tt[0, 3] = -0.11
    qi = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (4, 1))
    flat = [(c, np.array([0.1, 0.2, 0.1, 0.2])) for c in range(3)]
    base = dict(M=3, opt=cfg.optimization_config, n_gate=0)
    return [dict(base, name='behind', T01=T01, cam_q=q, cam_p=p, cam_qn=qn, cam_pn=pn, obs=[behind]),
            dict(base, name='zero_parallax', T01=Tt, cam_q=qi, cam_p=np.zeros((4, 3)), cam_qn=qi, cam_pn=np.zeros((4, 3)), obs=[flat])]


# ---- the fp64 oracle on a family -----------------------------------------------------------------------
class _Cam(object):
    pass


def oracle_triangulate(fam, i):
    cams = {}
    for k in range(len(fam['cam_q'])):
        c = _Cam()
        c.orientation, c.position = fam['cam_q'][k], fam['cam_p'][k]
        cams[k] = c
    f = O.OFeature(i, fam['opt'])
    for ci, z in fam['obs'][i]:
        f.observations[ci] = z
    with np.errstate(all='ignore'):
        ok = O.initialize_position(f, cams, fam['T01'][:3, :3], fam['T01'][:3, 3])
    return f.position.copy(), bool(ok)


def oracle_filter(fam, P, cfg):
    """An OracleMSCKF whose camera states, covariance and stereo transform are the family's."""
    flt = O.OracleMSCKF(cfg)
    flt.R_cam0_cam1, flt.t_cam0_cam1 = fam['T01'][:3, :3], fam['T01'][:3, 3]
    flt.gravity = GRAVITY.copy()
    for k in range(len(fam['cam_q'])):
        cs = O.OCAMState(k)
        cs.orientation, cs.position = fam['cam_q'][k].copy(), fam['cam_p'][k].copy()
        cs.orientation_null, cs.position_null = fam['cam_qn'][k].copy(), fam['cam_pn'][k].copy()
        flt.cam_states[k] = cs
    flt.state_cov = P.copy()
    return flt


def oracle_rows(flt, fam, i, pos, obs=None):
    """feature_jacobian + gating_test of the oracle on feature i (observations `obs`, default the family's) at position pos
    -> (H_o on the own columns, r_o, gamma, the full-width H_o)."""
    obs = fam['obs'][i] if obs is None else obs
    f = O.OFeature(i, fam['opt'])
    for ci, z in obs:
        f.observations[ci] = z
    f.position = np.array(pos, dtype=np.float64)
    flt.map_server[i] = f
    cam_ids = [ci for ci, _ in obs]
    Ho, ro = flt.feature_jacobian(i, cam_ids)
    flt.debug.pop('gamma', None)
    flt.gating_test(Ho, ro, dof_of(len(cam_ids)))
    return Ho[:, R.own_columns(obs)], ro, float(flt.debug['gamma'][-1]), Ho


def dof_of(M):
    """chi^2 degrees of freedom the filter gates a feature with: its two observations in the camera pruning (msckf.py:761), M - 1 for a
    lost feature (msckf.py:662)."""
    return 2 if M == 2 else M - 1


def make_cov(fam, cfg, pos0):
    """The family's covariance (see the module docstring), scaled on the projected Jacobian of feature 0 at position pos0."""
    rng = np.random.default_rng(fam['seed'] + 1000)
    n = 21 + 6 * len(fam['cam_q'])
    L = rng.normal(0, 1, (n, 3))
    D = np.diag(rng.uniform(0.5, 1.5, n))
    flt = oracle_filter(fam, np.eye(n), cfg)
    Ho = oracle_rows(flt, fam, 0, pos0)[3]
    s2 = cfg.observation_noise
    a = 1e3 * s2 / np.linalg.eigvalsh(Ho @ (L @ L.T) @ Ho.T).max()
    # (H_x has rank 3 per observation -- its rotation columns are H_f times a 3 x 3 matrix -- so the projected rows have rank 3M - 3 and
    #  H P H^T has M zero eigenvalues whatever P is: the span is that of the 3M - 3 others)
    b = 1e-6 * s2 / np.sort(np.linalg.eigvalsh(Ho @ D @ Ho.T))[::-1][3 * fam['M'] - 4]
    P = a * (L @ L.T) + b * D
    return (P + P.T) / 2


# ---- reference, oracle and bars of a family, computed once ---------------------------------------------
_cache = {}


def tri_reference(fam):
    """Per feature: the 50-digit triangulation (msckf_mp_ref.triangulate; a zero-by-zero two-view guess reads degenerate and invalid), the
    oracle's position and flag, and whether the feature is left out of the position / flag comparison."""
    key = ('tri', fam['name'])
    if key in _cache:
        return _cache[key]
    out = []
    for i, obs in enumerate(fam['obs']):
        try:
            t = R.triangulate(obs, fam['cam_q'], fam['cam_p'], fam['T01'], fam['opt'])
            t['degenerate'] = False
        except ZeroDivisionError:
            t = dict(pos=None, valid=False, degenerate=True, und=R.ZERO, depth=R.ONE, huber_margin=R.ONE, stop_margin=R.ONE, n_huber=0, outer=0)
        opos, ook = oracle_triangulate(fam, i)
        t['left_out'] = bool(min(t['huber_margin'], t['stop_margin']) < MARGIN_MIN)
        t['pos64'] = None if t['pos'] is None else R.F(t['pos'])
        t['oracle_pos'], t['oracle_valid'] = opos, ook
        d = abs(float(t['depth']))
        t['slack'] = float(t['und']) * d * max(1.0, d)
        t['oracle_err'] = pos_err(opos, t)
        out.append(t)
    _cache[key] = out
    return out


def pos_err(p64, t):
    """Error of an fp64 position against the reference entry t of tri_reference: |p64 - pos| relative to the size of the problem, the
    larger of |pos| and the depth in the first view.  (The 60 recorded cases have their cameras within a metre of the origin, so this is
    the relative error |p64 - pos| / |pos| there.)"""
    if t['pos'] is None:
        return np.inf
    return float(R.norm(R.M(p64) - t['pos']) / max(R.norm(t['pos']), abs(t['depth'])))


def tri_bar(fam):
    """e_fam: the oracle's largest position error (pos_err) over the family's decided (und = 0), valid, compared features, floored at
    4 ulp."""
    ref = tri_reference(fam)
    errs = [t['oracle_err'] for t in ref if t['und'] == 0 and not t['left_out'] and not t['degenerate'] and t['valid']]
    return max(errs + [4 * EPS])


def rel_err(x, xmp):
    """max |x - xmp| relative to the largest |entry| of xmp (x: fp64 or mpf values, xmp: mpf)."""
    x, xmp = R.M(np.asarray(x, dtype=object).reshape(-1)), np.asarray(xmp, dtype=object).reshape(-1)
    return float(max(abs(a - b) for a, b in zip(x, xmp)) / max(abs(b) for b in xmp))


def _ld_to_mp(a):
    """long double array -> mpf, exactly (two fp64 pieces)."""
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    lo = (a - hi).astype(np.float64)
    return R.M(hi) + R.M(lo)


def rows_errors(Ho_own, ro, ref):
    """Errors of projected rows (any null-space basis) against the three invariants of the reference, each relative to its own largest
    entry.  The rows enter exactly.  Up to 40 rows the products are formed in 50 digits; beyond (H_o^T H_o of a 20-observation track is
    a million 50-digit products) in the 64-bit mantissa of long double, whose error over 77 terms, 4e-18 of the scale, is two hundred
    times below the 4 ulp floor of every bar."""
    if len(ro) <= 40 or np.finfo(np.longdouble).nmant < 63:
        HtH, Htr, rtr = R.rows_invariants(Ho_own, ro)
    else:
        H, r = np.asarray(Ho_own, dtype=np.longdouble), np.asarray(ro, dtype=np.longdouble)
        HtH, Htr, rtr = _ld_to_mp(H.T @ H), _ld_to_mp(H.T @ r), _ld_to_mp([r @ r])[0]
    return rel_err(HtH, ref['HtH']), rel_err(Htr, ref['Htr']), rel_err([rtr], [ref['rtr']])


def gate_obs(fam):
    """The measurements the rows / gate stage is given for the family's first n_gate features (module docstring)."""
    rng = np.random.default_rng(fam['seed'] + 2000)
    obs = []
    for i in range(fam['n_gate']):
        s = 0.03 if i % 2 else 0.002    # every other feature: measurements off by about the observation noise, for the gate to reject
        obs.append([(c, _project(fam['cam_q'][c], fam['cam_p'][c], fam['T01'], fam['pts'][i]) + rng.normal(0, s, 4)) for c, _ in fam['obs'][i]])
    return obs


def gate_inputs(fam, cfg):
    """What the rows / gate stage is given for the family's first n_gate features: positions (fp64), observations, and the covariance."""
    key = ('gin', fam['name'])
    if key in _cache:
        return _cache[key]
    ref = tri_reference(fam)
    pos = np.array([ref[i]['pos64'] for i in range(fam['n_gate'])])
    obs = gate_obs(fam)
    P = make_cov(fam, cfg, pos[0]) if fam['n_gate'] else None
    _cache[key] = (pos, obs, P)
    return _cache[key]


def gate_reference(fam, cfg):
    """Per gated feature: the reference's invariants and gamma, its decision, the gate margin, and the oracle's errors."""
    key = ('gate', fam['name'])
    if key in _cache:
        return _cache[key]
    pos, gobs, P = gate_inputs(fam, cfg)
    flt = oracle_filter(fam, P, cfg) if fam['n_gate'] else None
    out = []
    for i in range(fam['n_gate']):
        obs = gobs[i]
        rows = R.feature_rows(obs, pos[i], fam['cam_q'], fam['cam_p'], fam['cam_qn'], fam['cam_pn'], fam['T01'], GRAVITY)
        own = R.own_columns(obs)
        g = R.gamma(rows, P[np.ix_(own, own)], cfg.observation_noise)
        thr = R.mpf(float(CHI2[dof_of(len(obs))]))
        Ho, ro, og, _ = oracle_rows(flt, fam, i, pos[i], obs)
        e = rows_errors(Ho, ro, rows)
        out.append(dict(rows=rows, gamma=g, ok=bool(g < thr), margin=float(abs(g - thr) / thr), dof=dof_of(len(obs)),
                        oracle_err=dict(HtH=e[0], Htr=e[1], rtr=e[2], gamma=float(abs(R.mpf(og) - g) / abs(g))), oracle_gamma=og,
                        left_out=bool(abs(g - thr) / thr < MARGIN_MIN)))
    _cache[key] = out
    return out


def gate_bars(fam, cfg):
    """e_fam of the three invariants and of gamma: the oracle's largest relative error over the family, floored at 4 ulp."""
    ref = gate_reference(fam, cfg)
    return {k: max([g['oracle_err'][k] for g in ref] + [4 * EPS]) for k in ('HtH', 'Htr', 'rtr', 'gamma')}
