"""tests/msckf_update_cases.py -- TEST INFRASTRUCTURE ONLY.

Seeded inputs for the batched measurement update's back end (upd_stack_kernel, the direct Cholesky pipeline on the matrix instruction,
the Gram-matrix row compression, the information form), with the fp64 oracle (oracle/msckf_np.py: measurement_update), the fp64
statements of the three methods (tests/msckf_update_methods.py) and the 50-digit reference (tests/msckf_mp_ref.py: measurement_update
and its push-through form) evaluated on them, and the bars the kernels are held to.  Shared by tests/test_msckf_mp_ref.py (CPU) and
tests/test_gpu_msckf_update.py; every reference value is computed once per process and cached.

A case is one stream: a symmetric positive definite covariance (msckf_predict_cases.make_cov), a window of camera states, and a list of
candidate features in map order -- camera slot of every observation, gate flag, first row of its block in the block buffer -- with the
blocks themselves.  The blocks lie in the buffer in a shuffled order with gaps between them, non-passing features stand among the
passing ones (their rows, the gaps and every column no stacked feature touches hold NaN: whatever reads them shows), so that no row map
is the identity.  Blocks come in two kinds: `geo` -- the oracle's feature_jacobian (projection onto the left null space of H_f
included) of synthetic tracks over the window, so that the stacked Jacobian has its real rank deficiency: it is blind to a rigid motion
of the observing cameras -- and `dense`: seeded normal entries in the observing cameras' columns.  A feature of M observations has
4 M - 3 rows; the stacked row count m of a case is composed of such blocks.

Errors: P+ entry by entry relative to sqrt(P+_ii P+_jj) of the reference's result; delta_x entry by entry relative to sqrt(P_ii) of the
PRIOR.  Bars, by the rule of msckf_feature_cases (no new constant, none from a kernel): per family and path e_fam is the larger of the
fp64 oracle's error and of the error of the path's method statement against the 50-digit reference, floored at 4 ulp; a kernel may be
FACTOR = 16 times that.  No case is left out: the only floating-point decision of this code is the pivot test, the stacking decisions
are integer.
"""
import time

import numpy as np

import msckf_feature_cases as Fc
import msckf_mp_ref as R
import msckf_predict_cases as Pc
import msckf_update_methods as Um
from msckf_feature_cases import EPS, FACTOR, GRAVITY      # noqa: F401  (the project's constants, no new one)
from oracle import msckf_np as O

CAM_STRIDE, LD = Pc.CAM_STRIDE, Pc.LD                     # every launch: a window of 24, ld = 165
FLOOR = 4 * EPS
OLD_BAR = 1e-6                                            # what tests/test_gpu_msckf.py already enforces on delta_x: no family's bar may be looser
DIRECT_REF_MAX = 3.0e5                                    # reference cost only (no bar depends on it): multiply-adds of the m x m form above which the cheaper
                                                          # of the two 50-digit forms, held equal by tests/test_msckf_mp_ref.py, is the reference (about 1 s here)


def C(name, n, cams, m, kind, **kw):
    return dict(name=name, n=n, cams=tuple(cams), m=m, kind=kind, **kw)


# family -> cases (n, touched camera slots, stacked rows m, kind of blocks).  path: which back end the launch configuration sends it to.
FAMILIES = {
    # phase 0 (cut at 1500 rows, no information form), kch = DEV_KCH: m <= 136 is factorised as it stands
    'direct': dict(phase=0, path='direct', cases=[
        C('k1', 27, [0], 1, 'geo'),                                   # a single one-row block: k = 1
        C('m5', 33, [0, 1], 5, 'dense'),
        C('m15', 45, [0, 1, 2, 3], 15, 'geo'), C('m16', 45, [0, 1, 2, 3], 16, 'dense'), C('m17', 45, [0, 1, 2, 3], 17, 'geo'),       # a tile edge at k = 16
        C('m31', 45, [0, 1, 2, 3], 31, 'dense'), C('m32', 45, [0, 1, 2, 3], 32, 'geo'), C('m33', 45, [0, 1, 2, 3], 33, 'dense'),     # a block edge at k = 32
        C('n69_m65', 69, [1, 2, 4, 5, 7], 65, 'geo'),                 # n and k both cross 64
        C('m136', 45, [0, 1, 2, 3], 136, 'dense'),                    # m = DEV_KCH: nine block columns in the factor, the last of 8 rows
        C('full_window', 165, [0, 11, 23], 13, 'geo'),                # n = ld; first, a middle and the last camera: columns up to 164
    ]),
    # the same configuration, m > DEV_KCH: Gram matrix, bordered Cholesky with E, then the direct pipeline on k = nc rows
    'compress': dict(phase=0, path='compress', cases=[
        C('m137', 51, [0, 1, 2, 3, 4], 137, 'geo'),                   # the first m over DEV_KCH; k1 = 31
        C('m256', 45, [1, 3], 256, 'dense'), C('m257', 45, [1, 3], 257, 'geo'),      # either side of GRAM_CHUNK
        C('m300', 57, [0, 1, 2, 3, 4, 5], 300, 'geo'),                # k1 = 37: a second 32-block in the Gram matrix and its factor
        C('m513', 39, [0, 1, 2], 513, 'dense'),                       # k1 = 19, three chunks
        C('cut', 45, [0, 1, 2, 3], 1508, 'dense', block=4, behind_cut=5),            # 116 blocks of 13 rows cross 1500; five passing features behind
        C('zero_cam', 45, [0, 1, 2], 150, 'dense', zero_cam=1),       # a touched camera whose six columns are exactly zero: what E is for
        C('cut_exact', 33, [0, 1], 1505, 'dense', block=2, behind_cut=3),             # 300 blocks of 5 rows stack exactly 1500: one more is taken, then the cut
        C('zero_r', 45, [1, 3], 150, 'dense', zero_r=True),           # r = 0 exactly: rho = 0, the border pivot is the `+ 1` alone; delta_x = 0
    ]),
    # phase 1 (no cut, information form allowed): compact 12-double rows of the two-camera pruning update, and full-width rows
    'info': dict(phase=1, path='info', cases=[
        C('c_m5', 33, [0, 1], 5, 'geo', hld=12),                      # m < nc
        C('c_m95', 33, [0, 1], 95, 'dense', hld=12), C('c_m96', 81, [0, 1], 96, 'geo', hld=12), C('c_m97', 165, [0, 1], 97, 'geo', hld=12),   # INFO_CH = 96
        C('c_m480', 165, [0, 23], 480, 'dense', hld=12),              # five chunks; the pair at window positions (0, 23)
        C('c_m96_far', 165, [0, 23], 96, 'geo', hld=12),              # the INFO_CH edge with the far pair and geometric blocks
        C('w_nc6', 45, [2], 30, 'dense'), C('w_nc24', 45, [0, 1, 2, 3], 100, 'geo'),           # full-width rows: nc = 6 and nc = 24 = INFO_NC
    ]),
}
THREE_WAYS = C('three_ways', 45, [1, 2], 40, 'geo')       # one problem through all three paths
SEEDS = {'direct': 1100, 'compress': 1200, 'info': 1300, 'three_ways': 1400, 'shapes': 1500, 'pivot': 1600}


def compose(m, Mmax):
    """Observation counts of blocks of 4 M - 3 rows (M <= Mmax) that add up to m rows, largest first."""
    out = []
    while m > 0:
        M = min(Mmax, (m + 3) // 4)
        out.append(M)
        m -= 4 * M - 3
    return out


def make_case(spec, seed, obs_noise, cfg):
    """-> dict(spec fields, P [n, n], feats: [dict(cams, ok, row)], H [rows_cap, ld or hld], r [rows_cap], cam_q/p/qn/pn, rows_cap)."""
    rng = np.random.default_rng(seed)
    n, touched, m, kind, hld = spec['n'], list(spec['cams']), spec['m'], spec['kind'], spec.get('hld', 0)
    ncam = (n - 21) // 6
    P = Pc.make_cov(rng, n)
    q, p, qn, pn = Fc._cameras(rng, ncam, 0.15)
    T01 = np.array(cfg.T_cn_cnm1, dtype=np.float64)
    fam = dict(name=spec['name'], M=len(touched), T01=T01, opt=cfg.optimization_config, cam_q=q, cam_p=p, cam_qn=qn, cam_pn=pn, obs=[], seed=seed)
    flt = Fc.oracle_filter(fam, P, cfg)
    Ms = [spec['block']] * (m // (4 * spec['block'] - 3)) if 'block' in spec else compose(m, len(touched))
    assert sum(4 * M - 3 for M in Ms) == m
    feats, blocks = [], []
    cols_all = np.array([21 + 6 * c + e for c in touched for e in range(6)])

    def block(cams, fid):
        rows = 4 * len(cams) - 3
        own = np.array([21 + 6 * c + e for c in cams for e in range(6)])
        Hb = np.zeros((rows, n))
        if kind == 'dense':
            Hb[:, own] = rng.normal(0, 1, (rows, len(own)))
            rb = rng.normal(0, 0.05, rows) * (0.0 if spec.get('zero_r') else 1.0)
            if 'zero_cam' in spec:
                zc = touched[spec['zero_cam']]
                Hb[:, 21 + 6 * zc:27 + 6 * zc] = 0.0
        else:
            c0, d = cams[0], 5.0 * rng.uniform(0.8, 1.25)
            pw = p[c0] + O.to_rotation(q[c0]).T @ np.array([rng.uniform(-0.25, 0.25) * d, rng.uniform(-0.2, 0.2) * d, d])
            f = O.OFeature(fid, fam['opt'])
            for c in cams:
                f.observations[c] = Fc._project(q[c], p[c], T01, pw) + rng.normal(0, 0.002, 4)
            f.position = pw + rng.normal(0, 0.005, 3)
            flt.map_server[fid] = f
            Hb, rb = flt.feature_jacobian(fid, list(cams))
        return Hb, rb

    k_rot = 0
    for j, M in enumerate(Ms):
        if M == len(touched):
            cams = list(touched)
        else:                                       # smaller blocks walk through the touched cameras
            cams = sorted(touched[(k_rot + e) % len(touched)] for e in range(M))
            k_rot += M
        feats.append(dict(cams=cams, ok=1))
        blocks.append(block(cams, j))
        if j % 2 == 1 or j == 0:                    # a candidate the gate rejected, seen from any cameras of the window
            Mr = int(rng.integers(1, min(ncam, 4) + 1))
            feats.append(dict(cams=sorted(int(c) for c in rng.choice(ncam, Mr, replace=False)), ok=0))
            blocks.append(None)
    for j in range(spec.get('behind_cut', 0)):      # passing features behind the cut: the reference never reaches them
        feats.append(dict(cams=list(touched), ok=1))
        blocks.append(None)
    assert sorted({c for f, b in zip(feats, blocks) if b is not None for c in f['cams']}) == sorted(touched)
    # the block buffer: blocks in a shuffled order with gaps, NaN wherever no stacked feature has a value to be read
    order = rng.permutation(len(feats))
    cursor = int(rng.integers(1, 4))
    for i in order:
        feats[i]['row'] = cursor
        cursor += 4 * len(feats[i]['cams']) - 3 + int(rng.integers(0, 3))
    rows_cap = cursor + 2
    width = hld if hld > 0 else LD
    H, r = np.full((rows_cap, width), np.nan), np.full(rows_cap, np.nan)
    for f, b in zip(feats, blocks):
        if b is None:
            continue
        sl = slice(f['row'], f['row'] + len(b[1]))
        if hld > 0:
            H[sl, :len(cols_all)] = b[0][:, cols_all]
        else:
            H[sl, cols_all] = b[0][:, cols_all]
        r[sl] = b[1]
    return dict(spec, P=P, feats=feats, H=H, r=r, rows_cap=rows_cap, cam_q=q, cam_p=p, cam_qn=qn, cam_pn=pn, ncam=ncam, hld=hld, fam=fam, obs_noise=obs_noise)


_cache = {}


def family(name, cfg):
    key = ('fam', name)
    if key not in _cache:
        specs = [THREE_WAYS] if name == 'three_ways' else FAMILIES[name]['cases']
        _cache[key] = [make_case(s, SEEDS[name] + 7 * i, cfg.observation_noise, cfg) for i, s in enumerate(specs)]
    return _cache[key]


def stacked_problem(case, phase, kch=Um.KCH):
    """The stacking rule on the case and the stacked (Hc, r, cols) it selects."""
    rule = Um.stack_rule(case['feats'], phase, kch=kch)
    Hc, r = Um.gather(case['feats'], rule['taken'], case['H'], case['r'], rule['cols'], case['hld'])
    assert np.isfinite(Hc).all() and np.isfinite(r).all() and len(r) == rule['m']
    return rule, Hc, r


def direct_cost(k, nc, n):
    return k * nc * n + k * k * nc + k ** 3 / 3 + k * k * n + n * n * k


def info_cost(m, nc, n):
    return m * nc * nc + nc ** 3 + n * nc * nc + n * n * nc


def reference(case, phase, cfg):
    """The 50-digit update of the case's stacked problem: dict(dx, P, sd: sqrt(diag P+), form, seconds, madds, rule, Hc, r); cached."""
    key = ('ref', case['name'], phase)
    if key not in _cache:
        rule, Hc, r = stacked_problem(case, phase)
        m, nc, n = rule['m'], rule['nc'], case['n']
        t0 = time.perf_counter()
        if direct_cost(m, nc, n) <= max(DIRECT_REF_MAX, info_cost(m, nc, n)):
            form, madds = 'direct', direct_cost(m, nc, n)
            dx, Pn = R.measurement_update(Hc, r, case['P'], rule['cols'], case['obs_noise'])
        else:
            form, madds = 'push-through', info_cost(m, nc, n)
            dx, Pn = R.measurement_update_info(Hc, r, case['P'], rule['cols'], case['obs_noise'])
        _cache[key] = dict(dx=dx, P=Pn, form=form, madds=madds, seconds=time.perf_counter() - t0, rule=rule, Hc=Hc, r=r)
    return _cache[key]


def errors(dx, Pn, ref, P_prior):
    """-> dict(P: largest |P_ij - ref_ij| / sqrt(ref_ii ref_jj), dx: largest |dx_i - ref_i| / sqrt(prior_ii))."""
    n = len(P_prior)
    d = np.abs(R.M(np.asarray(dx, dtype=np.float64)[:n]) - ref['dx'])
    sd = np.sqrt(np.diag(P_prior))
    return dict(P=Pc.cov_err(np.asarray(Pn)[:n, :n], ref['P']), dx=float(max(d[i] / R.mpf(float(sd[i])) for i in range(n))))


def oracle_errors(case, ref, cfg):
    rule, Hc, r = ref['rule'], ref['Hc'], ref['r']
    H = np.zeros((len(r), case['n']))
    H[:, rule['cols']] = Hc
    flt = Fc.oracle_filter(case['fam'], case['P'], cfg)
    flt.imu_state.velocity = np.zeros(3)        # (the oracle injects delta_x into its state IN PLACE, and a new filter's velocity is the config's own array)
    flt.measurement_update(H, r.copy())
    return errors(flt.debug['delta_x'], flt.state_cov, ref, case['P'])


def method_errors(case, ref, path):
    rule = ref['rule']
    dx, Pn = Um.METHODS[path](ref['Hc'], ref['r'], case['P'], rule['cols'], case['obs_noise'])
    return errors(dx, Pn, ref, case['P'])


def family_errors(name, cfg, path=None, phase=None):
    """Per case: dict(oracle, method: error dicts, left_out = 0); cached.  path / phase default to the family's."""
    path = FAMILIES[name]['path'] if path is None else path
    phase = FAMILIES[name]['phase'] if phase is None else phase
    key = ('err', name, path, phase)
    if key not in _cache:
        out = []
        for case in family(name, cfg):
            ref = reference(case, phase, cfg)
            out.append(dict(name=case['name'], oracle=oracle_errors(case, ref, cfg), method=method_errors(case, ref, path), left_out=0, ref=ref))
        _cache[key] = out
    return _cache[key]


def bars(name, cfg, path=None, phase=None):
    """e_fam per quantity: the larger of the oracle's and the method statement's error over the family, floored at 4 ulp."""
    errs = family_errors(name, cfg, path, phase)
    return {k: max([FLOOR] + [max(e['oracle'][k], e['method'][k]) for e in errs if not e['left_out']]) for k in ('P', 'dx')}


def shift_of_regulariser(case, ref):
    """What E itself moves, at 50 digits: the regularised problem's update against the reference's, in the two error measures."""
    rule = ref['rule']
    dx, Pn = R.measurement_update_regularised(ref['Hc'], ref['r'], case['P'], rule['cols'], case['obs_noise'])
    n = case['n']
    sd = np.sqrt(np.diag(case['P']))
    sdp = np.array([R.mp.sqrt(ref['P'][i, i]) for i in range(n)], dtype=object)
    return dict(P=float((np.abs(Pn - ref['P']) / np.outer(sdp, sdp)).max()), dx=float(max(abs(dx[i] - ref['dx'][i]) / R.mpf(float(sd[i])) for i in range(n))))
