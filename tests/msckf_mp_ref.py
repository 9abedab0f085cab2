"""tests/msckf_mp_ref.py -- TEST INFRASTRUCTURE ONLY.

A 50-digit (mpmath) restatement of the filter's per-feature chain, formula for formula after oracle/msckf_np.py
(initialize_position, measurement_jacobian, feature_jacobian, gating_test), with no cleverness: it is the yardstick the fp64
oracle and the HIP kernels are both measured against.  Inputs are fp64 and enter exactly; everything after that is 50 digits.

A null-space basis is not unique (the oracle takes one from a full SVD, the kernels from three Householder reflectors), so
feature_rows returns what does not depend on the basis: with Pi = I - H_f (H_f^T H_f)^-1 H_f^T and any orthonormal basis A of
the left null space of H_f, A A^T = Pi, hence for H_o = A^T H_x, r_o = A^T r

    H_o^T H_o = H_x^T Pi H_x,     H_o^T r_o = H_x^T Pi r,     r_o^T r_o = r^T Pi r.

gamma = r_o^T (H_o P H_o^T + s^2 I)^-1 r_o is basis-free as well.

An observation list is [(camera index, (u0, v0, u1, v1)), ...] in observation order; cam_q / cam_p are indexed by camera index.

The second half restates what a step does before it looks at any feature, after the oracle's predict_new_state, process_model (per IMU
sample, in the reference's order, with the symmetrisation of the whole matrix and the hand-over of the null states), state_augmentation,
the removal loop of prune_cam_state_buffer and find_redundant_cam_states.  The IMU state is a dict of mpf arrays (IMU_FIELDS), the
covariance an object array.  Every decision reports its relative margin in 50 digits: the `> 1e-5` rate branch, and the 0.2618 rad,
0.4 m and 0.5 tracking-rate tests of the redundancy rule.

The last part is the measurement update (measurement_update, msckf.py:548-602) written directly, the same by the push-through identity
for stacks too long for an m x m solve, and the update of the regularised problem the row compression solves.
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50

ZERO, ONE = mpf(0), mpf(1)


# ---- small dense helpers on numpy object arrays of mpf ------------------------------------------------
def M(a):
    """fp64 (or mpf) array-like -> object array of mpf; an fp64 value converts exactly."""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mpf(float(a[idx])) if not isinstance(a[idx], mpf) else a[idx]
    return out


def F(a):
    """object array of mpf -> float64 (rounded once)."""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape, dtype=np.float64)
    for idx in np.ndindex(a.shape):
        out[idx] = float(a[idx])
    return out


def zeros(*shape):
    out = np.empty(shape, dtype=object)
    out.fill(ZERO)
    return out


def eye(n):
    out = zeros(n, n)
    for i in range(n):
        out[i, i] = ONE
    return out


def norm(v):
    return mp.sqrt(sum((x * x for x in np.asarray(v, dtype=object).reshape(-1)), ZERO))


def solve(A, b):
    """x with A x = b: Gaussian elimination with partial pivoting (b a vector or a matrix of right-hand sides)."""
    A = np.array(A, dtype=object)
    b = np.array(b, dtype=object)
    vec = b.ndim == 1
    if vec:
        b = b.reshape(-1, 1)
    n = len(A)
    for k in range(n):
        piv = max(range(k, n), key=lambda i: abs(A[i, k]))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            if f != 0:
                A[i, k:] = A[i, k:] - A[k, k:] * f
                b[i] = b[i] - b[k] * f
    x = zeros(*b.shape)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:].dot(x[i + 1:])) / A[i, i]
    return x[:, 0] if vec else x


def skew(v):
    x, y, z = v
    return np.array([[ZERO, -z, y], [z, ZERO, -x], [-y, x, ZERO]], dtype=object)


def to_rotation(q):
    """utils.py:12-23 (normalises its input)."""
    q = M(q)
    q = q / norm(q)
    v, w = q[:3], q[3]
    return eye(3) * (2 * w * w - 1) - skew(v) * (2 * w) + np.outer(v, v) * 2


# ---- triangulation ------------------------------------------------------------------------------------
def _views(obs, cam_q, cam_p, T_cam0_cam1):
    """Relative poses (R, t) and measurements of the 2 M views, and the first view's pose in the world (initialize_position's
    first lines, feature_position_initializer.py:19-33)."""
    T = M(np.asarray(T_cam0_cam1, dtype=np.float64))
    R01, t01 = T[:3, :3], T[:3, 3]
    R10, t10 = R01.T, -R01.T.dot(t01)                       # inverse of cam0 -> cam1
    poses, meas = [], []
    for ci, z in obs:
        z = M(np.asarray(z, dtype=np.float64))
        meas.extend([z[:2], z[2:]])
        R0, p0 = to_rotation(cam_q[ci]).T, M(cam_p[ci])      # cam0 -> world
        poses.extend([(R0, p0), (R0.dot(R10), R0.dot(t10) + p0)])
    Rw, tw = poses[0]
    rel = []
    for R, t in poses:                                       # inverse(pose) * T_c0_w
        Ri = R.T
        rel.append((Ri.dot(Rw), Ri.dot(tw) - Ri.dot(t)))
    return rel, meas, (Rw, tw)


def _h(R, t, x):
    return R.dot(np.array([x[0], x[1], ONE], dtype=object)) + t * x[2]


def _cost(rel, meas, x):
    c = ZERO
    for (R, t), z in zip(rel, meas):
        h = _h(R, t, x)
        d0, d1 = h[0] / h[2] - z[0], h[1] / h[2] - z[1]
        c += d0 * d0 + d1 * d1
    return c


def triangulate(obs, cam_q, cam_p, T_cam0_cam1, opt):
    """initialize_position (feature_position_initializer.py:6-76 + feature_depth_estimator.py:4-14), branch for branch: the two-view
    initial guess, the Huber weights, Levenberg-Marquardt with the inner counter that is never reset, the depth check in every view.

    -> dict(pos: world position (3 mpf), valid, x: final (alpha, beta, rho), depth: depth in the first view,
            und: sum of |delta| over the steps whose cost comparison `cn < cost` had a relative margin below 1e-12 -- the steps
                 fp64 cannot decide: one of them taken or not moves the estimate by about |delta| in (alpha, beta, rho),
            huber_margin: smallest |e - huber_epsilon| / huber_epsilon over every weight evaluated,
            stop_margin: smallest |delta_norm - estimation_precision| / estimation_precision over every stop test,
            n_huber: weights below 1 that were applied, outer: outer iterations run)."""
    rel, meas, (Rw, tw) = _views(obs, cam_q, cam_p, T_cam0_cam1)
    huber, prec = mpf(float(opt.huber_epsilon)), mpf(float(opt.estimation_precision))
    # two-view initial guess
    R1, t1 = rel[1]
    m = R1.dot(np.array([meas[0][0], meas[0][1], ONE], dtype=object))
    a = m[:2] - meas[1] * m[2]
    b = meas[1] * t1[2] - t1[:2]
    depth = a.dot(b) / a.dot(a)
    p0 = np.array([meas[0][0], meas[0][1], ONE], dtype=object) * depth
    x = np.array([p0[0], p0[1], ONE], dtype=object) / p0[2]
    lam = mpf(float(opt.initial_damping))
    outer = inner = 0
    delta_norm = mp.inf
    cost = _cost(rel, meas, x)
    und, huber_margin, stop_margin, n_huber = ZERO, mp.inf, mp.inf, 0
    while outer < opt.outer_loop_max_iteration:
        if delta_norm != mp.inf:
            stop_margin = min(stop_margin, abs(delta_norm - prec) / prec)
        if not delta_norm > prec:
            break
        A, bv = zeros(3, 3), zeros(3)
        for (R, t), z in zip(rel, meas):
            h = _h(R, t, x)
            W = np.array([[R[0, 0], R[0, 1], t[0]], [R[1, 0], R[1, 1], t[1]], [R[2, 0], R[2, 1], t[2]]], dtype=object)
            J = np.array([W[0] / h[2] - W[2] * h[0] / (h[2] * h[2]), W[1] / h[2] - W[2] * h[1] / (h[2] * h[2])], dtype=object)
            r = np.array([h[0] / h[2] - z[0], h[1] / h[2] - z[1]], dtype=object)
            e = norm(r)
            huber_margin = min(huber_margin, abs(e - huber) / huber)
            w = ONE if e <= huber else huber / (2 * e)
            n_huber += w != ONE
            A = A + J.T.dot(J) * (w * w)
            bv = bv + J.T.dot(r) * (w * w)
        reduced = False
        while inner < opt.inner_loop_max_iteration and not reduced:
            delta = solve(A + eye(3) * lam, bv)
            xn = x - delta
            delta_norm = norm(delta)
            cn = _cost(rel, meas, xn)
            if abs(cn - cost) < mpf('1e-12') * cost:
                und += delta_norm
            if cn < cost:
                reduced = True
                x, cost = xn, cn
                lam = max(lam / 10, mpf('1e-10'))
            else:
                lam = min(lam * 10, mpf('1e12'))
            inner += 1
        outer += 1
    pf = np.array([x[0], x[1], ONE], dtype=object) / x[2]
    valid = all((R.dot(pf) + t)[2] > 0 for R, t in rel)
    return dict(pos=Rw.dot(pf) + tw, valid=bool(valid), x=x, depth=pf[2], und=und, huber_margin=huber_margin, stop_margin=stop_margin,
                n_huber=n_huber, outer=outer)


# ---- measurement Jacobian, projector invariants, gate -------------------------------------------------
def measurement_jacobian(z, q, p, qn, pn, p_w, T_cam0_cam1, gravity):
    """measurement_jacobian (msckf.py:443-507) of one observation -> H_x (4x6), H_f (4x3), r (4)."""
    T = M(np.asarray(T_cam0_cam1, dtype=np.float64))
    R01, t01 = T[:3, :3], T[:3, 3]
    g = M(gravity)
    z, p_w = M(z), M(p_w)
    R_w_c0, t_c0_w = to_rotation(q), M(p)
    R_w_c1 = R01.dot(R_w_c0)
    t_c1_w = t_c0_w - R_w_c1.T.dot(t01)
    p0 = R_w_c0.dot(p_w - t_c0_w)
    p1 = R_w_c1.dot(p_w - t_c1_w)
    dz0, dz1 = zeros(4, 3), zeros(4, 3)
    dz0[0, 0] = 1 / p0[2]
    dz0[1, 1] = 1 / p0[2]
    dz0[0, 2] = -p0[0] / (p0[2] * p0[2])
    dz0[1, 2] = -p0[1] / (p0[2] * p0[2])
    dz1[2, 0] = 1 / p1[2]
    dz1[3, 1] = 1 / p1[2]
    dz1[2, 2] = -p1[0] / (p1[2] * p1[2])
    dz1[3, 2] = -p1[1] / (p1[2] * p1[2])
    dp0, dp1 = zeros(3, 6), zeros(3, 6)
    dp0[:, :3] = skew(p0)
    dp0[:, 3:] = -R_w_c0
    dp1[:, :3] = R01.dot(skew(p0))
    dp1[:, 3:] = -R_w_c1
    A = dz0.dot(dp0) + dz1.dot(dp1)
    u = zeros(6)
    u[:3] = to_rotation(qn).dot(g)
    u[3:] = skew(p_w - M(pn)).dot(g)
    H_x = A - np.outer(A.dot(u), u) / u.dot(u)
    H_f = -H_x[:4, 3:6]
    r = z - np.array([p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]], dtype=object)
    return H_x, H_f, r


def stacked(obs, p_w, cam_q, cam_p, cam_qn, cam_pn, T_cam0_cam1, gravity):
    """H_x on the feature's own 6 M camera columns (observation j: rows 4j.., columns 6j..), H_f (4M x 3) and r (4M)."""
    Mo = len(obs)
    Hx, Hf, r = zeros(4 * Mo, 6 * Mo), zeros(4 * Mo, 3), zeros(4 * Mo)
    for j, (ci, z) in enumerate(obs):
        hx, hf, rj = measurement_jacobian(z, cam_q[ci], cam_p[ci], cam_qn[ci], cam_pn[ci], p_w, T_cam0_cam1, gravity)
        Hx[4 * j:4 * j + 4, 6 * j:6 * j + 6] = hx
        Hf[4 * j:4 * j + 4] = hf
        r[4 * j:4 * j + 4] = rj
    return Hx, Hf, r


def _bt_dot(Hx, X):
    """Hx^T X for the block-diagonal Hx of `stacked` (only the 4 x 6 blocks are multiplied)."""
    Mo = Hx.shape[0] // 4
    X2 = X.reshape(len(X), -1)
    out = zeros(6 * Mo, X2.shape[1])
    for j in range(Mo):
        out[6 * j:6 * j + 6] = Hx[4 * j:4 * j + 4, 6 * j:6 * j + 6].T.dot(X2[4 * j:4 * j + 4])
    return out[:, 0] if X.ndim == 1 else out


def invariants(Hx, Hf, r):
    """(H_x^T Pi H_x, H_x^T Pi r, r^T Pi r) with Pi = I - H_f (H_f^T H_f)^-1 H_f^T."""
    G = Hf.T.dot(Hf)
    PHx = Hx - Hf.dot(solve(G, _bt_dot(Hx, Hf).T))          # Pi H_x
    Pr = r - Hf.dot(solve(G, Hf.T.dot(r)))                  # Pi r
    return _bt_dot(Hx, PHx), _bt_dot(Hx, Pr), r.dot(Pr)


def feature_rows(obs, p_w, cam_q, cam_p, cam_qn, cam_pn, T_cam0_cam1, gravity):
    """-> dict(Hx, Hf, r: the stacked blocks; HtH, Htr, rtr: the three basis-free invariants of the projected rows)."""
    Hx, Hf, r = stacked(obs, p_w, cam_q, cam_p, cam_qn, cam_pn, T_cam0_cam1, gravity)
    HtH, Htr, rtr = invariants(Hx, Hf, r)
    return dict(Hx=Hx, Hf=Hf, r=r, HtH=HtH, Htr=Htr, rtr=rtr)


def rows_invariants(Ho, ro):
    """The same three quantities from projected rows H_o (K x 6M, own camera columns) and r_o, whatever basis produced them."""
    Ho, ro = M(Ho), M(ro)
    return Ho.T.dot(Ho), Ho.T.dot(ro), ro.dot(ro)


def null_basis(Hf):
    """An orthonormal basis (4M x (4M - 3)) of the left null space of H_f: the last columns of Q = H_0 H_1 H_2 (Householder)."""
    n = len(Hf)
    R = np.array(Hf, dtype=object)
    Q = eye(n)
    for k in range(3):
        v = np.array(R[k:, k], dtype=object)
        nv = norm(v)
        v[0] = v[0] + (nv if v[0] >= 0 else -nv)
        vv = v.dot(v)
        R[k:] = R[k:] - np.outer(v, 2 * v.dot(R[k:]) / vv)
        Q[:, k:] = Q[:, k:] - np.outer(2 * Q[:, k:].dot(v) / vv, v)
    return Q[:, 3:]


def gamma_basis(rows, P_sub, obs_noise):
    """gating_test (msckf.py:604-612) on the projected rows, as it is defined: r_o^T (H_o P H_o^T + s^2 I)^-1 r_o with H_o = A^T H_x,
    r_o = A^T r and A = null_basis(H_f).  rows = feature_rows(...); P_sub = the 6M x 6M block of the covariance over the feature's own
    camera columns, in observation order (only it enters).  Two million 50-digit products at 20 observations: see gamma."""
    A = null_basis(rows['Hf'])
    Ho = _bt_dot(rows['Hx'], A).T                           # A^T H_x
    ro = A.T.dot(rows['r'])
    S = Ho.dot(M(P_sub)).dot(Ho.T) + eye(len(Ho)) * mpf(float(obs_noise))
    return ro.dot(solve(S, ro))


def gamma(rows, P_sub, obs_noise):
    """The same number without a basis.  With W = H_x P H_x^T + s^2 I (4M x 4M, positive definite) and A^T A = I,
    H_o P H_o^T + s^2 I = A^T W A, and because the columns of A span the null space of H_f^T,

        A (A^T W A)^-1 A^T = W^-1 - W^-1 H_f (H_f^T W^-1 H_f)^-1 H_f^T W^-1,

    so gamma = r^T W^-1 r - b^T (H_f^T W^-1 H_f)^-1 b with b = H_f^T W^-1 r: one solve with W for four right-hand sides and a 3 x 3
    solve, a seventh of the products of gamma_basis at 20 observations.  tests/test_msckf_mp_ref.py holds the two forms to each other."""
    Hx, Hf, r = rows['Hx'], rows['Hf'], rows['r']
    Mo = len(r) // 4
    P = M(P_sub)
    W = eye(4 * Mo) * mpf(float(obs_noise))
    for j in range(Mo):
        Hj = Hx[4 * j:4 * j + 4, 6 * j:6 * j + 6]
        for l in range(Mo):
            W[4 * j:4 * j + 4, 4 * l:4 * l + 4] += Hj.dot(P[6 * j:6 * j + 6, 6 * l:6 * l + 6]).dot(Hx[4 * l:4 * l + 4, 6 * l:6 * l + 6].T)
    X = solve(W, np.column_stack([r, Hf]))                  # W^-1 [r | H_f]
    b = Hf.T.dot(X[:, 0])
    return r.dot(X[:, 0]) - b.dot(solve(Hf.T.dot(X[:, 1:]), b))


def own_columns(obs):
    """Indices of the feature's own camera columns in the full state (21 + 6 * camera + 0..5), observation order."""
    return np.concatenate([21 + 6 * ci + np.arange(6) for ci, _ in obs])


# ---- prediction, augmentation, pruning (the part of a step that runs before any feature is looked at) --
# The thresholds are the fp64 literals the code compares with, entered exactly.
RATE_THR = mpf(1e-5)
ANGLE_THR, DIST_THR, TRACK_THR = mpf(0.2618), mpf(0.4), mpf(0.5)
IMU_FIELDS = ('ts', 'q', 'p', 'v', 'bg', 'ba', 'R_ic', 't_ci', 'qn', 'pn', 'vn', 'gravity')


def to_quaternion(R):
    """utils.py:25-47."""
    if R[2, 2] < 0:
        if R[0, 0] > R[1, 1]:
            q = [1 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[2, 0] + R[0, 2], R[1, 2] - R[2, 1]]
        else:
            q = [R[0, 1] + R[1, 0], 1 - R[0, 0] + R[1, 1] - R[2, 2], R[2, 1] + R[1, 2], R[2, 0] - R[0, 2]]
    else:
        if R[0, 0] < -R[1, 1]:
            q = [R[0, 2] + R[2, 0], R[2, 1] + R[1, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2], R[0, 1] - R[1, 0]]
        else:
            q = [R[1, 2] - R[2, 1], R[2, 0] - R[0, 2], R[0, 1] - R[1, 0], 1 + R[0, 0] + R[1, 1] + R[2, 2]]
    q = np.array(q, dtype=object)
    return q / norm(q)


def imu_state(d):
    """dict of fp64 fields (IMU_FIELDS; R_ic 3 x 3) -> the same in mpf."""
    return {k: (M(d[k]) if np.ndim(d[k]) else mpf(float(d[k]))) for k in IMU_FIELDS}


def predict_new_state(s, dt, gyro, acc):
    """predict_new_state (msckf.py:341-388): RK4 with k2 and k3 sharing the half-step rotation; s['q'], s['v'], s['p'] are replaced.
    -> relative margin of the `> 1e-5` rate branch."""
    gn = norm(gyro)
    Om = zeros(4, 4)
    Om[:3, :3] = -skew(gyro)
    Om[:3, 3] = gyro
    Om[3, :3] = -gyro
    q, v, p, g = s['q'], s['v'], s['p'], s['gravity']
    if gn > RATE_THR:
        dq_dt = (eye(4) * mp.cos(gn * dt / 2) + Om * (mp.sin(gn * dt / 2) / gn)).dot(q)
        dq_dt2 = (eye(4) * mp.cos(gn * dt / 4) + Om * (mp.sin(gn * dt / 4) / gn)).dot(q)
    else:
        dq_dt = ((eye(4) + Om * (dt / 2)) * mp.cos(gn * dt / 2)).dot(q)
        dq_dt2 = ((eye(4) + Om * (dt / 4)) * mp.cos(gn * dt / 4)).dot(q)
    Rt, Rt2 = to_rotation(dq_dt).T, to_rotation(dq_dt2).T
    k1v = to_rotation(q).T.dot(acc) + g
    k1p = v
    k2v = Rt2.dot(acc) + g
    k2p = v + k1v * (dt / 2)
    k3v = Rt2.dot(acc) + g
    k3p = v + k2v * (dt / 2)
    k4v = Rt.dot(acc) + g
    k4p = v + k3v * dt
    s['q'] = dq_dt / norm(dq_dt)
    s['v'] = v + (k1v + k2v * 2 + k3v * 2 + k4v) * (dt / 6)
    s['p'] = p + (k1p + k2p * 2 + k3p * 2 + k4p) * (dt / 6)
    return abs(gn - RATE_THR) / RATE_THR


def process_model(s, P, time, m_gyro, m_acc, noise):
    """process_model (msckf.py:275-339) for one IMU sample, state and covariance, in the reference's order: F, G, Phi to third order
    from the OLD orientation, predict_new_state, the observability patches of Phi from the null-space states, Q = Phi G Qc G^T Phi^T dt,
    the IMU block, the cross blocks, (P + P^T) / 2 of the whole matrix, the null states handed over.  s is updated in place (its
    time stamp is batch_imu_processing's to set).  noise = the four continuous variances.  -> (P, rate margin)."""
    dt = mpf(float(time)) - s['ts']
    gyro, acc = M(m_gyro) - s['bg'], M(m_acc) - s['ba']
    Fm, G = zeros(21, 21), zeros(21, 12)
    R_w_i = to_rotation(s['q'])
    Fm[:3, :3] = -skew(gyro)
    Fm[:3, 3:6] = -eye(3)
    Fm[6:9, :3] = -R_w_i.T.dot(skew(acc))
    Fm[6:9, 9:12] = -R_w_i.T
    Fm[12:15, 6:9] = eye(3)
    G[:3, :3] = -eye(3)
    G[3:6, 3:6] = eye(3)
    G[6:9, 6:9] = -R_w_i.T
    G[9:12, 9:12] = eye(3)
    Fdt = Fm * dt
    Fdt2 = Fdt.dot(Fdt)
    Fdt3 = Fdt2.dot(Fdt)
    Phi = eye(21) + Fdt + Fdt2 / 2 + Fdt3 / 6
    margin = predict_new_state(s, dt, gyro, acc)
    g = s['gravity']
    R_kk_1 = to_rotation(s['qn'])
    Phi[:3, :3] = to_rotation(s['q']).dot(R_kk_1.T)
    u = R_kk_1.dot(g)
    sv = u / u.dot(u)
    A1 = Phi[6:9, :3]
    w1 = skew(s['vn'] - s['v']).dot(g)
    Phi[6:9, :3] = A1 - np.outer(A1.dot(u) - w1, sv)
    A2 = Phi[12:15, :3]
    w2 = skew(s['vn'] * dt + s['pn'] - s['p']).dot(g)
    Phi[12:15, :3] = A2 - np.outer(A2.dot(u) - w2, sv)
    Qc = zeros(12, 12)
    for i in range(12):
        Qc[i, i] = mpf(float(noise[i // 3]))
    Q = Phi.dot(G).dot(Qc).dot(G.T).dot(Phi.T) * dt
    P = np.array(P, dtype=object)
    P[:21, :21] = Phi.dot(P[:21, :21]).dot(Phi.T) + Q
    if len(P) > 21:
        P[:21, 21:] = Phi.dot(P[:21, 21:])
        P[21:, :21] = P[21:, :21].dot(Phi.T)
    P = (P + P.T) / 2
    s['qn'], s['pn'], s['vn'] = s['q'], s['p'], s['v']
    return P, margin


def batch_imu_processing(s, P, samples, noise):
    """The loop of batch_imu_processing (msckf.py:251-273) over the samples it applies: [(t, gyro, acc), ...] -> (P, smallest rate margin)."""
    margin = mp.inf
    for t, w, a in samples:
        P, m = process_model(s, P, t, w, a, noise)
        s['ts'] = mpf(float(t))
        margin = min(margin, m)
    return P, margin


def state_augmentation(s, P):
    """state_augmentation (msckf.py:390-423) -> (orientation, position of the new camera state, the grown covariance)."""
    R_i_c, t_c_i = s['R_ic'], s['t_ci']
    R_w_i = to_rotation(s['q'])
    cam_q = to_quaternion(R_i_c.dot(R_w_i))
    cam_p = s['p'] + R_w_i.T.dot(t_c_i)
    J = zeros(6, 21)
    J[:3, :3] = R_i_c
    J[:3, 15:18] = eye(3)
    J[3:6, :3] = skew(R_w_i.T.dot(t_c_i))
    J[3:6, 12:15] = eye(3)
    J[3:6, 18:21] = eye(3)
    n = len(P)
    Pn = zeros(n + 6, n + 6)
    Pn[:n, :n] = P
    Pn[n:, :n] = J.dot(Pn[:21, :n])
    Pn[:n, n:] = Pn[n:, :n].T
    Pn[n:, n:] = J.dot(Pn[:21, :21]).dot(J.T)
    return cam_q, cam_p, (Pn + Pn.T) / 2


def remove_cam_states(P, positions):
    """The removal loop of prune_cam_state_buffer (msckf.py:774-786): the camera states at the given window positions (ascending, in
    the numbering before any removal) leave one after the other, each at the position it has by then."""
    P = np.asarray(P)
    for k, i in enumerate(positions):
        a = 21 + 6 * (i - k)
        keep = np.r_[0:a, a + 6:len(P)]
        P = P[np.ix_(keep, keep)].copy()
    return P


def find_redundant_cam_states(cam_q, cam_p, tracking_rate):
    """find_redundant_cam_states (msckf.py:678-709) on a window of camera states -> (the two window positions, ascending,
    [dict(angle, dist, rate: relative margins to 0.2618 rad, 0.4 m, 0.5; redundant; margin) for the two candidates]).  `margin` is the margin
    of the decision: the smallest of the computed two (angle, distance) where all three tests hold, else the largest among the tests that
    fail (one clear failure decides; a failing rate test is exact)."""
    n = len(cam_q)
    key, idx, first = n - 4, n - 3, 0
    key_p, key_R = M(cam_p[key]), to_rotation(cam_q[key])
    rate = mpf(float(tracking_rate))
    out, info = [], []
    for _ in range(2):
        dist = norm(M(cam_p[idx]) - key_p)
        angle = 2 * mp.acos(to_quaternion(to_rotation(cam_q[idx]).dot(key_R.T))[3])
        tests = ((angle < ANGLE_THR, abs(angle - ANGLE_THR) / ANGLE_THR), (dist < DIST_THR, abs(dist - DIST_THR) / DIST_THR),
                 (rate > TRACK_THR, abs(rate - TRACK_THR) / TRACK_THR))
        red = all(t for t, _ in tests)
        dec = (tests[0], tests[1], (tests[2][0], mp.inf))      # the rate is an input compared as it is: exact in any precision
        info.append(dict(angle=tests[0][1], dist=tests[1][1], rate=tests[2][1], redundant=red,
                         margin=min(m for _, m in dec) if red else max(m for t, m in dec if not t)))
        if red:
            out.append(idx)
        else:
            out.append(first)
            first += 1
        idx += 1
    return sorted(out), info


# ---- the measurement update (oracle/msckf_np.py: measurement_update; msckf.py:548-602) -------------------------------------
# The stacked Jacobian is zero outside the touched columns `cols`, so every function takes Hc = H[:, cols] (m x nc) and forms the
# products with P through P[cols, :]: the same numbers as with the full-width H, without the multiplications by exact zeros.  No
# QR (a thin QR changes nothing mathematically) and no state injection: delta_x and P+ are the results.
def _sym(P):
    return (P + P.T) / mpf(2)


def measurement_update(Hc, r, P, cols, obs_noise):
    """S = H P H^T + s^2 I, K^T = S^-1 H P, delta_x = K r, P+ = sym((I - K H) P), written directly.  -> (delta_x [n], P+ [n, n])."""
    Hc, r, P, cols = M(Hc), M(r), M(P), list(cols)
    m, n = len(Hc), len(P)
    HP = Hc.dot(P[cols, :])                                  # H P, m x n
    S = HP[:, cols].dot(Hc.T) + eye(m) * mpf(float(obs_noise))
    Kt = solve(S, HP)                                        # K^T = S^-1 H P, m x n
    dx = Kt.T.dot(r)
    return dx, _sym(P - Kt.T.dot(HP))


def measurement_update_info(Hc, r, P, cols, obs_noise, reg=None):
    """The same two results by the push-through identity Hc^T (Hc Pcc Hc^T + s^2 I)^-1 = (A Pcc + s^2 I)^-1 Hc^T with A = Hc^T Hc,
    b = Hc^T r:  delta_x = P[:, c] (A Pcc + s^2 I)^-1 b,  P+ = sym(P - P[:, c] (A Pcc + s^2 I)^-1 A P[c, :]).  For stacks too long for an
    m x m solve in 50 digits.  reg: a multiple of max_i A_ii added to every diagonal entry of A (measurement_update_regularised)."""
    Hc, r, P, cols = M(Hc), M(r), M(P), list(cols)
    nc = len(cols)
    A, b = Hc.T.dot(Hc), Hc.T.dot(r)
    if reg is not None:
        A = A + eye(nc) * (mpf(float(reg)) * max(A[i, i] for i in range(nc)))
    Pc = P[cols, :]
    Mx = A.dot(Pc[:, cols]) + eye(nc) * mpf(float(obs_noise))
    X = solve(Mx, np.concatenate([A.dot(Pc), b.reshape(-1, 1)], axis=1))
    return Pc.T.dot(X[:, -1]), _sym(P - Pc.T.dot(X[:, :-1]))


def measurement_update_regularised(Hc, r, P, cols, obs_noise):
    """The update of the REGULARISED problem the row compression solves (msckf_mfma.inc, above chol_mfma_body): A + E in place of
    A = Hc^T Hc with E = 1e-12 max_i A_ii on every diagonal entry (any F with F^T F = A + E, F^T f = b stands in for (Hc, r)).  Against
    measurement_update it shows the shift E itself causes, apart from any rounding."""
    return measurement_update_info(Hc, r, P, cols, obs_noise, reg=1e-12)
