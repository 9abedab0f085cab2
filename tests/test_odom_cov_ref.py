"""The NumPy statement of the odometry-covariance record against central differences of the reference's own maps, the wire format,
and evaluate.nees on errors drawn from a known covariance.  No GPU."""
import numpy as np

import odom_cov_ref as R
from uav_airvision_amd import evaluate, msckf_ops


def _random_state(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    e = rng.normal(size=4)
    e /= np.linalg.norm(e)
    from oracle.msckf_np import to_rotation
    return q, rng.normal(size=3) * 3, rng.normal(size=3), to_rotation(e), rng.normal(size=3) * 0.2


def test_jacobian_matches_central_differences_of_the_reference_maps():
    """20 seeded states.  J's entries are O(1); with h = 1e-6 the truncation is ~1e-12 and the round-off ~eps / h = 2e-10, so the
    bar is 1e-7 absolute: a sign or frame mistake is O(1)."""
    worst = 0.0
    for seed in range(20):
        st = _random_state(np.random.default_rng(1000 + seed))
        Jn = R.numeric_jacobian(st, h=1e-6)
        Ja = R.odom_jacobian(st[0], st[3], st[4])
        err = float(np.abs(Jn - Ja).max())
        worst = max(worst, err)
        assert err < 1e-7, (seed, err)
        # the bias columns do not reach the published quantities
        assert not Ja[:, 3:6].any() and not Ja[:, 9:12].any()
    print('worst |J_fd - J| = %.3e' % worst)


def test_record_is_j_p_jt_and_selects_rows_exactly():
    rng = np.random.default_rng(7)
    st = _random_state(rng)
    A = rng.normal(size=(33, 33))
    P = A @ A.T
    Cm = R.odom_cov(P, st[0], st[3], st[4])
    assert Cm.shape == (15, 15)
    assert np.array_equal(Cm[:9, :9], P[np.ix_(R.SEL9, R.SEL9)])
    assert np.abs(Cm - Cm.T).max() <= 1e-12 * np.abs(Cm).max()
    assert np.all(np.linalg.eigvalsh(0.5 * (Cm + Cm.T)) > -1e-9)


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(4, 15, 15))
    Cm = A + np.swapaxes(A, 1, 2)
    w = msckf_ops.pack_odom_cov(Cm)
    assert w.shape == (4, 120) and msckf_ops.ODOM_COV_DOUBLES == 120
    # row-major upper triangle: (0,0) .. (0,14), (1,1) ..
    assert w[0, 0] == Cm[0, 0, 0] and w[0, 14] == Cm[0, 0, 14] and w[0, 15] == Cm[0, 1, 1] and w[0, 119] == Cm[0, 14, 14]
    back = msckf_ops.unpack_odom_cov(w)
    assert np.array_equal(back, Cm) and np.array_equal(back, np.swapaxes(back, 1, 2))
    assert np.array_equal(msckf_ops.pack_odom_cov(back), w)
    nan = msckf_ops.unpack_odom_cov(np.full(120, np.nan))
    assert nan.shape == (15, 15) and np.isnan(nan).all()
    names = [n for n, _ in msckf_ops.ODOM_COV_FIELDS]
    assert names == ['p', 'theta', 'v', 'p_c', 'theta_c']
    assert [(s.start, s.stop) for _, s in msckf_ops.ODOM_COV_FIELDS] == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15)]


def _nees_case(scale):
    rng = np.random.default_rng(11)
    n = 4000
    A = rng.normal(size=(3, 3))
    Sigma = A @ A.T * 1e-4 + 1e-5 * np.identity(3)
    L = np.linalg.cholesky(Sigma)
    t = np.arange(n) * 0.05
    ref_p = np.stack([np.cos(t), np.sin(t), 0.1 * t], axis=1)
    est_p = ref_p + rng.normal(size=(n, 3)) @ L.T
    cov = np.broadcast_to(Sigma * scale, (n, 3, 3)).copy()
    return est_p, cov, ref_p


def test_nees_of_errors_drawn_from_the_stated_covariance():
    """A chi-square(3) sample mean over 4,000 draws has standard deviation sqrt(6 / 4000) = 0.039: within 3 +- 0.2 without the
    alignment; a covariance four times too large is outside that band."""
    est_p, cov, ref_p = _nees_case(1.0)
    per, mean = evaluate.nees(est_p, cov, ref_p, align=False)
    assert per.shape == (4000,) and abs(mean - per.mean()) < 1e-12
    print('mean NEES %.4f' % mean)
    assert abs(mean - 3.0) < 0.2, mean
    _, mean4 = evaluate.nees(*_nees_case(4.0), align=False)
    print('mean NEES with 4 Sigma %.4f' % mean4)
    assert abs(mean4 - 3.0) > 0.2, mean4


def test_nees_alignment_rotates_the_covariance_with_the_errors():
    """The estimate expressed in a rotated, shifted frame, with its covariance in that frame: after the ATE alignment the NEES is that
    of the unrotated case (the fit itself absorbs six degrees of freedom of 12,000: far inside the band)."""
    est_p, cov, ref_p = _nees_case(1.0)
    c, s = np.cos(0.7), np.sin(0.7)
    Rz = np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])
    est_r = est_p @ Rz.T + np.array([1., -2., 0.5])
    cov_r = Rz @ cov @ Rz.T
    _, mean = evaluate.nees(est_r, cov_r, ref_p, align=True)
    assert abs(mean - 3.0) < 0.2, mean
