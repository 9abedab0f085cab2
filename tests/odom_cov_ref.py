"""NumPy statement of the odometry-covariance record (include/airvision.h, "Odometry covariance") and the helpers the tests of it share.
TEST INFRASTRUCTURE ONLY.

    C = J P[0:21, 0:21] J^T,   error coordinates p, theta, v, p_c, theta_c (3 each)

with the reference's error-state order theta 0:3, b_g 3:6, v 6:9, b_a 9:12, p 12:15, theta_ext 15:18, t_ext 18:21.
"""
import numpy as np

from oracle.msckf_np import quaternion_multiplication, skew, small_angle_quaternion, to_rotation

SEL9 = np.r_[12:15, 0:3, 6:9]          # the state indices that record rows 0:9 select


def odom_jacobian(q, R_ic, t_ci):
    """J [15, 21] of the record at the published state (q JPL xyzw, R_ic = R_imu_cam0, t_ci = t_cam0_imu)."""
    R_wb = to_rotation(np.asarray(q, dtype=np.float64)).T
    J = np.zeros((15, 21))
    J[0:3, 12:15] = np.identity(3)
    J[3:6, 0:3] = np.identity(3)
    J[6:9, 6:9] = np.identity(3)
    J[9:12, 12:15] = np.identity(3)
    J[9:12, 0:3] = -R_wb @ skew(t_ci)
    J[9:12, 18:21] = R_wb
    J[12:15, 0:3] = R_ic
    J[12:15, 15:18] = np.identity(3)
    return J


def odom_cov(P, q, R_ic, t_ci):
    """The 15 x 15 record of a stream whose covariance is P (at least 21 x 21) and whose published state is q, R_ic, t_ci."""
    J = odom_jacobian(q, R_ic, t_ci)
    return J @ np.asarray(P)[:21, :21] @ J.T


def odom_cov_bound(P, q, R_ic, t_ci):
    """|J| |P| |J^T|, entrywise: the scale of the rounding error of a computed record."""
    J = np.abs(odom_jacobian(q, R_ic, t_ci))
    return J @ np.abs(np.asarray(P)[:21, :21]) @ J.T


def rot_log(R):
    """Rotation vector of a rotation matrix near the identity: R = exp([w]x)."""
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])       # sin(a) * axis
    s = np.linalg.norm(w)
    if s < 1e-300:
        return w
    a = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    return w * (a / s)


def published(q, p, v, R_ic, t_ci):
    """What publish (msckf.py:845-867, T_imu_body = I) makes of the IMU state: p, R_wb, v, t_c_w, R_wc."""
    R_wb = to_rotation(q).T
    R_w_c = R_ic @ R_wb.T
    return p, R_wb, v, p + R_wb @ t_ci, R_w_c.T


def inject(state, dx):
    """measurement_update's injection of a 21-vector into (q, p, v, R_ic, t_ci) (msckf.py:568-595); biases are not published."""
    q, p, v, R_ic, t_ci = state
    return (quaternion_multiplication(small_angle_quaternion(dx[0:3]), q), p + dx[12:15], v + dx[6:9],
            to_rotation(small_angle_quaternion(dx[15:18])) @ R_ic, t_ci + dx[18:21])


def record_error(state0, state1):
    """The 15 error coordinates of publish(state1) against publish(state0): differences for the vectors, right-applied rotation
    logarithms for the two orientations."""
    p0, Rb0, v0, pc0, Rc0 = published(*state0)
    p1, Rb1, v1, pc1, Rc1 = published(*state1)
    return np.concatenate([p1 - p0, rot_log(Rb0.T @ Rb1), v1 - v0, pc1 - pc0, rot_log(Rc0.T @ Rc1)])


def numeric_jacobian(state, h=1e-6):
    """Central differences of the published quantities along the 21 error-state directions."""
    J = np.zeros((15, 21))
    for k in range(21):
        d = np.zeros(21)
        d[k] = h
        J[:, k] = (record_error(state, inject(state, d)) - record_error(state, inject(state, -d))) / (2 * h)
    return J
