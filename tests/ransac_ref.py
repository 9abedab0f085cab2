"""tests/ransac_ref.py -- TEST INFRASTRUCTURE ONLY (like tests/stepwise_msckf.py).

Plain NumPy restatement of the two-point RANSAC specified in include/airvision.h (av_two_point_ransac, steps 1-9), with
oracle.cvops.undistort_points for step 1.  Besides the markers it returns the DECISION MARGIN of the problem: the smallest relative
distance of any compared quantity from its threshold (the 50-unit cut, mean < unit, the standstill cut, the base-column choice, the
determinant, every residual test and the 0.2 n inlier count).  fp64 sums are taken in another order here than on the device (np.sum
against a per-lane sum and a butterfly), so a comparison closer than ~1e-13 can come out differently; a test leaves out problems
whose margin is below 1e-9.
"""
import math

import numpy as np

PATH_FEW, PATH_STILL, PATH_MODEL, PATH_NONE = 1, 2, 4, 8
M32 = 0xFFFFFFFF


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def ransac_hash(seed, frame, camera, k, draw):
    """include/airvision.h: mix(mix(mix(seed + 0x9e3779b9) ^ frame) ^ (camera << 16 | k << 1 | draw)), uint32 wrapping."""
    return mix(mix(mix((seed + 0x9e3779b9) & M32) ^ (frame & M32)) ^ ((camera << 16 | k << 1 | draw) & M32))


def num_hypotheses(p):
    if not (0.0 < p < 1.0):
        return 0
    return int(min(64, max(1, math.ceil(math.log(1.0 - p) / math.log(1.0 - 0.7 * 0.7)))))


def _rel(value, threshold):
    """relative distance of a compared quantity from its threshold"""
    value = np.asarray(value, dtype=np.float64)
    if value.size == 0:
        return np.inf
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(value - threshold) / abs(threshold)
    r = np.where(np.isfinite(r), r, 0.0)          # a non-finite comparison is as close as it gets
    return float(r.min())


def two_point_ransac(pts1, pts2, R_p_c, intrinsics, distortion_model, distortion_coeffs, inlier_error, success_probability=0.99,
                     seed=0, frame=0, camera=0):
    """-> (markers uint8[n], info dict(n_set, path, margin, m, best))."""
    from oracle import cvops
    p1 = np.asarray(pts1, dtype=np.float32).reshape(-1, 2)
    p2 = np.asarray(pts2, dtype=np.float32).reshape(-1, 2)
    n = len(p1)
    R = np.asarray(R_p_c, dtype=np.float64).reshape(3, 3)
    thr = float(inlier_error)
    markers = np.zeros(n, np.uint8)
    info = dict(n_set=0, path=PATH_FEW, margin=np.inf, m=0, best=-1)
    if n == 0:
        return markers, info
    # 1. (float64 in -> float64 out: nothing is rounded to float32)
    u1 = cvops.undistort_points(p1.astype(np.float64), intrinsics, distortion_coeffs, distortion_model=distortion_model).reshape(-1, 2)
    u2 = cvops.undistort_points(p2.astype(np.float64), intrinsics, distortion_coeffs, distortion_model=distortion_model).reshape(-1, 2)
    # 2.
    hx = (R[0, 0] * u1[:, 0] + R[0, 1] * u1[:, 1]) + R[0, 2] * 1.0
    hy = (R[1, 0] * u1[:, 0] + R[1, 1] * u1[:, 1]) + R[1, 2] * 1.0
    hz = (R[2, 0] * u1[:, 0] + R[2, 1] * u1[:, 1]) + R[2, 2] * 1.0
    u1 = np.stack([hx / hz, hy / hz], axis=1)
    # 3.
    total = float(np.sum(np.sqrt(u1[:, 0] * u1[:, 0] + u1[:, 1] * u1[:, 1])) + np.sum(np.sqrt(u2[:, 0] * u2[:, 0] + u2[:, 1] * u2[:, 1])))
    with np.errstate(all='ignore'):
        s = np.float64(math.sqrt(2.0) * float(2 * n)) / np.float64(total)
        unit = float((s * 2.0) / (float(intrinsics[0]) + float(intrinsics[1])))
        u1 = u1 * s
        u2 = u2 * s
        # 4.
        dx, dy = u1[:, 0] - u2[:, 0], u1[:, 1] - u2[:, 1]
        dn = np.sqrt(dx * dx + dy * dy)
        cut = 50.0 * unit
        raw = ~(dn > cut)
    margin = _rel(dn, cut)
    idx = np.nonzero(raw)[0]
    m = len(idx)
    info['m'] = m
    if m < 3:                                            # 5.
        info['margin'] = margin
        return markers, info
    mean = float(np.sum(dn[idx])) / float(m)
    margin = min(margin, _rel(mean, unit))
    thr_u = thr * unit
    if mean < unit:                                      # 6.
        keep = ~(dn[idx] > thr_u)
        margin = min(margin, _rel(dn[idx], thr_u))
        markers[idx[keep]] = 1
        info.update(n_set=int(keep.sum()), path=PATH_STILL, margin=margin)
        return markers, info
    # 7.
    c = np.stack([dy[idx], -dx[idx], u1[idx, 0] * u2[idx, 1] - u1[idx, 1] * u2[idx, 0]], axis=1)
    # 8.
    N = num_hypotheses(success_probability)
    best_cnt, best_set, best_k = 0, None, -1
    for k in range(N):
        r0, r1 = ransac_hash(seed, frame, camera, k, 0), ransac_hash(seed, frame, camera, k, 1)
        a = r0 % m
        b = (a + 1 + r1 % (m - 1)) % m
        ca, cb = c[a], c[b]
        norms = [abs(ca[q]) + abs(cb[q]) for q in range(3)]
        j = 0
        if norms[1] < norms[j]:
            j = 1
        if norms[2] < norms[j]:
            j = 2
        others = sorted(norms[q] for q in range(3) if q != j)
        margin = min(margin, (others[0] - norms[j]) / others[0] if others[0] > 0 else 0.0)
        p, q = (1 if j == 0 else 0), (1 if j == 2 else 2)
        with np.errstate(all='ignore'):
            det = ca[p] * cb[q] - ca[q] * cb[p]
            tp = (ca[q] * cb[j] - ca[j] * cb[q]) / det
            tq = (ca[j] * cb[p] - ca[p] * cb[j]) / det
        scale = abs(ca[p] * cb[q]) + abs(ca[q] * cb[p])
        margin = min(margin, abs(det) / scale if scale > 0 else 0.0)
        if det == 0.0 or not (np.isfinite(tp) and np.isfinite(tq)):
            continue
        t = np.zeros(3)
        t[j], t[p], t[q] = 1.0, tp, tq
        res = np.abs((c[:, 0] * t[0] + c[:, 1] * t[1]) + c[:, 2] * t[2])
        inl = res < thr_u
        margin = min(margin, _rel(res, thr_u))
        cnt = int(inl.sum())
        margin = min(margin, abs(cnt - 0.2 * n) / (0.2 * n))
        if float(cnt) < 0.2 * float(n):
            continue
        if cnt > best_cnt:
            best_cnt, best_set, best_k = cnt, inl, k
    info.update(path=PATH_MODEL, margin=margin, best=best_k, unit=unit, c=c, raw_index=idx)
    if best_set is None:                                 # 9.
        info['path'] |= PATH_NONE
        return markers, info
    markers[idx[best_set]] = 1
    info['n_set'] = best_cnt
    return markers, info


# ---- seeded problems for the tests ---------------------------------------------------------------------------------------------
def planted_problem(rng, n, cam, outlier_share=0.0, standstill=False, model='radtan', rot=0.02, trans=0.15, outlier_px=(8.0, 60.0)):
    """n pairs seen by a camera that rotates by a small R and translates by t between two frames, over random depths (no noise but
    the float32 rounding of the pixel positions), a share of them displaced in the second image by outlier_px pixels in a random
    direction.  cam = (intrinsics, distortion_coeffs).  Returns dict(p1, p2, R, planted_outlier bool[n], t)."""
    from oracle import cvops
    intr, dist = cam
    w = rng.normal(0, rot, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K) if th > 0 else np.eye(3)
    t = rng.normal(0, 1, 3)
    t = np.zeros(3) if standstill else t / np.linalg.norm(t) * trans       # |t| = trans metres, random direction
    x1 = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.4, 0.4, n), np.ones(n)], axis=1)
    depth = rng.uniform(2.0, 8.0, n)
    X2 = (R @ (x1 * depth[:, None]).T).T + t             # X_c = R X_p + t
    x2 = X2[:, :2] / X2[:, 2:3]
    p1 = cvops.distort_points(x1[:, :2].copy(), intr, dist, distortion_model=model).reshape(-1, 2) if n else np.zeros((0, 2))
    p2 = cvops.distort_points(x2.copy(), intr, dist, distortion_model=model).reshape(-1, 2) if n else np.zeros((0, 2))
    out = rng.random(n) < outlier_share
    ang = rng.uniform(0, 2 * np.pi, n)
    mag = rng.uniform(outlier_px[0], outlier_px[1], n)
    p2 = p2 + (out[:, None] * mag[:, None]) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return dict(p1=p1.astype(np.float32), p2=p2.astype(np.float32), R=R, planted_outlier=out, t=t)


EQUIDISTANT_COEFFS = (-0.0126, 0.0129, -0.0161, 0.0062)
OPERATOR_SIZES = (0, 1, 2, 3, 5, 64, 65, 100, 300, 1500)


def operator_problem_set(cfg, base_seed=2, reps=3):
    """The seeded problems of the operator-vs-reference test: every size x both distortion models x {outlier shares 0, 20, 40, 60 %,
    standstill with 10 % outliers, nothing but outliers} x reps.  Each entry: dict(p1, p2, R, model, intr, dist, frame, camera, seed)."""
    out = []
    k = 0
    for model in ('radtan', 'equidistant'):
        intr = np.asarray(cfg.cam0_intrinsics, dtype=np.float64)
        dist = np.asarray(cfg.cam0_distortion_coeffs if model == 'radtan' else EQUIDISTANT_COEFFS, dtype=np.float64)
        for n in OPERATOR_SIZES:
            for kind in (0.0, 0.2, 0.4, 0.6, 'still', 'junk'):
                for r in range(reps):
                    rng = np.random.default_rng([base_seed, k])
                    if kind == 'still':
                        pr = planted_problem(rng, n, (intr, dist), 0.1, standstill=True, model=model, outlier_px=(1.0, 8.0))
                    elif kind == 'junk':
                        pr = planted_problem(rng, n, (intr, dist), 1.0, model=model, trans=0.03, outlier_px=(25.0, 48.0))
                    else:
                        pr = planted_problem(rng, n, (intr, dist), kind, model=model, trans=(0.03, 0.08, 0.15)[r % 3])
                    pr.update(model=model, intr=intr, dist=dist, frame=k * 7 + 1, camera=k & 1, seed=base_seed + (k % 5), kind=kind, n=n)
                    out.append(pr)
                    k += 1
    return out
