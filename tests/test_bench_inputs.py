"""The benchmark's synthetic inputs, on the CPU: the batched renderer against SyntheticStream.frame_torch, the per-step IMU
arrays against a sample-by-sample construction, and the IMU feed of a run longer than its resident frames against the motion
those frames show."""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_batched_renderer_matches_frame_torch():
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    bench = _bench()
    cfg = bench.make_config()
    tex = make_texture(5)
    s0 = SyntheticStream(cfg, seed=1, n_frames=12, texture=tex)
    st = SyntheticStream(cfg, seed=2, n_frames=12, texture=tex, render=False, motion_scale=1.3, rest=0.2, tex_offset=(100.0, 50.0))
    st.tex, st.rays0, st.rays1 = tex, s0.rays0, s0.rays1
    st.pixel_noise = 0.0                                    # the noise draws differ by construction; the scene must not
    state = dict(tex=torch.from_numpy(tex), rays0=torch.from_numpy(s0.rays0), rays1=torch.from_numpy(s0.rays1))
    a0, a1 = bench.render_frames_torch(torch, st, state, range(3, 11), None)
    for i, k in enumerate(range(3, 11)):
        r0, r1 = st.frame_torch(k, state, None)
        assert torch.equal(a0[i], r0) and torch.equal(a1[i], r1), k


def test_imu_feed_steps_match_a_sample_by_sample_construction():
    bench = _bench()
    rng = np.random.default_rng(4)
    U, S, F = 5, 13, 9
    feeds, frame_times = [], np.zeros((F, U))
    for u in range(U):
        t = np.sort(rng.uniform(0.0, 10.0, rng.integers(20, 60)))
        feeds.append((t, rng.normal(size=(len(t), 3)), rng.normal(size=(len(t), 3))))
        frame_times[:, u] = np.sort(rng.uniform(0.0, 11.0, F))
    got = bench.imu_feed_steps(feeds, frame_times, S)
    pos = [0] * U
    for k in range(F):
        idx, ts, gy, ac = [], [], [], []
        for u, (t, g, a) in enumerate(feeds):
            lo = pos[u]
            while pos[u] < len(t) and t[pos[u]] <= frame_times[k, u]:
                pos[u] += 1
            for s in range(u, S, U):
                for j in range(lo, pos[u]):
                    idx.append(s); ts.append(t[j]); gy.append(g[j]); ac.append(a[j])
        want = (np.array(idx, np.int32), np.array(ts), np.array(gy).reshape(-1, 3), np.array(ac).reshape(-1, 3))
        for x, y in zip(got[k], want):
            assert x.dtype == y.dtype and np.array_equal(x, y), k


def test_mirrored_imu_follows_the_frames_shown():
    """Frames 0..P-1 once, then back and forth between P-1 and B: the specific force integrates to the velocity of the frames
    shown (sign included, through every turn) and the body rate is that of the content, negated on backward legs."""
    from uav_airvision_amd.synth import GRAVITY, SyntheticStream
    bench = _bench()
    cfg = bench.make_config()
    P, B, F = 40, 20, 200
    assert [bench.pool_index(k, P, B) for k in (0, 39, 40, 57, 58, 59, 76, 77, 78)] == [0, 39, 38, 21, 20, 21, 38, 39, 38]
    st = SyntheticStream(cfg, seed=3, n_frames=P, render=False, motion_scale=1.4, rest=0.3)
    t, g, a = bench.mirrored_imu(st, P, B, st.frame_time(F - 1))
    assert np.all(np.diff(t) > 0) and np.ptp(np.diff(t)) < 1e-9 and t[-1] <= st.frame_time(F - 1)
    t0, tE, tB = st.frame_time(0), st.frame_time(P - 1), st.frame_time(B)
    D = tE - tB

    def content(tau):                                       # (content time, +1 forward / -1 backward)
        if tau <= tE:
            return tau, 1.0
        m = (tau - tE) % (2 * D)
        return (tE - m, -1.0) if m <= D else (tB + m - D, 1.0)
    h = 1e-4
    v, worst = np.zeros(3), 0.0
    for i in range(1, len(t)):
        c, sg = content(t[i])
        v = v + (st.R_i_w(c) @ a[i] + GRAVITY) * (t[i] - t[i - 1])
        worst = max(worst, np.abs(v - sg * (st.position(c + h) - st.position(c - h)) / (2 * h)).max())
    assert worst < 0.05                                     # accelerometer noise only; a missed turn would leave 2 |v| ~ 0.5 m/s
    for i in np.nonzero(t > tE)[0][::97]:
        c, sg = content(t[i])
        w = st.R_i_w(c).T @ st.R_i_w(c + h)                 # body rate of the content, by finite differences
        rate = np.array([w[2, 1] - w[1, 2], w[0, 2] - w[2, 0], w[1, 0] - w[0, 1]]) / (2 * h)
        assert np.abs(g[i] - sg * rate).max() < 0.03        # gyro noise 0.005 rad/s, nearest-sample content time
