"""End-to-end parity of the device-resident front-end engine against the CPU oracle front-end:
same seeded synthetic stereo+IMU streams, bit-exact feature ids and bit-exact (u0,v0,u1,v1)."""
import numpy as np
import pytest

from fe_harness import against_oracle, run_engine, run_oracle, same

pytestmark = pytest.mark.gpu


def _run_engine(cfg, streams, max_corners=8192):
    """Both flavours of the engine: level 0 copied into the padded pyramid (inputs only valid during the step) and level 0 read
    in place from the caller's tensors (AV_FE_INPUTS_PERSIST).  They must agree bit for bit; the caller compares with the oracle."""
    a = run_engine(cfg, streams, 'step', max_corners=max_corners)
    b = run_engine(cfg, streams, 'persist', max_corners=max_corners)
    for sa, sb in zip(a, b):
        assert len(sa) == len(sb) and all(same(fa, fb) for fa, fb in zip(sa, sb))
    return b


def test_engine_matches_oracle_two_streams_default_grid(cfg):
    from uav_airvision_amd.synth import SyntheticStream
    streams = [SyntheticStream(cfg, seed=s, n_frames=7) for s in (0, 1)]
    got = _run_engine(cfg, streams)
    for i, st in enumerate(streams):
        ref = run_oracle(cfg, st)
        assert len(ref[0]['ids']) > 30 and len(ref[-1]['ids']) > 60
        against_oracle(ref, got[i], 'stream %d' % i)


def test_engine_matches_oracle_300_features_fast_motion():
    """BASELINE configs[1] shape: grid 4x5 with 15 features per cell (300 tracked features)."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream
    cfg = ConfigEuRoC(grid_max_feature_num=15, grid_min_feature_num=8)
    st = SyntheticStream(cfg, seed=5, n_frames=8, motion_scale=2.5)
    got = _run_engine(cfg, [st])
    ref = run_oracle(cfg, st)
    assert len(ref[-1]['ids']) > 200
    against_oracle(ref, got[0], 'n300')


@pytest.mark.parametrize('win,levels', [(21, 2), (9, 4)])
def test_engine_matches_oracle_with_another_lk_window_and_pyramid_depth(win, levels):
    """`config.win_size` / `config.pyramid_levels` are configuration (config.py:31-44), not constants of the path: a 21 x 21 window
    over 3 pyramid levels and a 9 x 9 window over 5 go through the whole engine (temporal + stereo LK on the general kernel) and
    must match the CPU oracle frame by frame, ids and coordinates bit for bit, like the 15 x 15 / 4-level default."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream
    cfg = ConfigEuRoC()
    cfg.patch_size = win
    cfg.win_size = (win, win)
    cfg.pyramid_levels = levels
    cfg.lk_params = dict(cfg.lk_params, winSize=cfg.win_size, maxLevel=levels)
    st = SyntheticStream(cfg, seed=9, n_frames=6, motion_scale=1.5)
    got = _run_engine(cfg, [st])
    ref = run_oracle(cfg, st)
    assert len(ref[-1]['ids']) > 40
    against_oracle(ref, got[0], 'win%d_levels%d' % (win, levels))


def test_engine_matches_oracle_with_the_equidistant_distortion_model():
    """`config.cam*_distortion_model = 'equidistant'` (config.py:98,117 allow it; camera_model.py:41-43, 69-70 and
    feature_publisher.py:53-54 then call cv2.fisheye.*): the stereo matcher's initial guess, the epipolar gate and the published
    coordinates go through the Kannala-Brandt model on the device.  Same restatement as the oracle's (parity with OpenCV itself is
    unpinned: no cv2 here); ids, counts and pixel coordinates must be identical, the published normalised coordinates equal to a
    few ulp (tan / atan come from the device math library on one side and libm on the other)."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream
    cfg = ConfigEuRoC()
    st = SyntheticStream(cfg, seed=4, n_frames=6, motion_scale=1.5)         # (rendered through the radtan calibration: any images do)
    cfg.cam0_distortion_model = cfg.cam1_distortion_model = 'equidistant'
    cfg.cam0_distortion_coeffs = np.array([-0.0126, 0.0129, -0.0161, 0.0062])
    cfg.cam1_distortion_coeffs = np.array([-0.0119, 0.0103, -0.0128, 0.0047])
    got = _run_engine(cfg, [st])[0]
    ref = run_oracle(cfg, st)
    assert len(ref[-1]['ids']) > 40
    for k, (r, g) in enumerate(zip(ref, got)):
        ids_r, uv_r, nf, add = r['ids'], r['uv'], r['nf'], r['add']
        ids_g, uv_g, cnt = g
        if k > 0:
            assert cnt['before_tracking'] == nf['before_tracking'] and cnt['after_tracking'] == nf.get('after_tracking', 0), k
            assert cnt['after_matching'] == nf.get('after_matching', 0) and cnt['n_new'] == add['n_new'], k
        assert cnt['overflow'] == 0 and np.array_equal(ids_r, ids_g), k
        assert np.abs(uv_r - uv_g).max() < 1e-12, (k, np.abs(uv_r - uv_g).max())
    # and the model matters: the radtan engine publishes other coordinates for the same images
    cfg2 = ConfigEuRoC()
    got2 = _run_engine(cfg2, [st])[0]
    assert np.abs(got2[0][1][:20] - got[0][1][:20]).max() > 1e-4


def test_engine_capacity_overflow_is_reported(cfg):
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(cfg, seed=0, n_frames=1)
    with pytest.raises(AirvisionError):
        _run_engine(cfg, [st], max_corners=500)


def test_read_grid_state(cfg):
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(cfg, seed=2, n_frames=1)
    m = st.frame(0)
    eng = FrontendEngine(cfg, 1)
    eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
    (ids, uv), = eng.read_features()
    g = eng.read_grid(0)
    assert np.array_equal(g['ids'], ids) and g['next_feature_id'] == len(ids)
    assert (g['lifetime'] == 1).all() and (np.diff(g['cell']) >= 0).all()
    assert np.bincount(g['cell']).max() <= cfg.grid_min_feature_num
    eng.close()


def test_engine_matches_oracle_fine_grid_config5_shape():
    """BASELINE configs[4] shape: 10x15 grid (48x51-pixel cells, several cells per FAST tile), up to
    10 features per cell (1500 per frame)."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream
    cfg = ConfigEuRoC(grid_row=10, grid_col=15, grid_max_feature_num=10, grid_min_feature_num=4)
    st = SyntheticStream(cfg, seed=9, n_frames=5, motion_scale=2.0)
    got = _run_engine(cfg, [st])
    ref = run_oracle(cfg, st)
    assert len(ref[-1]['ids']) > 1000
    against_oracle(ref, got[0], 'n1500')


def test_engine_blank_and_late_texture_streams(cfg):
    """Edge cases: a stream of flat images (no corners, empty feature messages, nothing to track) next to a
    stream whose first frames are flat and then become textured (first-frame initialisation has already
    happened on an empty image, so features can only enter through the adder)."""
    from uav_airvision_amd.synth import SyntheticStream, stereo_msg_t, img_msg_t

    class Patched(object):
        def __init__(self, base, blank_until):
            self.base, self.blank_until = base, blank_until
            self.imu, self.n_frames = base.imu, base.n_frames

        def frame_time(self, k):
            return self.base.frame_time(k)

        def frame(self, k):
            m = self.base.frame(k)
            if k < self.blank_until:
                z0 = np.full_like(m.cam0_image, 97); z1 = np.full_like(m.cam1_image, 97)
                return stereo_msg_t(m.timestamp, z0, z1, img_msg_t(m.timestamp, z0), img_msg_t(m.timestamp, z1))
            return m
    base = SyntheticStream(cfg, seed=12, n_frames=6)
    streams = [Patched(base, 99), Patched(base, 2)]
    got = _run_engine(cfg, streams)
    for i, st in enumerate(streams):
        ref = run_oracle(cfg, st)
        against_oracle(ref, got[i], 'edge %d' % i)
    assert all(len(g[0]) == 0 for g in got[0])
    assert len(got[1][1][0]) == 0 and len(got[1][-1][0]) > 50


def test_two_phase_read_back_matches_blocking_read_and_checks_misuse(cfg):
    """av_frontend_read_features_begin/_end: same features as the blocking read, also when the next step is enqueued
    between the two halves; _end without a matching _begin is an error, not a hang."""
    import torch
    from uav_airvision_amd._native import AirvisionError
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(cfg, seed=17, n_frames=4)
    dev = torch.device('cuda', 0)

    def run(two_phase):
        eng = FrontendEngine(cfg, n_streams=1, device=0)
        it = iter(st.imu); pend = next(it, None)
        out = []
        imgs = []
        for k in range(4):
            m = st.frame(k)
            imgs.append((torch.from_numpy(m.cam0_image[None]).to(dev), torch.from_numpy(m.cam1_image[None]).to(dev), m.timestamp))
        def push(k):
            nonlocal pend
            idx, ts, gy = [], [], []
            while pend is not None and pend.timestamp <= imgs[k][2]:
                idx.append(0); ts.append(pend.timestamp); gy.append(pend.angular_velocity); pend = next(it, None)
            if idx:
                eng.push_imu_batch(np.array(idx, np.int32), np.array(ts), np.array(gy).reshape(-1, 3))
        if two_phase:
            with pytest.raises(AirvisionError):
                eng.read_features_end(1)
            push(0); eng.step(imgs[0][0], imgs[0][1], [imgs[0][2]]); eng.read_features_begin(0)
            for k in range(4):
                if k + 1 < 4:
                    push(k + 1); eng.step(imgs[k + 1][0], imgs[k + 1][1], [imgs[k + 1][2]]); eng.read_features_begin((k + 1) & 1)
                ids, uv, n = eng.read_features_end(k & 1)
                out.append((ids[0, :n[0]].copy(), uv[0, :n[0]].copy()))
        else:
            for k in range(4):
                push(k); eng.step(imgs[k][0], imgs[k][1], [imgs[k][2]])
                ids, uv, n = eng.read_features_raw()
                out.append((ids[0, :n[0]].copy(), uv[0, :n[0]].copy()))
        eng.close()
        return out

    a, b = run(False), run(True)
    for k in range(4):
        assert len(a[k][0]) > 20
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1].view(np.uint64), b[k][1].view(np.uint64)), k


def test_step_host_double_buffering_matches_resident_inputs(cfg):
    """av_frontend_step_host (pinned double-buffered H2D on a copy stream) gives the same features as the step on
    device-resident tensors, frame after frame, with the caller's host arrays overwritten right after each call."""
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream
    S, n_frames = 3, 6
    streams = [SyntheticStream(cfg, seed=23 + s, n_frames=n_frames) for s in range(S)]
    dev = torch.device('cuda', 0)

    def run(host):
        eng = FrontendEngine(cfg, n_streams=S, device=0)
        its = [iter(st.imu) for st in streams]
        pend = [next(it, None) for it in its]
        out = []
        buf0 = np.zeros((S, cfg.height if hasattr(cfg, 'height') else 480, 752), np.uint8)
        buf1 = np.zeros_like(buf0)
        for k in range(n_frames):
            msgs = [st.frame(k) for st in streams]
            idx, ts, gy = [], [], []
            for s, m in enumerate(msgs):
                while pend[s] is not None and pend[s].timestamp <= m.timestamp:
                    idx.append(s); ts.append(pend[s].timestamp); gy.append(pend[s].angular_velocity); pend[s] = next(its[s], None)
            if idx:
                eng.push_imu_batch(np.array(idx, np.int32), np.array(ts), np.array(gy).reshape(-1, 3))
            for s, m in enumerate(msgs):
                buf0[s] = m.cam0_image; buf1[s] = m.cam1_image
            tss = [m.timestamp for m in msgs]
            if host:
                eng.step_host(buf0, buf1, tss)
                buf0[:] = 0; buf1[:] = 255                    # the engine must have taken its copy already
            else:
                eng.step(torch.from_numpy(buf0.copy()).to(dev), torch.from_numpy(buf1.copy()).to(dev), tss)
            out.append(eng.read_features())
        eng.close()
        return out

    a, b = run(False), run(True)
    for k in range(n_frames):
        for s in range(S):
            assert len(a[k][s][0]) > 20
            assert np.array_equal(a[k][s][0], b[k][s][0]) and np.array_equal(a[k][s][1].view(np.uint64), b[k][s][1].view(np.uint64)), (k, s)


def test_shared_frame_store_matches_per_stream_steps_and_idles_finished_streams(cfg):
    """run.bat:4-12 replays one sequence from several start offsets (dataset.py:206-214 only moves the start index): the streams
    read the SAME frames a few steps apart.  `frames_upload` puts every distinct frame into the device store once (copy, pyramids,
    FAST), `step_frames` hands each stream its entry; the result must be bit-identical to `step_host` fed the per-stream images,
    frame by frame, and a stream whose sequence is over (entry -1) publishes nothing while the others go on -- also when a store
    entry is REUSED for a later frame (the store below has fewer entries than the sequence has frames)."""
    from uav_airvision_amd.euroc import SharedFramePlan
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream
    NF = 14
    st = SyntheticStream(cfg, seed=5, n_frames=NF)
    frames = [st.frame(k) for k in range(NF)]
    imu = list(st.imu)
    starts = [0, 2, 5]

    class Seq(object):                     # what SharedFramePlan needs of a dataset: (timestamp, cam0 key, cam1 key) per frame
        def __init__(self, s0):
            self.stereo_files = [(frames[f].timestamp, 'cam0/%d' % f, 'cam1/%d' % f) for f in range(s0, NF)]
    plan = SharedFramePlan([Seq(s0) for s0 in starts])
    assert plan.n_steps == NF and plan.n_frames_distinct == NF and plan.n_slots < NF        # entries are recycled
    S = len(starts)
    ref = FrontendEngine(cfg, n_streams=S)
    eng = FrontendEngine(cfg, n_streams=S)
    eng.frames_reserve(plan.n_slots)
    last = [-1e9] * S

    def upload(k):
        new = plan.new[k]
        fr = [int(p0.split('/')[1]) for _e, p0, _p1 in new]
        eng.frames_upload(np.array([e for e, _a, _b in new], np.int32), np.stack([frames[f].cam0_image for f in fr]), np.stack([frames[f].cam1_image for f in fr]))
    upload(0)
    for k in range(plan.n_steps):
        if k + 1 < plan.n_steps and plan.new[k + 1]:
            upload(k + 1)                  # before step k is enqueued: the protocol that overlaps the two (airvision.h)
        img0 = np.zeros((S, eng.height, eng.width), np.uint8); img1 = np.zeros_like(img0)
        ts = np.zeros(S)
        for s in range(S):
            f = starts[s] + k
            if f < NF:
                img0[s] = frames[f].cam0_image; img1[s] = frames[f].cam1_image; ts[s] = frames[f].timestamp
                assert plan.ts[k, s] == ts[s] and plan.slots[k, s] >= 0
                for m in imu:
                    if last[s] < m.timestamp <= ts[s]:
                        ref.push_imu(s, m.timestamp, m.angular_velocity); eng.push_imu(s, m.timestamp, m.angular_velocity)
                last[s] = ts[s]
            else:
                assert plan.slots[k, s] == -1
                ts[s] = last[s] + 0.05 * (f - NF + 1)
        ref.step_host(img0, img1, ts)
        eng.step_frames(plan.slots[k], ts)
        a, b = ref.read_features(), eng.read_features()
        for s in range(S):
            if plan.slots[k, s] < 0:
                assert len(b[s][0]) == 0, (k, s)
                continue
            assert len(b[s][0]) >= 40
            assert np.array_equal(a[s][0], b[s][0]), (k, s)
            assert np.array_equal(a[s][1].view(np.uint64), b[s][1].view(np.uint64)), (k, s)
            assert ref.read_counters(s) == eng.read_counters(s), (k, s)
    ref.close(); eng.close()
