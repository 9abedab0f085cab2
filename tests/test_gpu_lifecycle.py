"""What an object of the library holds on the device, from create to close (uav_airvision_amd/csrc/av_resources.h), read through
av_debug_live_resources: [bytes of device memory, bytes of pinned memory, events, streams] of the whole process.

Every case starts from four zeros (a leak of an earlier case fails here, not later), sees the counts the object must have above zero
while it is alive, sees four zeros after close(), and runs twice: the two cycles peak at the same counts.  What the runs compute is
not asserted here; the parity tests do that.  Small shapes throughout: two streams, 376 x 240 images, three frames."""
import ctypes

import numpy as np
import pytest

from fe_harness import Frames, run_engine, scaled_cfg

pytestmark = pytest.mark.gpu

DEV, PINNED, EVENTS, STREAMS = range(4)
S, W, H, N_FRAMES = 2, 376, 240, 3


def live():
    from uav_airvision_amd import _native as N
    out = (ctypes.c_int64 * 4)()
    N.check(N.lib().av_debug_live_resources(ctypes.byref(out)))
    return tuple(int(v) for v in out)


class Peak(object):
    """The largest value of each count over the samples taken."""

    def __init__(self):
        self.max = [0, 0, 0, 0]

    def sample(self):
        now = live()
        self.max = [max(a, b) for a, b in zip(self.max, now)]
        return now


def two_cycles(cycle, must_have):
    """cycle(peak) creates an object, runs it (sampling into peak while the object is alive) and closes it."""
    peaks = []
    for _ in range(2):
        assert live() == (0, 0, 0, 0)
        peak = Peak()
        cycle(peak)
        assert live() == (0, 0, 0, 0), 'alive after close'
        assert all(peak.max[c] > 0 for c in must_have), (peak.max, must_have)
        peaks.append(peak.max)
    assert peaks[0] == peaks[1], peaks
    return peaks[0]


# ---- front-end -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def grey():
    """Two streams of three 376 x 240 frames, rendered once, with their 16-bit twins for the raw variants."""
    from uav_airvision_amd.synth import SyntheticStream
    cfg = scaled_cfg(W, H)
    streams = [Frames.cached(SyntheticStream(cfg, seed=11 + i, n_frames=N_FRAMES)) for i in range(S)]
    raw = [Frames.raw_twin(st, lambda g: g.astype(np.uint16) << 8, lambda r: (r >> 8).astype(np.uint8), N_FRAMES) for st in streams]
    return streams, raw


@pytest.mark.parametrize('mode,raw', [('step', False), ('persist', False), ('prestage', False), ('host', False), ('frames', False),
                                      ('step', True), ('prestage', True), ('host', True), ('frames', True)])
def test_frontend_entry_paths_release_everything(grey, mode, raw):
    streams = grey[1] if raw else grey[0]
    cfg = scaled_cfg(W, H, image_format='gray16') if raw else scaled_cfg(W, H)

    def cycle(peak):
        run_engine(cfg, streams, mode=mode, raw=raw, read=lambda eng, i: (peak.sample(),))      # (creates the engine, closes it at the end)
    # the copy stream exists on the two paths that stage host frames
    two_cycles(cycle, (DEV, PINNED, EVENTS) + ((STREAMS,) if mode in ('host', 'frames') else ()))


def _all_options(fmt, **kw):
    """Every optional buffer of an engine that takes frames of `fmt`: binning, photometric tables and exposure, CLAHE, RANSAC, masks."""
    from uav_airvision_amd.frontend import circle_mask
    w, h = 2 * W, 2 * H                                   # the frames; binned 2 x 2 the engine works on 376 x 240
    y, x = np.mgrid[0:h, 0:w]
    vignette = 1.0 - 0.3 * ((x - w / 2.0) ** 2 + (y - h / 2.0) ** 2) / float(w * w)
    response = 255.0 * (np.arange(256) / 255.0) ** 1.1
    return scaled_cfg(w, h, image_format=fmt, image_downscale=2, use_clahe=True, use_ransac=True, exposure_reference=0.01,
                      cam0_response=response, cam1_response=response, cam0_vignette=vignette, cam1_vignette=vignette,
                      cam0_mask=circle_mask(w, h, w / 2.0, h / 2.0, 0.6 * w), cam1_mask=circle_mask(w, h, w / 2.0, h / 2.0, 0.55 * w), **kw)


def _raw_frames(eng, grey, n, first):
    """n frames per camera in the format of an _all_options engine, cut from the rendered streams: each 376 x 240 grey frame doubled to
    the engine's input size (binned 2 x 2 it is the frame again), as 16-bit samples or packed 10-bit ones."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import pack_frames
    msgs = [st.frame(k) for k in range(N_FRAMES) for st in grey[0]]
    out = []
    for cam in range(2):
        g = np.stack([(msgs[(first + i) % len(msgs)].cam1_image if cam else msgs[(first + i) % len(msgs)].cam0_image) for i in range(n)])
        big = g.repeat(2, axis=1).repeat(2, axis=2).astype(np.uint16)
        out.append(big << 8 if N.is_16bit(eng.pixel_format) else pack_frames(big << 2, eng.pixel_format))
    return out


def _expo(eng, n):
    return dict(exposure_q=(np.full(n, 4096, np.uint16), np.full(n, 5000, np.uint16))) if eng.exposure else {}


def _imu(eng, t):
    for i in range(S):
        eng.push_imu(i, t - 0.01, (0.01, -0.02, 0.005))


@pytest.mark.parametrize('fmt,kw', [('bayer_rggb10p', {}), ('gray16', dict(gray16_scale='auto'))])
def test_frontend_with_every_optional_buffer_through_the_frame_store(grey, fmt, kw):
    """Every optional buffer at once (a packed mosaic format has the mosaic scratch; the range scratch needs 'gray16', so a second
    engine has that one), timing on, through the frame store: uploads of 2 frames fill the staging ring's four entries, then one
    upload of 20 (> 2 + 16) makes the first entry and every store scratch take their grow path."""
    from uav_airvision_amd.frontend import FrontendEngine
    cfg = _all_options(fmt, **kw)

    def cycle(peak):
        eng = FrontendEngine(cfg, n_streams=S)
        try:
            eng.enable_timing(64)
            eng.frames_reserve(24)
            peak.sample()
            for k in range(4):
                a0, a1 = _raw_frames(eng, grey, 2, 2 * k)
                eng.frames_upload([2 * k, 2 * k + 1], a0, a1, **_expo(eng, 2))
            small = peak.sample()
            a0, a1 = _raw_frames(eng, grey, 20, 0)
            eng.frames_upload(np.arange(20), a0, a1, **_expo(eng, 20))
            grown = peak.sample()
            assert grown[DEV] > small[DEV] and grown[PINNED] > small[PINNED] and grown[EVENTS:] == small[EVENTS:], (small, grown)
            for k in range(N_FRAMES):
                _imu(eng, 100.0 + 0.05 * k)
                eng.step_frames([2 * k, 2 * k + 1], [100.0 + 0.05 * k] * S)
                eng.read_features()
                eng.read_timing()
                peak.sample()
        finally:
            eng.close()
    two_cycles(cycle, (DEV, PINNED, EVENTS, STREAMS))


def test_frontend_with_every_optional_buffer_through_the_step_paths(grey):
    """The same engine on device frames (prestaged from the second frame on) and, a second one, on host frames."""
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    cfg = _all_options('bayer_rggb10p')

    def cycle(peak):
        for host in (False, True):
            eng = FrontendEngine(cfg, n_streams=S, inputs_persist=not host)
            try:
                eng.enable_timing(64)
                frames = [_raw_frames(eng, grey, S, S * k) for k in range(N_FRAMES)]
                dev = [[torch.from_numpy(a).cuda() for a in f] for f in frames]
                for k in range(N_FRAMES):
                    ts = [100.0 + 0.05 * k] * S
                    _imu(eng, ts[0])
                    if host:
                        eng.step_host(frames[k][0], frames[k][1], ts, **_expo(eng, S))
                    else:
                        eng.step(dev[k][0], dev[k][1], ts, **({} if k else _expo(eng, S)))
                        if k + 1 < N_FRAMES:
                            eng.prestage(dev[k + 1][0], dev[k + 1][1], **_expo(eng, S))
                    eng.read_features()
                    eng.read_timing()
                    peak.sample()
                assert peak.sample()[STREAMS] == (1 if host else 0)
            finally:
                eng.close()
            assert live() == (0, 0, 0, 0)
    two_cycles(cycle, (DEV, PINNED, EVENTS, STREAMS))


# ---- filter --------------------------------------------------------------------------------------------------------------------
# `devbuf_growths` of counters() after filter_sequence, as the parent commit (the last one with the four hand-written allocators)
# reports it for the same sequence on the same GPU: the wider message of the later steps rebuilds the device-resident store once.
PARENT_GROWTHS = {'device': 1}


def filter_sequence(store, on_step=lambda: None):
    """Two streams with odom_cov (store 'device': the only store there is): ten steps with 64-wide messages, two with 192-wide ones.
    Returns counters()."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticFeatureStream
    cfg = ConfigEuRoC()
    n_frames = 12
    streams = [SyntheticFeatureStream(cfg, seed=41 + i, n_frames=n_frames, n_features=40) for i in range(S)]
    bat = BatchedMSCKF(cfg, S, odom_cov=(store == 'device'))
    try:
        assert bat.device_resident() == (store == 'device')
        its = [iter(st.imu) for st in streams]
        pend = [next(it, None) for it in its]
        published = 0
        for k in range(n_frames):
            msgs = [st.frame(k) for st in streams]
            si, ts, gy, ac = [], [], [], []
            for i, m in enumerate(msgs):
                while pend[i] is not None and pend[i].timestamp <= m.timestamp:
                    si.append(i); ts.append(pend[i].timestamp); gy.append(pend[i].angular_velocity); ac.append(pend[i].linear_acceleration)
                    pend[i] = next(its[i], None)
            if si:
                bat.push_imu(si, ts, gy, ac)
            cap = 64 if k < 10 else 192
            ids = np.zeros((S, cap), np.int64); uv = np.zeros((S, cap, 4)); nf = np.zeros(S, np.int32)
            for i, m in enumerate(msgs):
                nf[i] = len(m.features)
                for j, f in enumerate(m.features):
                    ids[i, j] = f.id; uv[i, j] = (f.u0, f.v0, f.u1, f.v1)
            out = bat.step(ids, uv, nf, [m.timestamp for m in msgs], cov=True if store == 'device' else None)
            published += int(out[:, 0].sum())
            on_step()
        assert published > 0
        return bat.counters()
    finally:
        bat.close()


@pytest.mark.parametrize('store', ['device'])
def test_batched_filter_releases_everything_and_grows_as_the_parent_did(store, monkeypatch):
    monkeypatch.delenv('AV_MSCKF_STORE', raising=False)
    counters = []
    # a batch of one stream group runs on the caller's stream and owns none of its own; every group of several owns one
    monkeypatch.delenv('AV_MSCKF_GROUPS', raising=False)
    two_cycles(lambda peak: counters.append(filter_sequence(store, peak.sample)), (DEV, PINNED, EVENTS))
    for c in counters:
        assert c['devbuf_growths'] == PARENT_GROWTHS[store], c
    monkeypatch.setenv('AV_MSCKF_GROUPS', '2')
    two_cycles(lambda peak: filter_sequence(store, peak.sample), (DEV, PINNED, EVENTS, STREAMS))


def test_single_filter_releases_everything():
    from uav_airvision_amd.msckf_ops import MsckfDevice

    def cycle(peak):
        flt = MsckfDevice(max_cam_states=20, rows_cap=2048)
        try:
            P = np.eye(flt.dim)
            flt.set_cov(P)
            assert np.array_equal(flt.get_cov(), P)
            peak.sample()
        finally:
            flt.close()
    two_cycles(cycle, (DEV,))
