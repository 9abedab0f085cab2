"""The front-end engine with exposure-time normalisation on (config.exposure_reference) fed the frames of an auto-exposing rig --
every frame and each camera at an exposure of its own, behind a vignetting lens and a gamma-like sensor -- against the unmodified CPU
oracle front-end fed the frames the NumPy definition of tests/exposure_ref.py corrected: every entry path, exposure alone, behind a
conversion and ahead of binning and CLAHE, placement in a batch, an entry named twice in one upload, the identity against a
photometric-only engine, the refusals, the pending rule, the read-back, the drop-in, and off is off."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bayer_ref as br
import clahe_ref as cr
import downscale_ref as dr
import exposure_ref as er
import photometric_ref as pr
from conftest import ROOT
from exposure_helpers import T_REF, exposed_stream, run_engine
from fe_harness import MODES, Frames, against_oracle, bare_cfg, make_cfg as _cfg, run_engine as run_plain, run_oracle, same as _same

pytestmark = pytest.mark.gpu

W, H = 752, 480
NF = 3
MIN_FEATURES = 20             # every compared oracle run publishes at least this many features in every frame
# exposure ratios t / t_ref by stream, camera and frame: stream 0 those of the motivating measurement, stream 1 others
RATIOS = (er.RATIOS, ((1.0, 0.6, 1.5, 0.7), (1.0, 0.7, 1.4, 0.9)))


class T(object):
    """The calibration of the rig (that of tests/test_gpu_photometric_engine.py): u, v the float tables of the config object, q their
    quantised twins, fwd the sensors."""
    v = (pr.radial_vignette(W, H, 0.35), pr.radial_vignette(W, H, 0.45))
    u = (pr.gamma_inverse_response(2.2), pr.gamma_inverse_response(1.8))
    fwd = (pr.gamma_forward(2.2), pr.gamma_forward(1.8))
    q = ((pr.quantise_response(u[0]), pr.quantise_vignette(v[0])), (pr.quantise_response(u[1]), pr.quantise_vignette(v[1])))


def photo_cfg(**kw):
    return _cfg(cam0_response=T.u[0], cam1_response=T.u[1], cam0_vignette=T.v[0], cam1_vignette=T.v[1], **kw)


def expo_cfg(**kw):
    return photo_cfg(exposure_reference=T_REF, **kw)


def check_reference(refs):
    for r in refs:
        assert len(r) == NF and all(len(f['ids']) >= MIN_FEATURES for f in r), [len(f['ids']) for f in r]


def factors(stream, k):
    return tuple(int(er.quantise(t, T_REF)) for t in stream.exposure[k])


@pytest.fixture(scope='module')
def bases():
    from uav_airvision_amd.synth import SyntheticStream
    return [Frames.cached(SyntheticStream(_cfg(), seed=s, n_frames=NF, motion_scale=m)) for s, m in er.SEEDS]


@pytest.fixture(scope='module')
def expo(bases):
    """Two streams behind gamma + vignette + exposure, their reference-corrected twins and the oracle on those: computed once."""
    streams = [exposed_stream(b, NF, RATIOS[i], T.q, T.v, T.fwd) for i, b in enumerate(bases)]
    d, c = streams[0].raw[1][1], streams[0].frame(1).cam0_image
    assert np.array_equal(c, er.correct(d, *T.q[0], k=7447)) and not np.array_equal(c, pr.correct(d, *T.q[0]))
    assert factors(streams[0], 1) == (7447, 6827) and factors(streams[1], 2) == (2731, 2926) and factors(streams[0], 0) == (4096, 4096)
    refs = [run_oracle(_cfg(), s) for s in streams]
    check_reference(refs)
    return streams, refs


@pytest.fixture(scope='module')
def runs(expo):
    streams, _refs = expo
    return {mode: run_engine(expo_cfg(), streams, mode=mode, images_of=1) for mode in MODES}


def _check_paths(streams, refs, runs, mode, tag):
    got, images = runs[mode]
    against_oracle(refs[1], got[1], '%s %s stream 1' % (tag, mode), images, streams[1], min_features=MIN_FEATURES)
    against_oracle(refs[0], got[0], '%s %s stream 0' % (tag, mode), min_features=MIN_FEATURES)
    for s in (0, 1):                                   # read_exposure: the factors of the frame the step worked on
        assert [f[3] for f in got[s]] == [factors(streams[s], k) for k in range(NF)], (tag, mode, s)


def _check_agreement(runs):
    first, first_images = runs[MODES[0]]
    for mode in MODES[1:]:
        got, images = runs[mode]
        for s in range(2):
            assert all(_same(a, b) for a, b in zip(first[s], got[s])), (mode, s)
        assert all(np.array_equal(a[c], b[c]) for a, b in zip(first_images, images) for c in (0, 1)), mode


@pytest.mark.parametrize('mode', MODES)
def test_every_entry_path_matches_the_oracle_on_corrected_frames(expo, runs, mode):
    """read_image of both cameras is the definition applied to the recorded frame with the camera's tables and the frame's factor; ids,
    points and counters are the unmodified oracle's on those frames; the caller's frames are unchanged (run_engine)."""
    _check_paths(expo[0], expo[1], runs, mode, 'exposure')


def test_the_entry_paths_agree(runs):
    _check_agreement(runs)


def test_without_the_normalisation_the_same_frames_lose_their_tracks(expo, runs):
    """What the stage buys: on frame 2 the engine with the normalisation continues the oracle's tracks, and the photometric-only
    engine on the same frames less than half of them."""
    streams, refs = expo
    on = runs['step'][0][0][2][2]['after_matching']
    off = run_plain(photo_cfg(), [streams[0]], mode='step', raw=True)[0][2][2]['after_matching']
    assert on == refs[0][2]['nf']['after_matching'] >= 60 and 2 * off < on, (on, off, refs[0][2]['nf'])


# ---- exposure alone: flag 16 only, no tables -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def alone(bases):
    st = exposed_stream(bases[0], NF, RATIOS[0])
    ref = run_oracle(_cfg(), st)
    check_reference([ref])
    return st, ref


@pytest.mark.parametrize('mode', ['step', 'prestage', 'frames'])
def test_exposure_alone(alone, mode):
    """A linear sensor behind a lens without fall-off: the engine has AV_FE_EXPOSURE only, av_frontend_set_photometric is never called
    and the tables are the identity."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine, pack_frontend_config
    cfg = _cfg(exposure_reference=T_REF)
    assert pack_frontend_config(cfg).flags & (N.AV_FE_EXPOSURE | N.AV_FE_PHOTOMETRIC) == N.AV_FE_EXPOSURE == 16
    st, ref = alone
    got, images = run_engine(cfg, [st], mode=mode, images_of=0)
    against_oracle(ref, got[0], 'alone ' + mode, images, st, min_features=MIN_FEATURES)
    if mode == 'step':
        eng = FrontendEngine(cfg, n_streams=1)
        assert eng.exposure and not eng.photometric
        with pytest.raises(N.AirvisionError, match='without AV_FE_PHOTOMETRIC'):
            eng.set_photometric(*T.q[0], *T.q[1])
        eng.close()


# ---- behind a conversion, ahead of binning and CLAHE ------------------------------------------------------------------------------
FMT = 'bayer_rggb16'


@pytest.fixture(scope='module')
def chain(bases):
    """The recorded frames as 16-bit mosaics; the reference chain demosaic -> correct -> bin by two -> equalise; the oracle on that."""
    from uav_airvision_amd.frontend import downscaled_config
    streams = [exposed_stream(b, NF, RATIOS[i], T.q, T.v, T.fwd, lambda g: br.mosaic(g, FMT, br.GAINS, 8), lambda r: br.to_gray8(r, FMT, 8),
                              lambda a: cr.clahe(dr.downscale(a, 2), 2.0, (8, 8))) for i, b in enumerate(bases)]
    assert streams[0].frame(0).cam0_image.shape == (H // 2, W // 2) and streams[0].raw[0][1].dtype == np.uint16
    refs = [run_oracle(downscaled_config(_cfg(image_downscale=2)), s) for s in streams]
    check_reference(refs)
    return streams, refs


@pytest.mark.parametrize('mode', ['step', 'frames'])
def test_behind_a_conversion_and_ahead_of_binning_and_clahe(chain, mode):
    """Demosaic into the full-size scratch, the correction with the frame's factor in place there, binning into level 0, equalisation
    in place: byte for byte the reference chain, and the oracle's message on it."""
    streams, refs = chain
    got, images = run_engine(expo_cfg(image_format=FMT, image_downscale=2, use_clahe=True), streams, mode=mode, images_of=1)
    _check_paths(streams, refs, {mode: (got, images)}, mode, 'chain')


def test_a_stream_gives_the_same_result_at_either_end_of_a_batch(expo):
    """Entries 0 and 5 of a six-stream batch hold stream 0 (the others stream 1, at other exposures): every stream's factor goes with
    its own frames, in the device path and through the frame store."""
    streams, refs = expo
    batch = [streams[0], streams[1], streams[1], streams[1], streams[1], streams[0]]
    for mode in ('step', 'frames'):
        got = run_engine(expo_cfg(), batch, mode=mode)
        for pos in (0, 5):
            against_oracle(refs[0], got[pos], 'batch %s entry %d' % (mode, pos), min_features=MIN_FEATURES)
        against_oracle(refs[1], got[3], 'batch %s entry 3' % mode, min_features=MIN_FEATURES)
        assert not all(_same(a, b) for a, b in zip(got[0], got[1])), mode


def test_an_entry_named_twice_takes_the_later_frame_and_the_later_factor(expo):
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = expo
    eng = FrontendEngine(expo_cfg(), n_streams=2)
    eng.frames_reserve(4)
    (ta, a0, a1), (_tb, b0, b1), (tx, x0, x1) = streams[0].raw[1], streams[0].raw[2], streams[1].raw[1]
    ea, eb, ex = streams[0].exposure[1], streams[0].exposure[2], streams[1].exposure[1]
    up = dict(exposure=(np.array([eb[0], ex[0], ea[0]]), np.array([eb[1], ex[1], ea[1]])))
    eng.frames_upload(np.array([2, 1, 2], np.int32), np.stack([b0, x0, a0]), np.stack([b1, x1, a1]), **up)
    eng.step_frames([2, 1], [ta, tx])
    eng.read_features()
    for s, want in ((0, streams[0].frame(1)), (1, streams[1].frame(1))):
        assert np.array_equal(eng.read_image(s, 0), want.cam0_image) and np.array_equal(eng.read_image(s, 1), want.cam1_image), s
    assert eng.read_exposure(0) == factors(streams[0], 1) != factors(streams[0], 2) and eng.read_exposure(1) == factors(streams[1], 1)
    # (the earlier frame's factor on the later frame, or a second pass, would have shown)
    assert not np.array_equal(er.correct(a0, *T.q[0], k=factors(streams[0], 2)[0]), streams[0].frame(1).cam0_image)
    eng.close()
    with_clahe = FrontendEngine(expo_cfg(use_clahe=True), n_streams=2)
    with_clahe.frames_reserve(4)
    with pytest.raises(N.AirvisionError, match='named twice'):                       # with CLAHE the refusal of duplicates stands
        with_clahe.frames_upload(np.array([2, 1, 2], np.int32), np.stack([b0, x0, a0]), np.stack([b1, x1, a1]), **up)
    with_clahe.close()


def test_all_exposures_at_the_reference_is_a_photometric_engine(bases):
    """k = 4096 for every frame: the same features, the same images and the same timing spans as an engine with the tables alone."""
    ones = ((1.0,) * NF, (1.0,) * NF)
    st = exposed_stream(bases[0], NF, ones, T.q, T.v, T.fwd)
    for mode in ('step', 'frames'):
        (a, im_a, sp_a) = run_plain(photo_cfg(), [st], mode=mode, raw=True, images_of=0, timing=True)
        (b, im_b, sp_b) = run_engine(expo_cfg(), [st], mode=mode, images_of=0, timing=True)
        assert all(len(f[0]) >= MIN_FEATURES for f in a[0])
        assert all(_same(x, y[:3]) for x, y in zip(a[0], b[0])), mode
        assert all(np.array_equal(x[c], y[c]) for x, y in zip(im_a, im_b) for c in (0, 1)), mode
        assert sp_a == sp_b and (mode != 'step' or all(s['pyramid'] == 1 for s in sp_b)) and sum(sp_b[-1].values()) > 10, (mode, sp_a, sp_b)


# ---- refusals, the pending rule, the read-back ------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_a_frame_without_factors_is_refused(expo):
    """Through ctypes (the Python methods raise ValueError before the call): step, prestage, step_host and upload on an engine with the
    flag and nothing pending name av_frontend_next_exposure; the engine then works with them."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = expo
    ts, d0, d1 = streams[0].raw[1]
    eng = FrontendEngine(expo_cfg(), n_streams=1, inputs_persist=True)
    eng.frames_reserve(2)
    t0, t1 = torch.from_numpy(d0[None]).cuda(), torch.from_numpy(d1[None]).cuda()
    L, fb, st = N.lib(), W * H, N.current_stream()
    tsd = (C.c_double * 1)(ts)
    slot = np.array([0], np.int32)
    calls = dict(step=lambda: L.av_frontend_step(eng._h, N.dptr(t0), N.dptr(t1), fb, tsd, st),
                 prestage=lambda: L.av_frontend_prestage(eng._h, N.dptr(t0), N.dptr(t1), fb, st),
                 step_host=lambda: L.av_frontend_step_host(eng._h, _ptr(d0), _ptr(d1), fb, tsd, st),
                 upload=lambda: L.av_frontend_frames_upload(eng._h, _ptr(slot), 1, _ptr(d0), _ptr(d1), fb, st))
    for name, call in calls.items():
        assert call() == N.AV_E_INVALID, name
        assert b'av_frontend_next_exposure' in L.av_last_error() and b'AV_FE_EXPOSURE' in L.av_last_error(), (name, L.av_last_error())
    # the Python methods say so before the call
    for call in (lambda: eng.step(t0, t1, [ts]), lambda: eng.prestage(t0, t1), lambda: eng.step_host(d0, d1, [ts]), lambda: eng.frames_upload([0], d0[None], d1[None])):
        with pytest.raises(ValueError, match='exposure='):
            call()
    k = np.array([4096], np.uint16)
    zero = np.array([0], np.uint16)
    for k0, k1, n, text in ((zero, k, 1, b'is 0'), (k, zero, 1, b'is 0'), (None, k, 1, b'null'), (k, None, 1, b'null'), (k, k, 0, b'n = 0')):
        assert L.av_frontend_next_exposure(eng._h, None if k0 is None else _ptr(k0), None if k1 is None else _ptr(k1), n) == N.AV_E_INVALID
        assert text in L.av_last_error(), L.av_last_error()
        assert calls['step']() == N.AV_E_INVALID                                   # (nothing was left pending by the refused call)
    # a wrong n is found by the call that consumes the factors, and leaves nothing pending
    two = np.array([4096, 4096], np.uint16)
    for name in ('step', 'prestage', 'step_host', 'upload'):
        assert L.av_frontend_next_exposure(eng._h, _ptr(two), _ptr(two), 2) == N.AV_OK
        assert calls[name]() == N.AV_E_INVALID and b'2 frames' in L.av_last_error(), (name, L.av_last_error())
        assert calls[name]() == N.AV_E_INVALID and b'av_frontend_next_exposure' in L.av_last_error(), name
    with pytest.raises(ValueError, match='exposures per camera'):
        eng.step_host(d0, d1, [ts], exposure=([8.0, 8.0], [8.0, 8.0]))
    with pytest.raises(ValueError, match='uint16'):
        eng.step_host(d0, d1, [ts], exposure_q=([4096], [4096]))
    with pytest.raises(ValueError, match='factor of 0'):
        eng.step_host(d0, d1, [ts], exposure_q=(zero, k))
    with pytest.raises(ValueError, match='finite and > 0'):
        eng.step_host(d0, d1, [ts], exposure=([0.0], [8.0]))
    # and with the factors the engine works: ready uint16 factors through exposure_q
    q = factors(streams[0], 1)
    eng.step_host(d0, d1, [ts], exposure_q=(np.array([q[0]], np.uint16), np.array([q[1]], np.uint16)))
    eng.read_features()
    assert np.array_equal(eng.read_image(0, 0), streams[0].frame(1).cam0_image) and eng.read_exposure(0) == q
    eng.close()


def test_factors_given_to_an_engine_without_the_flag_are_refused(expo):
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = expo
    ts, d0, d1 = streams[0].raw[0]
    eng = FrontendEngine(photo_cfg(), n_streams=1)
    assert not eng.exposure
    k = np.array([4096], np.uint16)
    assert N.lib().av_frontend_next_exposure(eng._h, _ptr(k), _ptr(k), 1) == N.AV_E_INVALID and b'without AV_FE_EXPOSURE' in N.lib().av_last_error()
    with pytest.raises(N.AirvisionError, match='without AV_FE_EXPOSURE'):
        eng.read_exposure(0)
    with pytest.raises(ValueError, match='without config.exposure_reference'):
        eng.step_host(d0, d1, [ts], exposure=([8.0], [8.0]))
    eng.step_host(d0, d1, [ts])                        # and takes its frames as before
    eng.read_features()
    eng.close()


def test_factors_left_pending_across_a_step_that_skipped_the_stage_are_discarded(expo):
    """Factors given before a prestage belong to the prestaged frames; the step that follows with the same tensors skips the stage,
    needs none, and discards what it finds pending: the next frame does not get them."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = expo
    st = streams[0]
    eng = FrontendEngine(expo_cfg(), n_streams=1, inputs_persist=True)
    dev = [(torch.from_numpy(st.raw[k][1][None]).cuda(), torch.from_numpy(st.raw[k][2][None]).cuda()) for k in range(NF)]
    e = lambda k: dict(exposure=([st.exposure[k][0]], [st.exposure[k][1]]))      # noqa: E731
    with pytest.raises(N.AirvisionError, match='no step has run'):
        eng.read_exposure(0)
    eng.step(*dev[0], [st.raw[0][0]], **e(0))
    eng.prestage(*dev[1], **e(1))
    eng.read_features()
    assert eng.read_exposure(0) == factors(st, 0)                                  # (the prestaged frame's factors wait for its step)
    stale = np.array([12345], np.uint16)
    assert N.lib().av_frontend_next_exposure(eng._h, _ptr(stale), _ptr(stale), 1) == N.AV_OK
    eng.step(*dev[1], [st.raw[1][0]])                                              # skips the stage; the stale factors go
    eng.read_features()
    assert eng.read_exposure(0) == factors(st, 1) and np.array_equal(eng.read_image(0, 0), st.frame(1).cam0_image)
    ts2 = (C.c_double * 1)(st.raw[2][0])
    assert N.lib().av_frontend_step(eng._h, N.dptr(dev[2][0]), N.dptr(dev[2][1]), W * H, ts2, N.current_stream()) == N.AV_E_INVALID
    assert b'av_frontend_next_exposure' in N.lib().av_last_error()
    eng.step(*dev[2], [st.raw[2][0]], **e(2))
    eng.read_features()
    assert eng.read_exposure(0) == factors(st, 2) and np.array_equal(eng.read_image(0, 1), st.frame(2).cam1_image)
    eng.close()


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------
class _Img(object):
    """An image message that carries its exposure time (the reference's namedtuple has no room for it)."""

    def __init__(self, timestamp, image, exposure=None):
        self.timestamp, self.image = timestamp, image
        if exposure is not None:
            self.exposure = exposure


def test_the_drop_in_image_processor_reads_the_exposure_off_the_messages(expo):
    from uav_airvision_amd.synth import replay
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    streams, refs = expo
    st, ref = streams[0], refs[0]

    def messages(with_exposure):
        out = []
        for k in range(NF):
            m, (_ts, r0, r1), (e0, e1) = st.frame(k), st.raw[k], st.exposure[k]
            out.append(type(m)(m.timestamp, r0, r1, _Img(m.timestamp, r0, e0 if with_exposure else None), _Img(m.timestamp, r1, e1 if with_exposure else None)))
        return Frames(st, out)
    proc = ip.ImageProcessor(expo_cfg())
    seen = []
    replay(messages(True), [proc.imu_callback], lambda m: seen.append(proc.stereo_callback(m)))
    assert len(seen) == NF
    for k, msg in enumerate(seen):
        assert np.array_equal(np.array([f.id for f in msg.features], np.int64), ref[k]['ids']), k
        assert np.array_equal(np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features]).reshape(-1, 4).view(np.uint64), ref[k]['uv'].view(np.uint64)), k
    assert np.array_equal(proc.equalized_image(1), st.frame(NF - 1).cam1_image)
    proc.close()
    proc = ip.ImageProcessor(expo_cfg())
    with pytest.raises(ValueError, match='cam0_msg carries no attribute `exposure`'):
        proc.stereo_callback(messages(False).frame(0))
    proc.close()
    # without exposure_reference nothing is read: the reference's own namedtuple messages pass
    proc = ip.ImageProcessor(photo_cfg())
    m, (_ts, r0, r1) = st.frame(0), st.raw[0]
    assert len(proc.stereo_callback(type(m)(m.timestamp, r0, r1, type(m.cam0_msg)(m.timestamp, r0), type(m.cam1_msg)(m.timestamp, r1))).features) >= MIN_FEATURES
    proc.close()


# ---- off changes nothing (these two pass without the feature) ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def plain_run(bases):
    return run_plain(_cfg(), [bases[0]], mode='step', timing=True)


def test_exposure_reference_none_is_a_plain_engine(bases, plain_run):
    off, sp_off = plain_run
    got, sp = run_plain(_cfg(exposure_reference=None), [bases[0]], mode='step', timing=True)
    assert all(len(a[0]) > 40 for a in off[0])
    assert all(_same(a, b) for a, b in zip(off[0], got[0])) and sp == sp_off


def test_a_config_object_without_the_attribute_is_a_plain_engine(bases, plain_run):
    off, sp_off = plain_run
    bare = bare_cfg(lambda k: k == 'exposure_reference')
    assert not hasattr(bare, 'exposure_reference')
    for mode in ('step', 'frames'):
        got, sp = run_plain(bare, [bases[0]], mode=mode, timing=True)
        assert all(_same(a, b) for a, b in zip(off[0], got[0])), mode
        if mode == 'step':
            assert sp == sp_off
