"""The front-end engine with the photometric calibration on (config.cam*_response / cam*_vignette) fed frames degraded by a vignetting
lens and a gamma-like sensor, against the unmodified CPU oracle front-end fed the frames the NumPy definition of
tests/photometric_ref.py corrected: every entry path, behind a conversion and ahead of binning and CLAHE, with a packed format, with a
static mask, placement in a batch, an entry named twice in one upload, the refusals, the timing spans, the drop-in, and off is off."""
import os
import sys

import numpy as np
import pytest

import bayer_ref as br
import clahe_ref as cr
import downscale_ref as dr
import mask_ref as mr
import packed_ref as kr
import photometric_ref as pr
from conftest import ROOT
from fe_harness import MODES, Frames, against_oracle, bare_cfg, make_cfg as _cfg, run_engine, run_oracle, same as _same, with_images

pytestmark = pytest.mark.gpu

W, H = 752, 480
NF = 3
MIN_FEATURES = 20             # every compared oracle run publishes at least this many features in every frame
ATTRS = ('cam0_response', 'cam1_response', 'cam0_vignette', 'cam1_vignette')


class T(object):
    """The calibration of the rig: a radial cos^4-style vignette down to 0.35 (cam0) / 0.45 (cam1) at the corners and a gamma 2.2 / 1.8
    sensor; u, v the float tables the config object is given, q their quantised twins (tests/photometric_ref.py), fwd the sensors."""
    v = (pr.radial_vignette(W, H, 0.35), pr.radial_vignette(W, H, 0.45))
    u = (pr.gamma_inverse_response(2.2), pr.gamma_inverse_response(1.8))
    fwd = (pr.gamma_forward(2.2), pr.gamma_forward(1.8))
    q = ((pr.quantise_response(u[0]), pr.quantise_vignette(v[0])), (pr.quantise_response(u[1]), pr.quantise_vignette(v[1])))


def photo_cfg(**kw):
    return _cfg(cam0_response=T.u[0], cam1_response=T.u[1], cam0_vignette=T.v[0], cam1_vignette=T.v[1], **kw)


def degrade(img, cam):
    """round(G(img * V)), clipped: what camera `cam` would have recorded."""
    return np.clip(np.floor(T.fwd[cam](img.astype(np.float64) * T.v[cam]) + 0.5), 0, 255).astype(np.uint8)


def degraded_stream(base, n_frames, encode=None, convert=None, post=None):
    """The first n frames of `base` as each camera records them, encode(degraded) (`.raw`: what the engine is fed), and their reference
    twin post(correct(convert(raw))) with each camera's own tables (`.frame`: what the unmodified oracle is fed)."""
    raw, conv = [], []
    for k in range(n_frames):
        m = base.frame(k)
        r = [degrade(im, c) for c, im in enumerate((m.cam0_image, m.cam1_image))]
        if encode is not None:
            r = [encode(x) for x in r]
        g = [pr.correct(x if convert is None else convert(x), *T.q[c]) for c, x in enumerate(r)]
        if post is not None:
            g = [post(x) for x in g]
        raw.append((m.timestamp, r[0], r[1]))
        conv.append(with_images(m, g[0], g[1]))
    return Frames(base, conv, raw)


def check_reference(refs):
    for r in refs:
        assert len(r) == NF and all(len(f['ids']) >= MIN_FEATURES for f in r), [len(f['ids']) for f in r]


@pytest.fixture(scope='module')
def bases():
    from uav_airvision_amd.synth import SyntheticStream
    return [Frames.cached(SyntheticStream(_cfg(), seed=17 + i, n_frames=NF, motion_scale=2.0 - 0.5 * i)) for i in range(2)]


@pytest.fixture(scope='module')
def photo(bases):
    """Two degraded streams, their reference-corrected twins and the oracle on those, computed once and never changed."""
    streams = [degraded_stream(b, NF) for b in bases]
    a, d, c = bases[0].frame(0).cam0_image, streams[0].raw[0][1], streams[0].frame(0).cam0_image
    assert np.array_equal(c, pr.correct(d, *T.q[0])) and not np.array_equal(c, d)
    assert T.v[0][0, 0] < 0.36 and T.v[0].max() > 0.999 and 11000 < T.q[0][1].max() < 12000
    # (the degradation is large and the correction undoes most of it: mean absolute difference to the undegraded frame)
    assert np.abs(d.astype(int) - a).mean() > 4 * np.abs(c.astype(int) - a).mean()
    refs = [run_oracle(_cfg(), s) for s in streams]
    check_reference(refs)
    return streams, refs


@pytest.fixture(scope='module')
def runs(photo):
    """Every entry path once: per mode the features of both streams and the images of stream 1."""
    streams, _refs = photo
    return {mode: run_engine(photo_cfg(), streams, mode=mode, raw=True, images_of=1) for mode in MODES}


def _check_paths(streams, refs, runs, mode, tag):
    got, images = runs[mode]
    against_oracle(refs[1], got[1], '%s %s stream 1' % (tag, mode), images, streams[1], min_features=MIN_FEATURES)
    against_oracle(refs[0], got[0], '%s %s stream 0' % (tag, mode), min_features=MIN_FEATURES)


def _check_agreement(runs):
    first, first_images = runs[MODES[0]]
    for mode in MODES[1:]:
        got, images = runs[mode]
        for s in range(2):
            assert all(_same(a, b) for a, b in zip(first[s], got[s])), (mode, s)
        assert all(np.array_equal(a[c], b[c]) for a, b in zip(first_images, images) for c in (0, 1)), mode


@pytest.mark.parametrize('mode', MODES)
def test_every_entry_path_matches_the_oracle_on_corrected_frames(photo, runs, mode):
    """read_image of both cameras is the definition applied to the degraded frame, each camera with its own tables; ids, points and
    counters are the unmodified oracle's on those frames, for both streams; the caller's frames are unchanged (run_engine)."""
    _check_paths(photo[0], photo[1], runs, mode, 'photometric')


def test_the_entry_paths_agree(runs):
    _check_agreement(runs)


# ---- behind a conversion, ahead of binning and CLAHE ------------------------------------------------------------------------------
FMT = 'bayer_rggb16'


@pytest.fixture(scope='module')
def chain(bases):
    """The degraded frames as 16-bit mosaics; the reference chain demosaic -> correct -> bin by two -> equalise; the oracle on that."""
    from uav_airvision_amd.frontend import downscaled_config
    streams = [degraded_stream(b, NF, lambda g: br.mosaic(g, FMT, br.GAINS, 8), lambda r: br.to_gray8(r, FMT, 8),
                               lambda a: cr.clahe(dr.downscale(a, 2), 2.0, (8, 8))) for b in bases]
    assert streams[0].frame(0).cam0_image.shape == (H // 2, W // 2) and streams[0].raw[0][1].dtype == np.uint16
    refs = [run_oracle(downscaled_config(_cfg(image_downscale=2)), s) for s in streams]
    check_reference(refs)
    return streams, refs


@pytest.fixture(scope='module')
def chain_runs(chain):
    streams, _refs = chain
    return {mode: run_engine(photo_cfg(image_format=FMT, image_downscale=2, use_clahe=True), streams, mode=mode, raw=True, images_of=1) for mode in MODES}


@pytest.mark.parametrize('mode', MODES)
def test_all_four_stages_in_every_entry_path(chain, chain_runs, mode):
    """Conversion into the full-size scratch, the correction in place there (the gain map is at the input size), binning into level 0,
    equalisation in place: byte for byte the reference chain, and the oracle's message on it."""
    _check_paths(chain[0], chain[1], chain_runs, mode, 'chain')


def test_all_four_stages_agree_across_the_entry_paths(chain_runs):
    _check_agreement(chain_runs)


@pytest.mark.parametrize('mode', ['step', 'frames'])
def test_behind_a_packed_format(bases, photo, mode):
    """gray12p: the unpacking writes level 0 (the store's entries through the `first` list) and the correction runs in place there.  The
    low four bits fall off at shift 8, so the reference frames and the oracle's run are those of the 8-bit degraded stream."""
    from uav_airvision_amd.frontend import pack_frames
    rng = np.random.default_rng(5)
    st = degraded_stream(bases[0], NF, lambda g: pack_frames((g.astype(np.uint16) << 4) | rng.integers(0, 16, g.shape, dtype=np.uint16), 'gray12p'),
                         lambda r: kr.to_gray8(r, 'gray12p'))
    assert st.raw[0][1].shape == (H, W * 3 // 2) and all(np.array_equal(st.frame(k).cam1_image, photo[0][0].frame(k).cam1_image) for k in range(NF))
    got, images = run_engine(photo_cfg(image_format='gray12p'), [st], mode=mode, raw=True, images_of=0)
    against_oracle(photo[1][0], got[0], 'gray12p ' + mode, images, st, min_features=MIN_FEATURES)


def test_with_a_cam0_circle_mask(photo):
    """Static masks are independent: a masked pixel is corrected like any other (read_image is the whole corrected frame) and the three
    gates work on the corrected frames -- against the masked oracle of tests/mask_ref.py."""
    from uav_airvision_amd.frontend import circle_mask
    streams, refs = photo
    c = circle_mask(W, H, 376, 240, 240)
    ref, _fe = mr.run_masked_oracle(_cfg(), streams[0], c, None)
    check_reference([ref])
    assert all(len(m['ids']) < len(f['ids']) for m, f in zip(ref, refs[0]))            # (the mask bites: fewer features than without it)
    for mode in ('step', 'frames'):
        got, images = run_engine(photo_cfg(cam0_mask=c), [streams[0]], mode=mode, raw=True, images_of=0)
        against_oracle(ref, got[0], 'circle ' + mode, images, streams[0], min_features=MIN_FEATURES)


def test_a_stream_gives_the_same_result_at_either_end_of_a_batch(photo, runs):
    """Entries 0 and 5 of a six-stream batch hold stream 0 (the others stream 1): one gain map for every stream, each stream's frames at
    its own place, in the device path and through the frame store."""
    streams, refs = photo
    batch = [streams[0], streams[1], streams[1], streams[1], streams[1], streams[0]]
    for mode in ('step', 'frames'):
        got = run_engine(photo_cfg(), batch, mode=mode, raw=True)
        for pos in (0, 5):
            against_oracle(refs[0], got[pos], 'batch %s entry %d' % (mode, pos), min_features=MIN_FEATURES)
        against_oracle(refs[1], got[3], 'batch %s entry 3' % mode, min_features=MIN_FEATURES)
        assert not all(_same(a, b) for a, b in zip(got[0], got[1])), mode


def test_an_entry_named_twice_takes_the_later_frame_corrected_once(photo):
    """The stage alone (8-bit grey in, no binning): it is then the launch that first writes the store, through the list that skips all
    but the last frame of an entry: the later frame, corrected exactly once, and the entry named once between the two its own."""
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = photo
    eng = FrontendEngine(photo_cfg(), n_streams=2)
    eng.frames_reserve(4)
    (ta, a0, a1), (_tb, b0, b1), (tx, x0, x1) = streams[0].raw[0], streams[0].raw[1], streams[1].raw[0]
    eng.frames_upload(np.array([2, 1, 2], np.int32), np.stack([b0, x0, a0]), np.stack([b1, x1, a1]))
    eng.step_frames([2, 1], [ta, tx])
    eng.read_features()
    for s, want in ((0, streams[0].frame(0)), (1, streams[1].frame(0))):
        assert np.array_equal(eng.read_image(s, 0), want.cam0_image) and np.array_equal(eng.read_image(s, 1), want.cam1_image), s
    assert not np.array_equal(streams[0].frame(0).cam0_image, streams[0].frame(1).cam0_image)
    twice = pr.correct(streams[0].frame(0).cam0_image, *T.q[0])
    assert not np.array_equal(twice, streams[0].frame(0).cam0_image)                 # (a second pass would have shown)
    eng.close()
    with_clahe = FrontendEngine(photo_cfg(use_clahe=True), n_streams=2)
    with_clahe.frames_reserve(4)
    from uav_airvision_amd import _native as N
    with pytest.raises(N.AirvisionError, match='named twice'):                       # with CLAHE the refusal of duplicates stands
        with_clahe.frames_upload(np.array([2, 1, 2], np.int32), np.stack([b0, x0, a0]), np.stack([b1, x1, a1]))
    with_clahe.close()


def test_refusals_and_read_back(photo):
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = photo
    ts, d0, d1 = streams[0].raw[0]
    # an engine without the flag refuses the call
    plain = FrontendEngine(_cfg(), n_streams=1)
    assert not plain.photometric
    with pytest.raises(N.AirvisionError, match='without AV_FE_PHOTOMETRIC') as e:
        plain.set_photometric(*T.q[0], *T.q[1])
    assert e.value.code == N.AV_E_INVALID
    with pytest.raises(N.AirvisionError, match='AV_FE_PHOTOMETRIC'):
        plain.read_photometric(0)
    plain.close()
    # read_photometric returns what was set; a part left out reads back as the identity
    eng = FrontendEngine(photo_cfg(), n_streams=1, inputs_persist=True)
    assert eng.photometric
    for cam in (0, 1):
        r, g = eng.read_photometric(cam)
        assert r.dtype == np.uint16 and g.dtype == np.uint16 and np.array_equal(r, T.q[cam][0]) and np.array_equal(g, T.q[cam][1]), cam
    eng.set_photometric(None, T.q[1][1], T.q[0][0], None)
    r, g = eng.read_photometric(0)
    assert np.array_equal(r, np.arange(256) * 256) and np.array_equal(g, T.q[1][1])
    r, g = eng.read_photometric(1)
    assert np.array_equal(r, T.q[0][0]) and (g == 4096).all()
    # the host-side checks: nothing is cast
    with pytest.raises(ValueError, match=r'cam0 response.*float64'):
        eng.set_photometric(T.u[0], None, None, None)
    with pytest.raises(ValueError, match=r'cam1 gain.*\(480, 752\).*\(240, 376\)'):
        eng.set_photometric(None, None, None, T.q[1][1][::2, ::2])
    with pytest.raises(ValueError, match='cam1 response.*65280'):
        eng.set_photometric(None, None, np.full(256, 65281, np.uint16), None)
    # the C entry refuses an entry above 65280 itself
    bad = np.full(256, 65281, np.uint16)
    assert N.lib().av_frontend_set_photometric(eng._h, bad.ctypes.data, None, None, None) == N.AV_E_INVALID and b'65280' in N.lib().av_last_error()
    # after a frame the tables stay: step, prestage and upload each count
    eng.set_photometric(*T.q[0], *T.q[1])
    eng.prestage(torch.from_numpy(d0[None]).cuda(), torch.from_numpy(d1[None]).cuda())
    with pytest.raises(N.AirvisionError, match='already been handed a frame'):
        eng.set_photometric(*T.q[0], *T.q[1])
    eng.close()
    for feed in ('step_host', 'frames_upload'):
        eng = FrontendEngine(photo_cfg(), n_streams=1)
        if feed == 'step_host':
            eng.step_host(d0, d1, [ts])
        else:
            eng.frames_reserve(2)
            eng.frames_upload([1], d0[None], d1[None])
        with pytest.raises(N.AirvisionError, match='already been handed a frame'):
            eng.set_photometric(*T.q[0], *T.q[1])
        eng.close()


def _engine_with_the_flag_and_no_tables():
    """A one-stream FrontendEngine around a native engine created with AV_FE_PHOTOMETRIC (and AV_FE_INPUTS_PERSIST, for prestage) from
    the packed configuration of a plain config object: the Python constructor never leaves an engine in that state."""
    import ctypes as C
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine, pack_frontend_config

    class Bare(FrontendEngine):
        def __init__(self):
            self.config, self.n_streams, self.device, self._keep, self._h = _cfg(), 1, 0, None, C.c_void_p()
            self._cfg = pack_frontend_config(self.config)
            self._cfg.flags |= N.AV_FE_PHOTOMETRIC | N.AV_FE_INPUTS_PERSIST
            N.check(N.lib().av_frontend_create(C.byref(self._cfg), 1, 0, C.byref(self._h)))
            self.max_features = N.lib().av_frontend_max_features(self._h)
            self._set_sizes(self._cfg)
            self._ids, self._uv, self._n = np.zeros((1, self.max_features), np.int64), np.zeros((1, self.max_features, 4), np.float64), np.zeros(1, np.int32)
    return Bare()


def test_a_step_before_the_tables_are_set_is_refused(photo):
    """An engine created with the flag but never given its tables (the C interface allows that; the Python constructor always sets
    them) refuses step, prestage, step_host and upload, naming the call that is missing, and works once it has them."""
    import torch
    from uav_airvision_amd import _native as N
    streams, _refs = photo
    ts, d0, d1 = streams[0].raw[0]
    eng = _engine_with_the_flag_and_no_tables()
    t0, t1 = torch.from_numpy(d0[None]).cuda(), torch.from_numpy(d1[None]).cuda()
    eng.frames_reserve(2)
    for call in (lambda: eng.step(t0, t1, [ts]), lambda: eng.prestage(t0, t1), lambda: eng.step_host(d0, d1, [ts]), lambda: eng.frames_upload([0], d0[None], d1[None])):
        with pytest.raises(N.AirvisionError, match='av_frontend_set_photometric') as e:
            call()
        assert e.value.code == N.AV_E_INVALID
    eng.set_photometric(*T.q[0], *T.q[1])
    eng.step_host(d0, d1, [ts])
    eng.read_features()
    assert np.array_equal(eng.read_image(0, 0), streams[0].frame(0).cam0_image)
    eng.close()


def test_parts_left_out_are_the_identity(photo):
    """cam0 with a response only and cam1 with a vignette only (the cameras then take a launch each), and cam0 with both and cam1 with
    nothing (cam1 passes unchanged): read_image against the definition with those tables."""
    from uav_airvision_amd.frontend import FrontendEngine
    streams, _refs = photo
    ts, d0, d1 = streams[0].raw[0]
    for mode in ('host', 'frames'):
        for kw, want in ((dict(cam0_response=T.u[0], cam1_vignette=T.v[1]), (pr.correct(d0, T.q[0][0], None), pr.correct(d1, None, T.q[1][1]))),
                         (dict(cam0_response=T.u[0], cam0_vignette=T.v[0]), (pr.correct(d0, *T.q[0]), d1))):
            eng = FrontendEngine(_cfg(**kw), n_streams=1)
            if mode == 'host':
                eng.step_host(d0, d1, [ts])
            else:
                eng.frames_reserve(2)
                eng.frames_upload([1], d0[None], d1[None])
                eng.step_frames([1], [ts])
            eng.read_features()
            assert np.array_equal(eng.read_image(0, 0), want[0]) and np.array_equal(eng.read_image(0, 1), want[1]), (mode, sorted(kw))
            eng.close()


def test_the_timing_spans_are_those_of_a_gray16_engine(photo):
    """One input-stage span per step, the stage's launches inside it: the span counts per class equal those of an engine whose input
    stage is a conversion."""
    streams, _refs = photo
    g16 = Frames.raw_twin(streams[0], lambda g: g.astype(np.uint16) << 8, lambda r: (r >> 8).astype(np.uint8), NF)
    _a, sp_16 = run_engine(_cfg(image_format='gray16'), [g16], mode='step', raw=True, timing=True)
    _b, sp_ph = run_engine(photo_cfg(), [streams[0]], mode='step', raw=True, timing=True)
    assert sp_ph == sp_16 and all(s['pyramid'] == 1 for s in sp_ph) and sum(sp_ph[-1].values()) > 10, (sp_ph, sp_16)


def test_the_drop_in_image_processor_takes_the_config_through(photo):
    from uav_airvision_amd.synth import replay
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    streams, refs = photo
    st, ref = streams[0], refs[0]
    raw = Frames(st, [with_images(st.frame(k), st.raw[k][1], st.raw[k][2]) for k in range(NF)])
    proc = ip.ImageProcessor(photo_cfg())
    seen = []
    replay(raw, [proc.imu_callback], lambda m: seen.append(proc.stereo_callback(m)))
    assert len(seen) == NF
    for k, msg in enumerate(seen):
        assert np.array_equal(np.array([f.id for f in msg.features], np.int64), ref[k]['ids']), k
        assert np.array_equal(np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features]).reshape(-1, 4).view(np.uint64), ref[k]['uv'].view(np.uint64)), k
    assert np.array_equal(proc.equalized_image(1), st.frame(NF - 1).cam1_image)
    proc.close()


# ---- off changes nothing (these two pass without the feature) ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def plain_run(bases):
    return run_engine(_cfg(), [bases[0]], mode='step', timing=True)


def test_all_four_attributes_none_is_a_plain_engine(bases, plain_run):
    off, sp_off = plain_run
    got, sp = run_engine(_cfg(**{k: None for k in ATTRS}), [bases[0]], mode='step', timing=True)
    assert all(len(a[0]) > 40 for a in off[0])
    assert all(_same(a, b) for a, b in zip(off[0], got[0])) and sp == sp_off


def test_a_config_object_without_the_attributes_is_a_plain_engine(bases, plain_run):
    off, sp_off = plain_run
    bare = bare_cfg(lambda k: k in ATTRS)
    assert not any(hasattr(bare, k) for k in ATTRS)
    for mode in ('step', 'frames'):
        got, sp = run_engine(bare, [bases[0]], mode=mode, timing=True)
        assert all(_same(a, b) for a, b in zip(off[0], got[0])), mode
        if mode == 'step':
            assert sp == sp_off
