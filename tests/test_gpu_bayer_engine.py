"""The front-end engine fed raw Bayer mosaics (config.image_format = 'bayer_*') against the unmodified CPU oracle front-end fed the
frames the NumPy reference of tests/bayer_ref.py converted, in every entry path; with CLAHE; placement in a batch; off is off."""
import numpy as np
import pytest

import bayer_ref as br
import clahe_ref as cr
from bayer_helpers import mosaicked_stream
from fe_harness import MODES, Frames, against_oracle, bare_cfg, make_cfg as _cfg, run_engine, run_oracle, same as _same

pytestmark = pytest.mark.gpu

NF = 8
STREAM = dict(seed=17, n_frames=NF, motion_scale=2.0)
SHIFTS = {'bayer_rggb8': 8, 'bayer_gbrg16': 4, 'bayer_bggr8': 8}


@pytest.fixture(scope='module')
def base():
    from uav_airvision_amd.synth import SyntheticStream
    return SyntheticStream(_cfg(), **STREAM)


@pytest.fixture(scope='module')
def mosaicked(base):
    """Per format: the raw stream and the oracle's output on its reference-converted frames (computed once, shared, never changed)."""
    out = {}
    for fmt, shift in SHIFTS.items():
        st = mosaicked_stream(base, fmt, NF, shift=shift)
        out[fmt] = (st, run_oracle(_cfg(), st))
    return out


def _against_oracle(fmt, mode, st, ref, **cfg_kw):
    got, images = run_engine(_cfg(image_format=fmt, gray16_shift=SHIFTS[fmt], **cfg_kw), [st], mode=mode, raw=True, images_of=0)
    assert len(ref) == NF
    against_oracle(ref, got[0], '%s %s' % (fmt, mode), images, st, min_features=41)      # read_image: the converted frames; the scene has features


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('fmt', ['bayer_rggb8', 'bayer_gbrg16'])
def test_engine_matches_the_oracle_on_converted_frames(mosaicked, fmt, mode):
    """ids, uv bits, the tracker's stage counters and n_published on every frame; read_image returns exactly the reference-converted
    frames; the caller's arrays and tensors are unchanged (asserted inside run_engine)."""
    _against_oracle(fmt, mode, *mosaicked[fmt])


@pytest.mark.parametrize('mode', ['step', 'frames'])
def test_a_third_pattern_matches_the_oracle(mosaicked, mode):
    _against_oracle('bayer_bggr8', mode, *mosaicked['bayer_bggr8'])


def test_the_mosaics_are_not_trivially_grey(mosaicked, base):
    """The gains colour the scene: neighbouring sites differ by the gain ratio, the converted frames differ from the stream's own grey
    frames by several grey levels on average, and the 16-bit samples use shift 4."""
    st = mosaicked['bayer_rggb8'][0]
    g = base.frame(0).cam0_image.astype(int)
    assert np.abs(st.frame(0).cam0_image.astype(int) - g).mean() > 5
    raw = st.raw[0][1].astype(int)
    assert abs(raw[0::2, 0::2].mean() / max(1.0, raw[1::2, 1::2].mean()) - 0.8 / 0.6) < 0.1
    st16 = mosaicked['bayer_gbrg16'][0]
    assert st16.raw[0][1].dtype == np.uint16 and int(st16.raw[0][1].max()) <= 255 << 4 and int(st16.raw[0][1].max()) > 255


def test_with_clahe_in_the_host_path(base):
    """Demosaicing, then equalisation in place: against the oracle on clahe_ref.clahe(bayer_ref(...))."""
    st = mosaicked_stream(base, 'bayer_rggb8', NF, post=lambda a: cr.clahe(a, 2.0, (8, 8)))
    _against_oracle('bayer_rggb8', 'host', st, run_oracle(_cfg(), st), use_clahe=True)


def test_a_stream_gives_the_same_result_anywhere_in_a_batch():
    """Two streams of different content in one batch, in the device path and through the frame store (entries out of order): each
    publishes what it publishes alone."""
    from uav_airvision_amd.synth import SyntheticStream
    fmt = 'bayer_grbg8'
    cfg = _cfg(image_format=fmt)
    batch = [mosaicked_stream(SyntheticStream(cfg, seed=200 + i, n_frames=NF, motion_scale=1.0 + 0.3 * i), fmt, NF) for i in range(2)]
    assert not np.array_equal(batch[0].raw[0][1], batch[1].raw[0][1])
    alone = [run_engine(cfg, [b], raw=True)[0] for b in batch]
    assert all(len(a[0]) > 20 for al in alone for a in al)
    assert not all(_same(a, b) for a, b in zip(alone[0], alone[1]))
    for mode in ('step', 'frames'):
        got = run_engine(cfg, batch, mode=mode, raw=True)
        for pos in range(2):
            assert all(_same(a, b) for a, b in zip(alone[pos], got[pos])), (mode, pos)


def test_an_entry_named_twice_takes_the_later_frame(mosaicked):
    """One upload that names an entry twice: the demosaic writes the store through the list whose entry for the earlier frame is
    negative, so the later frame wins, as with the other conversions (tests/test_gpu_pixfmt_engine.py)."""
    from uav_airvision_amd.frontend import FrontendEngine
    fmt = 'bayer_gbrg16'
    st = mosaicked[fmt][0]
    eng = FrontendEngine(_cfg(image_format=fmt, gray16_shift=SHIFTS[fmt]), n_streams=1)
    eng.frames_reserve(4)
    t, a0, a1 = st.raw[0]
    _t, b0, b1 = st.raw[1]
    eng.frames_upload(np.array([2, 2], np.int32), np.stack([b0, a0]), np.stack([b1, a1]))
    eng.step_frames([2], [t])
    eng.read_features()
    assert np.array_equal(eng.read_image(0, 0), st.frame(0).cam0_image) and np.array_equal(eng.read_image(0, 1), st.frame(0).cam1_image)
    assert not np.array_equal(st.frame(0).cam0_image, st.frame(1).cam0_image)
    eng.close()


def test_gray8_is_what_it_was(base):
    """image_format = 'gray8' equals a bare config without the two attributes, outputs and timing span counts per step; a Bayer format
    adds no span to a step (the conversion counts inside the input stage's)."""
    bare = bare_cfg(lambda k: k in ('image_format', 'gray16_shift'))
    st = Frames.cached(base)
    off, sp_off = run_engine(_cfg(image_format='gray8'), [st], n_frames=NF, timing=True)
    none, sp_none = run_engine(bare, [st], n_frames=NF, timing=True)
    assert all(len(a[0]) > 40 for a in off[0])
    assert all(_same(a, b) for a, b in zip(off[0], none[0])) and sp_off == sp_none
    on, sp_on = run_engine(_cfg(image_format='bayer_rggb8'), [mosaicked_stream(base, 'bayer_rggb8', NF)], mode='step', raw=True, timing=True)
    assert sp_on == sp_off and all(s['pyramid'] == 1 for s in sp_on)


def test_wrong_frames_are_refused_by_name(base):
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    eng = FrontendEngine(_cfg(image_format='bayer_gbrg16', gray16_shift=4), n_streams=1)
    m = base.frame(0)
    with pytest.raises(ValueError, match=r'bayer_gbrg16.*uint16'):
        eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
    with pytest.raises(ValueError, match='uint16'):
        eng.step(torch.zeros((1, 480, 752), dtype=torch.uint8, device='cuda'), torch.zeros((1, 480, 752), dtype=torch.uint8, device='cuda'), [0.0])
    eng.close()
    eng = FrontendEngine(_cfg(image_format='bayer_rggb8'), n_streams=1)
    with pytest.raises(ValueError, match=r'bayer_rggb8.*uint8'):
        eng.frames_upload([0], np.zeros((1, 480, 752, 3), np.uint8), np.zeros((1, 480, 752, 3), np.uint8))
    eng.close()
