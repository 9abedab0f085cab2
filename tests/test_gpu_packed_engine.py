"""The front-end engine fed packed 10 / 12-bit frames (config.image_format = 'gray12p', 'bayer_rggb12p', ..) against the unmodified CPU
oracle front-end fed the frames the NumPy reference of tests/packed_ref.py converted, in every entry path; packed mosaics through both
scratches with binning and CLAHE; placement in a batch; off is off; the drop-in ImageProcessor."""
import os
import sys

import numpy as np
import pytest

import bayer_ref as br
import clahe_ref as cr
import packed_ref as kr
from conftest import ROOT
from downscale_helpers import FLOOR, binned_stream
from fe_harness import MODES, Frames, against_oracle, bare_cfg, make_cfg as _cfg, run_engine, run_oracle, same as _same, with_images

pytestmark = pytest.mark.gpu

NF = 8
STREAM = dict(seed=17, n_frames=NF, motion_scale=2.0)


def packed_stream(base, fmt, n_frames, seed=5, post=None):
    """The first n frames of `base` as packed frames of `fmt` (`.raw`) and their reference conversion (`.frame`).  A grey value g -- for
    a mosaic format the site value of bayer_ref.mosaic(g) -- becomes the sample (g << (d - 8)) | random low bits, packed by the package's
    own pack_frames; the conversion is tests/packed_ref.py's, at the default shift 8."""
    from uav_airvision_amd.frontend import pack_frames
    rng = np.random.default_rng(seed)
    d = kr.depth(fmt)

    def encode(g):
        m = br.mosaic(g, 'bayer_%s8' % fmt[6:10]) if fmt in kr.BAYER else g
        return pack_frames((m.astype(np.uint16) << (d - 8)) | rng.integers(0, 1 << (d - 8), m.shape, dtype=np.uint16), fmt)
    return Frames.raw_twin(base, encode, lambda r: kr.to_gray8(r, fmt), n_frames, post)


@pytest.fixture(scope='module')
def base():
    from uav_airvision_amd.synth import SyntheticStream
    return SyntheticStream(_cfg(), **STREAM)


@pytest.fixture(scope='module')
def grey_ref(base):
    """The grey packings convert back to the stream's own frames (the low bits fall off at shift 8): one oracle run serves them all."""
    return run_oracle(_cfg(), Frames.cached(base, NF))


@pytest.fixture(scope='module')
def packed(base, grey_ref):
    """Per format: the packed stream and the oracle's output on its reference-converted frames (computed once, shared, never changed)."""
    out = {}
    for fmt in ('gray12p', 'gray10_csi2', 'bayer_rggb12p'):
        st = packed_stream(base, fmt, NF)
        out[fmt] = (st, grey_ref if fmt in kr.GREY else run_oracle(_cfg(), st))
    return out


def _against_oracle(fmt, mode, st, ref, **cfg_kw):
    got, images = run_engine(_cfg(image_format=fmt, **cfg_kw), [st], mode=mode, raw=True, images_of=0)
    assert len(ref) == NF
    against_oracle(ref, got[0], '%s %s' % (fmt, mode), images, st, min_features=41)      # read_image: the converted frames; the scene has features


def test_the_packed_streams_are_what_they_claim(packed, base):
    """uint8 rows of w d / 8 bytes; the low bits are used; the grey packings convert back to the stream's frames; the mosaic does not."""
    st = packed['gray12p'][0]
    raw = st.raw[0][1]
    assert raw.dtype == np.uint8 and raw.shape == (480, 752 * 3 // 2)
    assert (kr.unpack(raw, 'gray12p') & 15).any() and np.array_equal(st.frame(0).cam0_image, base.frame(0).cam0_image)
    assert packed['gray10_csi2'][0].raw[0][1].shape == (480, 752 * 5 // 4)
    assert np.array_equal(packed['gray10_csi2'][0].frame(3).cam1_image, base.frame(3).cam1_image)
    assert np.abs(packed['bayer_rggb12p'][0].frame(0).cam0_image.astype(int) - base.frame(0).cam0_image.astype(int)).mean() > 5


@pytest.mark.parametrize('mode', MODES)
def test_gray12p_matches_the_oracle_in_every_entry_path(packed, mode):
    """ids, uv bits, the tracker's stage counters and n_published on every frame; read_image returns exactly the reference-converted
    frames; the caller's arrays and tensors are unchanged (asserted inside run_engine)."""
    _against_oracle('gray12p', mode, *packed['gray12p'])


@pytest.mark.parametrize('mode', ['step', 'frames'])
def test_gray10_csi2_matches_the_oracle(packed, mode):
    _against_oracle('gray10_csi2', mode, *packed['gray10_csi2'])


@pytest.mark.parametrize('mode', ['step', 'prestage', 'host', 'frames'])
def test_bayer_rggb12p_matches_the_oracle(packed, mode):
    """Two passes: the reduced mosaic into the engine's scratch (the frame store's own in `frames`), the 8-bit demosaic from there.
    `prestage`: the next frame's conversion is enqueued behind the step on the same stream, through the same scratch."""
    _against_oracle('bayer_rggb12p', mode, *packed['bayer_rggb12p'])


def test_bayer_grbg10p_with_binning_and_clahe_in_the_host_path(base):
    """Both scratches: raw -> mosaic scratch -> full-size grey -> binned level 0, equalised in place: against the oracle on
    clahe_ref.clahe(downscale_ref.downscale(packed_ref.to_gray8(raw)))."""
    from uav_airvision_amd.frontend import downscaled_config
    fmt = 'bayer_grbg10p'
    st = packed_stream(base, fmt, NF)
    binned = binned_stream(st, 2, post=lambda a: cr.clahe(a, 2.0, (8, 8)))
    ref = run_oracle(downscaled_config(_cfg(image_downscale=2)), binned)
    got, images = run_engine(_cfg(image_format=fmt, image_downscale=2, use_clahe=True), [st], mode='host', raw=True, images_of=0)
    against_oracle(ref, got[0], fmt + ' f2 clahe host', images, binned, **FLOOR)


def test_a_stream_gives_the_same_result_anywhere_in_a_batch():
    """Two streams of different content in one batch, in the device path and through the frame store (entries out of order): each
    publishes what it publishes alone."""
    from uav_airvision_amd.synth import SyntheticStream
    fmt = 'gray10p'
    cfg = _cfg(image_format=fmt)
    batch = [packed_stream(SyntheticStream(cfg, seed=200 + i, n_frames=NF, motion_scale=1.0 + 0.3 * i), fmt, NF, seed=9 + i) for i in range(2)]
    assert not np.array_equal(batch[0].raw[0][1], batch[1].raw[0][1])
    alone = [run_engine(cfg, [b], raw=True)[0] for b in batch]
    assert all(len(a[0]) > 20 for al in alone for a in al)
    assert not all(_same(a, b) for a, b in zip(alone[0], alone[1]))
    for mode in ('step', 'frames'):
        got = run_engine(cfg, batch, mode=mode, raw=True)
        for pos in range(2):
            assert all(_same(a, b) for a, b in zip(alone[pos], got[pos])), (mode, pos)


def test_an_entry_named_twice_takes_the_later_frame(packed):
    """One upload that names an entry twice: the unpacking of a grey format writes the store through the list whose entry for the
    earlier frame is negative, so the later frame wins, as with the other conversions (tests/test_gpu_pixfmt_engine.py)."""
    from uav_airvision_amd.frontend import FrontendEngine
    st = packed['gray12p'][0]
    eng = FrontendEngine(_cfg(image_format='gray12p'), n_streams=1)
    eng.frames_reserve(4)
    t, a0, a1 = st.raw[0]
    _t, b0, b1 = st.raw[1]
    eng.frames_upload(np.array([2, 2], np.int32), np.stack([b0, a0]), np.stack([b1, a1]))
    eng.step_frames([2], [t])
    eng.read_features()
    assert np.array_equal(eng.read_image(0, 0), st.frame(0).cam0_image) and np.array_equal(eng.read_image(0, 1), st.frame(0).cam1_image)
    assert not np.array_equal(st.frame(0).cam0_image, st.frame(1).cam0_image)
    eng.close()


def test_gray8_is_what_it_was(base, packed):
    """image_format = 'gray8' equals a bare config without the two attributes, outputs and timing span counts per step; a packed format
    -- grey, or a mosaic with its two passes -- adds no span to a step (the conversion counts inside the input stage's)."""
    bare = bare_cfg(lambda k: k in ('image_format', 'gray16_shift'))
    st = Frames.cached(base)
    off, sp_off = run_engine(_cfg(image_format='gray8'), [st], n_frames=NF, timing=True)
    none, sp_none = run_engine(bare, [st], n_frames=NF, timing=True)
    assert all(len(a[0]) > 40 for a in off[0])
    assert all(_same(a, b) for a, b in zip(off[0], none[0])) and sp_off == sp_none
    for fmt in ('gray12p', 'bayer_rggb12p'):
        on, sp_on = run_engine(_cfg(image_format=fmt), [packed[fmt][0]], mode='step', raw=True, timing=True)
        assert sp_on == sp_off and all(s['pyramid'] == 1 for s in sp_on), fmt
        if fmt == 'gray12p':                                       # the same frames after conversion: the same message
            assert all(_same(a, b) for a, b in zip(off[0], on[0]))


def test_the_drop_in_image_processor_takes_packed_frames(base, packed):
    """The drop-in pipeline hands the packed arrays through as they are: its messages are the engine's, and its image read-back is the
    converted frame."""
    from uav_airvision_amd.synth import replay
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    fmt = 'gray12p'
    st, ref = packed[fmt]
    n = 4
    raw = Frames(st, [with_images(st.frame(k), st.raw[k][1], st.raw[k][2]) for k in range(n)])
    proc = ip.ImageProcessor(_cfg(image_format=fmt))
    seen = []
    replay(raw, [proc.imu_callback], lambda m: seen.append(proc.stereo_callback(m)))
    assert len(seen) == n
    for k, msg in enumerate(seen):
        assert np.array_equal(np.array([f.id for f in msg.features], np.int64), ref[k]['ids']), k
        assert np.array_equal(np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features]).reshape(-1, 4).view(np.uint64), ref[k]['uv'].view(np.uint64)), k
    assert np.array_equal(proc.equalized_image(0), st.frame(n - 1).cam0_image)
    with pytest.raises(ValueError, match=r'gray12p.*uint8'):
        proc.stereo_callback(st.frame(0))                          # an unpacked frame where a packed one is wanted: refused by name
    proc.close()


def test_wrong_frames_are_refused_by_name(base):
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    eng = FrontendEngine(_cfg(image_format='gray12p'), n_streams=1)
    assert eng._frame_bytes == 752 * 480 * 3 // 2
    m = base.frame(0)
    with pytest.raises(ValueError, match=r'gray12p.*\(1, 480, 1128\).*\(480, 752\)'):
        eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
    with pytest.raises(ValueError, match='gray12p'):
        eng.step(torch.zeros((1, 480, 752), dtype=torch.uint8, device='cuda'), torch.zeros((1, 480, 752), dtype=torch.uint8, device='cuda'), [0.0])
    with pytest.raises(ValueError, match='gray12p'):
        eng.frames_upload([0], np.zeros((1, 480, 1128), np.uint16), np.zeros((1, 480, 1128), np.uint16))
    eng.close()
