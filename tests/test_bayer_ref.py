"""The NumPy statement of the Bayer conversion (tests/bayer_ref.py) against the properties and the worked example of include/airvision.h,
and the host layers that list pixel formats: names, codes, bytes, configuration, frame checks, PNG staging, the sweep's arguments."""
import ctypes as C

import numpy as np
import pytest

import bayer_ref as br
from uav_airvision_amd import _native as N
from uav_airvision_amd.config import ConfigEuRoC
from uav_airvision_amd.frontend import check_device_frames, check_host_frames, pack_frontend_config


# ---- the reference itself ----

@pytest.mark.parametrize('pattern', br.PATTERNS)
def test_uniform_images_are_the_identity(pattern):
    for v in (0, 1, 77, 255):
        for (h, w) in ((2, 2), (3, 2), (5, 7), (8, 16)):
            assert (br.to_gray8(np.full((h, w), v, np.uint8), 'bayer_%s8' % pattern) == v).all(), (pattern, v, h, w)
            assert (br.to_gray8(np.full((h, w), v << 4, np.uint16), 'bayer_%s16' % pattern, 4) == v).all(), (pattern, v, h, w)


def test_the_worked_example_of_the_header():
    img = np.array([[10, 200], [30, 90]], np.uint8)
    assert br.to_gray8(img, 'bayer_rggb8').tolist() == [[81, 131], [31, 81]]
    # pixel (0, 0) by hand: R4 = 40, G4 = 200 + 200 + 30 + 30, B4 = 4 * 90
    assert 9798 * 40 + 19235 * 460 + 3735 * 360 + 65536 == 10650156 and 10650156 >> 17 == 81


def test_shifted_mosaics_are_the_neighbouring_patterns():
    """A mosaic moved by one column under rggb is the unmoved one under grbg, away from the first and last columns (where the
    reflected border differs); by one row: rggb against gbrg."""
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (21, 30), dtype=np.uint8)
    assert np.array_equal(br.to_gray8(a[:, 1:], 'bayer_rggb8')[:, 1:-1], br.to_gray8(a, 'bayer_grbg8')[:, 2:-1])
    assert np.array_equal(br.to_gray8(a[1:], 'bayer_rggb8')[1:-1], br.to_gray8(a, 'bayer_gbrg8')[2:-1])
    assert np.array_equal(br.to_gray8(a[1:, 1:], 'bayer_rggb8')[1:-1, 1:-1], br.to_gray8(a, 'bayer_bggr8')[2:-1, 2:-1])


def test_the_four_patterns_differ_and_nothing_exceeds_255():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (3, 12, 18), dtype=np.uint8)
    outs = [br.to_gray8(a, 'bayer_%s8' % p) for p in br.PATTERNS]
    assert outs[0].shape == a.shape and outs[0].dtype == np.uint8
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(outs[i], outs[j]), (i, j)
    assert (br.to_gray8(np.full((7, 9), 255, np.uint8), 'bayer_gbrg8') == 255).all()
    # 16-bit with shift 8 of v << 8 | low byte is the 8-bit result of v
    low = rng.integers(0, 256, a.shape).astype(np.uint16)
    assert np.array_equal(br.to_gray8(a.astype(np.uint16) << 8 | low, 'bayer_grbg16', 8), br.to_gray8(a, 'bayer_grbg8'))


def test_16_bit_samples_saturate_before_interpolation():
    """shift 0: a sample of 1000 counts as 255, not as 1000 averaged with its neighbours and clipped afterwards."""
    a = np.zeros((6, 6), np.uint16)
    a[2, 2] = 1000
    want = np.zeros((6, 6), np.uint8)
    want[2, 2] = 255
    assert np.array_equal(br.to_gray8(a, 'bayer_rggb16', 0), br.to_gray8(want, 'bayer_rggb8'))
    assert br.to_gray8(a, 'bayer_rggb16', 0)[2, 3] == (2 * 9798 * 255 + 65536) >> 17        # the G site right of it: R4 = 2 hs


def test_bad_arguments_raise():
    for shift in (-1, 9, 2.5):
        with pytest.raises(ValueError, match='shift'):
            br.to_gray8(np.zeros((4, 4), np.uint16), 'bayer_rggb16', shift)
    for shape in ((1, 8), (8, 1), (1, 1), (3, 1, 4)):
        with pytest.raises(ValueError, match='2 x 2'):
            br.to_gray8(np.zeros(shape, np.uint8), 'bayer_rggb8')
    for name in ('bayer', 'bayer_rggb', 'BayerBG', 'bayer_rgbg8'):
        with pytest.raises(ValueError, match='format'):
            br.to_gray8(np.zeros((4, 4), np.uint8), name)


def test_mosaic_places_the_gains_by_colour():
    g = np.full((4, 6), 100, np.uint8)
    assert br.mosaic(g, 'bayer_rggb8')[:2, :2].tolist() == [[80, 100], [100, 60]]
    assert br.mosaic(g, 'bayer_gbrg8')[:2, :2].tolist() == [[100, 60], [80, 100]]
    assert br.mosaic(g, 'bayer_bggr16', shift=4)[:2, :2].tolist() == [[60 << 4, 100 << 4], [100 << 4, 80 << 4]]


# ---- names, codes, bytes ----

def test_names_codes_and_bytes():
    assert [N.PIXEL_FORMATS[f] for f in ('gray8', 'gray16', 'rgb8', 'bgr8', 'rgba8', 'bgra8')] == [0, 1, 2, 3, 4, 5]
    assert [N.PIXEL_BYTES[c] for c in range(6)] == [1, 2, 3, 3, 4, 4]
    assert {f: N.PIXEL_FORMATS[f] for f in br.FORMATS} == br.CODES and sorted(br.CODES.values()) == list(range(16, 24))
    assert [N.PIXEL_BYTES[br.CODES[f]] for f in br.FORMATS] == [1, 1, 1, 1, 2, 2, 2, 2]
    assert all(N.PIXEL_FORMAT_NAMES[c] == f for f, c in br.CODES.items())
    assert (N.AV_PIX_BAYER_RGGB8, N.AV_PIX_BAYER_BGGR8, N.AV_PIX_BAYER_GRBG8, N.AV_PIX_BAYER_GBRG8) == (16, 17, 18, 19)
    assert (N.AV_PIX_BAYER_RGGB16, N.AV_PIX_BAYER_BGGR16, N.AV_PIX_BAYER_GRBG16, N.AV_PIX_BAYER_GBRG16) == (20, 21, 22, 23)
    assert len(N.PIXEL_FORMATS) == 14 and 'bayer' not in N.PIXEL_FORMATS
    cfg = ConfigEuRoC()
    for f, c in br.CODES.items():
        cfg.image_format, cfg.gray16_shift = f, 4
        p = pack_frontend_config(cfg)
        assert (p.pixel_format, p.gray16_shift) == (c, 4)


@pytest.mark.parametrize('code', list(range(6, 16)) + [24, 25, 255])
def test_the_codes_between_and_beyond_are_refused(code):
    cfg = ConfigEuRoC()
    cfg.image_format = code
    with pytest.raises(ValueError, match='format'):
        pack_frontend_config(cfg)
    # av_frontend_create: AV_E_INVALID with text before a device is touched (a good configuration gives AV_E_NODEVICE without a GPU)
    c = pack_frontend_config(ConfigEuRoC())
    c.pixel_format = code
    h = C.c_void_p()
    assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID
    assert b'pixel format' in N.lib().av_last_error()


def test_engine_creation_takes_the_bayer_codes_past_the_format_check():
    """A Bayer code with a bad shift is refused for the shift, not for the format: the format check knows the code."""
    for code in range(16, 24):
        c = pack_frontend_config(ConfigEuRoC())
        c.pixel_format, c.gray16_shift = code, 9
        h = C.c_void_p()
        assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID
        assert b'shift' in N.lib().av_last_error() and b'pixel format' not in N.lib().av_last_error()


# ---- host layers ----

def test_png_flavour_and_frame_arrays():
    from uav_airvision_amd.euroc import FrameStager, frame_array, png_pixel_format
    for f in br.FORMATS:
        wide = br.BYTES[f] == 2
        assert png_pixel_format(f) == ('gray16' if wide else 'gray8') == png_pixel_format(br.CODES[f])
        a = frame_array(f, 3, 4, 6)
        assert a.shape == (3, 4, 6) and a.dtype == (np.uint16 if wide else np.uint8)
        assert frame_array(br.CODES[f], 1, 4, 6, zeros=False).dtype == a.dtype
    st = FrameStager([], 4, 6, pixel_format='bayer_grbg16')
    assert st.buf[0].shape == (2, 0, 4, 6) and st.buf[0].dtype == np.uint16
    st.close()


def test_frame_checks_name_dtype_and_shape():
    import torch
    h, w = 6, 8
    assert check_host_frames('x', np.zeros((2, h, w), np.uint8), N.AV_PIX_BAYER_GRBG8, 2, h, w).shape == (2, h, w)
    assert check_host_frames('x', np.zeros((h, w), np.uint16), N.AV_PIX_BAYER_GBRG16, 1, h, w).shape == (1, h, w)
    for arr, fmt in ((np.zeros((2, h, w), np.uint16), N.AV_PIX_BAYER_RGGB8), (np.zeros((2, h, w), np.uint8), N.AV_PIX_BAYER_RGGB16),
                     (np.zeros((2, h, w, 3), np.uint8), N.AV_PIX_BAYER_BGGR8), (np.zeros((2, w, h), np.uint8), N.AV_PIX_BAYER_BGGR8),
                     (np.zeros((2, h, w), np.int16), N.AV_PIX_BAYER_GBRG16)):
        with pytest.raises(ValueError) as e:
            check_host_frames('step_host: img0', arr, fmt, 2, h, w)
        msg = str(e.value)
        assert str(arr.dtype) in msg and str(tuple(arr.shape)) in msg and 'step_host: img0' in msg and N.PIXEL_FORMAT_NAMES[fmt] in msg
    for t, fmt in ((torch.zeros((2, h, w), dtype=torch.int16), N.AV_PIX_BAYER_RGGB8), (torch.zeros((2, h, w), dtype=torch.uint8), N.AV_PIX_BAYER_RGGB16),
                   (torch.zeros((2, h, w, 3), dtype=torch.uint8), N.AV_PIX_BAYER_GRBG8)):
        with pytest.raises(ValueError) as e:
            check_device_frames('step: img1', t, fmt, 2, h, w)
        assert 'step: img1' in str(e.value) and N.PIXEL_FORMAT_NAMES[fmt] in str(e.value) and str((2, h, w)) in str(e.value)
    with pytest.raises(ValueError, match='cuda'):                                     # right dtype and shape, but host memory
        check_device_frames('step: img0', torch.zeros((2, h, w), dtype=torch.int16), N.AV_PIX_BAYER_GBRG16, 2, h, w)
    with pytest.raises(ValueError, match='cuda'):
        check_device_frames('step: img0', torch.zeros((2, h, w), dtype=torch.uint8), N.AV_PIX_BAYER_GBRG8, 2, h, w)


def test_sweep_arguments():
    from uav_airvision_amd.sweep import apply_args, batch_pixel_format, make_parser
    ap = make_parser()
    for f in br.FORMATS:
        a = ap.parse_args(['--sequences', 'X', '--pixel-format', f, '--gray16-shift', '4'])
        cfg = apply_args(ConfigEuRoC(), a)
        assert (cfg.image_format, cfg.gray16_shift) == (f, 4)
        assert pack_frontend_config(cfg).pixel_format == br.CODES[f]
        assert batch_pixel_format(['nowhere'], f) == f                # a named format is taken as given, nothing is probed
    with pytest.raises(SystemExit):
        ap.parse_args(['--sequences', 'X', '--pixel-format', 'bayer'])
    assert 'auto never chooses a Bayer format' in ' '.join(ap.format_help().split())


def test_encode_frame_matches_the_reference_mosaic():
    from uav_airvision_amd.euroc import BAYER_GAINS, bayer_site_colours, encode_frame
    rng = np.random.default_rng(3)
    g = rng.integers(0, 256, (9, 14), dtype=np.uint8)
    assert tuple(BAYER_GAINS) == br.GAINS
    for f in br.FORMATS:
        assert np.array_equal(bayer_site_colours(f, 9, 14), br.site_colours(f[6:10], 9, 14))
        assert np.array_equal(encode_frame(g, f), br.mosaic(g, f)) and encode_frame(g, f).dtype == (np.uint16 if br.BYTES[f] == 2 else np.uint8)
    assert np.array_equal(encode_frame(g, 'bayer_gbrg16', shift=4), br.mosaic(g, 'bayer_gbrg16', shift=4))
    assert np.array_equal(encode_frame(g, 'bayer_rggb8', gains=(1.0, 0.5, 0.25)), br.mosaic(g, 'bayer_rggb8', gains=(1.0, 0.5, 0.25)))
    assert (encode_frame(np.full((4, 4), 255, np.uint8), 'bayer_rggb8', gains=(2.0, 1.0, 1.0)) == 255).all()      # clipped


@pytest.mark.parametrize('fmt, shift', [('bayer_rggb8', 8), ('bayer_gbrg16', 4)])
def test_written_mosaics_decode_to_what_was_written(tmp_path, fmt, shift):
    """write_euroc_layout writes the mosaic as a grey PNG; av_png_decode (through decode_batch) returns it bit for bit."""
    from uav_airvision_amd.euroc import EuRoCDataset, decode_batch, frame_array, probe_png, write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(ConfigEuRoC(), seed=5, n_frames=2, motion_scale=1.0)
    root = write_euroc_layout(str(tmp_path / 'SEQ'), st, compress_level=1, pixel_format=fmt, gray16_shift=shift)
    files = EuRoCDataset._list_images(str(tmp_path / 'SEQ' / 'mav0' / 'cam0' / 'data'))[0]
    assert len(files) == 2 and root == str(tmp_path / 'SEQ')
    assert probe_png(files[0]) == (752, 480, 'gray16' if br.BYTES[fmt] == 2 else 'gray8')
    out = frame_array(fmt, 2, 480, 752)
    decode_batch(files, out)
    for k in range(2):
        want = br.mosaic(st.frame(k).cam0_image, fmt, shift=shift)
        assert np.array_equal(out[k], want), k
        assert not np.array_equal(br.to_gray8(want, fmt, shift), st.frame(k).cam0_image)      # the gains do colour the scene
    with pytest.raises(ValueError, match='Bayer'):
        write_euroc_layout(str(tmp_path / 'BAD'), st, pixel_format='bayer')
