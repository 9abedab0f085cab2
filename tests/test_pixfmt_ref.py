"""The pixel-format reference (tests/pixfmt_ref.py) holds the properties include/airvision.h states, and the Python surface reads the
two config attributes and checks its arguments without a device.  No GPU needed."""
import numpy as np
import pytest

import pixfmt_ref as pr
from uav_airvision_amd import _native as N
from uav_airvision_amd.config import ConfigEuRoC
from uav_airvision_amd.frontend import check_device_frames, check_host_frames, pack_frontend_config


def test_equal_channels_map_to_themselves():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for fmt in ('rgb8', 'bgr8', 'rgba8', 'bgra8'):
        img = np.repeat(g[..., None], pr.BYTES[fmt], -1)
        assert np.array_equal(pr.to_gray8(img, fmt), g), fmt
    assert 9798 + 19235 + 3735 == 1 << 15
    assert int(pr.to_gray8(np.full((1, 1, 3), 255, np.uint8), 'rgb8')[0, 0]) == 255


def test_gray16_high_byte_and_truncation():
    g, low = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    v = (g << 8 | low).astype(np.uint16)
    assert np.array_equal(pr.to_gray8(v, 'gray16'), g.astype(np.uint8))              # (g << 8 | low) >> 8 == g: truncates, never rounds
    assert np.array_equal(pr.to_gray8(v, 'gray16', 8), pr.to_gray8(v, 'gray16'))       # 8 is the default


def test_gray16_saturates_at_small_shifts():
    v = np.array([[0, 1, 255, 256, 4095, 4096, 65535]], np.uint16)
    assert pr.to_gray8(v, 'gray16', 0).tolist() == [[0, 1, 255, 255, 255, 255, 255]]
    assert pr.to_gray8(v, 'gray16', 4).tolist() == [[0, 0, 15, 16, 255, 255, 255]]
    assert pr.to_gray8(v, 'gray16', 8).tolist() == [[0, 0, 0, 1, 15, 16, 255]]


def test_alpha_is_ignored_and_bgr_is_rgb_swapped():
    rng = np.random.default_rng(5)
    rgb = pr.random_frames(rng, 'rgb8', (9, 13))
    want = pr.to_gray8(rgb, 'rgb8')
    assert np.array_equal(pr.to_gray8(rgb[..., ::-1], 'bgr8'), want)
    for alpha in (0, 77, 255):
        a = np.full(rgb.shape[:-1] + (1,), alpha, np.uint8)
        assert np.array_equal(pr.to_gray8(np.concatenate([rgb, a], -1), 'rgba8'), want)
        assert np.array_equal(pr.to_gray8(np.concatenate([rgb[..., ::-1], a], -1), 'bgra8'), want)
    px = np.array([[[200, 10, 30]]], np.uint8)                                         # by hand: (9798*200 + 19235*10 + 3735*30 + 16384) >> 15
    assert int(pr.to_gray8(px, 'rgb8')[0, 0]) == (9798 * 200 + 19235 * 10 + 3735 * 30 + 16384) >> 15 == 69
    assert pr.to_gray8(px, 'rgb8')[0, 0] != pr.to_gray8(px, 'bgr8')[0, 0]
    g = rng.integers(0, 256, (4, 4), dtype=np.uint8)
    assert np.array_equal(pr.to_gray8(g, 'gray8'), g)


def test_reference_refuses_bad_arguments():
    with pytest.raises(ValueError):
        pr.to_gray8(np.zeros((2, 2), np.uint8), 'yuv')
    with pytest.raises(ValueError):
        pr.to_gray8(np.zeros((2, 2), np.uint16), 'gray16', 9)


def test_config_defaults_and_stripped_config():
    cfg = ConfigEuRoC()
    assert cfg.image_format == 'gray8' and cfg.gray16_shift == 8
    c = pack_frontend_config(cfg)
    assert (c.pixel_format, c.gray16_shift, c.reserved0) == (N.AV_PIX_GRAY8, 8, 0)
    bare = ConfigEuRoC()
    del bare.image_format, bare.gray16_shift
    c = pack_frontend_config(bare)
    assert (c.pixel_format, c.gray16_shift) == (0, 8)
    for name, code in N.PIXEL_FORMATS.items():
        cfg.image_format = name
        assert pack_frontend_config(cfg).pixel_format == code
    cfg.image_format, cfg.gray16_shift = 'gray16', 4
    c = pack_frontend_config(cfg)
    assert (c.pixel_format, c.gray16_shift) == (N.AV_PIX_GRAY16, 4)
    assert [N.PIXEL_BYTES[N.PIXEL_FORMATS[f]] for f in pr.FORMATS] == [pr.BYTES[f] for f in pr.FORMATS]
    assert [N.PIXEL_FORMATS[f] for f in pr.FORMATS] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize('attr, value', [('image_format', 'yuv'), ('image_format', 'GRAY8'), ('image_format', 6), ('image_format', None),
                                         ('gray16_shift', 9), ('gray16_shift', -1), ('gray16_shift', 2.5)])
def test_bad_format_or_shift_raises(attr, value):
    cfg = ConfigEuRoC()
    setattr(cfg, attr, value)
    with pytest.raises(ValueError, match='format|shift'):
        pack_frontend_config(cfg)


def test_engine_creation_refuses_a_bad_format_before_a_device_is_touched():
    """av_frontend_create on a machine without a GPU reports AV_E_NODEVICE for a good configuration; a bad format or shift is
    AV_E_INVALID with text either way, so the check comes first."""
    import ctypes as C
    for field, value, text in (('pixel_format', 6, b'pixel format'), ('pixel_format', -1, b'pixel format'), ('gray16_shift', 9, b'shift')):
        c = pack_frontend_config(ConfigEuRoC())
        setattr(c, field, value)
        h = C.c_void_p()
        assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID
        assert text in N.lib().av_last_error()


def test_host_frame_checks_name_dtype_and_shape():
    h, w = 6, 8
    ok16 = np.zeros((2, h, w), np.uint16)
    assert check_host_frames('x', ok16, N.AV_PIX_GRAY16, 2, h, w).shape == (2, h, w)
    assert check_host_frames('x', np.zeros((h, w, 3), np.uint8), N.AV_PIX_BGR8, 1, h, w).shape == (1, h, w, 3)
    assert check_host_frames('x', np.zeros((h, w), np.uint16), N.AV_PIX_GRAY16, 1, h, w).shape == (1, h, w)
    for arr, fmt in ((np.zeros((2, h, w), np.uint8), N.AV_PIX_GRAY16), (np.zeros((2, h, w), np.int16), N.AV_PIX_GRAY16),
                     (np.zeros((2, h, w, 4), np.uint8), N.AV_PIX_RGB8), (np.zeros((2, h, w, 3), np.uint8), N.AV_PIX_RGBA8),
                     (np.zeros((2, h, w), np.uint8), N.AV_PIX_BGR8), (np.zeros((2, w, h, 3), np.uint8), N.AV_PIX_BGR8),
                     (np.zeros((2, h, w, 3), np.float32), N.AV_PIX_RGB8), (np.zeros((3, h, w), np.uint16), N.AV_PIX_GRAY16)):
        with pytest.raises(ValueError) as e:
            check_host_frames('step_host: img0', arr, fmt, 2, h, w)
        assert str(arr.dtype) in str(e.value) and str(tuple(arr.shape)) in str(e.value) and 'step_host: img0' in str(e.value)
    # a non-contiguous view is copied, never reinterpreted
    big = np.arange(2 * h * w * 2, dtype=np.uint16).reshape(2, h, 2 * w)
    got = check_host_frames('x', big[:, :, ::2], N.AV_PIX_GRAY16, 2, h, w)
    assert got.flags['C_CONTIGUOUS'] and np.array_equal(got, big[:, :, ::2])


def test_device_frame_checks_name_dtype_and_shape():
    import torch
    h, w = 6, 8
    for t, fmt in ((torch.zeros((2, h, w), dtype=torch.uint8), N.AV_PIX_GRAY16), (torch.zeros((2, h, w), dtype=torch.int32), N.AV_PIX_GRAY16),
                   (torch.zeros((2, h, w), dtype=torch.uint8), N.AV_PIX_RGB8), (torch.zeros((2, h, w, 3), dtype=torch.uint8), N.AV_PIX_BGRA8),
                   (np.zeros((2, h, w, 3), np.uint8), N.AV_PIX_RGB8)):
        with pytest.raises(ValueError) as e:
            check_device_frames('step: img1', t, fmt, 2, h, w)
        assert 'step: img1' in str(e.value) and str((2, h, w)) [:-1] in str(e.value)
    with pytest.raises(ValueError, match='cuda'):                                     # right dtype and shape, but host memory
        check_device_frames('step: img0', torch.zeros((2, h, w), dtype=torch.int16), N.AV_PIX_GRAY16, 2, h, w)


def test_decode_batch_refuses_arrays_of_no_png_flavour(tmp_path):
    from uav_airvision_amd.euroc import decode_batch, frame_array
    for out in (np.zeros((1, 4, 4), np.int16), np.zeros((1, 4, 4, 2), np.uint8), np.zeros((1, 4, 4, 3), np.uint16), np.zeros((4, 4), np.uint16)):
        with pytest.raises(ValueError, match='uint16'):
            decode_batch(['nowhere.png'], out)
    with pytest.raises(ValueError, match='contiguous'):
        decode_batch(['nowhere.png'], np.zeros((1, 4, 8), np.uint16)[:, :, ::2])
    assert frame_array('gray16', 2, 3, 4).dtype == np.uint16 and frame_array('rgba8', 2, 3, 4).shape == (2, 3, 4, 4)
    assert frame_array('gray8', 2, 3, 4).shape == (2, 3, 4) and frame_array(N.AV_PIX_RGB8, 1, 3, 4).shape == (1, 3, 4, 3)
    with pytest.raises(ValueError):
        frame_array('bayer', 1, 3, 4)


def test_png_staging_refuses_bgr_orders():
    """PNG files are in RGB order: the stagers refuse 'bgr8' / 'bgra8' instead of handing RGB bytes to an engine that reads BGR."""
    from uav_airvision_amd.euroc import FrameStager, SharedFrameStager, png_pixel_format
    assert [png_pixel_format(f) for f in ('gray8', 'gray16', 'rgb8', 'rgba8', N.AV_PIX_RGB8)] == ['gray8', 'gray16', 'rgb8', 'rgba8', 'rgb8']
    for fmt in ('bgr8', 'bgra8', N.AV_PIX_BGR8):
        with pytest.raises(ValueError, match='RGB order'):
            png_pixel_format(fmt)
        with pytest.raises(ValueError, match='RGB order'):
            FrameStager([], 4, 4, pixel_format=fmt)
        with pytest.raises(ValueError, match='RGB order'):
            SharedFrameStager(None, 4, 4, pixel_format=fmt)


def test_sweep_arguments():
    from uav_airvision_amd.sweep import apply_args, make_parser
    ap = make_parser()
    a = ap.parse_args(['--sequences', 'X'])
    cfg = apply_args(ConfigEuRoC(), a)
    assert a.pixel_format == 'gray8' and (cfg.image_format, cfg.gray16_shift) == ('gray8', 8)
    a = ap.parse_args(['--sequences', 'X', '--pixel-format', 'gray16', '--gray16-shift', '4'])
    cfg = apply_args(ConfigEuRoC(), a)
    assert (cfg.image_format, cfg.gray16_shift) == ('gray16', 4)
    a = ap.parse_args(['--sequences', 'X', '--pixel-format', 'auto'])
    assert apply_args(ConfigEuRoC(), a).image_format == 'gray8'                      # auto: decided per batch from the files
