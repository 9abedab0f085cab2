"""2 x 2 / 4 x 4 binning without a GPU: the NumPy reference on hand-written blocks, the scaled calibration as literals, the packed
configuration, av_frontend_create's refusals (before a device is touched) and the frame shapes the entry points ask for."""
import ctypes as C

import numpy as np
import pytest

import downscale_ref as dr
from fe_harness import make_cfg as _cfg
from uav_airvision_amd import _native as N
from uav_airvision_amd.config import ConfigEuRoC
from uav_airvision_amd.frontend import check_device_frames, check_host_frames, default_max_corners, downscaled_config, pack_frontend_config

pytestmark = pytest.mark.filterwarnings('ignore')


# ---- the reference itself ----

def test_reference_on_hand_written_blocks():
    # 2 x 2: block sums 0, 1, 2, 3 mod 4 round as (s + 2) >> 2: 4 -> 1, 5 -> 1, 6 -> 2, 7 -> 2; all 255 stays 255
    img = np.array([[1, 1, 1, 2, 1, 2, 2, 2, 255, 255],
                    [1, 1, 1, 1, 2, 1, 2, 1, 255, 255],
                    [0, 0, 1, 2, 250, 251, 0, 1, 7, 9],
                    [0, 0, 3, 5, 252, 253, 0, 0, 8, 10]], np.uint8)
    assert dr.downscale(img, 2).tolist() == [[1, 1, 2, 2, 255], [0, 3, 252, 0, 9]]
    # (11 + 2) >> 2 = 3: the header's example; (1006 + 2) >> 2 = 252; (1 + 2) >> 2 = 0; (34 + 2) >> 2 = 9
    # 4 x 4: sums 16 k + r round as (s + 8) >> 4: r = 7 down, r = 8 up; all 255 -> (4080 + 8) >> 4 = 255
    blocks = []
    for s in (0, 7, 8, 16 * 9 + 7, 16 * 9 + 8, 16 * 255):
        b = np.full(16, s // 16, np.int64)
        b[:s % 16] += 1
        assert b.sum() == s
        blocks.append(b.reshape(4, 4))
    img4 = np.concatenate(blocks, 1).astype(np.uint8)
    assert dr.downscale(img4, 4).tolist() == [[0, 0, 1, 9, 10, 255]]
    # sums congruent to 1, 2, 3 mod 4 through the 4 x 4 rule too: 17 -> 1, 18 -> 1, 19 -> 1, 24 -> 2
    for s, want in ((17, 1), (18, 1), (19, 1), (23, 1), (24, 2)):
        b = np.zeros(16, np.uint8); b[:s % 16] = 1; b += s // 16
        assert dr.downscale(b.reshape(4, 4), 4).tolist() == [[want]]


def test_reference_shapes_and_refusals():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (3, 8, 12), dtype=np.uint8)
    for f in dr.FACTORS:
        out = dr.downscale(a, f)
        assert out.shape == (3, 8 // f, 12 // f) and out.dtype == np.uint8
        assert np.array_equal(out[1], dr.downscale(a[1], f))
        assert out[2, 1, 2] == (int(a[2, f:2 * f, 2 * f:3 * f].astype(int).sum()) + f * f // 2) // (f * f)
    assert np.array_equal(dr.downscale(np.full((4, 4), 255, np.uint8), 4), [[255]])
    assert np.array_equal(dr.downscale(np.full((8, 8), 93, np.uint8), 2), np.full((4, 4), 93))
    for bad in (lambda: dr.downscale(a, 3), lambda: dr.downscale(a[:, :7], 2), lambda: dr.downscale(a.astype(np.uint16), 2)):
        with pytest.raises(ValueError):
            bad()


# ---- calibration ----

def test_the_scaled_calibration_as_literals():
    d2 = downscaled_config(_cfg(image_downscale=2))
    assert list(d2.cam0_intrinsics) == [229.327, 228.648, (367.215 - 0.5) / 2, (248.375 - 0.5) / 2]
    assert list(d2.cam1_intrinsics) == [457.587 / 2, 456.134 / 2, (379.999 - 0.5) / 2, (255.238 - 0.5) / 2]
    assert list(d2.cam0_resolution) == [376, 240] == list(d2.cam1_resolution) and d2.image_downscale == 1
    d4 = downscaled_config(_cfg(image_downscale=4))
    assert list(d4.cam0_intrinsics) == [458.654 / 4, 457.296 / 4, (367.215 - 1.5) / 4, (248.375 - 1.5) / 4]
    assert list(d4.cam1_intrinsics) == [457.587 / 4, 456.134 / 4, (379.999 - 1.5) / 4, (255.238 - 1.5) / 4]
    assert list(d4.cam0_resolution) == [188, 120] == list(d4.cam1_resolution) and d4.image_downscale == 1
    assert list(d4.cam0_intrinsics) == dr.scaled_intrinsics(ConfigEuRoC().cam0_intrinsics, 4)
    # everything else is the full-size camera's, and the source object is untouched
    src = _cfg(image_downscale=2)
    d = downscaled_config(src)
    assert list(src.cam0_resolution) == [752, 480] and list(src.cam0_intrinsics) == [458.654, 457.296, 367.215, 248.375] and src.image_downscale == 2
    for name in ('cam0_distortion_coeffs', 'cam1_distortion_coeffs', 'T_imu_cam0', 'T_imu_cam1'):
        assert np.array_equal(getattr(d, name), getattr(src, name))
    assert (d.fast_threshold, d.stereo_threshold, d.ransac_threshold, d.grid_row, d.grid_col, d.patch_size) == \
           (src.fast_threshold, src.stereo_threshold, src.ransac_threshold, src.grid_row, src.grid_col, src.patch_size)
    # factor 1: a plain copy
    d1 = downscaled_config(_cfg())
    assert list(d1.cam0_intrinsics) == [458.654, 457.296, 367.215, 248.375] and list(d1.cam0_resolution) == [752, 480]


def test_norm_unit_of_the_scaled_calibration_is_the_full_size_one_times_the_factor():
    """The engine multiplies norm_unit by f; the oracle computes it from the scaled intrinsics: the same bits (powers of two)."""
    for f in (2, 4):
        full = pack_frontend_config(_cfg())
        small = pack_frontend_config(downscaled_config(_cfg(image_downscale=f)))
        assert small.norm_unit == full.norm_unit * f
        assert (small.width, small.height, small.image_downscale) == (752 // f, 480 // f, 1)


# ---- packing ----

def test_config_default_and_abi_fields():
    assert ConfigEuRoC().image_downscale == 1
    names = [n for n, _t in N.FrontendConfig._fields_]
    assert names[-2:] == ['image_downscale', 'reserved1'] and C.sizeof(N.FrontendConfig) % 8 == 0
    assert 'av_downscale' in N.SIGNATURES
    assert len(N.PIXEL_FORMATS) == 14                    # binning adds no pixel format


def test_packing_carries_the_factor():
    class Bare(object):
        pass
    bare = Bare()
    for k, v in vars(ConfigEuRoC()).items():
        if k != 'image_downscale':
            setattr(bare, k, v)
    c = pack_frontend_config(bare)
    assert (c.image_downscale, c.reserved1, c.width, c.height, c.max_corners) == (1, 0, 752, 480, 8192)
    for f in (1, 2, 4):
        c = pack_frontend_config(_cfg(image_downscale=f))
        assert (c.image_downscale, c.reserved1) == (f, 0)
        assert (c.width, c.height) == (752, 480)                                   # the input size
        assert list(c.cam0_intrinsics) == [458.654, 457.296, 367.215, 248.375]     # the full-size camera
        assert c.max_corners == default_max_corners(752 // f, 480 // f) == 8192
    big = _cfg(image_downscale=2, cam0_resolution=np.array([1920, 1200]), cam1_resolution=np.array([1920, 1200]))
    assert pack_frontend_config(big).max_corners == default_max_corners(960, 600) < default_max_corners(1920, 1200)
    assert pack_frontend_config(_cfg(image_downscale=2.0)).image_downscale == 2
    assert pack_frontend_config(_cfg(image_downscale=np.int64(4))).image_downscale == 4


@pytest.mark.parametrize('bad', [3, 0.5, 8, True, 0, -2, '2', None])
def test_other_factors_are_refused(bad):
    with pytest.raises(ValueError, match='downscale'):
        pack_frontend_config(_cfg(image_downscale=bad))
    with pytest.raises(ValueError, match='downscale'):
        downscaled_config(_cfg(image_downscale=bad))


def test_a_size_the_factor_does_not_divide_is_refused():
    odd = dict(cam0_resolution=np.array([750, 480]), cam1_resolution=np.array([750, 480]))
    assert pack_frontend_config(_cfg(image_downscale=2, **odd)).image_downscale == 2
    with pytest.raises(ValueError, match='downscale'):
        pack_frontend_config(_cfg(image_downscale=4, **odd))
    with pytest.raises(ValueError, match='downscale'):
        downscaled_config(_cfg(image_downscale=4, **odd))
    with pytest.raises(ValueError, match='downscale'):
        pack_frontend_config(_cfg(image_downscale=2, cam0_resolution=np.array([752, 481]), cam1_resolution=np.array([752, 481])))


# ---- av_frontend_create, before a device is touched ----

def _create(c):
    h = C.c_void_p()
    rc = N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h))
    if rc == 0:                                          # (a machine with a GPU: the good configurations do create an engine)
        N.lib().av_frontend_destroy(h)
    return rc, N.lib().av_last_error()


def test_creation_refuses_bad_factors_without_a_device():
    for field, value in (('image_downscale', 3), ('image_downscale', 8), ('image_downscale', -1), ('reserved1', 1)):
        c = pack_frontend_config(ConfigEuRoC())
        setattr(c, field, value)
        rc, text = _create(c)
        assert rc == N.AV_E_INVALID and b'downscale' in text, (field, value, text)
    c = pack_frontend_config(ConfigEuRoC())
    c.width, c.image_downscale = 750, 4
    rc, text = _create(c)
    assert rc == N.AV_E_INVALID and b'downscale' in text and b'750' in text
    c = pack_frontend_config(ConfigEuRoC())
    c.height, c.image_downscale = 481, 2
    rc, text = _create(c)
    assert rc == N.AV_E_INVALID and b'downscale' in text
    # the binned size must pass the size rules: 752 x 480 by 4 is 188 x 120, whose fourth level is 24 x 15, not above AV_PYR_BORDER
    c = pack_frontend_config(ConfigEuRoC())
    assert c.lk_levels == 4
    c.image_downscale = 4
    rc, text = _create(c)
    assert rc == N.AV_E_INVALID and b'downscale' in text and b'188 x 120' in text


@pytest.mark.parametrize('f', [0, 1, 2, 4])
def test_a_good_configuration_gets_past_the_checks(f):
    """Without a GPU a good configuration is refused for the missing device only (with one it creates an engine)."""
    c = pack_frontend_config(ConfigEuRoC())
    c.image_downscale = f
    if f == 4:
        c.lk_levels = 3                                  # 188 x 120 holds three levels (47 x 30), not four
    rc, text = _create(c)
    assert rc in (N.AV_OK, N.AV_E_NODEVICE), text
    if N.lib().av_device_count() <= 0:
        assert rc == N.AV_E_NODEVICE and b'downscale' not in text


# ---- frame shapes ----

def test_the_entry_points_want_input_size_frames():
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    # the engine's own arithmetic of sizes, without creating one
    eng = FrontendEngine.__new__(FrontendEngine)
    eng._h = None
    cfg = pack_frontend_config(_cfg(image_downscale=2))
    FrontendEngine._set_sizes(eng, cfg)
    assert (eng.width, eng.height, eng.input_width, eng.input_height, eng.downscale) == (376, 240, 752, 480, 2)
    assert eng._frame_bytes == 752 * 480
    full = np.zeros((2, 480, 752), np.uint8)
    assert check_host_frames('x', full, eng.pixel_format, 2, eng.input_height, eng.input_width).shape == (2, 480, 752)
    with pytest.raises(ValueError, match=r'\(2, 480, 752\)'):
        check_host_frames('x', np.zeros((2, 240, 376), np.uint8), eng.pixel_format, 2, eng.input_height, eng.input_width)
    with pytest.raises(ValueError, match=r'\(2, 480, 752\)'):
        check_device_frames('x', torch.zeros((2, 240, 376), dtype=torch.uint8), eng.pixel_format, 2, eng.input_height, eng.input_width)
    cfg16 = pack_frontend_config(_cfg(image_downscale=4, image_format='bayer_rggb16'))
    FrontendEngine._set_sizes(eng, cfg16)
    assert (eng.width, eng.height, eng.input_width, eng.input_height, eng._frame_bytes) == (188, 120, 752, 480, 752 * 480 * 2)
