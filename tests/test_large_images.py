"""Images above 2^19 pixels, the part that needs no GPU: the engine's own size limit, the two keypoint word formats, the synthetic
streams at another resolution."""
import ctypes
import hashlib

import numpy as np
import pytest


def test_frontend_create_refuses_an_image_above_the_limit_itself():
    """4097 x 4096 is one row of pixels too many: av_frontend_create answers AV_E_INVALID before it looks for a device, and the text
    names the engine and the limit."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import pack_frontend_config
    cfg = ConfigEuRoC()
    cfg.cam0_resolution = cfg.cam1_resolution = np.array([4097, 4096])
    c = pack_frontend_config(cfg)
    h = ctypes.c_void_p()
    assert N.lib().av_frontend_create(ctypes.byref(c), 1, 0, ctypes.byref(h)) == N.AV_E_INVALID
    text = N.lib().av_last_error().decode()
    assert 'av_frontend_create' in text and 'AV_MAX_IMAGE_PIXELS' in text and str(1 << 24) in text and '4097 x 4096' in text
    assert not h.value
    assert N.AV_MAX_IMAGE_PIXELS == 1 << 24


@pytest.mark.parametrize('bits,w,h', [(19, 1024, 512), (19, 752, 480), (24, 4096, 4096), (24, 832, 640), (24, 1280, 720)])
def test_keypoint_words_of_both_formats_round_trip(bits, w, h):
    """Planted (x, y, score) triples -> words -> triples, in raster order; the first and the last raster of the image, the highest
    score a FAST corner can have (254) and the lowest (0) among them.  At 4096 x 4096 the last raster is 2^24 - 1."""
    from uav_airvision_amd import ops
    assert ops.kp_raster_bits(w, h) == bits
    rng = np.random.default_rng(bits * 1000 + w)
    raster = np.unique(np.concatenate([[0, 1, w - 1, w, w * h - w, w * h - 2, w * h - 1], rng.integers(0, w * h, 500)]))
    score = rng.integers(0, 255, len(raster))
    score[[0, -1]] = 254, 254
    score[[1, -2]] = 0, 0
    x, y = raster % w, raster // w
    words = ops.pack_keypoints(x, y, score, w, bits)
    assert words.dtype == np.uint32 and len(np.unique(words)) == len(words)
    assert words.max() < 0xFFFFFFFF and words[-1] == np.uint32(254 << bits | ((1 << bits) - 1 - (w * h - 1)))
    if w * h == 1 << bits:
        assert words[-1] == np.uint32(254 << bits) and words[-2] == 1           # the last raster leaves the low bits empty
    shuffled = words[rng.permutation(len(words))]
    gx, gy, gs = ops.unpack_keypoints(shuffled, w, bits)
    assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gs, score)
    # the order of the words is (score, then raster descending) in either format
    order = np.argsort(words.astype(np.int64), kind='stable')[::-1]
    key = list(zip((-score[order]).tolist(), raster[order].tolist()))
    assert key == sorted(key)


def test_keypoint_words_refuse_what_the_format_cannot_hold():
    from uav_airvision_amd import ops
    with pytest.raises(ValueError):
        ops.pack_keypoints([0], [512], [10], 1024, 19)          # raster 2^19
    with pytest.raises(ValueError):
        ops.pack_keypoints([0], [0], [256], 4096, 24)           # a score that would spill out of 32 bits
    with pytest.raises(ValueError):
        ops.kp_raster_bits(4097, 4096)
    assert ops.kp_raster_bits(1024, 512) == 19 and ops.kp_raster_bits(1025, 512) == 24


def test_default_max_corners_grows_with_the_image():
    from uav_airvision_amd.frontend import default_max_corners
    assert default_max_corners(752, 480) == 8192 and default_max_corners(640, 480) == 8192
    assert default_max_corners(1504, 960) == 4 * 8192
    assert default_max_corners(1920, 1200) >= 8192 * 1920 * 1200 // (752 * 480)


def test_synthetic_stream_renders_at_the_configs_resolution_and_is_unchanged_at_the_default():
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream, make_texture, scaled_config
    tex = make_texture(0xA1B0 + 7)
    # the default size: the bytes the renderer gave before it took a size (sha-256 of frame 1, both cameras, of seed 7)
    st = SyntheticStream(ConfigEuRoC(), seed=7, n_frames=2, motion_scale=1.5, texture=tex)
    m = st.frame(1)
    assert m.cam0_image.shape == m.cam1_image.shape == (480, 752) and (st.width, st.height) == (752, 480)
    assert hashlib.sha256(m.cam0_image.tobytes() + m.cam1_image.tobytes()).hexdigest() == \
        '20ea9f9082de7d4131f6b2650ce96f2ebcd6207ffa83ccbc859939b2ff6a5780'
    # 1280 x 720 from a scaled config
    cfg = scaled_config(ConfigEuRoC(), 1280, 720)
    assert list(cfg.cam0_resolution) == [1280, 720] == list(cfg.cam1_resolution)
    assert np.allclose(cfg.cam0_intrinsics, [458.654 * 1280 / 752, 457.296 * 720 / 480, 367.215 * 1280 / 752, 248.375 * 720 / 480])
    big = SyntheticStream(cfg, seed=7, n_frames=2, motion_scale=1.5, texture=tex)
    b = big.frame(1)
    assert b.cam0_image.shape == b.cam1_image.shape == (720, 1280) and b.cam0_image.dtype == np.uint8
    assert b.cam0_image.std() > 10 and not np.array_equal(b.cam0_image, b.cam1_image)
    # the same scene through scaled intrinsics: the centre of the large image shows what the centre of the small one shows
    c_small = m.cam0_image[200:280, 336:416].astype(np.float64).mean()
    c_big = b.cam0_image[int(200 * 1.5):int(280 * 1.5), int(336 * 1280 / 752):int(416 * 1280 / 752)].astype(np.float64).mean()
    assert abs(c_small - c_big) < 3.0, (c_small, c_big)
    # explicit width / height override the config's
    ex = SyntheticStream(ConfigEuRoC(), seed=7, n_frames=1, texture=tex, width=100, height=60)
    assert ex.frame(0).cam0_image.shape == (60, 100)
