"""CLAHE without a GPU: the NumPy reference of tests/clahe_ref.py on cases that can be worked out by hand, one pinned output, and the
plumbing of the switch (configuration, packed configuration, sweep command line, SyntheticStream's new arguments)."""
import hashlib

import numpy as np
import pytest

import clahe_ref as cr

PINNED_IMAGE = (7, 752, 480)
PINNED_SHA1 = '2f643a22f9378728691c1fd9192f08454d4c1aae'
# sha1 over cam0 + cam1 bytes of frames 0, 1 and 4 of SyntheticStream(ConfigEuRoC(), seed=0, n_frames=6), taken on the commit before
# the contrast / brightness_offset arguments existed
SYNTH_SHA1 = '2a60e780b446a75187a7f993a97ed5be95c1378a'


def _expected_lut_of_single_value(c, area, clip_limit):
    """A tile whose pixels all have grey value c, by hand: one bin of `area`, clipped to clip, the rest spread evenly."""
    if clip_limit <= 0:
        cum = np.where(np.arange(256) >= c, area, 0)
    else:
        clip = max(1, int(clip_limit * area / 256))
        assert area > clip
        clipped = area - clip
        batch, residual = divmod(clipped, 256)
        step = max(256 // residual, 1) if residual else 1
        extra = np.array([1 if residual and i % step == 0 and i // step < residual else 0 for i in range(256)])
        hist = batch + extra
        hist[c] += clip
        cum = np.cumsum(hist)
        assert cum[-1] == area
    return np.clip(np.rint(cum.astype(np.float32) * (np.float32(255.0) / np.float32(area))), 0, 255).astype(np.uint8)


@pytest.mark.parametrize('clip_limit', [0.0, 2.0, 40.0])
def test_constant_image(clip_limit):
    """Every tile has the same table, so the interpolation weights (which sum to 1 up to float32 rounding of xa1 = 1 - xa) return
    that table's entry: the output is constant and equals the hand-computed lut[c]; without a clip limit that is 255."""
    c, w, h = 93, 64, 48
    img = np.full((h, w), c, np.uint8)
    out, lut = cr.clahe(img, clip_limit, (8, 8), return_lut=True)
    want = _expected_lut_of_single_value(c, (w // 8) * (h // 8), clip_limit)
    assert (lut == want[None, :]).all()
    assert (out == want[c]).all()
    if clip_limit == 0.0:
        assert want[c] == 255 and want[c - 1] == 0


def test_a_tile_with_a_single_grey_value():
    img = cr.seeded_image(3, 64, 64)
    img[16:32, 32:48] = 200                      # tile (x 2, y 1) of a 4 x 4 grid
    lut = cr.luts(img, 3.0, (4, 4))
    assert (lut[1 * 4 + 2] == _expected_lut_of_single_value(200, 256, 3.0)).all()
    assert not (lut[0] == lut[1 * 4 + 2]).all()


def test_no_clip_limit_is_plain_equalisation_per_tile():
    img = cr.seeded_image(4, 96, 64)
    lut = cr.luts(img, 0.0, (3, 2))
    for j in range(2):
        for i in range(3):
            tile = img[j * 32:(j + 1) * 32, i * 32:(i + 1) * 32]
            cdf = np.array([(tile <= v).sum() for v in range(256)], dtype=np.float32)
            want = np.clip(np.rint(cdf * (np.float32(255.0) / np.float32(1024))), 0, 255).astype(np.uint8)
            assert (lut[j * 3 + i] == want).all(), (i, j)


def test_one_tile_has_no_interpolation():
    img = cr.seeded_image(5, 80, 60)
    out, lut = cr.clahe(img, 2.0, (1, 1), return_lut=True)
    assert lut.shape == (1, 256)
    assert (out == lut[0][img]).all()


def test_padding_on_both_axes():
    """30 x 21 with an 8 x 8 grid: 2 columns and 3 rows are mirrored (101) in, tiles are 4 x 3; the last tile's table is that of its
    twelve pixels, all of them mirrored rows."""
    img = cr.seeded_image(6, 30, 21, smooth=False)
    ext, tw, th = cr.padded(img, (8, 8))
    assert ext.shape == (24, 32) and (tw, th) == (4, 3)
    assert (ext == np.pad(img, ((0, 3), (0, 2)), mode='reflect')).all()
    assert (ext[:, 30] == ext[:, 28]).all() and (ext[21] == ext[19]).all() and ext[23, 31] == img[17, 27]
    last = np.array([[img[19, 28], img[19, 29], img[19, 28], img[19, 27]],          # rows 21, 22, 23 mirror to 19, 18, 17
                     [img[18, 28], img[18, 29], img[18, 28], img[18, 27]],          # columns 30, 31 to 28, 27
                     [img[17, 28], img[17, 29], img[17, 28], img[17, 27]]], np.uint8)
    lut = cr.luts(img, 0.0, (8, 8))
    cdf = np.array([(last <= v).sum() for v in range(256)], dtype=np.float32)
    assert (lut[63] == np.clip(np.rint(cdf * (np.float32(255.0) / np.float32(12))), 0, 255).astype(np.uint8)).all()
    # one ragged axis pads that axis only
    assert cr.padded(img[:16], (8, 8))[0].shape == (16, 32) and cr.padded(img[:, :24], (8, 8))[0].shape == (24, 24)
    out = cr.clahe(img, 2.0, (8, 8))
    assert out.shape == img.shape and out.dtype == np.uint8


@pytest.mark.parametrize('residual, bins', [(3, [0, 85, 170]), (100, list(range(0, 200, 2))), (200, list(range(200))), (255, list(range(255)))])
def test_residual_redistribution_stride(residual, bins):
    """clip 10, one bin of 10 + residual: nothing to hand out evenly, step = max(256 / residual, 1), `residual` bins get one each."""
    hist = [0] * 256
    hist[10] = 10 + residual
    got = cr.redistribute(hist, 10)
    want = [0] * 256
    want[10] = 10
    for b in bins:
        want[b] += 1
    assert got == want and sum(got) == 10 + residual
    # 256 more: every bin gets one on top
    hist[10] += 256
    assert cr.redistribute(hist, 10) == [v + 1 for v in want]


def test_clip_value():
    assert cr.clip_value(2.0, 94 * 60) == 44 and cr.clip_value(0.001, 100) == 1 and cr.clip_value(0.0, 100) == 0
    assert cr.clip_value(40.0, 94 * 60) == 881


def test_pinned_output_of_a_seeded_image():
    seed, w, h = PINNED_IMAGE
    out, lut = cr.clahe(cr.seeded_image(seed, w, h), 2.0, (8, 8), return_lut=True)
    assert hashlib.sha1(out.tobytes() + lut.tobytes()).hexdigest() == PINNED_SHA1


# ---- the switch -----------------------------------------------------------------------------------------------------------------
def test_config_defaults(cfg):
    assert cfg.use_clahe is False and cfg.clahe_clip_limit == 2.0 and tuple(cfg.clahe_tiles) == (8, 8)


def test_packed_config_carries_the_fields_and_only_use_clahe_sets_the_flag():
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import pack_frontend_config
    cfg = ConfigEuRoC()
    c = pack_frontend_config(cfg)
    assert c.flags == 0 and c.clahe_clip_limit == 2.0 and (c.clahe_tiles_x, c.clahe_tiles_y) == (8, 8) and c.reserved0 == 0
    cfg.clahe_clip_limit, cfg.clahe_tiles = 3.5, (4, 6)
    c = pack_frontend_config(cfg)
    assert c.flags == 0 and c.clahe_clip_limit == 3.5 and (c.clahe_tiles_x, c.clahe_tiles_y) == (4, 6)
    cfg.use_clahe = True
    assert pack_frontend_config(cfg).flags == N.AV_FE_CLAHE == 4
    cfg.use_ransac = True
    assert pack_frontend_config(cfg).flags == N.AV_FE_CLAHE | N.AV_FE_RANSAC
    cfg.use_clahe = False
    assert pack_frontend_config(cfg).flags == N.AV_FE_RANSAC

    class Bare(object):
        pass
    bare = Bare()
    for k, v in vars(ConfigEuRoC()).items():
        if 'clahe' not in k:
            setattr(bare, k, v)
    c = pack_frontend_config(bare)
    assert c.flags == 0 and c.clahe_clip_limit == 2.0 and (c.clahe_tiles_x, c.clahe_tiles_y) == (8, 8)


def test_sweep_command_line():
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.sweep import apply_args, make_parser
    ap = make_parser()
    cfg = apply_args(ConfigEuRoC(), ap.parse_args(['--sequences', 'a']))
    assert cfg.use_clahe is False and cfg.clahe_clip_limit == 2.0 and tuple(cfg.clahe_tiles) == (8, 8) and cfg.use_ransac is False
    cfg = apply_args(ConfigEuRoC(), ap.parse_args(['--sequences', 'a', '--clahe']))
    assert cfg.use_clahe is True and cfg.clahe_clip_limit == 2.0 and tuple(cfg.clahe_tiles) == (8, 8)
    cfg = apply_args(ConfigEuRoC(), ap.parse_args(['--sequences', 'a', '--clahe', '--clahe-clip', '3', '--clahe-tiles', '4', '6', '--ransac']))
    assert cfg.use_clahe is True and cfg.clahe_clip_limit == 3.0 and tuple(cfg.clahe_tiles) == (4, 6) and cfg.use_ransac is True


def _sha(frames):
    hs = hashlib.sha1()
    for m in frames:
        hs.update(m.cam0_image.tobytes())
        hs.update(m.cam1_image.tobytes())
    return hs.hexdigest()


def test_synthetic_stream_defaults_render_what_they_always_did(cfg, stream0):
    from uav_airvision_amd.synth import SyntheticStream
    assert _sha([stream0.frame(k) for k in (0, 1, 4)]) == SYNTH_SHA1
    same = SyntheticStream(cfg, seed=0, n_frames=6, contrast=1.0, brightness_offset=0.0)
    assert _sha([same.frame(1)]) == _sha([stream0.frame(1)])


def test_synthetic_stream_contrast_and_offset(cfg, stream0):
    """contrast 0.25 shrinks the spread of the grey values about the texture's mean to a quarter (noise and quantisation aside);
    the offset moves the mean."""
    from uav_airvision_amd.synth import SyntheticStream
    flat = SyntheticStream(cfg, seed=0, n_frames=6, contrast=0.25, brightness_offset=-40.0, pixel_noise=0.0)
    plain = SyntheticStream(cfg, seed=0, n_frames=6, pixel_noise=0.0)
    a, b = flat.frame(2).cam0_image.astype(np.float64), plain.frame(2).cam0_image.astype(np.float64)
    inside = (b > 0) & (b < 255)                 # where the plain render did not saturate
    want = float(plain.tex_mean) + 0.25 * (b - float(plain.tex_mean)) - 40.0
    assert np.abs(a - want)[inside & (want > 0.5)].max() <= 0.75
    assert a.std() < 0.3 * b.std()
