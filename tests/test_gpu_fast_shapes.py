"""fast_kernel at the shapes where its paths part: tiles whose row / column tests can bind beside the interior tile that skips them,
ragged last tiles, dword and byte rows, dword and byte masks, contents at the ends of the biased range, keypoints on both sides of
the tile seams, batches that leave slots of an XCD group empty, and the per-tile lists through the engine.  Every case is compared
with oracle.cvops.fast_detect exactly (x, y, score), the engine cases with the oracle front-end frame by frame."""
import numpy as np
import pytest

from fe_harness import Frames, against_oracle, run_engine, run_oracle, scaled_cfg

pytestmark = pytest.mark.gpu

THRESHOLD = 15


def _noise(w, h):
    return np.random.default_rng(w + h).integers(0, 256, (h, w), dtype=np.uint8)


def _same_as_oracle(img, threshold, mask=None):
    """Both detectors on one image; returns the oracle's keypoints once the kernel's have been found equal to them."""
    from oracle import cvops
    from uav_airvision_amd import ops
    want = cvops.fast_detect(img, threshold, mask)
    got = ops.fast_detect(img, threshold, mask)
    for g, c in zip(got, want):
        assert np.array_equal(g, c), (img.shape, threshold, len(got[0]), len(want[0]))
    return want


# (w, h, keypoints of the oracle at threshold 15)
SHAPES = [(7, 7, 1),            # the smallest legal image, its one possible centre
          (64, 48, 261),        # exactly one tile, every border at once
          (67, 51, 282),        # a second tile column / row holding no valid centre
          (71, 55, 340),        # a second tile column / row 7 pixels wide with valid centres, byte rows
          (128, 96, 1162),      # 2 x 2 whole tiles, every tile a corner tile, dword rows
          (131, 97, 1171),      # ragged, byte rows
          (192, 144, 2626),     # 3 x 3 tiles: the one fully interior tile
          (196, 150, 2803)]     # the same with ragged edges, dword rows


@pytest.mark.parametrize('w,h,n', SHAPES)
def test_noise_image_matches_the_oracle(w, h, n):
    x, _y, _s = _same_as_oracle(_noise(w, h), THRESHOLD)
    assert len(x) > 0 and len(x) == n


@pytest.mark.parametrize('threshold,n', [(1, 2912), (100, 273)])
def test_thresholds_at_196x150(threshold, n):
    x, _y, _s = _same_as_oracle(_noise(196, 150), threshold)
    assert len(x) > 0 and len(x) == n


W, H = 128, 96


def _flat_and_checkerboards():
    yy, xx = np.mgrid[0:H, 0:W]
    return {'all 0': np.zeros((H, W), np.uint8), 'all 255': np.full((H, W), 255, np.uint8),
            'checkerboard 1': (((xx + yy) & 1) * 255).astype(np.uint8),
            'checkerboard 4': ((((xx >> 2) + (yy >> 2)) & 1) * 255).astype(np.uint8)}


@pytest.mark.parametrize('name', ['all 0', 'all 255', 'checkerboard 1', 'checkerboard 4'])
def test_content_extremes_have_no_keypoint(name):
    """Every biased ring difference is 1, 256 or 511: the ends of the range the half-precision patterns are compared over."""
    x, _y, _s = _same_as_oracle(_flat_and_checkerboards()[name], THRESHOLD)
    assert len(x) == 0


# isolated pixels at the first and last valid centre of both axes and on both sides of both tile seams, no two within 8 pixels of
# each other; the crossing of the seams has four pixels that touch one another, so two of them go into a set of their own
LONE = [[(3, 3), (W - 4, 3), (3, H - 4), (W - 4, H - 4), (63, 14), (64, 26), (63, 70), (64, 82), (16, 47), (28, 48), (96, 47), (108, 48), (63, 47)],
        [(3, 3), (W - 4, H - 4), (64, 48), (63, 30), (40, 47)],
        [(3, H - 4), (W - 4, 3), (64, 47), (63, 60), (30, 48)],
        [(63, 48), (64, 20), (90, 47), (90, 60)]]


@pytest.mark.parametrize('k', range(len(LONE)))
@pytest.mark.parametrize('inverse', [False, True])
def test_isolated_pixels_at_the_borders_and_the_tile_seams(k, inverse):
    """A lone 255 on black (or 0 on white) is a keypoint of score 254 at every threshold up to 254 and none at 255 (the oracle's answers
    on the CPU: all of them with score 254 at 15, 230 and 254, nothing at 255)."""
    img = np.zeros((H, W), np.uint8)
    for x, y in LONE[k]:
        img[y, x] = 255
    if inverse:
        img = 255 - img
    for threshold in (THRESHOLD, 230, 254):
        x, y, s = _same_as_oracle(img, threshold)
        assert sorted(zip(x.tolist(), y.tolist())) == sorted(LONE[k]) and np.all(s == 254), threshold
    x, _y, _s = _same_as_oracle(img, 255)
    assert len(x) == 0


def test_adjacent_pairs_across_the_seams_suppress_each_other():
    """Two neighbours of equal score: neither is a strict maximum, whichever tile judges it."""
    img = np.zeros((H, W), np.uint8)
    for y in (10, 30, 80):
        img[y, 63] = img[y, 64] = 255
    for x in (10, 30, 100):
        img[47, x] = img[48, x] = 255
    x, _y, _s = _same_as_oracle(img, THRESHOLD)
    assert len(x) == 0
    img[10, 63] = 254                    # ... and the brighter one of a pair survives: the tile left of the seam sees the other's score
    x, y, s = _same_as_oracle(img, THRESHOLD)
    assert len(x) == 1 and (x[0], y[0]) == (64, 10)


@pytest.mark.parametrize('w,h,counts', [(196, 150, (2015, 1534)),       # the mask can be read as dwords
                                        (131, 97, (845, 643))])         # only as bytes
def test_random_masks(w, h, counts):
    img = _noise(w, h)
    mask = (np.random.default_rng(7).uniform(size=img.shape) > 0.3).astype(np.uint8)
    for threshold, n in zip((7, 40), counts):
        x, _y, _s = _same_as_oracle(img, threshold, mask)
        assert len(x) > 0 and len(x) == n
    # any non-zero mask value keeps a pixel
    _same_as_oracle(img, 7, mask * np.random.default_rng(8).integers(1, 256, img.shape, dtype=np.uint8))


def _batch_words(imgs, threshold, cap=1 << 12):
    """The unordered packed words of every image of one av_fast_detect call, sorted per image."""
    import torch
    from uav_airvision_amd import _native as N
    n, h, w = imgs.shape
    t = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    kp = torch.empty(n * cap, dtype=torch.int32, device='cuda')
    cnt = torch.zeros(n, dtype=torch.int32, device='cuda')
    N.check(N.lib().av_fast_detect(N.dptr(t), w * h, None, 0, n, w, h, int(threshold), N.dptr(kp), N.dptr(cnt), cap, N.current_stream()))
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert np.all(c <= cap)
    words = kp.cpu().numpy().view(np.uint32).reshape(n, cap)
    return [np.sort(words[i, :c[i]]) for i in range(n)]


def test_batches_of_1_3_and_9_images():
    """One call, several images: nine leave seven slots of the second XCD group without an image."""
    from oracle import cvops
    from uav_airvision_amd.ops import KP_RASTER_BITS
    w, h = 131, 97
    imgs = np.stack([np.random.default_rng(1000 + i).integers(0, 256, (h, w), dtype=np.uint8) for i in range(9)])
    single = [_batch_words(imgs[i:i + 1], THRESHOLD)[0] for i in range(9)]
    for i in range(9):
        x, y, s = cvops.fast_detect(imgs[i], THRESHOLD)
        want = (s.astype(np.uint32) << KP_RASTER_BITS) | ((1 << KP_RASTER_BITS) - 1 - (y.astype(np.uint32) * w + x.astype(np.uint32)))
        assert len(x) > 0 and np.array_equal(single[i], np.sort(want)), i
    for n in (1, 3, 9):
        got = _batch_words(imgs[:n], THRESHOLD)
        assert len(got) == n
        for i in range(n):
            assert np.array_equal(got[i], single[i]), (n, i)


# ---- per-tile lists through the engine: 376 x 240 is 6 x 5 tiles, the last column 56 wide ------------------------------------------
ENGINE_FLOOR = 60          # what the oracle publishes at the least on these streams (60, 100, 100 features on frames 0, 1, 2)


@pytest.fixture(scope='module')
def engine_case():
    from uav_airvision_amd.synth import SyntheticStream
    cfg = scaled_cfg(376, 240)
    streams = [Frames.cached(SyntheticStream(cfg, seed=s, n_frames=3)) for s in (61, 62)]
    refs = [run_oracle(cfg, st) for st in streams]
    for ref in refs:
        assert min(len(r['ids']) for r in ref) == ENGINE_FLOOR and all(r['add']['n_fast'] > 1000 for r in ref[1:])
    return cfg, streams, refs


@pytest.mark.parametrize('mode', ['step', 'persist', 'frames'])
def test_tile_lists_through_the_engine(engine_case, mode):
    """step reads the padded level 0 (frame of 16 pixels), persist the image in place (the benchmark's path), frames the shared frame
    store through its index map."""
    cfg, streams, refs = engine_case
    got = run_engine(cfg, streams, mode=mode)
    for i, ref in enumerate(refs):
        against_oracle(ref, got[i], '%s stream %d' % (mode, i), min_features=ENGINE_FLOOR)
