"""The fused pyramid kernels at every shape that takes another of their paths, bit for bit against the CPU oracle.

Every case compares all levels, interior and 16-pixel frame, with oracle.cvops.build_pyramid plus np.pad(..., 16, mode='reflect')
(numpy's 'reflect' is BORDER_REFLECT_101), as test_gpu_ops.test_pyramid_matches_oracle_including_border does for the fixture frames.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (w, h, levels): what the shape exercises
SHAPES = [
    (384, 288, 4),    # 3 x 3 tall tiles: the only fully interior tile (the lean path) and all eight kinds of border tile
    (256, 192, 4),    # 2 x 2 tall tiles, every tile a corner, w % 128 == 0
    (752, 480, 4),    # the workload's shape: ragged last column of 112, five tile rows
    (160, 96, 3),     # 32-row tiles, ragged column of 32
    (64, 64, 2),      # the smallest fused image, one tile column narrower than a tile
    (144, 96, 3),     # w % 128 == 16: the unfused fallback (the dispatch boundary)
    (272, 160, 4),    # 32-row tiles with the fused levels 2 and 3
]


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from uav_airvision_amd import ops as o
    return o


def _random(w, h, n=1, seed=0):
    return np.random.default_rng(1000 * seed + w + h).integers(0, 256, (n, h, w), dtype=np.uint8)


def _check(ops, pyr_row, lay, img, levels, first=0):
    from oracle import cvops
    ref = cvops.build_pyramid(img, levels - 1)
    for l in range(first, levels):
        full = ops.pyramid_level(pyr_row, lay, l, with_border=True)
        exp = np.pad(ref[l], 16, mode='reflect')
        assert full.shape == exp.shape
        assert np.array_equal(full[16:-16, 16:-16], ref[l]), 'level %d interior differs' % l
        bad = np.argwhere(full != exp)
        assert bad.size == 0, 'level %d frame differs at %d pixels, first (row, col) %s' % (l, len(bad), bad[0])


@pytest.mark.parametrize('w,h,levels', SHAPES)
def test_shape_matches_oracle(ops, w, h, levels):
    imgs = _random(w, h, 2)
    pyr, lay = ops.build_pyramids(imgs, levels)
    for i in range(2):
        _check(ops, pyr[i], lay, imgs[i], levels)


@pytest.mark.parametrize('content', ['all255', 'all0', 'checker'])
def test_content_extremes(ops, content):
    # all 255 drives every packed 16-bit lane of the column filter to its bound (65,408); the checkerboard sits on the rounding
    w, h = 384, 288
    if content == 'checker':
        yy, xx = np.mgrid[0:h, 0:w]
        img = (((yy + xx) & 1) * 255).astype(np.uint8)
    else:
        img = np.full((h, w), 255 if content == 'all255' else 0, np.uint8)
    pyr, lay = ops.build_pyramids(img, 4)
    _check(ops, pyr[0], lay, img, 4)


@pytest.mark.parametrize('n', [1, 3, 9])
def test_batch_of_distinct_images(ops, n):
    imgs = _random(256, 192, n, seed=n)
    pyr, lay = ops.build_pyramids(imgs, 4)
    for i in range(n):
        _check(ops, pyr[i], lay, imgs[i], 4)


def test_misaligned_images_through_the_c_abi(ops):
    # base 4 bytes past a 16-byte boundary, image stride w * h + 4: rows are dword- but not 16-byte-aligned; the kernels stay fused
    import torch
    from uav_airvision_amd import _native as N
    w, h, levels, n = 384, 288, 4, 3
    imgs = _random(w, h, n, seed=5)
    stride = w * h + 4
    buf = torch.zeros(4 + n * stride + 64, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    for i in range(n):
        buf[4 + i * stride:4 + i * stride + w * h] = torch.from_numpy(imgs[i].reshape(-1)).cuda()
    lay = ops.pyramid_layout(w, h, levels)
    pyr = torch.zeros((n, lay.bytes), dtype=torch.uint8, device='cuda')
    N.check(N.lib().av_pyramid_build(C.c_void_p(buf.data_ptr() + 4), stride, n, w, h, levels, N.dptr(pyr), lay.bytes, N.current_stream()))
    torch.cuda.synchronize()
    for i in range(n):
        _check(ops, pyr[i], lay, imgs[i], levels)


@pytest.mark.parametrize('w,h', [(384, 288), (752, 480)])
def test_build_levels_leaves_level0_alone(ops, w, h):
    import torch
    imgs = _random(w, h, 2, seed=7)
    lay = ops.pyramid_layout(w, h, 4)
    out = torch.full((2, lay.bytes), 0xA5, dtype=torch.uint8, device='cuda')
    pyr, lay = ops.build_pyramids(imgs, 4, write_level0=False, out=out)
    assert pyr is out
    a = pyr.cpu().numpy()
    assert (a[:, lay.offset[0]:lay.offset[1]] == 0xA5).all(), 'the level-0 region was written'
    for i in range(2):
        _check(ops, pyr[i], lay, imgs[i], 4, first=1)
