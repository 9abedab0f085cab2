"""ops.clahe / av_clahe against the NumPy reference of tests/clahe_ref.py: bytes and look-up tables, bit for bit."""
import numpy as np
import pytest

import clahe_ref as cr

pytestmark = pytest.mark.gpu

SIZES = ((752, 480), (640, 480), (331, 203), (24, 17))          # (w, h): EuRoC, VGA, an odd size that pads on both axes, a tiny image
TILES = ((8, 8), (4, 4), (1, 1), (16, 8))
CLIPS = (0.0, 1.0, 2.0, 4.0, 40.0)


def _check(img, clip, tiles, **kw):
    from uav_airvision_amd import ops
    out, lut = ops.clahe(img, clip, tiles, return_lut=True, **kw)
    want, want_lut = cr.clahe(img, clip, tiles, return_lut=True)
    got, got_lut = out.cpu().numpy(), lut.cpu().numpy()[0]
    assert np.array_equal(got_lut, want_lut), ('lut', img.shape, clip, tiles, int((got_lut != want_lut).sum()))
    assert np.array_equal(got, want), ('image', img.shape, clip, tiles, int((got != want).sum()))


@pytest.mark.parametrize('size', SIZES)
def test_sizes_and_tile_grids(size):
    w, h = size
    img = cr.seeded_image(11 + w, w, h)
    for tiles in TILES:
        _check(img, 2.0, tiles)


@pytest.mark.parametrize('clip', CLIPS)
def test_clip_limits(clip):
    _check(cr.seeded_image(21, 752, 480), clip, (8, 8))
    _check(cr.seeded_image(22, 331, 203, lo=90, hi=140), clip, (4, 4))          # a narrow histogram: most bins are clipped
    _check(np.full((48, 64), 93, np.uint8), clip, (8, 8))                        # every lane of a wavefront on one bin


def test_batch_with_a_stride_larger_than_the_image_and_without_tables():
    """Five images at a stride of w * h + 1,052 bytes (whole dwords) and at w * h + 3 (the byte path), through the C entry point; the
    bytes between the images are not touched; the tables may be left out."""
    import torch
    from uav_airvision_amd import _native as N
    w, h, n = 640, 480, 5
    imgs = np.stack([cr.seeded_image(30 + i, w, h, lo=20 * i, hi=256 - 10 * i) for i in range(n)])
    want = [cr.clahe(im, 2.0, (8, 8), return_lut=True) for im in imgs]
    for gap in (1052, 3):
        stride = w * h + gap
        src = torch.full((n, stride), 0xAB, dtype=torch.uint8, device='cuda')
        src[:, :w * h] = torch.from_numpy(imgs.reshape(n, -1)).cuda()
        dst = torch.full((n, stride + 4), 0xCD, dtype=torch.uint8, device='cuda')
        lut = torch.zeros((n, 64, 256), dtype=torch.uint8, device='cuda')
        for tables in (lut, None):
            dst.fill_(0xCD)
            N.check(N.lib().av_clahe(N.dptr(src), stride, n, w, h, 2.0, 8, 8, N.dptr(dst), stride + 4, None if tables is None else N.dptr(tables),
                                     N.current_stream()))
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            for i in range(n):
                assert np.array_equal(got[i, :w * h].reshape(h, w), want[i][0]), (gap, i)
                assert (got[i, w * h:] == 0xCD).all(), (gap, i)
        assert np.array_equal(lut.cpu().numpy(), np.stack([t for _o, t in want]))
        assert (src.cpu().numpy()[:, w * h:] == 0xAB).all()


def test_in_place_and_out_argument():
    import torch
    from uav_airvision_amd import ops
    imgs = np.stack([cr.seeded_image(40 + i, 752, 480) for i in range(3)])
    want = np.stack([cr.clahe(im, 2.0, (8, 8)) for im in imgs])
    t = torch.from_numpy(imgs).cuda()
    keep = t.clone()
    out = torch.empty_like(t)
    r = ops.clahe(t, out=out)
    assert r is out and np.array_equal(out.cpu().numpy(), want) and torch.equal(t, keep)
    r = ops.clahe(t, out=t)
    assert r is t and np.array_equal(t.cpu().numpy(), want)
    # an odd size in place (byte path, mirrored columns are read from the image being rewritten only by the first kernel)
    im = cr.seeded_image(44, 331, 203)
    t = torch.from_numpy(im).cuda()
    ops.clahe(t, 4.0, (16, 8), out=t)
    assert np.array_equal(t.cpu().numpy(), cr.clahe(im, 4.0, (16, 8)))


def test_bad_arguments_are_refused():
    import torch
    from uav_airvision_amd import _native as N
    t = torch.zeros((480, 752), dtype=torch.uint8, device='cuda')
    o = torch.zeros_like(t)

    def call(w=752, h=480, clip=2.0, tx=8, ty=8, n=1, stride=752 * 480, ostride=752 * 480, src=t, dst=o):
        return N.lib().av_clahe(None if src is None else N.dptr(src), stride, n, w, h, clip, tx, ty, None if dst is None else N.dptr(dst), ostride,
                                None, N.current_stream())
    assert call() == N.AV_OK
    for kw in (dict(tx=0), dict(ty=0), dict(tx=17), dict(ty=17), dict(clip=-1.0), dict(clip=float('nan')), dict(w=1024, h=513), dict(w=0),
               dict(stride=752 * 480 - 1), dict(ostride=100), dict(n=-1), dict(src=None), dict(dst=None)):
        assert call(**kw) == N.AV_E_INVALID, kw
        assert N.lib().av_last_error(), kw
    lut = torch.zeros(64 * 256 + 16, dtype=torch.uint8, device='cuda')
    assert N.lib().av_clahe(N.dptr(t), 752 * 480, 1, 752, 480, 2.0, 8, 8, N.dptr(o), 752 * 480, N.dptr(lut[4:]), N.current_stream()) == N.AV_E_INVALID
    assert N.lib().av_clahe(N.dptr(t), 752 * 480, 1, 752, 480, 2.0, 8, 8, N.dptr(o), 752 * 480, N.dptr(lut[16:]), N.current_stream()) == N.AV_OK
    torch.cuda.synchronize()
    with pytest.raises(N.AirvisionError):
        from uav_airvision_amd import ops
        ops.clahe(t, tiles=(32, 8))
