"""ops.to_gray8 (av_to_gray8) on Bayer mosaics, bit-identical to the NumPy reference of tests/bayer_ref.py: all eight formats at the
small sizes at which either kernel can go wrong -- every pixel on a border, one vector with both edges in one lane, rows that cross a
wavefront, strip heights around the kernel's own -- on both paths, in batches, with saturating shifts; argument errors."""
import ctypes as C

import numpy as np
import pytest

import bayer_ref as br

pytestmark = pytest.mark.gpu

R = 16            # BY_ROWS of csrc/bayer.hip: the rows one lane of the vector path walks down; the heights below straddle it
# (w, h).  Generic path (w % 16 != 0): every pixel touches a border; 72 x 10 is wide but no multiple of 16.  Vector path: one vector
# (both image edges in one lane), odd heights, 65 vectors per row (a row crosses a wavefront boundary, where edge samples are loaded
# instead of exchanged), heights R - 1, R, R + 1, 2 R + 1.
GENERIC = ((2, 2), (3, 2), (2, 3), (5, 7), (72, 10))
VECTOR = ((16, 2), (16, 3), (32, 5), (80, 9), (1040, 4), (48, R - 1), (48, R), (48, R + 1), (48, 2 * R + 1))
SHIFT = 4


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


def _cases(rng, fmt, shape):
    yield 'full', br.random_frames(rng, fmt, shape)
    yield 'ends', br.random_frames(rng, fmt, shape, 'ends')


@pytest.mark.parametrize('fmt', br.FORMATS)
def test_every_size_alone_and_in_batches(fmt):
    """n = 1 contiguous (aligned: the vector path where w % 16 == 0), and n = 3 cut out of a taller batch: the image stride is then a
    multiple of 16 bytes whenever w is (vector path in a batch), and the rows past each image must not leak into it."""
    from uav_airvision_amd import ops
    rng = np.random.default_rng(61)
    for (w, h) in GENERIC + VECTOR:
        for kind, one in _cases(rng, fmt, (h, w)):
            got = ops.to_gray8(_dev(one), fmt, shift=SHIFT).cpu().numpy()
            assert np.array_equal(got, br.to_gray8(one, fmt, SHIFT)), (fmt, w, h, kind)
        tall = br.random_frames(rng, fmt, (3, h + 3, w))
        got = ops.to_gray8(_dev(tall)[:, :h], fmt, shift=SHIFT)
        assert tuple(got.shape) == (3, h, w)
        assert np.array_equal(got.cpu().numpy(), br.to_gray8(tall[:, :h], fmt, SHIFT)), (fmt, w, h)


@pytest.mark.parametrize('fmt', ['bayer_rggb8', 'bayer_bggr8', 'bayer_grbg16', 'bayer_gbrg16'])
def test_misaligned_base_and_odd_strides_take_the_generic_path(fmt):
    """A source that starts one sample into a buffer (8-bit: one byte), and n = 3 images whose stride is no multiple of 16 bytes, at
    widths the vector path would otherwise take."""
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(62)
    for (w, h) in ((16, 3), (32, 5), (48, R + 1), (5, 7)):
        n = 2
        flat = br.random_frames(rng, fmt, (n * h * w + 1,))
        img = _dev(flat)[1:].reshape(n, h, w)
        assert img.data_ptr() % 16 != 0
        assert np.array_equal(ops.to_gray8(img, fmt, shift=SHIFT).cpu().numpy(), br.to_gray8(flat[1:].reshape(n, h, w), fmt, SHIFT)), (fmt, w, h)
        # aligned base, stride = image + one sample
        per = h * w
        host = br.random_frames(rng, fmt, (3 * (per + 1),))
        d = _dev(host)
        img = d.as_strided((3, h, w), (per + 1, w, 1))
        want = br.to_gray8(np.stack([host[i * (per + 1):i * (per + 1) + per].reshape(h, w) for i in range(3)]), fmt, SHIFT)
        assert (img.stride(0) * img.element_size()) % 16 != 0
        assert np.array_equal(ops.to_gray8(img, fmt, shift=SHIFT).cpu().numpy(), want), (fmt, w, h)
        # an output that starts one byte into its buffer: the bytes around it stay
        obuf = torch.full((n * per + 2,), 0xA5, dtype=torch.uint8, device='cuda')
        out = obuf[1:-1].reshape(n, h, w)
        src = flat[:-1].reshape(n, h, w)
        assert ops.to_gray8(_dev(src), fmt, shift=SHIFT, out=out) is out
        got = obuf.cpu().numpy()
        assert got[0] == 0xA5 and got[-1] == 0xA5 and np.array_equal(got[1:-1].reshape(n, h, w), br.to_gray8(src, fmt, SHIFT)), (fmt, w, h)


@pytest.mark.parametrize('fmt', ['bayer_grbg8', 'bayer_bggr16'])
def test_batches_with_aligned_strides_larger_than_an_image(fmt):
    """n = 3 at 16-byte aligned addresses and strides on both sides, larger than an image: the vector path; the gaps between the
    outputs, preset to a sentinel, stay what they were."""
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(63)
    n = 3
    for (w, h) in ((16, 3), (80, 9), (1040, 4), (48, 2 * R + 1)):
        frames = br.random_frames(rng, fmt, (n, h, w))
        per, esize = h * w, frames.dtype.itemsize
        stride = per + 48 // esize                                # elements: three vectors more than an image
        host = br.random_frames(rng, fmt, (n * stride,))          # the gaps hold random samples that must not be read into the images
        for i in range(n):
            host[i * stride:i * stride + per] = frames[i].ravel()
        img = _dev(host).as_strided((n, h, w), (stride, w, 1))
        ostride = per + 32
        obuf = torch.full((n * ostride,), 0xA5, dtype=torch.uint8, device='cuda')
        out = obuf.as_strided((n, h, w), (ostride, w, 1))
        assert img.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and (stride * esize) % 16 == 0 and ostride % 16 == 0
        assert ops.to_gray8(img, fmt, shift=SHIFT, out=out) is out
        got = obuf.cpu().numpy().reshape(n, ostride)
        assert np.array_equal(got[:, :per].reshape(n, h, w), br.to_gray8(frames, fmt, SHIFT)), (fmt, w, h)
        assert (got[:, per:] == 0xA5).all(), (fmt, w, h)


@pytest.mark.parametrize('shift', [0, 4, 8])
def test_shifts_saturate_before_interpolation(shift):
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(64)
    for (w, h) in ((37, 9), (32, 5)):                             # generic and vector
        v = rng.integers(0, 65536, (2, h, w), dtype=np.uint16)
        v[0, 0, :7] = [0, 1, 255, 256, 4095, 4096, 65535]
        want = br.to_gray8(v, 'bayer_gbrg16', shift)
        if shift < 8:
            assert (want == 255).sum() > want.size // 2           # the data does saturate
        assert np.array_equal(ops.to_gray8(_dev(v), 'bayer_gbrg16', shift=shift).cpu().numpy(), want), (w, h)
        assert np.array_equal(ops.to_gray8(_dev(v).view(torch.int16), 'bayer_gbrg16', shift=shift).cpu().numpy(), want)      # int16 storage, same bits
        assert np.array_equal(ops.to_gray8(v, br.CODES['bayer_gbrg16'], shift=shift).cpu().numpy(), want)                     # a host array, the code



def test_the_camera_size_and_the_header_example():
    from uav_airvision_amd import ops
    rng = np.random.default_rng(65)
    for fmt in ('bayer_rggb8', 'bayer_gbrg16'):
        a = br.random_frames(rng, fmt, (2, 480, 752))
        assert np.array_equal(ops.to_gray8(_dev(a), fmt, shift=SHIFT).cpu().numpy(), br.to_gray8(a, fmt, SHIFT)), fmt
    assert ops.to_gray8(np.array([[10, 200], [30, 90]], np.uint8), 'bayer_rggb8').cpu().numpy().tolist() == [[81, 131], [31, 81]]
    for v in (0, 1, 77, 255):
        for fmt in br.FORMATS[:4]:
            assert bool((ops.to_gray8(np.full((33, 48), v, np.uint8), fmt) == v).all()), (fmt, v)


def test_one_image_of_4096_by_4096_16_bit_samples():
    """Byte offsets past 2^24 pixels x 2 bytes = 2^25 in one image: 64-bit row offsets on the vector path."""
    from uav_airvision_amd import ops
    a = np.random.default_rng(66).integers(0, 65536, (4096, 4096), dtype=np.uint16)
    got = ops.to_gray8(_dev(a), 'bayer_rggb16', shift=SHIFT).cpu().numpy()
    want = br.to_gray8(a, 'bayer_rggb16', SHIFT)
    assert np.array_equal(got, want)


def test_argument_errors_are_invalid_without_a_launch():
    import torch
    from uav_airvision_amd import _native as N, ops
    w, h = 16, 4
    src = torch.zeros(4 * w * h * 2, dtype=torch.uint8, device='cuda')
    dst = torch.full((4 * w * h,), 0x5A, dtype=torch.uint8, device='cuda')
    L = N.lib()

    def call(fmt=N.AV_PIX_BAYER_RGGB8, shift=8, ww=w, hh=h, n=2, in_stride=None, out_stride=None, out=None, inp=None):
        bpp = N.PIXEL_BYTES.get(fmt, 1)
        return L.av_to_gray8(C.c_void_p(src.data_ptr() if inp is None else inp), ww * hh * bpp if in_stride is None else in_stride, n, ww, hh, fmt, shift,
                             C.c_void_p(dst.data_ptr() if out is None else out), ww * hh if out_stride is None else out_stride, N.current_stream())
    assert call() == 0 and call(fmt=N.AV_PIX_BAYER_GBRG16) == 0
    for kw, text in ((dict(fmt=15), b'pixel format'), (dict(fmt=24), b'pixel format'), (dict(shift=9), b'shift'),
                     (dict(ww=1, hh=64), b'2 x 2'), (dict(ww=64, hh=1), b'2 x 2'), (dict(fmt=N.AV_PIX_BAYER_BGGR16, ww=1, hh=1), b'2 x 2'),
                     (dict(ww=4097, hh=4096, n=0), b'AV_MAX_IMAGE_PIXELS'),
                     (dict(in_stride=w * h - 1), b'strides'), (dict(out_stride=w * h - 1), b'strides'),
                     (dict(fmt=N.AV_PIX_BAYER_RGGB16, in_stride=w * h), b'strides'),
                     (dict(out=src.data_ptr()), b'overlaps'), (dict(out=src.data_ptr() + 2 * w * h - 1), b'overlaps'),
                     (dict(inp=dst.data_ptr() + w * h - 1, n=1), b'overlaps')):
        torch.cuda.synchronize()
        dst.fill_(0x5A)
        assert call(**kw) == N.AV_E_INVALID, kw
        assert text in L.av_last_error(), (kw, L.av_last_error())
        torch.cuda.synchronize()
        assert bool((dst == 0x5A).all()), kw                                  # nothing ran
    assert call(out=src.data_ptr() + 2 * w * h) == 0                          # right behind the input is fine
    for shape in ((2, 1, 8), (2, 8, 1), (1, 1)):
        with pytest.raises(ValueError, match='2 x 2'):
            ops.to_gray8(torch.zeros(shape, dtype=torch.uint8, device='cuda'), 'bayer_rggb8')
    with pytest.raises(ValueError, match='bayer_rggb16'):
        ops.to_gray8(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), 'bayer_rggb16')
    with pytest.raises(ValueError, match='bayer_bggr8'):
        ops.to_gray8(torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device='cuda'), 'bayer_bggr8')
