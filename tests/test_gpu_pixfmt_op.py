"""ops.to_gray8 (av_to_gray8) bit-identical to the NumPy reference of tests/pixfmt_ref.py: every format at sizes on both sides of the
16-pixel vector body, batches with a stride larger than an image, unaligned base addresses, saturating shifts, argument errors."""
import ctypes as C

import numpy as np
import pytest

import pixfmt_ref as pr

pytestmark = pytest.mark.gpu

FORMATS = ('gray16', 'rgb8', 'bgr8', 'rgba8', 'bgra8')
SIZES = ((1, 1), (17, 5), (33, 3), (64, 2), (752, 480))          # (w, h): 1, 85, 99, 128 pixels -- tail only, body + tail, whole vectors -- and the camera's


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize('fmt', FORMATS)
def test_every_size_single_and_batched_with_a_wide_stride(fmt):
    """n = 1 contiguous: aligned addresses, the strides are not applied, so the vector body runs with its ragged end (1 x 1: the end
    alone; 17 x 5, 33 x 3: body + end; 64 x 2, 752 x 480: body alone).  n = 3 cut out of a taller batch, so that the images lie further
    apart than their size: a multiple of 16 bytes only where the row size makes it so, the byte-wise path otherwise."""
    from uav_airvision_amd import ops
    rng = np.random.default_rng(31)
    for (w, h) in SIZES:
        one = pr.random_frames(rng, fmt, (h, w))
        assert np.array_equal(ops.to_gray8(_dev(one), fmt).cpu().numpy(), pr.to_gray8(one, fmt)), (fmt, w, h)
        tall = pr.random_frames(rng, fmt, (3, h + 2, w))
        got = ops.to_gray8(_dev(tall)[:, :h], fmt)
        assert tuple(got.shape) == (3, h, w)
        assert np.array_equal(got.cpu().numpy(), pr.to_gray8(tall[:, :h], fmt)), (fmt, w, h)


@pytest.mark.parametrize('fmt', FORMATS)
def test_batches_with_vector_strides_and_ragged_ends(fmt):
    """n = 3 images whose size is no multiple of 16 pixels, at 16-byte aligned addresses and strides on both sides (frames cut from a
    padded buffer, `out` a slice with a padded stride): the vector body and the byte-wise end of every image of a batch; the padding
    between the outputs stays what it was."""
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(35)
    n = 3
    for (w, h) in ((1, 1), (17, 5), (33, 3), (37, 9), (64, 2)):
        frames = pr.random_frames(rng, fmt, (n, h, w))
        c = frames.shape[3] if frames.ndim == 4 else 1
        per = h * w * c                                           # elements of one frame
        esize = frames.dtype.itemsize
        stride = (per * esize + 15) // 16 * 16 // esize + 16 // esize      # elements: the next multiple of 16 bytes, and one vector more
        host = np.zeros(n * stride, frames.dtype)
        for i in range(n):
            host[i * stride:i * stride + per] = frames[i].ravel()
        flat = torch.from_numpy(host).cuda()
        img = flat.as_strided(tuple(frames.shape), (stride, w * c, c, 1) if c > 1 else (stride, w, 1))
        ostride = (h * w + 15) // 16 * 16 + 16
        obuf = torch.full((n * ostride,), 0xA5, dtype=torch.uint8, device='cuda')
        out = obuf.as_strided((n, h, w), (ostride, w, 1))
        assert img.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and (stride * esize) % 16 == 0 and ostride % 16 == 0
        assert ops.to_gray8(img, fmt, out=out) is out
        got = obuf.cpu().numpy().reshape(n, ostride)
        assert np.array_equal(got[:, :h * w].reshape(n, h, w), pr.to_gray8(frames, fmt)), (fmt, w, h)
        assert (got[:, h * w:] == 0xA5).all(), (fmt, w, h)


@pytest.mark.parametrize('fmt', FORMATS)
def test_unaligned_base_and_output(fmt):
    """The images start one pixel into a larger buffer (a slice of a flat tensor), and so does the output: the byte-wise path; the bytes
    around the output stay what they were."""
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(32)
    for (w, h) in ((17, 5), (64, 2), (752, 480)):
        n = 2
        flat = pr.random_frames(rng, fmt, (n * h * w + 1,))
        d = _dev(flat)
        img = d[1:].reshape((n, h, w) + tuple(flat.shape[1:]))
        want = pr.to_gray8(flat[1:].reshape((n, h, w) + tuple(flat.shape[1:])), fmt)
        assert img.data_ptr() % 16 != 0
        assert np.array_equal(ops.to_gray8(img, fmt).cpu().numpy(), want), (fmt, w, h)
        obuf = torch.full((n * h * w + 2,), 0xA5, dtype=torch.uint8, device='cuda')
        out = obuf[1:-1].reshape(n, h, w)
        assert ops.to_gray8(_dev(flat[:-1].reshape((n, h, w) + tuple(flat.shape[1:]))), fmt, out=out) is out
        got = obuf.cpu().numpy()
        assert got[0] == 0xA5 and got[-1] == 0xA5
        assert np.array_equal(got[1:-1].reshape(n, h, w), pr.to_gray8(flat[:-1].reshape((n, h, w) + tuple(flat.shape[1:])), fmt)), (fmt, w, h)


@pytest.mark.parametrize('shift', [0, 4, 8])
def test_gray16_shifts_saturate(shift):
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(33)
    v = rng.integers(0, 65536, (2, 9, 37), dtype=np.uint16)
    v[0, 0, :7] = [0, 1, 255, 256, 4095, 4096, 65535]
    want = pr.to_gray8(v, 'gray16', shift)
    if shift < 8:
        assert (want == 255).sum() > want.size // 2                      # the data does saturate
    assert np.array_equal(ops.to_gray8(_dev(v), 'gray16', shift=shift).cpu().numpy(), want)
    assert np.array_equal(ops.to_gray8(_dev(v).view(torch.int16), 'gray16', shift=shift).cpu().numpy(), want)      # int16 storage, same bits
    assert np.array_equal(ops.to_gray8(v, 'gray16', shift=shift).cpu().numpy(), want)                               # a host array is uploaded


def test_gray8_is_the_identity():
    from uav_airvision_amd import ops
    rng = np.random.default_rng(34)
    g = rng.integers(0, 256, (3, 11, 19), dtype=np.uint8)
    d = _dev(g)
    assert np.array_equal(ops.to_gray8(d, 'gray8').cpu().numpy(), g)
    assert ops.to_gray8(d, 'gray8', out=d) is d and np.array_equal(d.cpu().numpy(), g)
    tall = _dev(rng.integers(0, 256, (3, 13, 19), dtype=np.uint8))
    assert np.array_equal(ops.to_gray8(tall[:, :11], 'gray8').cpu().numpy(), tall[:, :11].cpu().numpy())
    # an overlap that is not the exact in-place call is refused for gray8 as for every format
    from uav_airvision_amd import _native as N
    with pytest.raises(N.AirvisionError, match='overlaps'):
        ops.to_gray8(tall[:, :11], 'gray8', out=tall[:, 1:12])


def test_argument_errors_are_invalid_without_a_launch():
    import torch
    from uav_airvision_amd import _native as N, ops
    w, h = 16, 4
    src = torch.zeros(4 * w * h * 4, dtype=torch.uint8, device='cuda')
    dst = torch.full((4 * w * h,), 0x5A, dtype=torch.uint8, device='cuda')
    L = N.lib()

    def call(fmt=N.AV_PIX_RGB8, shift=8, ww=w, hh=h, n=2, in_stride=None, out_stride=None, out=None, inp=None):
        bpp = N.PIXEL_BYTES.get(fmt, 1)
        return L.av_to_gray8(C.c_void_p(src.data_ptr() if inp is None else inp), ww * hh * bpp if in_stride is None else in_stride, n, ww, hh, fmt, shift,
                             C.c_void_p(dst.data_ptr() if out is None else out), ww * hh if out_stride is None else out_stride, N.current_stream())
    assert call() == 0
    for kw, text in ((dict(fmt=6), b'pixel format'), (dict(fmt=-1), b'pixel format'), (dict(shift=9), b'shift'), (dict(shift=-1), b'shift'),
                     (dict(ww=4097, hh=4096, n=0), b'AV_MAX_IMAGE_PIXELS'), (dict(ww=0), b'AV_MAX_IMAGE_PIXELS'),
                     (dict(in_stride=w * h * 3 - 1), b'strides'), (dict(out_stride=w * h - 1), b'strides'),
                     (dict(fmt=N.AV_PIX_GRAY16, in_stride=w * h), b'strides'),
                     (dict(out=src.data_ptr()), b'overlaps'), (dict(out=src.data_ptr() + 2 * w * h * 3 - 1), b'overlaps'),
                     (dict(inp=dst.data_ptr() + w * h - 1, n=1), b'overlaps')):
        torch.cuda.synchronize()
        dst.fill_(0x5A)
        assert call(**kw) == N.AV_E_INVALID, kw
        assert text in L.av_last_error(), (kw, L.av_last_error())
        torch.cuda.synchronize()
        assert bool((dst == 0x5A).all()), kw                                  # nothing ran
    assert call(out=src.data_ptr() + 2 * w * h * 3) == 0                      # right behind the input is fine
    with pytest.raises(ValueError, match='gray16'):
        ops.to_gray8(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), 'gray16')
    with pytest.raises(ValueError, match='rgb8'):
        ops.to_gray8(torch.zeros((2, 4, 4, 4), dtype=torch.uint8, device='cuda'), 'rgb8')
    with pytest.raises(ValueError, match='format'):
        ops.to_gray8(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), 'bayer')
    with pytest.raises(ValueError, match='out must be'):
        ops.to_gray8(torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device='cuda'), 'rgb8', out=torch.zeros((2, 4, 5), dtype=torch.uint8, device='cuda'))
