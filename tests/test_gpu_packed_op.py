"""ops.to_gray8 (av_to_gray8) on the packed 10 / 12-bit transports, bit-identical to the NumPy reference of tests/packed_ref.py: all
four packings at sizes on both sides of every lane span (16, 32 or 64 samples), batches with unaligned and with padded aligned strides,
unaligned base addresses, saturating shifts; packed mosaics on both demosaic paths; argument errors; and against the existing
GRAY16 / 16-bit Bayer operator run on the device on the left-justified unpacked samples."""
import ctypes as C

import numpy as np
import pytest

import packed_ref as kr

pytestmark = pytest.mark.gpu

# (w, h): one group (the ragged end alone); 180 samples (body + ragged end for every span); 128 (whole vectors only); 16,900 (past one
# workgroup's share -- 256 lanes x 32 or 64 samples -- with a ragged end); the camera's own
SIZES = ((4, 1), (36, 5), (64, 2), (260, 65), (752, 480))
BAYER_SIZES = ((4, 2), (36, 6), (64, 18), (752, 480))            # generic demosaic twice, the vector demosaic past its 16-row strip, the camera's
BAYER_FORMATS = ('bayer_rggb10p', 'bayer_bggr10_csi2', 'bayer_grbg12_csi2', 'bayer_rggb12p', 'bayer_bggr12p', 'bayer_grbg12p', 'bayer_gbrg12p')


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize('fmt', kr.GREY)
def test_every_size_single_and_batched_with_a_wide_stride(fmt):
    """n = 1 contiguous: aligned addresses, the strides are not applied, so the vector body runs with its ragged end.  n = 3 cut out of
    a taller batch, so that the images lie further apart than their size: a multiple of 16 bytes only where the row size makes it so,
    the group-wise path otherwise."""
    from uav_airvision_amd import ops
    rng = np.random.default_rng(71)
    for (w, h) in SIZES:
        one = kr.random_frames(rng, fmt, (h, w))
        got = ops.to_gray8(_dev(one), fmt)
        assert tuple(got.shape) == (h, w)
        assert np.array_equal(got.cpu().numpy(), kr.to_gray8(one, fmt)), (fmt, w, h)
        tall = kr.random_frames(rng, fmt, (3, h + 2, w))
        got = ops.to_gray8(_dev(tall)[:, :h], fmt, shift=6)
        assert tuple(got.shape) == (3, h, w)
        assert np.array_equal(got.cpu().numpy(), kr.to_gray8(tall[:, :h], fmt, 6)), (fmt, w, h)


@pytest.mark.parametrize('fmt', kr.GREY)
def test_batches_with_vector_strides_and_ragged_ends(fmt):
    """n = 3 at 16-byte aligned addresses and padded strides on both sides: the vector body and the group-wise end of every image of a
    batch; the gaps between the inputs hold random bytes that must not be read into the images, the padding between the outputs stays
    what it was."""
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(72)
    n = 3
    for (w, h) in SIZES:
        frames = kr.random_frames(rng, fmt, (n, h, w))
        per = h * frames.shape[2]                                 # bytes of one frame
        stride = (per + 15) // 16 * 16 + 16
        host = rng.integers(0, 256, n * stride, dtype=np.uint8)
        for i in range(n):
            host[i * stride:i * stride + per] = frames[i].ravel()
        img = _dev(host).as_strided(tuple(frames.shape), (stride, frames.shape[2], 1))
        ostride = (h * w + 15) // 16 * 16 + 16
        obuf = torch.full((n * ostride,), 0xA5, dtype=torch.uint8, device='cuda')
        out = obuf.as_strided((n, h, w), (ostride, w, 1))
        assert img.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and stride % 16 == 0 and ostride % 16 == 0
        assert ops.to_gray8(img, fmt, shift=7, out=out) is out
        got = obuf.cpu().numpy().reshape(n, ostride)
        assert np.array_equal(got[:, :h * w].reshape(n, h, w), kr.to_gray8(frames, fmt, 7)), (fmt, w, h)
        assert (got[:, h * w:] == 0xA5).all(), (fmt, w, h)


@pytest.mark.parametrize('fmt', kr.GREY)
def test_unaligned_base_and_output(fmt):
    """The images start one byte into a larger buffer, and so does the output: the group-wise path; the guard bytes around the output
    stay what they were."""
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(73)
    for (w, h) in SIZES:
        n = 2
        frames = kr.random_frames(rng, fmt, (n, h, w))
        flat = np.concatenate([np.array([0x3C], np.uint8), frames.ravel()])
        img = _dev(flat)[1:].reshape(frames.shape)
        want = kr.to_gray8(frames, fmt)
        assert img.data_ptr() % 16 != 0
        assert np.array_equal(ops.to_gray8(img, fmt).cpu().numpy(), want), (fmt, w, h)
        obuf = torch.full((n * h * w + 2,), 0xA5, dtype=torch.uint8, device='cuda')
        out = obuf[1:-1].reshape(n, h, w)
        assert ops.to_gray8(_dev(frames), fmt, out=out) is out
        got = obuf.cpu().numpy()
        assert got[0] == 0xA5 and got[-1] == 0xA5
        assert np.array_equal(got[1:-1].reshape(n, h, w), want), (fmt, w, h)


@pytest.mark.parametrize('shift', [0, 4, 8])
@pytest.mark.parametrize('fmt', kr.GREY)
def test_shifts_saturate(fmt, shift):
    from uav_airvision_amd import _native as N, ops
    rng = np.random.default_rng(74)
    d = kr.depth(fmt)
    v = rng.integers(0, 1 << d, (2, 9, 36), dtype=np.uint16)
    v[0, 0, :5] = [0, 1, (1 << (d - 8)) - 1, 1 << (d - 8), (1 << d) - 1]
    v[1, 8, -5:] = [0, 1, (1 << (d - 8)) - 1, 1 << (d - 8), (1 << d) - 1]         # in the ragged end too
    raw = kr.pack(v, fmt)
    want = kr.to_gray8(raw, fmt, shift)
    assert want[0, 0, :5].tolist() == [min(255, (int(x) << (16 - d)) >> shift) for x in v[0, 0, :5]]
    if shift == 0:
        assert (want == 255).sum() > want.size // 2                              # the data does saturate
    assert np.array_equal(ops.to_gray8(_dev(raw), fmt, shift=shift).cpu().numpy(), want)
    assert np.array_equal(ops.to_gray8(raw, N.PACKED_FORMATS[fmt], shift=shift).cpu().numpy(), want)      # a host array, the code


@pytest.mark.parametrize('fmt', BAYER_FORMATS)
def test_packed_mosaics(fmt):
    """Every packing with one pattern and 12p with all four: the unpack pass into the scratch, then the 8-bit demosaic (generic where
    w % 16 != 0, 16 columns per lane otherwise), alone and in a batch cut from a taller one."""
    from uav_airvision_amd import ops
    rng = np.random.default_rng(75)
    for (w, h) in BAYER_SIZES:
        one = kr.random_frames(rng, fmt, (h, w))
        assert np.array_equal(ops.to_gray8(_dev(one), fmt, shift=7).cpu().numpy(), kr.to_gray8(one, fmt, 7)), (fmt, w, h)
        if w < 752:
            tall = kr.random_frames(rng, fmt, (3, h + 2, w))
            got = ops.to_gray8(_dev(tall)[:, :h], fmt)
            assert tuple(got.shape) == (3, h, w) and np.array_equal(got.cpu().numpy(), kr.to_gray8(tall[:, :h], fmt)), (fmt, w, h)


@pytest.mark.parametrize('fmt', kr.GREY + ('bayer_gbrg10p', 'bayer_rggb12_csi2'))
def test_the_device_agrees_with_the_16_bit_operator_on_the_unpacked_samples(fmt):
    """The same frames as left-justified uint16 through the existing GRAY16 / bayer_*16 kernels, on the device: two paths, one result."""
    from uav_airvision_amd import ops
    rng = np.random.default_rng(76)
    d = kr.depth(fmt)
    wide = 'gray16' if fmt in kr.GREY else 'bayer_%s16' % fmt[6:10]
    for (w, h) in ((36, 6), (260, 66)):
        raw = kr.random_frames(rng, fmt, (2, h, w))
        v16 = (kr.unpack(raw, fmt).astype(np.uint32) << (16 - d)).astype(np.uint16)
        for shift in (3, 8):
            a = ops.to_gray8(_dev(raw), fmt, shift=shift)
            b = ops.to_gray8(_dev(v16), wide, shift=shift)
            assert bool((a == b).all()), (fmt, w, h, shift)


def test_argument_errors_are_invalid_without_a_launch():
    import torch
    from uav_airvision_amd import _native as N, ops
    w, h = 16, 4
    src = torch.zeros(4 * w * h * 2, dtype=torch.uint8, device='cuda')
    dst = torch.full((4 * w * h,), 0x5A, dtype=torch.uint8, device='cuda')
    L = N.lib()

    def call(fmt=N.AV_PIX_GRAY12P, shift=8, ww=w, hh=h, n=2, in_stride=None, out_stride=None, out=None, inp=None):
        fb = N.frame_bytes(fmt, ww, hh)
        return L.av_to_gray8(C.c_void_p(src.data_ptr() if inp is None else inp), fb if in_stride is None else in_stride, n, ww, hh, fmt, shift,
                             C.c_void_p(dst.data_ptr() if out is None else out), ww * hh if out_stride is None else out_stride, N.current_stream())
    fb12, fb10 = w * h * 3 // 2, w * h * 5 // 4
    assert call() == 0 and call(fmt=N.AV_PIX_GRAY10_CSI2) == 0 and call(fmt=N.AV_PIX_BAYER_RGGB12P + 1) == 0
    for kw, text in ((dict(fmt=31), b'pixel format'), (dict(fmt=36), b'pixel format'), (dict(fmt=39), b'pixel format'), (dict(fmt=56), b'pixel format'),
                     (dict(shift=9), b'shift'),
                     (dict(in_stride=fb12 - 1), b'strides'), (dict(fmt=N.AV_PIX_GRAY10P, in_stride=fb10 - 1), b'strides'), (dict(out_stride=w * h - 1), b'strides'),
                     (dict(fmt=N.AV_PIX_GRAY10P, ww=18, in_stride=4096), b'gray10p'), (dict(ww=15, in_stride=4096), b'gray12p'),
                     (dict(fmt=N.AV_PIX_BAYER_RGGB10_CSI2 + 3, ww=6, in_stride=4096), b'bayer_gbrg10_csi2'),
                     (dict(fmt=N.AV_PIX_BAYER_RGGB12P, ww=64, hh=1), b'2 x 2'),
                     (dict(ww=4098, hh=4096, n=0), b'AV_MAX_IMAGE_PIXELS'),
                     (dict(out=src.data_ptr()), b'overlaps'), (dict(out=src.data_ptr() + 2 * fb12 - 1), b'overlaps'),
                     (dict(inp=dst.data_ptr() + w * h - 1, n=1), b'overlaps')):
        torch.cuda.synchronize()
        dst.fill_(0x5A)
        assert call(**kw) == N.AV_E_INVALID, kw
        assert text in L.av_last_error(), (kw, L.av_last_error())
        torch.cuda.synchronize()
        assert bool((dst == 0x5A).all()), kw                                  # nothing ran
    assert call(out=src.data_ptr() + 2 * fb12) == 0                           # right behind the input is fine
    with pytest.raises(ValueError, match='gray12p'):
        ops.to_gray8(torch.zeros((2, 4, 6), dtype=torch.int16, device='cuda'), 'gray12p')
    with pytest.raises(ValueError, match=r'gray10_csi2.*5-byte'):
        ops.to_gray8(torch.zeros((2, 4, 6), dtype=torch.uint8, device='cuda'), 'gray10_csi2')
    with pytest.raises(ValueError, match='out must be'):
        ops.to_gray8(torch.zeros((2, 4, 6), dtype=torch.uint8, device='cuda'), 'gray12p', out=torch.zeros((2, 4, 6), dtype=torch.uint8, device='cuda'))
