"""av_downscale / ops.downscale against the NumPy definition of tests/downscale_ref.py, bit for bit (the arithmetic is integer: the
tolerance is zero by derivation): both kernels, both factors, strides, an unaligned base, the smallest sizes, the argument errors."""
import ctypes as C

import numpy as np
import pytest

import downscale_ref as dr

pytestmark = pytest.mark.gpu

# (W, H, f): the smallest shapes that reach every branch -- output widths 32 (whole vectors) and 25 / 9 (one pixel per lane)
VECTOR = [(64, 32, 2), (128, 16, 4)]
GENERIC = [(50, 6, 2), (36, 8, 4)]
PATTERNS = ('random', 'ones', 'zeros', 'ramp')


def _images(pattern, n, H, W, seed=0):
    if pattern == 'random':
        return np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    if pattern == 'ones':
        return np.full((n, H, W), 255, np.uint8)
    if pattern == 'zeros':
        return np.zeros((n, H, W), np.uint8)
    return ((np.arange(n * H * W, dtype=np.int64) * 7) % 256).astype(np.uint8).reshape(n, H, W)      # a ramp that wraps, odd step


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vector(src, dst, f):
    """The launcher's own word on which kernel a call with these [n, H, W] / [n, h, w] tensors takes (av_downscale_vector_path)."""
    from uav_airvision_amd import _native as N
    n, H, W = src.shape
    return bool(N.lib().av_downscale_vector_path(C.c_void_p(src.data_ptr()), src.stride(0) if n > 1 else H * W, n, W, f,
                                                 C.c_void_p(dst.data_ptr()), dst.stride(0) if n > 1 else dst[0].numel()))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H,f', VECTOR + GENERIC)
def test_both_paths_match_the_definition(W, H, f, pattern):
    from uav_airvision_amd import ops
    img = _images(pattern, 3, H, W, seed=W + f)
    want = dr.downscale(img, f)
    d = _dev(img)
    got = ops.downscale(d, f)
    assert _vector(d, got, f) == ((W, H, f) in VECTOR)                                      # the case reaches the kernel it is named for
    assert tuple(got.shape) == (3, H // f, W // f) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.downscale(img[1], f).cpu().numpy(), want[1])                 # one host image, [H, W]
    if pattern == 'random':
        assert want.std() > 10 and len(np.unique(want)) > 30                                # (the comparison is not vacuous)


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H,f', VECTOR + GENERIC)
def test_a_batch_with_an_input_stride_that_is_no_multiple_of_16(W, H, f, pattern):
    """Nine images cut out of a taller tensor whose image stride is odd: every image goes one pixel per lane."""
    import torch
    from uav_airvision_amd import ops
    n = 9
    img = _images(pattern, n, H, W, seed=5)
    flat = torch.zeros(n * (H * W + 3), dtype=torch.uint8, device='cuda')
    view = torch.as_strided(flat, (n, H, W), (H * W + 3, W, 1))
    view.copy_(_dev(img))
    assert view.stride(0) % 16 != 0
    got = ops.downscale(view, f)
    assert not _vector(view, got, f)
    assert np.array_equal(got.cpu().numpy(), dr.downscale(img, f))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H,f', VECTOR + GENERIC)
def test_a_batch_with_padded_16_multiple_strides(W, H, f, pattern):
    """Nine images (more than eight) with input and output strides padded by whole vectors: the vector path where the width allows
    it, every image at its own place, the padding untouched."""
    import torch
    from uav_airvision_amd import ops
    n, h, w = 9, H // f, W // f
    img = _images(pattern, n, H, W, seed=6)
    flat = torch.zeros(n * (H * W + 48), dtype=torch.uint8, device='cuda')
    view = torch.as_strided(flat, (n, H, W), (H * W + 48, W, 1))
    view.copy_(_dev(img))
    ostride = (h * w + 15) // 16 * 16 + 32
    oflat = torch.full((n * ostride,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.as_strided(oflat, (n, h, w), (ostride, w, 1))
    assert ops.downscale(view, f, out=out) is out
    assert _vector(view, out, f) == ((W, H, f) in VECTOR)
    assert np.array_equal(out.cpu().numpy(), dr.downscale(img, f))
    pad = oflat.cpu().numpy().reshape(n, ostride)[:, h * w:]
    assert (pad == 0xA5).all()


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('W,H,f', VECTOR + GENERIC)
def test_an_output_offset_by_one_byte(W, H, f, pattern):
    import torch
    from uav_airvision_amd import ops
    n, h, w = 2, H // f, W // f
    img = _images(pattern, n, H, W, seed=7)
    oflat = torch.full((n * h * w + 2,), 0xA5, dtype=torch.uint8, device='cuda')
    out = oflat[1:1 + n * h * w].view(n, h, w)
    assert out.data_ptr() % 16 == 1
    d = _dev(img)
    ops.downscale(d, f, out=out)
    assert not _vector(d, out, f)
    assert np.array_equal(out.cpu().numpy(), dr.downscale(img, f))
    assert int(oflat[0]) == 0xA5 and int(oflat[-1]) == 0xA5
    # and an input offset by one byte
    iflat = torch.zeros(n * H * W + 1, dtype=torch.uint8, device='cuda')
    iflat[1:].copy_(_dev(img).view(-1))
    assert np.array_equal(ops.downscale(iflat[1:].view(n, H, W), f).cpu().numpy(), dr.downscale(img, f))


@pytest.mark.parametrize('f', [2, 4])
def test_the_smallest_size(f):
    from uav_airvision_amd import ops
    for pattern in PATTERNS:
        img = _images(pattern, 1, f, f, seed=f)
        got = ops.downscale(_dev(img), f)
        assert tuple(got.shape) == (1, 1, 1) and np.array_equal(got.cpu().numpy(), dr.downscale(img, f)), pattern


def test_several_blocks_per_image():
    """More than one workgroup per image in either path (vector: 32 x 144 vectors of 16; generic: 250 x 40 pixels > 4096)."""
    from uav_airvision_amd import ops
    for W, H, f in ((1024, 288, 2), (500, 80, 2), (2048, 160, 4), (1000, 160, 4)):
        img = _images('random', 2, H, W, seed=W)
        assert np.array_equal(ops.downscale(_dev(img), f).cpu().numpy(), dr.downscale(img, f)), (W, H, f)


def test_no_image_is_ok_and_argument_errors_are_invalid_without_a_launch():
    import torch
    from uav_airvision_amd import _native as N, ops
    W, H, f = 64, 8, 2
    src = torch.zeros(4 * W * H, dtype=torch.uint8, device='cuda')
    dst = torch.full((4 * W * H,), 0x5A, dtype=torch.uint8, device='cuda')
    L = N.lib()

    def call(ww=W, hh=H, ff=f, n=2, in_stride=None, out_stride=None, out=-1, inp=-1):
        return L.av_downscale(C.c_void_p(src.data_ptr() if inp == -1 else inp), ww * hh if in_stride is None else in_stride, n, ww, hh, ff,
                              C.c_void_p(dst.data_ptr() if out == -1 else out), (ww // max(ff, 1)) * (hh // max(ff, 1)) if out_stride is None else out_stride,
                              N.current_stream())
    assert call() == 0
    torch.cuda.synchronize()
    dst.fill_(0x5A)
    assert call(n=0) == N.AV_OK
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    for kw, text in ((dict(ff=3), b'factor'), (dict(ff=1), b'factor'), (dict(ff=8), b'factor'), (dict(ff=0), b'factor'), (dict(ff=-2), b'factor'),
                     (dict(ww=62, ff=4), b'divisible'), (dict(hh=7), b'divisible'), (dict(ww=63), b'divisible'),
                     (dict(ww=4098, hh=4096, n=0), b'AV_MAX_IMAGE_PIXELS'), (dict(ww=0), b'AV_MAX_IMAGE_PIXELS'), (dict(hh=-2), b'AV_MAX_IMAGE_PIXELS'),
                     (dict(in_stride=W * H - 1), b'strides'), (dict(out_stride=W * H // 4 - 1), b'strides'),
                     (dict(inp=None), b'bad arguments'), (dict(out=None), b'bad arguments'), (dict(n=-1), b'bad arguments'),
                     (dict(out=src.data_ptr()), b'overlaps'), (dict(out=src.data_ptr() + 2 * W * H - 1), b'overlaps'),
                     (dict(inp=dst.data_ptr() + W * H // 4 - 1, n=1), b'overlaps')):
        torch.cuda.synchronize()
        dst.fill_(0x5A)
        assert call(**kw) == N.AV_E_INVALID, kw
        assert text in L.av_last_error(), (kw, L.av_last_error())
        torch.cuda.synchronize()
        assert bool((dst == 0x5A).all()), kw                                  # nothing ran
    assert call(out=src.data_ptr() + 2 * W * H) == 0                          # right behind the input is fine
    with pytest.raises(ValueError, match='factor'):
        ops.downscale(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), 3)
    with pytest.raises(ValueError, match='factor'):
        ops.downscale(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), True)
    with pytest.raises(ValueError, match='divisible'):
        ops.downscale(torch.zeros((2, 6, 8), dtype=torch.uint8, device='cuda'), 4)
    with pytest.raises(ValueError, match='uint8'):
        ops.downscale(torch.zeros((2, 4, 4), dtype=torch.int16, device='cuda'), 2)
    with pytest.raises(ValueError, match='out must be'):
        ops.downscale(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), 2, out=torch.zeros((2, 2, 3), dtype=torch.uint8, device='cuda'))
