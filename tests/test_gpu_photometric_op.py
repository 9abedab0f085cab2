"""av_photometric / ops.photometric against the NumPy definition of tests/photometric_ref.py, bit for bit (the arithmetic is integer: the
tolerance is zero by derivation): both bodies, the three table combinations, strides, unaligned bases, in place, the argument errors."""
import ctypes as C

import numpy as np
import pytest

import photometric_ref as pr

pytestmark = pytest.mark.gpu

# (w, h): the smallest shapes that reach every branch -- 256 pixels = 16 whole vectors; 350 = 21 vectors and a ragged end of 14
WHOLE, RAGGED = (64, 4), (50, 7)
PATTERNS = ('random', 'ones', 'zeros', 'ramp')
COMBOS = ('both', 'response', 'gain')


def _images(pattern, n, h, w, seed=0):
    if pattern == 'random':
        return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)
    if pattern == 'ones':
        return np.full((n, h, w), 255, np.uint8)
    if pattern == 'zeros':
        return np.zeros((n, h, w), np.uint8)
    return ((np.arange(n * h * w, dtype=np.int64) * 7) % 256).astype(np.uint8).reshape(n, h, w)      # a ramp that wraps, odd step


def _tables(combo, h, w, seed=1):
    """A gamma-like response with the two extreme entries and a gain map over the whole Q12 range, 0 and 65535 included."""
    rng = np.random.default_rng(seed)
    resp = pr.quantise_response(pr.gamma_inverse_response(2.2))
    resp[255] = pr.RESPONSE_MAX
    gain = rng.integers(2048, 20000, (h, w)).astype(np.uint16)
    gain.reshape(-1)[:4] = [0, 65535, 4096, 1]
    gain.reshape(-1)[-1] = 65535
    return (resp if combo != 'gain' else None), (gain if combo != 'response' else None)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _vector(src, dst, r, g):
    """The launcher's own word on which body a call with these [n, h, w] tensors and tables takes (av_photometric_vector_path)."""
    from uav_airvision_amd import _native as N
    n, h, w = src.shape
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    return bool(N.lib().av_photometric_vector_path(p(src), p(dst), n, w, h, src.stride(0) if n > 1 else h * w, dst.stride(0) if n > 1 else h * w, p(r), p(g)))


@pytest.mark.parametrize('combo', COMBOS)
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('w,h', [WHOLE, RAGGED])
def test_the_vector_body_matches_the_definition(w, h, pattern, combo):
    """n = 3 contiguous images (stride 256 / 350 bytes: 350 is no multiple of 16, so the ragged shape goes byte-wise as a batch and
    through the vector body with its ragged end as single images)."""
    from uav_airvision_amd import ops
    img = _images(pattern, 3, h, w, seed=w)
    resp, gain = _tables(combo, h, w)
    want = pr.correct(img, resp, gain)
    d, r, g = _dev(img), None if resp is None else _dev(resp), None if gain is None else _dev(gain)
    got = ops.photometric(d, r, g)
    assert _vector(d, got, r, g) == ((w, h) == WHOLE)
    assert got.dtype == d.dtype and tuple(got.shape) == (3, h, w) and np.array_equal(got.cpu().numpy(), want)
    d1 = _dev(img[1])                                                                    # one image at an aligned address: no stride applies
    one = ops.photometric(d1, r, g)
    assert _vector(d1.unsqueeze(0), one.unsqueeze(0), r, g) and np.array_equal(one.cpu().numpy(), want[1])
    assert np.array_equal(ops.photometric(img[2], resp, gain).cpu().numpy(), want[2])   # host image, host tables
    if pattern == 'random':
        assert want.std() > 10 and len(np.unique(want)) > 30                             # (the comparison is not vacuous)
        assert not np.array_equal(want, img)


@pytest.mark.parametrize('combo', COMBOS)
@pytest.mark.parametrize('n', [1, 3, 9])
@pytest.mark.parametrize('w,h', [WHOLE, RAGGED])
def test_padded_16_multiple_strides(w, h, n, combo):
    """Strides padded by whole vectors on both sides: the vector body (with its ragged end at 50 x 7), every image at its own place, the
    padding untouched."""
    import torch
    from uav_airvision_amd import ops
    img = _images('random', n, h, w, seed=6 + n)
    resp, gain = _tables(combo, h, w)
    istride = (h * w + 15) // 16 * 16 + 48
    flat = torch.zeros(n * istride, dtype=torch.uint8, device='cuda')
    view = torch.as_strided(flat, (n, h, w), (istride, w, 1))
    view.copy_(_dev(img))
    ostride = (h * w + 15) // 16 * 16 + 32
    oflat = torch.full((n * ostride,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.as_strided(oflat, (n, h, w), (ostride, w, 1))
    r, g = None if resp is None else _dev(resp), None if gain is None else _dev(gain)
    assert ops.photometric(view, r, g, out=out) is out
    assert _vector(view, out, r, g)
    assert np.array_equal(out.cpu().numpy(), pr.correct(img, resp, gain))
    assert (oflat.cpu().numpy().reshape(n, ostride)[:, h * w:] == 0xA5).all()


@pytest.mark.parametrize('combo', COMBOS)
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('w,h', [WHOLE, RAGGED])
def test_the_byte_wise_body(w, h, pattern, combo):
    """An image stride that is no multiple of 16 (nine images), an input and an output base offset by one byte, and a gain base offset
    by two bytes: each goes one pixel per lane."""
    import torch
    from uav_airvision_amd import ops
    n = 9
    img = _images(pattern, n, h, w, seed=5)
    resp, gain = _tables(combo, h, w)
    want = pr.correct(img, resp, gain)
    r, g = None if resp is None else _dev(resp), None if gain is None else _dev(gain)
    flat = torch.zeros(n * (h * w + 3), dtype=torch.uint8, device='cuda')
    view = torch.as_strided(flat, (n, h, w), (h * w + 3, w, 1))
    view.copy_(_dev(img))
    assert view.stride(0) % 16 != 0
    got = ops.photometric(view, r, g)
    assert not _vector(view, got, r, g) and np.array_equal(got.cpu().numpy(), want)
    # an output offset by one byte, its neighbours untouched
    oflat = torch.full((2 * h * w + 2,), 0xA5, dtype=torch.uint8, device='cuda')
    out = oflat[1:1 + 2 * h * w].view(2, h, w)
    assert out.data_ptr() % 16 == 1
    d2 = _dev(img[:2])
    ops.photometric(d2, r, g, out=out)
    assert not _vector(d2, out, r, g) and np.array_equal(out.cpu().numpy(), want[:2])
    assert int(oflat[0]) == 0xA5 and int(oflat[-1]) == 0xA5
    # an input offset by one byte
    iflat = torch.zeros(2 * h * w + 1, dtype=torch.uint8, device='cuda')
    iflat[1:].copy_(d2.view(-1))
    src = iflat[1:].view(2, h, w)
    got = ops.photometric(src, r, g)
    assert not _vector(src, got, r, g) and np.array_equal(got.cpu().numpy(), want[:2])
    # a gain map offset by two bytes: one aligned image, byte-wise all the same
    if g is not None:
        gflat = torch.zeros(h * w + 1, dtype=torch.int16, device='cuda')
        gflat[1:].copy_(g.view(-1))
        g2 = gflat[1:].view(h, w)
        assert g2.data_ptr() % 16 == 2
        one = ops.photometric(d2[0], r, g2)
        assert not _vector(d2[:1], one.unsqueeze(0), r, g2) and _vector(d2[:1], one.unsqueeze(0), r, g)
        assert np.array_equal(one.cpu().numpy(), want[0])


@pytest.mark.parametrize('combo', COMBOS)
def test_extreme_tables(combo):
    """Gain 0 and 65535 everywhere, response 0 and 65280 everywhere: saturation at both ends, and the largest product does not wrap."""
    from uav_airvision_amd import ops
    w, h = RAGGED
    img = _images('ramp', 2, h, w)
    for rv in ((None,) if combo == 'gain' else (0, pr.RESPONSE_MAX)):
        for gv in ((None,) if combo == 'response' else (0, 65535)):
            resp = None if rv is None else np.full(256, rv, np.uint16)
            gain = None if gv is None else np.full((h, w), gv, np.uint16)
            want = pr.correct(img, resp, gain)
            assert np.array_equal(ops.photometric(img, resp, gain).cpu().numpy(), want), (rv, gv)
            if rv == pr.RESPONSE_MAX and gv == 65535:
                assert (want == 255).all()
            if rv == 0 or gv == 0:
                assert (want == 0).all()


@pytest.mark.parametrize('combo', COMBOS)
@pytest.mark.parametrize('w,h', [WHOLE, RAGGED])
def test_in_place(w, h, combo):
    """out = the input itself, as a batch and image by image (50 x 7: byte-wise as a batch and at the odd image addresses, the vector
    body with its ragged end at image 0)."""
    from uav_airvision_amd import ops
    img = _images('random', 3, h, w, seed=8)
    resp, gain = _tables(combo, h, w)
    want = pr.correct(img, resp, gain)
    d = _dev(img)
    assert ops.photometric(d, resp, gain, out=d) is d
    assert np.array_equal(d.cpu().numpy(), want)
    d = _dev(img)
    for i in range(3):
        ops.photometric(d[i], resp, gain, out=d[i])
    assert np.array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize('combo', COMBOS)
def test_one_752_x_480_image(combo):
    """89 workgroups: the last one's lanes past the image do nothing."""
    from uav_airvision_amd import ops
    w, h = 752, 480
    img = _images('random', 1, h, w, seed=2)
    resp, gain = _tables(combo, h, w)
    d, r, g = _dev(img), None if resp is None else _dev(resp), None if gain is None else _dev(gain)
    got = ops.photometric(d, r, g)
    assert _vector(d, got, r, g)
    assert np.array_equal(got.cpu().numpy(), pr.correct(img, resp, gain))


def test_argument_errors_are_invalid_without_a_launch():
    import torch
    from uav_airvision_amd import _native as N, ops
    w, h = WHOLE
    src = torch.zeros(4 * w * h, dtype=torch.uint8, device='cuda')
    dst = torch.full((4 * w * h,), 0x5A, dtype=torch.uint8, device='cuda')
    resp = _dev((np.arange(256) * 256).astype(np.uint16))
    bad = _dev(np.r_[np.zeros(255), pr.RESPONSE_MAX + 1].astype(np.uint16))
    gain = _dev(np.full((h, w), 8192, np.uint16))
    L = N.lib()

    def call(ww=w, hh=h, n=2, in_stride=None, out_stride=None, out=-1, inp=-1, r=resp, g=gain):
        return L.av_photometric(C.c_void_p(src.data_ptr() if inp == -1 else inp), C.c_void_p(dst.data_ptr() if out == -1 else out), n, ww, hh,
                                ww * hh if in_stride is None else in_stride, ww * hh if out_stride is None else out_stride,
                                None if r is None else C.c_void_p(r.data_ptr()), None if g is None else C.c_void_p(g.data_ptr()), N.current_stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((dst[:2 * w * h] == 0).all()) and bool((dst[2 * w * h:] == 0x5A).all())
    dst.fill_(0x5A)
    assert call(n=0) == N.AV_OK
    for kw, text in ((dict(r=None, g=None), b'both null'), (dict(r=bad), b'65280'), (dict(r=bad, g=None), b'65280'),
                     (dict(out=src.data_ptr() + 16), b'overlaps'), (dict(out=src.data_ptr() + 2 * w * h - 1), b'overlaps'),
                     (dict(out=src.data_ptr(), out_stride=w * h + 16), b'overlaps'),
                     (dict(ww=4098, hh=4096, n=0), b'AV_MAX_IMAGE_PIXELS'), (dict(ww=0), b'AV_MAX_IMAGE_PIXELS'),
                     (dict(in_stride=w * h - 1), b'bad arguments'), (dict(out_stride=w * h - 1), b'bad arguments'),
                     (dict(inp=None), b'bad arguments'), (dict(out=None), b'bad arguments'), (dict(n=-1), b'bad arguments')):
        torch.cuda.synchronize()
        dst.fill_(0x5A)
        src.zero_()
        assert call(**kw) == N.AV_E_INVALID, kw
        assert text in L.av_last_error(), (kw, L.av_last_error())
        torch.cuda.synchronize()
        assert bool((dst == 0x5A).all()) and bool((src == 0).all()), kw                  # nothing ran
    assert call(out=src.data_ptr() + 2 * w * h) == 0                                     # right behind the input is fine
    assert call(out=src.data_ptr()) == 0                                                 # and so is the input itself
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='neither'):
        ops.photometric(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='uint8'):
        ops.photometric(torch.zeros((2, 4, 4), dtype=torch.int16, device='cuda'), resp)
    with pytest.raises(ValueError, match='gain'):
        ops.photometric(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), None, np.zeros((4, 5), np.uint16))
    with pytest.raises(ValueError, match='response'):
        ops.photometric(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), np.zeros(256, np.float32))
    with pytest.raises(ValueError, match='out must be'):
        ops.photometric(torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda'), resp, out=torch.zeros((2, 4, 5), dtype=torch.uint8, device='cuda'))
