"""tests/pixfmt_ref.py -- TEST INFRASTRUCTURE ONLY: the pixel-format conversion of include/airvision.h (av_to_gray8) in NumPy.  The
kernel, the engine and the sweep are held to this bit for bit.
  GRAY16:  min(255, v >> shift), shift 0 .. 8 (truncates)
  colour:  (9798 R + 19235 G + 3735 B + 16384) >> 15, integers; alpha ignored
  GRAY8:   the identity"""
import numpy as np

FORMATS = ('gray8', 'gray16', 'rgb8', 'bgr8', 'rgba8', 'bgra8')
BYTES = dict(gray8=1, gray16=2, rgb8=3, bgr8=3, rgba8=4, bgra8=4)


def to_gray8(img, fmt, shift=8):
    """img: uint8 [..., h, w] (gray8), uint16 [..., h, w] (gray16), uint8 [..., h, w, 3 | 4] (colour) -> uint8 [..., h, w]."""
    a = np.asarray(img)
    if fmt not in FORMATS:
        raise ValueError('unknown format %r' % (fmt,))
    if not (isinstance(shift, (int, np.integer)) and 0 <= shift <= 8):
        raise ValueError('shift %r outside 0 .. 8' % (shift,))
    if fmt == 'gray8':
        assert a.dtype == np.uint8
        return a.copy()
    if fmt == 'gray16':
        assert a.dtype == np.uint16
        return np.minimum(255, a.astype(np.int64) >> shift).astype(np.uint8)
    assert a.dtype == np.uint8 and a.shape[-1] == BYTES[fmt]
    c = a.astype(np.int64)
    r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if fmt.startswith('bgr') else (c[..., 0], c[..., 1], c[..., 2])
    return ((9798 * r + 19235 * g + 3735 * b + 16384) >> 15).astype(np.uint8)


def random_frames(rng, fmt, shape):
    """Random frames of a format, shape = (..., h, w): every bit of every sample used."""
    if fmt == 'gray16':
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    if fmt == 'gray8':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.integers(0, 256, tuple(shape) + (BYTES[fmt],), dtype=np.uint8)
