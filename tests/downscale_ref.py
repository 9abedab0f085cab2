"""tests/downscale_ref.py -- TEST INFRASTRUCTURE ONLY: the NumPy statement of av_downscale (include/airvision.h): f x f binning of 8-bit
grey images, out = (sum of the block + f * f / 2) >> 2 log2 f, integers only.  The HIP kernels are held to it bit for bit."""
import numpy as np

FACTORS = (2, 4)


def downscale(img, f):
    """uint8 [..., H, W] with H % f == 0 and W % f == 0 -> uint8 [..., H / f, W / f]."""
    if f not in FACTORS:
        raise ValueError('factor %r is neither 2 nor 4' % (f,))
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim < 2 or a.shape[-2] % f or a.shape[-1] % f:
        raise ValueError('uint8 [..., H, W] divisible by %d wanted, got %s %s' % (f, a.dtype, a.shape))
    lead, h, w = a.shape[:-2], a.shape[-2] // f, a.shape[-1] // f
    s = a.reshape(lead + (h, f, w, f)).astype(np.uint32).sum((-3, -1))
    return ((s + f * f // 2) >> (2 * int(np.log2(f)))).astype(np.uint8)


def scaled_intrinsics(intr, f):
    """[fx, fy, cx, cy] of the binned image, in double precision and in the order include/airvision.h gives."""
    fx, fy, cx, cy = [float(v) for v in intr]
    return [fx / f, fy / f, (cx - (f - 1) / 2.0) / f, (cy - (f - 1) / 2.0) / f]
