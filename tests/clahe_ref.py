"""tests/clahe_ref.py -- TEST INFRASTRUCTURE ONLY (like tests/ransac_ref.py).

Plain NumPy restatement of the contrast-limited adaptive histogram equalisation specified in include/airvision.h (av_clahe): integer
histograms, clip and redistribution in Python integers, and the few float32 operations per pixel as float32 NumPy operations in the
order the header gives (NumPy never fuses a multiply with an add), so the kernels can be held to it bit for bit.
"""
import numpy as np

F = np.float32


def padded(img, tiles):
    """The image extended right / bottom to whole tiles with BORDER_REFLECT_101, each axis only if it is ragged; (padded, tw, th)."""
    h, w = img.shape
    tx, ty = tiles
    pw = tx - w % tx if w % tx else 0
    ph = ty - h % ty if h % ty else 0

    def refl(p, n):                       # cv::borderInterpolate(p, n, BORDER_REFLECT_101) for any overshoot
        if n == 1:
            return 0
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * n - 2 - p
        return p
    ys = [refl(y, h) for y in range(h + ph)]
    xs = [refl(x, w) for x in range(w + pw)]
    ext = img[np.ix_(ys, xs)]
    return ext, (w + pw) // tx, (h + ph) // ty


def clip_value(clip_limit, area):
    if clip_limit <= 0:
        return 0
    return max(1, int(clip_limit * area / 256))


def redistribute(hist, clip):
    """Step 2 of the header on a list of 256 Python ints; returns the new list."""
    hist = [int(v) for v in hist]
    clipped = 0
    for i in range(256):
        if hist[i] > clip:
            clipped += hist[i] - clip
            hist[i] = clip
    batch = clipped // 256
    residual = clipped - 256 * batch
    hist = [v + batch for v in hist]
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    return hist


def round_u8(a):
    """saturate_u8(round half to even) of a float32 array."""
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def tile_lut(tile, clip_limit):
    area = tile.size
    hist = np.bincount(tile.reshape(-1), minlength=256).tolist()
    clip = clip_value(clip_limit, area)
    if clip > 0:
        hist = redistribute(hist, clip)
    scale = F(255.0) / F(area)
    cum = np.cumsum(np.array(hist, dtype=np.int64))
    return round_u8(cum.astype(F) * scale)


def luts(img, clip_limit=2.0, tiles=(8, 8)):
    """uint8 [tiles_y * tiles_x, 256]"""
    ext, tw, th = padded(img, tiles)
    tx, ty = tiles
    out = np.zeros((ty * tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            out[j * tx + i] = tile_lut(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw], clip_limit)
    return out


def _axis(n, t, tiles_n):
    """(index 1, index 2, weight of 2, weight of 1) per coordinate, float32 as the header writes it."""
    inv = F(1.0) / F(t)
    f = np.arange(n, dtype=F) * inv - F(0.5)
    fl = np.floor(f)
    a = (f - fl).astype(F)
    a1 = (F(1.0) - a).astype(F)
    i1 = fl.astype(np.int64)
    i2 = i1 + 1
    return np.maximum(i1, 0), np.minimum(i2, tiles_n - 1), a, a1


def clahe(img, clip_limit=2.0, tiles=(8, 8), return_lut=False):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 2
    h, w = img.shape
    tx, ty = tiles
    _ext, tw, th = padded(img, tiles)
    lut = luts(img, clip_limit, tiles).reshape(ty, tx, 256).astype(F)
    x1, x2, xa, xa1 = _axis(w, tw, tx)
    y1, y2, ya, ya1 = _axis(h, th, ty)
    Y1, Y2, YA, YA1 = y1[:, None], y2[:, None], ya[:, None], ya1[:, None]
    X1, X2, XA, XA1 = x1[None, :], x2[None, :], xa[None, :], xa1[None, :]
    top = lut[Y1, X1, img] * XA1 + lut[Y1, X2, img] * XA
    bot = lut[Y2, X1, img] * XA1 + lut[Y2, X2, img] * XA
    res = top * YA1 + bot * YA
    assert res.dtype == F
    out = round_u8(res)
    return (out, lut.astype(np.uint8).reshape(ty * tx, 256)) if return_lut else out


def seeded_image(seed, w, h, lo=0, hi=256, smooth=True):
    """A test image with structure at several scales: blocks of random level plus noise, values inside [lo, hi)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(lo, hi, (h, w)).astype(np.float64)
    if smooth:
        coarse = rng.integers(lo, hi, ((h + 31) // 32, (w + 31) // 32)).astype(np.float64)
        img = 0.35 * img + 0.65 * np.kron(coarse, np.ones((32, 32)))[:h, :w]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
