"""tests/bayer_ref.py -- TEST INFRASTRUCTURE ONLY: the Bayer-mosaic conversion of include/airvision.h (av_to_gray8, "Bayer mosaics") in
NumPy.  The kernels, the engine and the sweep are held to this bit for bit.
  1. reduce    8-bit s = v; 16-bit s = min(255, v >> shift), before anything else
  2. extend    BORDER_REFLECT_101 (index -1 reads 1, index w reads w - 2)
  3. channels  c, hs (row neighbours), vs (column neighbours), ds (diagonal neighbours):
               R site R4 = 4c, G4 = hs + vs, B4 = ds; B site B4 = 4c, G4 = hs + vs, R4 = ds;
               G site with R row neighbours G4 = 4c, R4 = 2 hs, B4 = 2 vs; G site with B row neighbours G4 = 4c, B4 = 2 hs, R4 = 2 vs
  4. grey      (9798 R4 + 19235 G4 + 3735 B4 + 65536) >> 17
A pattern is named by the colours of the top-left 2 x 2 block in reading order."""
import numpy as np

PATTERNS = ('rggb', 'bggr', 'grbg', 'gbrg')
FORMATS = tuple('bayer_%s%d' % (p, b) for b in (8, 16) for p in PATTERNS)
CODES = {f: 16 + i for i, f in enumerate(FORMATS)}
BYTES = {f: 2 if f.endswith('16') else 1 for f in FORMATS}
GAINS = (0.8, 1.0, 0.6)


def site_colours(pattern, h, w):
    """[h, w] of 'r' / 'g' / 'b' codes 0 / 1 / 2: site (x, y) has the colour pattern[2 * (y & 1) + (x & 1)]."""
    block = np.array(['rgb'.index(ch) for ch in pattern]).reshape(2, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    return block[yy & 1, xx & 1]


def to_gray8(img, fmt, shift=8):
    """img: uint8 [..., h, w] ('bayer_*8') or uint16 [..., h, w] ('bayer_*16') -> uint8 [..., h, w]."""
    if fmt not in FORMATS:
        raise ValueError('unknown format %r' % (fmt,))
    if not (isinstance(shift, (int, np.integer)) and 0 <= shift <= 8):
        raise ValueError('shift %r outside 0 .. 8' % (shift,))
    a = np.asarray(img)
    assert a.dtype == (np.uint16 if BYTES[fmt] == 2 else np.uint8), a.dtype
    if a.ndim < 2 or a.shape[-1] < 2 or a.shape[-2] < 2:
        raise ValueError('a Bayer mosaic is at least 2 x 2 samples, got %s' % (tuple(a.shape),))
    h, w = a.shape[-2:]
    s = a.astype(np.int64)
    if BYTES[fmt] == 2:
        s = np.minimum(255, s >> shift)
    p = np.pad(s, [(0, 0)] * (s.ndim - 2) + [(1, 1), (1, 1)], mode='reflect')
    c = p[..., 1:-1, 1:-1]
    hs = p[..., 1:-1, :-2] + p[..., 1:-1, 2:]
    vs = p[..., :-2, 1:-1] + p[..., 2:, 1:-1]
    ds = p[..., :-2, :-2] + p[..., :-2, 2:] + p[..., 2:, :-2] + p[..., 2:, 2:]
    col = site_colours(fmt[6:10], h, w)
    row_r = (col == 0).any(axis=1)[:, None]                   # rows that hold the R sites: their G sites have R row neighbours
    is_r, is_b, is_g = col == 0, col == 2, col == 1
    g_r, g_b = is_g & row_r, is_g & ~row_r
    r4 = np.where(is_r, 4 * c, np.where(is_b, ds, np.where(g_r, 2 * hs, 2 * vs)))
    b4 = np.where(is_b, 4 * c, np.where(is_r, ds, np.where(g_b, 2 * hs, 2 * vs)))
    g4 = np.where(is_g, 4 * c, hs + vs)
    return ((9798 * r4 + 19235 * g4 + 3735 * b4 + 65536) >> 17).astype(np.uint8)


def mosaic(gray, fmt, gains=GAINS, shift=8):
    """An 8-bit grey frame as the raw mosaic of a scene with R, G, B = grey x gains: rint(g * gain at the site), clipped; the 16-bit
    formats hold that value << shift."""
    g = np.asarray(gray, np.uint8)
    gain = np.asarray(gains, np.float64)[site_colours(fmt[6:10], g.shape[-2], g.shape[-1])]
    m = np.clip(np.rint(g.astype(np.float64) * gain), 0, 255).astype(np.uint8)
    return m.astype(np.uint16) << shift if BYTES[fmt] == 2 else m


def random_frames(rng, fmt, shape, kind='full'):
    """Random mosaics, shape = (..., h, w).  kind 'full': every bit of every sample used; 'ends': samples concentrated at the two ends
    of the 8-bit range after reduction (0, 1, 254, 255 and, for 16-bit data, values that saturate)."""
    wide = BYTES[fmt] == 2
    if kind == 'full':
        return rng.integers(0, 65536 if wide else 256, shape, dtype=np.uint16 if wide else np.uint8)
    pick = rng.choice(np.array([0, 1, 254, 255, 255, 0]), size=shape)
    if wide:
        return np.where(rng.random(shape) < 0.2, 65535, pick << 4 | rng.integers(0, 16, shape)).astype(np.uint16)      # for shift 4
    return pick.astype(np.uint8)
