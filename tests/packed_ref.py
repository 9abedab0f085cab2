"""tests/packed_ref.py -- TEST INFRASTRUCTURE ONLY: the packed 10 / 12-bit transports of include/airvision.h ("Packed 10 / 12-bit
transports") in NumPy, byte by byte as the table there writes them.  The kernel, the engine and the package's own pack_frames /
unpack_frames are held to this bit for bit.
  10p      4 px = 5 B   p0[7:0], p1[5:0]<<2 | p0[9:8], p2[3:0]<<4 | p1[9:6], p3[1:0]<<6 | p2[9:4], p3[9:2]
  12p      2 px = 3 B   p0[7:0], p1[3:0]<<4 | p0[11:8], p1[11:4]
  10_csi2  4 px = 5 B   p0[9:2], p1[9:2], p2[9:2], p3[9:2], p3[1:0]<<6 | p2[1:0]<<4 | p1[1:0]<<2 | p0[1:0]
  12_csi2  2 px = 3 B   p0[11:4], p1[11:4], p1[3:0]<<4 | p0[3:0]
  value    s = min(255, (v << (16 - d)) >> shift); grey formats stop there, mosaics are the 8-bit mosaic of their s values."""
import numpy as np

import bayer_ref as br

PACKINGS = ('10p', '12p', '10_csi2', '12_csi2')
GREY = tuple('gray' + k for k in PACKINGS)
BAYER = tuple('bayer_%s%s' % (p, k) for k in PACKINGS for p in br.PATTERNS)
FORMATS = GREY + BAYER
CODES = dict([(f, 32 + i) for i, f in enumerate(GREY)] + [(f, 40 + i) for i, f in enumerate(BAYER)])


def packing(fmt):
    """'gray12p' / 'bayer_rggb12p' -> '12p'."""
    if fmt not in FORMATS:
        raise ValueError('unknown packed format %r' % (fmt,))
    return fmt[4:] if fmt.startswith('gray') else fmt[10:]


def depth(fmt):
    return 10 if packing(fmt).startswith('10') else 12


def group(fmt):
    """(samples, bytes) of one group."""
    return (4, 5) if depth(fmt) == 10 else (2, 3)


def row_bytes(fmt, w):
    gpx, gb = group(fmt)
    if w <= 0 or w % gpx:
        raise ValueError('%s: width %d is not whole groups of %d samples' % (fmt, w, gpx))
    return w // gpx * gb


def pack(v, fmt):
    """Right-aligned samples uint16 [..., h, w] -> uint8 [..., h, w * d / 8]."""
    v = np.asarray(v)
    assert v.dtype == np.uint16
    d, (gpx, gb) = depth(fmt), group(fmt)
    wb = row_bytes(fmt, v.shape[-1])
    if v.size and int(v.max()) >= 1 << d:
        raise ValueError('%s: sample %d is not below 2^%d' % (fmt, int(v.max()), d))
    p = [v[..., j::gpx].astype(np.int64) for j in range(gpx)]
    k = packing(fmt)
    if k == '10p':
        b = [p[0] & 255, (p[1] & 63) << 2 | p[0] >> 8, (p[2] & 15) << 4 | p[1] >> 6, (p[3] & 3) << 6 | p[2] >> 4, p[3] >> 2]
    elif k == '12p':
        b = [p[0] & 255, (p[1] & 15) << 4 | p[0] >> 8, p[1] >> 4]
    elif k == '10_csi2':
        b = [p[0] >> 2, p[1] >> 2, p[2] >> 2, p[3] >> 2, (p[3] & 3) << 6 | (p[2] & 3) << 4 | (p[1] & 3) << 2 | (p[0] & 3)]
    else:
        b = [p[0] >> 4, p[1] >> 4, (p[1] & 15) << 4 | (p[0] & 15)]
    out = np.empty(v.shape[:-1] + (wb,), np.uint8)
    for i in range(gb):
        out[..., i::gb] = b[i]
    return out


def unpack(raw, fmt):
    """uint8 [..., h, w * d / 8] -> right-aligned samples uint16 [..., h, w]."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8
    gpx, gb = group(fmt)
    if raw.shape[-1] == 0 or raw.shape[-1] % gb:
        raise ValueError('%s: a row of %d bytes is not whole groups of %d' % (fmt, raw.shape[-1], gb))
    b = [raw[..., i::gb].astype(np.int64) for i in range(gb)]
    k = packing(fmt)
    if k == '10p':
        p = [b[0] | (b[1] & 3) << 8, b[1] >> 2 | (b[2] & 15) << 6, b[2] >> 4 | (b[3] & 63) << 4, b[3] >> 6 | b[4] << 2]
    elif k == '12p':
        p = [b[0] | (b[1] & 15) << 8, b[1] >> 4 | b[2] << 4]
    elif k == '10_csi2':
        p = [b[j] << 2 | (b[4] >> (2 * j)) & 3 for j in range(4)]
    else:
        p = [b[j] << 4 | (b[2] >> (4 * j)) & 15 for j in range(2)]
    out = np.empty(raw.shape[:-1] + (raw.shape[-1] // gb * gpx,), np.uint16)
    for j in range(gpx):
        out[..., j::gpx] = p[j]
    return out


def reduce8(raw, fmt, shift=8):
    """The value rule on every sample: uint8 [..., h, w] of s = min(255, (v << (16 - d)) >> shift)."""
    if not (isinstance(shift, (int, np.integer)) and 0 <= shift <= 8):
        raise ValueError('shift %r outside 0 .. 8' % (shift,))
    v = unpack(raw, fmt).astype(np.int64)
    return np.minimum(255, (v << (16 - depth(fmt))) >> shift).astype(np.uint8)


def to_gray8(raw, fmt, shift=8):
    """Packed frames uint8 [..., h, w * d / 8] -> uint8 [..., h, w]: the reduced samples for the grey formats, steps 2 - 4 of the Bayer
    definition (bayer_ref) on the reduced 8-bit mosaic for the mosaics."""
    s = reduce8(raw, fmt, shift)
    if fmt in GREY:
        return s
    return br.to_gray8(s, 'bayer_%s8' % fmt[6:10])


def random_frames(rng, fmt, shape):
    """Random packed frames for sample shape (..., h, w): every bit of every sample used."""
    return pack(rng.integers(0, 1 << depth(fmt), shape, dtype=np.uint16), fmt)
