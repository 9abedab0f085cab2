"""tests/range16_ref.py -- TEST INFRASTRUCTURE ONLY: the NumPy statement of "Range scaling of 16-bit grey" (include/airvision.h), which
the kernels of csrc/range16.hip either match bit for bit or are wrong.  Integer arithmetic only (Python ints and int64 arrays).

    mapping   m = ((255 << 16) + span // 2) // span;  d = min(max(v, lo), hi) - lo;  out = min(255, (d * m + 32768) >> 16)
    auto      a 4,096-bin histogram of v >> 4 over a GROUP (the `pool` = 1 or 2 images of a stereo pair, pooled), N its samples,
              k_lo = N * ppm_lo // 10**6, k_hi = N * ppm_hi // 10**6;  b_lo = the smallest bin with hist[0 .. b_lo].sum() > k_lo,
              b_hi = the largest bin with hist[b_hi .. 4095].sum() > k_hi;  lo = 16 * b_lo, hi = 16 * b_hi + 15
    widening  if hi - lo < min_span:  need = min_span - (hi - lo);  lo = max(0, min(lo - need // 2, 65535 - min_span));  hi = lo + min_span
              The new range always contains the old one: lo only moves down, and hi = lo + min_span is at least the old hi in each of
              the three cases (lo - need // 2: old hi + need - need // 2; the clamp at 0: old hi < need // 2 + old span <= min_span; the
              clamp at 65535 - min_span: 65535).  tests/test_range16_ref.py checks it over every case."""
import numpy as np

BINS = 4096
DEFAULT_CLIP = (100, 100)
DEFAULT_MIN_SPAN = 256
MAX_CLIP_PPM = 500000


def multiplier(lo, hi):
    span = int(hi) - int(lo)
    assert 0 <= lo < hi <= 65535
    return ((255 << 16) + span // 2) // span


def apply(v, lo, hi):
    """uint16 array -> uint8 array of the same shape through the window (lo, hi)."""
    m = multiplier(lo, hi)
    d = np.minimum(np.maximum(np.asarray(v).astype(np.int64), int(lo)), int(hi)) - int(lo)
    return np.minimum(255, (d * m + 32768) >> 16).astype(np.uint8)


def clip_counts(n_samples, clip=DEFAULT_CLIP):
    ppm_lo, ppm_hi = [int(c) for c in clip]
    assert ppm_lo >= 0 and ppm_hi >= 0 and ppm_lo + ppm_hi <= MAX_CLIP_PPM
    return int(n_samples) * ppm_lo // 10 ** 6, int(n_samples) * ppm_hi // 10 ** 6


def histogram_range(group, clip=DEFAULT_CLIP):
    """(lo, hi) of one group before the minimum-span rule."""
    g = np.asarray(group)
    assert g.dtype == np.uint16 and g.size > 0
    hist = np.bincount((g >> 4).reshape(-1).astype(np.int64), minlength=BINS)
    k_lo, k_hi = clip_counts(g.size, clip)
    c = 0
    for b_lo in range(BINS):
        c += int(hist[b_lo])
        if c > k_lo:
            break
    c = 0
    for b_hi in range(BINS - 1, -1, -1):
        c += int(hist[b_hi])
        if c > k_hi:
            break
    return 16 * b_lo, 16 * b_hi + 15


def widen(lo, hi, min_span=DEFAULT_MIN_SPAN):
    assert 16 <= min_span <= 65535
    if hi - lo < min_span:
        need = min_span - (hi - lo)
        lo = max(0, min(lo - need // 2, 65535 - min_span))
        hi = lo + min_span
    return lo, hi


def auto_range(group, clip=DEFAULT_CLIP, min_span=DEFAULT_MIN_SPAN):
    return widen(*histogram_range(group, clip), min_span=min_span)


def to_gray8(frames, scale='auto', window=None, clip=DEFAULT_CLIP, min_span=DEFAULT_MIN_SPAN, pool=1):
    """frames uint16 [n, h, w] in groups of `pool` consecutive images -> (uint8 [n, h, w], int32 [n // pool, 2] of (lo, hi))."""
    a = np.asarray(frames)
    assert a.dtype == np.uint16 and a.ndim == 3 and pool in (1, 2) and a.shape[0] % pool == 0 and scale in ('window', 'auto')
    out = np.empty(a.shape, np.uint8)
    ranges = np.empty((a.shape[0] // pool, 2), np.int32)
    for g in range(a.shape[0] // pool):
        grp = a[g * pool:(g + 1) * pool]
        lo, hi = (int(window[0]), int(window[1])) if scale == 'window' else auto_range(grp, clip, min_span)
        out[g * pool:(g + 1) * pool] = apply(grp, lo, hi)
        ranges[g] = (lo, hi)
    return out, ranges


def pair_to_gray8(img0, img1, **kw):
    """One stereo pair, pooled: (grey cam0, grey cam1, (lo, hi))."""
    out, ranges = to_gray8(np.stack([img0, img1]), pool=2, **kw)
    return out[0], out[1], (int(ranges[0, 0]), int(ranges[0, 1]))
