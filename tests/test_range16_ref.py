"""The NumPy reference of the 16-bit range scaling (tests/range16_ref.py) against the definition's own properties, none of them checked
through the reference's code: exact integer arithmetic for the mapping, a brute-force sort for the percentiles, every case of the
widening rule.  Also the product's NumPy helper, frontend.gray16_range, against the reference, and the settings' refusals.  No GPU."""
import numpy as np
import pytest

import range16_ref as rr

ALL_SPANS = np.arange(1, 65536, dtype=np.int64)
# every d of a span is walked for: every span up to 4096, every 61st above, and the last 64 (2.6e7 values in all); every span is
# checked at its end points and for the bounds that do not depend on d
SWEPT_SPANS = sorted(set(range(1, 4097)) | set(range(4097, 65536, 61)) | set(range(65472, 65536)))


def _m(span):
    return ((255 << 16) + span // 2) // span


def test_end_points_and_the_32_bit_bound_for_every_span():
    m = ((255 << 16) + ALL_SPANS // 2) // ALL_SPANS
    assert m.min() >= 255 and m.max() == 255 << 16                           # span 65535 -> 255, span 1 -> 255 << 16
    assert np.all((0 * m + 32768) >> 16 == 0)                                # out(lo) = 0
    top = ALL_SPANS * m + 32768                                              # the largest d * m + 32768 of a span
    assert np.all(np.minimum(255, top >> 16) == 255)                         # out(hi) = 255
    assert top.max() < 2 ** 24 + 2 ** 16 < 2 ** 32
    assert [rr.multiplier(0, int(s)) for s in (1, 2, 255, 256, 65535)] == [_m(s) for s in (1, 2, 255, 256, 65535)]


def test_monotone_and_less_than_one_level_from_the_quotient():
    for span in SWEPT_SPANS:
        d = np.arange(span + 1, dtype=np.int64)
        out = np.minimum(255, (d * _m(span) + 32768) >> 16)
        assert out[0] == 0 and out[-1] == 255, span
        assert np.all(np.diff(out) >= 0), span
        assert np.all(np.abs(out * span - 255 * d) < span), span            # |out - 255 d / span| < 1, in integers
    # every span at d = span (where an error in m weighs most) and around the middle
    m = ((255 << 16) + ALL_SPANS // 2) // ALL_SPANS
    for d in (ALL_SPANS, ALL_SPANS // 2, (ALL_SPANS + 1) // 2, ALL_SPANS - 1):
        out = np.minimum(255, (d * m + 32768) >> 16)
        assert np.all(np.abs(out * ALL_SPANS - 255 * d) < ALL_SPANS)


def test_apply_is_the_formula_and_clamps_outside_the_window():
    rng = np.random.default_rng(1)
    v = rng.integers(0, 65536, 5000, dtype=np.uint16)
    for lo, hi in ((0, 65535), (7800, 8300), (100, 101), (65534, 65535), (0, 1), (12345, 54321)):
        want = [min(255, ((min(max(int(x), lo), hi) - lo) * _m(hi - lo) + 32768) >> 16) for x in v]
        assert rr.apply(v, lo, hi).tolist() == want
    assert rr.apply(np.array([0, 99, 100, 101, 65535], np.uint16), 100, 101).tolist() == [0, 0, 0, 255, 255]


@pytest.mark.parametrize('clip', [(100, 100), (0, 0), (250000, 250000), (500000, 0), (0, 500000), (12345, 400000)])
def test_range_against_a_brute_force_sort(clip):
    rng = np.random.default_rng(sum(clip))
    groups = [rng.integers(0, 65536, (2, 37, 41), dtype=np.uint16),
              rng.integers(7800, 8301, (1, 64, 48), dtype=np.uint16),
              (rng.normal(30000, 900, (2, 30, 50)).clip(0, 65535)).astype(np.uint16),
              np.full((1, 5, 5), 4111, np.uint16)]
    for g in groups:
        lo, hi = rr.histogram_range(g, clip)
        s = np.sort(g.reshape(-1).astype(np.int64))
        k_lo, k_hi = g.size * clip[0] // 10 ** 6, g.size * clip[1] // 10 ** 6
        assert lo % 16 == 0 and hi % 16 == 15 and lo <= hi
        assert lo <= s[k_lo] <= lo + 15                                      # the k_lo-th smallest sample, zero-based
        assert hi - 15 <= s[g.size - 1 - k_hi] <= hi                         # the k_hi-th largest


def test_a_cumulative_count_equal_to_k_moves_on_to_the_next_bin():
    # 16 samples, 25 % at each end: k = 4.  Four samples in the outermost bins do not exceed it, five do
    def group(n_low, n_high):
        return np.array([5] * n_low + [1000] * (16 - n_low - n_high) + [60000] * n_high, np.uint16).reshape(1, 4, 4)
    clip = (250000, 250000)
    assert rr.clip_counts(16, clip) == (4, 4)
    assert rr.histogram_range(group(4, 4), clip) == (992, 1007)
    assert rr.histogram_range(group(5, 4), clip) == (0, 1007)
    assert rr.histogram_range(group(4, 5), clip) == (992, 60015)
    assert rr.histogram_range(group(5, 5), clip) == (0, 60015)
    assert rr.histogram_range(group(4, 4), (0, 0)) == (0, 60015)


def test_widening_contains_the_old_range_at_both_clamps_and_between():
    bins = [0, 1, 2, 7, 8, 9, 100, 2047, 2048, 4000, 4086, 4087, 4088, 4094, 4095]
    for min_span in (16, 17, 255, 256, 257, 1000, 4096, 65535):
        for b_lo in bins:
            for b_hi in [b for b in bins if b >= b_lo]:
                lo, hi = 16 * b_lo, 16 * b_hi + 15
                nlo, nhi = rr.widen(lo, hi, min_span)
                assert 0 <= nlo <= lo and hi <= nhi <= 65535, (min_span, lo, hi, nlo, nhi)
                if hi - lo >= min_span:
                    assert (nlo, nhi) == (lo, hi)
                else:
                    assert nhi - nlo == min_span
    assert rr.widen(0, 15) == (0, 256)                                       # the clamp at 0
    assert rr.widen(65520, 65535) == (65279, 65535)                          # the clamp at 65535 - min_span
    assert rr.widen(32768, 32783) == (32768 - 120, 32768 - 120 + 256)        # need = 241, need // 2 = 120
    assert rr.auto_range(np.zeros((1, 3, 3), np.uint16)) == (0, 256)
    assert rr.auto_range(np.full((1, 3, 3), 65535, np.uint16)) == (65279, 65535)


def test_two_values_on_either_side_of_a_bin_edge():
    sixteen = np.array([[4096, 4112]], np.uint16).reshape(1, 1, 2)          # 16 apart: two bins
    fifteen = np.array([[4096, 4111]], np.uint16).reshape(1, 1, 2)          # 15 apart: one bin
    assert rr.histogram_range(sixteen, (0, 0)) == (4096, 4127)
    assert rr.histogram_range(fifteen, (0, 0)) == (4096, 4111)


def test_a_pair_is_pooled_into_one_range():
    rng = np.random.default_rng(3)
    a = rng.integers(1000, 1400, (20, 30), dtype=np.uint16)
    b = rng.integers(5000, 5400, (20, 30), dtype=np.uint16)
    g0, g1, (lo, hi) = rr.pair_to_gray8(a, b, scale='auto', clip=(0, 0))
    assert lo <= a.min() and b.max() <= hi and (lo, hi) == rr.auto_range(np.stack([a, b]), (0, 0))
    assert np.array_equal(g0, rr.apply(a, lo, hi)) and np.array_equal(g1, rr.apply(b, lo, hi))
    alone, r1 = rr.to_gray8(np.stack([a, b]), 'auto', clip=(0, 0), pool=1)
    assert r1[0, 1] < r1[1, 0] and not np.array_equal(alone[0], g0)


def test_the_products_numpy_helper_is_the_reference():
    from uav_airvision_amd.frontend import gray16_range
    rng = np.random.default_rng(9)
    frames = np.concatenate([rng.integers(0, 65536, (2, 33, 47), dtype=np.uint16), rng.integers(7800, 8301, (2, 33, 47), dtype=np.uint16),
                             np.zeros((2, 33, 47), np.uint16)])
    for kw in (dict(scale='auto'), dict(scale='auto', pool=2), dict(scale='auto', clip=(0, 0), min_span=16, pool=2),
               dict(scale='auto', clip=(250000, 250000), min_span=4096), dict(scale='window', window=(7800, 8300)), dict(scale='window', window=(0, 65535), pool=2)):
        want, want_r = rr.to_gray8(frames, **kw)
        got, got_r = gray16_range(frames, **kw)
        assert got.dtype == np.uint8 and got_r.dtype == np.int32
        assert np.array_equal(got, want) and np.array_equal(got_r, want_r), kw


def test_settings_are_checked_for_the_scale_that_reads_them():
    from uav_airvision_amd import _native as N
    assert N.gray16_range_settings() == (0, 0, 65535, 100, 100, 256)
    assert N.gray16_range_settings('shift', window=(9, 1), clip=(-1, 0), min_span=3)[0] == 0      # not read, not checked
    assert N.gray16_range_settings('window', (7800, 8300)) == (1, 7800, 8300, 100, 100, 256)
    assert N.gray16_range_settings('auto', None, (0, 500000), 16) == (2, 0, 65535, 0, 500000, 16)
    for bad in (dict(scale='percentile'), dict(scale='window'), dict(scale='window', window=(5, 5)), dict(scale='window', window=(-1, 5)),
                dict(scale='window', window=(0, 65536)), dict(scale='window', window=(1.5, 9)), dict(scale='auto', clip=(-1, 0)),
                dict(scale='auto', clip=(250001, 250000)), dict(scale='auto', clip=(1,)), dict(scale='auto', min_span=15), dict(scale='auto', min_span=65536),
                dict(scale='auto', min_span=True)):
        with pytest.raises(ValueError, match='gray16_'):
            N.gray16_range_settings(**bad)


def test_the_engine_settings_come_from_the_config_object_and_other_formats_are_refused():
    from fe_harness import bare_cfg, make_cfg
    from uav_airvision_amd.frontend import gray16_scale_settings
    assert gray16_scale_settings(make_cfg()) == (0, 0, 65535, 100, 100, 256)
    bare = bare_cfg(lambda k: k.startswith('gray16_'))                       # a caller's config from before the attributes existed: 'shift'
    assert not hasattr(bare, 'gray16_scale') and gray16_scale_settings(bare)[0] == 0
    assert gray16_scale_settings(make_cfg(image_format='gray16', gray16_scale='auto', gray16_auto_clip=(50, 2000), gray16_auto_min_span=512)) == (2, 0, 65535, 50, 2000, 512)
    assert gray16_scale_settings(make_cfg(image_format='gray16', gray16_scale='window', gray16_window=(7800, 8300)))[:3] == (1, 7800, 8300)
    for fmt in ('gray8', 'bayer_rggb16', 'gray12p', 'rgb8'):
        with pytest.raises(ValueError, match="gray16_scale 'auto'.*image_format '%s'" % fmt):
            gray16_scale_settings(make_cfg(image_format=fmt, gray16_scale='auto'))
    with pytest.raises(ValueError, match='gray16_window'):
        gray16_scale_settings(make_cfg(image_format='gray16', gray16_scale='window', gray16_window=(8300, 7800)))
