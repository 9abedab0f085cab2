"""av_to_gray8_range / ops.to_gray8_range (csrc/range16.hip) against the NumPy reference of tests/range16_ref.py, ranges and pixels, bit
for bit: every path of the three kernels (one vector, ragged, aligned, vector body plus ragged end, several workgroups per image,
unaligned bases and strides, the index list), pooled and single groups, the data that decides a range (constants at both clamps, a
bin edge, a thermal band, outliers inside and outside the clip, a cumulative count equal to k), the window mode, the re-zeroing of the
histograms, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import range16_ref as rr

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1), (37, 3), (64, 48), (130, 5)]            # (w, h): one vector; ragged, N % 8 != 0; aligned; vector body plus ragged end
BIG = (752, 480)                                           # six histogram workgroups per image, the last one short


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _band(rng, shape):
    return rng.integers(7800, 8301, shape, dtype=np.uint16)


def _data(rng, n, h, w):
    """name -> uint16 [n, h, w]: what decides a range."""
    shape = (n, h, w)
    two16 = np.where(rng.integers(0, 2, shape) == 1, 4112, 4096).astype(np.uint16)
    two15 = np.where(rng.integers(0, 2, shape) == 1, 4111, 4096).astype(np.uint16)
    two16.reshape(-1)[:2] = (4096, 4112)
    two15.reshape(-1)[:2] = (4096, 4111)
    return {'zeros': np.zeros(shape, np.uint16), 'full': np.full(shape, 65535, np.uint16), 'mid': np.full(shape, 32768, np.uint16),
            'two16': two16, 'two15': two15, 'band': _band(rng, shape), 'uniform': rng.integers(0, 65536, shape, dtype=np.uint16)}


def _check(frames, tag, **kw):
    from uav_airvision_amd import ops
    want, want_r = rr.to_gray8(frames, **kw)
    got, got_r = ops.to_gray8_range(_dev(frames), **kw)
    assert np.array_equal(got_r.cpu().numpy(), want_r), (tag, got_r.cpu().numpy().tolist(), want_r.tolist())
    assert np.array_equal(got.cpu().numpy(), want), tag
    return want_r


@pytest.mark.parametrize('pool', [1, 2])
@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('w,h', SHAPES)
def test_auto_matches_the_reference(w, h, groups, pool):
    rng = np.random.default_rng(w * 131 + h * 7 + groups * 3 + pool)
    for name, frames in _data(rng, groups * pool, h, w).items():
        r = _check(frames, name, scale='auto', pool=pool)
        if name == 'zeros':
            assert r.tolist() == [[0, 256]] * groups
        if name == 'full':
            assert r.tolist() == [[65279, 65535]] * groups
        if name == 'mid':
            assert r.tolist() == [[32768 - 120, 32768 + 136]] * groups
    frames = _data(rng, groups * pool, h, w)
    _check(frames['two16'], 'two16 unwidened', scale='auto', pool=pool, clip=(0, 0), min_span=16)
    _check(frames['two15'], 'two15 unwidened', scale='auto', pool=pool, clip=(0, 0), min_span=16)
    _check(frames['uniform'], 'uniform, wide clip', scale='auto', pool=pool, clip=(250000, 150000), min_span=1000)


def test_groups_of_a_batch_get_their_own_ranges_and_a_pair_shares_one():
    rng = np.random.default_rng(5)
    frames = np.stack([rng.integers(1000 + 3000 * i, 1400 + 3000 * i, (48, 64), dtype=np.uint16) for i in range(6)])
    single = _check(frames, 'six groups', scale='auto', pool=1)
    pooled = _check(frames, 'three pairs', scale='auto', pool=2)
    assert len({tuple(r) for r in single.tolist()}) == 6 and len({tuple(r) for r in pooled.tolist()}) == 3
    assert all(pooled[g, 0] == single[2 * g, 0] and pooled[g, 1] == single[2 * g + 1, 1] for g in range(3))


@pytest.mark.parametrize('pool', [1, 2])
def test_full_size_frames_and_outliers_inside_and_outside_the_clip(pool):
    w, h = BIG
    rng = np.random.default_rng(11 + pool)
    band = _band(rng, (pool, h, w))
    _check(band, 'band', scale='auto', pool=pool)
    _check(rng.integers(0, 65536, (pool, h, w), dtype=np.uint16), 'uniform', scale='auto', pool=pool)
    # 20 samples at each end of the scale: k = 36 * pool at 100 ppm leaves them outside, (0, 0) takes them in
    spiked = band.copy()
    at = rng.choice(spiked.size, 40, replace=False)
    spiked.reshape(-1)[at[:20]] = 0
    spiked.reshape(-1)[at[20:]] = 65535
    assert rr.clip_counts(spiked.size, (100, 100)) == (36 * pool, 36 * pool)
    outside = _check(spiked, 'spikes outside', scale='auto', pool=pool)
    inside = _check(spiked, 'spikes inside', scale='auto', pool=pool, clip=(0, 0))
    assert 7700 <= outside[0, 0] <= 7800 and 8300 <= outside[0, 1] <= 8400 and inside.tolist() == [[0, 65535]]


def test_a_cumulative_count_equal_to_k_moves_on_to_the_next_bin():
    def frame(n_low, n_high):
        return np.array([5] * n_low + [1000] * (16 - n_low - n_high) + [60000] * n_high, np.uint16).reshape(1, 1, 16)
    kw = dict(scale='auto', clip=(250000, 250000), min_span=16)
    assert _check(frame(4, 4), '4 / 4', **kw).tolist() == [[992, 1008]]      # one bin, 15 wide: widened to the smallest span, 16
    assert _check(frame(5, 4), '5 / 4', **kw).tolist() == [[0, 1007]]
    assert _check(frame(4, 5), '4 / 5', **kw).tolist() == [[992, 60015]]
    assert _check(frame(5, 5), '5 / 5', **kw).tolist() == [[0, 60015]]


@pytest.mark.parametrize('w,h', SHAPES)
def test_window_matches_the_reference(w, h):
    rng = np.random.default_rng(w + h)
    frames = np.concatenate([rng.integers(0, 65536, (2, h, w), dtype=np.uint16), _band(rng, (2, h, w))])
    frames.reshape(-1)[:4] = (0, 65535, 7800, 8300)
    for window in ((0, 65535), (7800, 8300), (8000, 8001), (65534, 65535), (0, 1)):
        for pool in (1, 2):
            r = _check(frames, window, scale='window', window=window, pool=pool)
            assert r.tolist() == [list(window)] * (4 // pool)


@pytest.mark.parametrize('scale', ['auto', 'window'])
def test_unaligned_bases_and_strides_take_the_sample_by_sample_path(scale):
    """A batch whose stride is not a multiple of 16 bytes, and a base that is not: same results as the aligned call."""
    import torch
    from uav_airvision_amd import ops
    w, h, n = 64, 48, 4
    rng = np.random.default_rng(21)
    frames = np.concatenate([_band(rng, (2, h, w)), rng.integers(0, 65536, (2, h, w), dtype=np.uint16)])
    kw = dict(scale=scale, window=(7900, 8200) if scale == 'window' else None)
    for pool in (1, 2):
        want, want_r = rr.to_gray8(frames, pool=pool, **kw)
        # stride of h * w + 3 samples = 6150 bytes
        wide = torch.zeros((n, h * w + 3), dtype=torch.int16, device='cuda')
        wide[:, :h * w] = _dev(frames).reshape(n, h * w)
        src = wide.as_strided((n, h, w), (h * w + 3, w, 1))
        assert (src.stride(0) * 2) % 16 != 0
        out_wide = torch.full((n, h * w + 5), 7, dtype=torch.uint8, device='cuda')
        out = out_wide.as_strided((n, h, w), (h * w + 5, w, 1))
        got, got_r = ops.to_gray8_range(src, pool=pool, out=out, **kw)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_r.cpu().numpy(), want_r), (pool, 'stride')
        assert bool((out_wide[:, h * w:] == 7).all())                        # the bytes between the images are untouched
        # a base one sample (2 bytes) into an aligned allocation
        flat = torch.zeros(n * h * w + 8, dtype=torch.int16, device='cuda')
        flat[1:1 + n * h * w] = _dev(frames).reshape(-1)
        src = flat[1:1 + n * h * w].view(n, h, w)
        assert src.data_ptr() % 16 == 2
        got, got_r = ops.to_gray8_range(src, pool=pool, **kw)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_r.cpu().numpy(), want_r), (pool, 'base')


@pytest.mark.parametrize('pool', [1, 2])
@pytest.mark.parametrize('w,h', [(37, 3), (64, 48)])
def test_index_list_skips_and_writes_a_repeated_entry_once(w, h, pool):
    import torch
    from uav_airvision_amd import ops
    rng = np.random.default_rng(31 + pool)
    groups = 4
    frames = np.stack([rng.integers(2000 * i, 2000 * i + 900, (h, w), dtype=np.uint16) for i in range(groups * pool)])
    index = [2, 0, 2, -1]                       # entry 2 named twice (group 2 wins), group 3 skipped, entries 1 and 3 never named
    want, want_r = rr.to_gray8(frames, 'auto', pool=pool)
    out = torch.full((4 * pool, h, w), 201, dtype=torch.uint8, device='cuda')
    got, got_r = ops.to_gray8_range(_dev(frames), 'auto', pool=pool, index=index, out=out)
    assert got is out
    o = out.cpu().numpy().reshape(4, pool, h, w)
    wv = want.reshape(groups, pool, h, w)
    assert np.array_equal(o[0], wv[1]) and np.array_equal(o[2], wv[2])
    assert np.all(o[1] == 201) and np.all(o[3] == 201)                       # untouched
    r = got_r.cpu().numpy()
    assert r[0].tolist() == [-1, -1] and r[3].tolist() == [-1, -1]           # groups that were not written have no range
    assert np.array_equal(r[1], want_r[1]) and np.array_equal(r[2], want_r[2])
    # the window mode through the same list
    out.fill_(201)
    ops.to_gray8_range(_dev(frames), 'window', window=(1000, 5000), pool=pool, index=index, out=out)
    o = out.cpu().numpy().reshape(4, pool, h, w)
    ww = rr.to_gray8(frames, 'window', window=(1000, 5000), pool=pool)[0].reshape(groups, pool, h, w)
    assert np.array_equal(o[0], ww[1]) and np.array_equal(o[2], ww[2]) and np.all(o[1] == 201) and np.all(o[3] == 201)


def test_two_launches_on_the_same_buffers_give_the_same_result():
    """The pick kernel leaves every histogram zero: a second launch on the same work buffer, never cleared in between, finds it so."""
    import torch
    from uav_airvision_amd import _native as N, ops
    rng = np.random.default_rng(41)
    w, h, groups, pool = 130, 5, 3, 2
    a = np.concatenate([_band(rng, (2, h, w)), rng.integers(0, 65536, (2, h, w), dtype=np.uint16), np.zeros((2, h, w), np.uint16)])
    b = rng.integers(0, 65536, (6, h, w), dtype=np.uint16)
    work = torch.zeros(groups * N.AV_GRAY16_WORK_WORDS, dtype=torch.int32, device='cuda')
    for k, frames in enumerate((a, a, b, a)):
        want, want_r = rr.to_gray8(frames, 'auto', pool=pool)
        got, got_r = ops.to_gray8_range(_dev(frames), 'auto', pool=pool, work=work)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_r.cpu().numpy(), want_r), k
        assert not bool(work[:groups * 4096].any()), k
        rec = work[groups * 4096:].cpu().numpy().reshape(groups, 4)
        assert np.array_equal(rec[:, :2], want_r) and rec[:, 2].tolist() == [rr.multiplier(lo, hi) for lo, hi in want_r.tolist()], k


def test_bad_arguments_are_refused_with_av_e_invalid():
    import torch
    from uav_airvision_amd import _native as N, ops
    w, h = 64, 48
    src = torch.zeros((2, h, w), dtype=torch.int16, device='cuda')
    dst = torch.full((2, h, w), 9, dtype=torch.uint8, device='cuda')

    def call(n=2, w=w, h=h, mode=2, lo=0, hi=65535, ppm=(100, 100), span=256, pool=1, in_stride=2 * w * h, out_stride=w * h, inp=src, out=dst):
        return N.lib().av_to_gray8_range(N.dptr(inp) if inp is not None else None, in_stride, n, w, h, mode, lo, hi, ppm[0], ppm[1], span, pool, None,
                                         N.dptr(out) if out is not None else None, out_stride, None, None, N.current_stream())
    assert call() == N.AV_OK
    bad = [dict(mode=0), dict(mode=3), dict(mode=1, lo=5, hi=5), dict(mode=1, lo=-1, hi=5), dict(mode=1, lo=0, hi=65536), dict(mode=1, lo=9, hi=3),
           dict(ppm=(-1, 0)), dict(ppm=(0, -1)), dict(ppm=(250001, 250000)), dict(span=15), dict(span=65536), dict(pool=0), dict(pool=3),
           dict(n=1, pool=2), dict(n=-1), dict(w=0), dict(h=0), dict(w=8192, h=4096), dict(in_stride=2 * w * h - 2), dict(out_stride=w * h - 1),
           dict(inp=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) == N.AV_E_INVALID, kw
        assert b'av_to_gray8_range' in N.lib().av_last_error(), kw
    # the output on top of the input
    alias = torch.zeros(4 * w * h, dtype=torch.uint8, device='cuda')
    assert N.lib().av_to_gray8_range(N.dptr(alias), 2 * w * h, 2, w, h, 2, 0, 0, 100, 100, 256, 1, None, N.dptr(alias), w * h, None, None,
                                     N.current_stream()) == N.AV_E_INVALID
    assert b'overlaps' in N.lib().av_last_error()
    torch.cuda.synchronize()
    assert bool((dst.cpu() == 0).all())                                      # only the good call wrote (zeros map to 0)
    for kw in (dict(scale='shift'), dict(scale='window'), dict(scale='auto', pool=3), dict(scale='auto', min_span=8)):
        with pytest.raises(ValueError):
            ops.to_gray8_range(src, **kw)
    with pytest.raises(ValueError, match='uint16'):
        ops.to_gray8_range(torch.zeros((2, h, w), dtype=torch.uint8, device='cuda'))
