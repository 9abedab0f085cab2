"""The level set-up of the 16-lane LK kernel against the CPU oracle, bit for bit, on the inputs its shortened arithmetic can get wrong.

lk.hip builds the Scharr values times 4 and takes the interpolated derivative from the HIGH half of the accumulator (no shift), sums
a11 and a22 as unsigned 32-bit integers, compares the eigenvalue numerator with a bound computed on the host instead of dividing it by
450, takes the square root without the range handling, addresses both stagings from scalar row bases and keeps the fifth staged dword
of an I row unshifted.  The cases (129 x 129 images as in tests/test_gpu_lk_diet.py, whose harness this file imports):

  extreme    stripe images of period 4 (0, 0, 255, 255), vertical, horizontal and diagonal, and a 0 / 255 checkerboard: every |Ix| or
             |Iy| of the upright stripes is 16 x 255 = 4080, a window's a11 or a22 is 225 x 4080^2 > 2^31 (the diagonal ones have
             Ix = Iy = +-2550, a11 = a12 = a22; the checkerboard's Scharr derivatives are all zero); points at the fractions 0, 0.5,
             1 - 2^-18 and the weight-tie fractions, in the interior and with their windows over the border (the derivative masks).
             Pure stripes have one flat direction and fail the eigenvalue test whatever a11 is; the two 'dots' patterns are the
             stripes with one pixel in 32 set to 128: a11 or a22 stays above 2^31, the other direction has texture, the test is
             passed and the large sum goes into the determinant and into every Newton step;
  eigen      49 windows, flat but for n = 0 .. 48 single pixels three grey levels up: minEig grows by about 9e-6 per pixel at a
             zero fraction (a single pixel of amplitude a adds a^2 (2 x 10^2 + 4 x 3^2) = 236 a^2 to the sums of Ix^2 and of Iy^2,
             minEig = 2 lambda_min / 450 ~ a^2 n 2^-20 x 472 / 450) and by about half of that at the fraction 0.5, which averages
             neighbours, so that it crosses the thresholds 1e-4 and 1.6e-4 inside the batch; window 0 is exactly flat
             (all sums zero: the square root of zero); and the strongest edge there is (0 | 255, Iy = 0 exactly) with 0 .. 5 single
             pixels one grey level up beside it: A12 = 0, A22 = 0 or tiny against A11, threshold 2.5e-6 between two and three pixels;
  staging    points whose window origin is the last column / row a level admits (w - 1: the 18-byte rows of the neighbourhood end at
             the last byte of the padded row, and at the top level in the last rows of the pyramid) or the first (-15), for each of the
             four levels, mixed with interior and border points in batches of 4 k + 1, 2 and 3.

Every case runs twice: level 0 from the pyramid, and level 0 in place from the caller's image (the border path where a window leaves it).
"""
import functools

import numpy as np
import pytest

from test_gpu_lk_diet import SIZE, _f32, images as diet_images, ops, point_sets        # noqa: F401 (ops is the module's GPU fixture)

LEVEL_W = (129, 65, 33, 17)
PATTERNS = ('vstripe', 'hstripe', 'dstripe', 'checker', 'vstripe_dots', 'hstripe_dots')
EIG_CASES = (('steps', 1e-4), ('steps', 1.6e-4), ('edge', 2.5e-6))
TILE = 18                     # pitch of the 'steps' windows: 15 window columns, one more for a fraction, the Scharr ring
EDGE_X = 64                   # the 'edge' image is 0 left of it and 255 from it on
EDGE_YS = (12, 32, 52, 72, 92, 112)


@functools.lru_cache(maxsize=None)
def pattern(name):
    ys, xs = np.mgrid[0:SIZE, 0:SIZE]
    p4 = np.array([0, 0, 255, 255], np.uint8)
    I = {'vstripe': p4[xs % 4], 'hstripe': p4[ys % 4], 'dstripe': p4[(xs + ys) % 4], 'checker': ((xs + ys) % 2 * 255).astype(np.uint8)}[name[:7]]
    I = np.ascontiguousarray(I)
    if name.endswith('_dots'):
        I[np.random.default_rng(30).random(I.shape) < 1 / 32] = 128
    J = np.ascontiguousarray(np.roll(I, (1, 1), (0, 1)))              # the same pattern one pixel down and right
    return I, J


@functools.lru_cache(maxsize=None)
def eig_image(name):
    if name == 'steps':
        rng = np.random.default_rng(31)
        I = np.full((SIZE, SIZE), 90, np.uint8)
        cells = [(r, c) for r in range(3, 13) for c in range(3, 13)]            # inside the window, Scharr ring included
        for n in range(49):
            oy, ox = (n // 7) * TILE, (n % 7) * TILE
            for k in rng.permutation(len(cells))[:n]:
                I[oy + 1 + cells[k][0], ox + 1 + cells[k][1]] = 93
        return I, I.copy()
    I = np.zeros((SIZE, SIZE), np.uint8)
    I[:, EDGE_X:] = 255
    for n, y in enumerate(EDGE_YS):                                           # n single pixels beside the edge, three rows apart
        for k in range(n):
            I[y - 6 + 3 * k, EDGE_X - 5] = 1
    return I, I.copy()


@functools.lru_cache(maxsize=None)
def eig_points(name):
    if name == 'steps':
        fr = (0.0, 0.5, 0.25)
        p = [((n % 7) * TILE + 8 + fr[n % 3], (n // 7) * TILE + 8 + fr[(n // 3) % 3]) for n in range(49)]
    else:
        p = [(float(EDGE_X), float(y)) for y in EDGE_YS]
    return _f32(p), _f32(p)


@functools.lru_cache(maxsize=None)
def extreme_points():
    odd = [1, 3, 5, 16383, 16385, 32767]
    fr = [0.0, 0.5, 1.0 - 2.0 ** -18] + [o * 2.0 ** -15 for o in odd]
    prev = []
    for k, f in enumerate(fr):
        bx, by = 30.0 + (k % 3) * 21, 28.0 + (k // 3) * 23
        prev += [(bx + f, by), (bx, by + f), (bx + f, by + f), (bx + 1 + f, by + 2 + f)]
    for f in (0.0, 0.5, 1.0 - 2.0 ** -18):                               # windows over the border: masks on extreme derivatives
        prev += [(3.0 + f, 60.0), (60.0, 2.0 + f), (SIZE - 4.0 - f, 64.0), (64.0, SIZE - 3.0 - f), (1.0 + f, 1.0 + f), (SIZE - 2.0 - f, SIZE - 2.0 - f)]
    prev = _f32(prev)
    init = prev.copy()
    init[1::2] += np.float32(1.0)                                        # every other guess at the pattern's shift
    return prev, init


def level_edge_coords():
    """Per level: the coordinate whose window origin is w - 1 (the last one admitted) and the one whose origin is -15 (the first)."""
    return [((w - 1 + 7.5) * 2 ** l, -7.5 * 2 ** l) for l, w in enumerate(LEVEL_W)]


@functools.lru_cache(maxsize=None)
def staging_points(n_tail):
    prev = []
    for hi, lo in level_edge_coords():
        prev += [(hi, 64.0), (64.0, hi), (hi, hi), (lo, 64.0), (64.0, lo), (lo, lo), (hi, lo), (lo, hi)]
    prev = _f32(prev)
    s = point_sets()
    prev = np.concatenate([prev, prev + np.float32(0.25), s['interior'][0][:40], s['borders'][0][::7]])
    init = np.concatenate([prev[:64], s['interior'][1][:40], s['borders'][1][::7]])
    order = np.random.default_rng(40 + n_tail).permutation(len(prev))
    n = (len(prev) - 4) // 4 * 4 + n_tail
    return prev[order][:n].copy(), init[order][:n].copy()


def _kw(min_eig=1e-4):
    return dict(winSize=(15, 15), maxLevel=3, criteria=(3, 30, 0.01), flags=4, minEigThreshold=min_eig)


def case(kind, arg):
    """(I, J, prev, init, lk arguments) of one case."""
    if kind == 'extreme':
        return pattern(arg) + extreme_points() + (_kw(),)
    if kind == 'eigen':
        return eig_image(arg[0]) + eig_points(arg[0]) + (_kw(arg[1]),)
    return diet_images('shift') + staging_points(arg) + (_kw(),)


@functools.lru_cache(maxsize=None)
def oracle(kind, arg):
    """The reference, computed once per case and shared (read-only) among the tests."""
    from oracle import cvops
    I, J, prev, init, kw = case(kind, arg)
    p, s, _ = cvops.calc_optical_flow_pyr_lk(I, J, prev, init.copy(), **kw)
    p.setflags(write=False)
    s.setflags(write=False)
    return p, s


def _compare(ops, kind, arg, in_place):
    I, J, prev, init, kw = case(kind, arg)
    p_cpu, s_cpu = oracle(kind, arg)
    p_gpu, s_gpu, _ = ops.calc_optical_flow_pyr_lk(I, J, prev, init.copy(), level0_in_place=in_place, **kw)
    bad = np.flatnonzero(s_gpu[:, 0] != s_cpu[:, 0])
    assert bad.size == 0, (kind, arg, 'status differs at', bad[:8], prev[bad[:8]], init[bad[:8]])
    diff = np.flatnonzero((p_gpu.view(np.uint32) != p_cpu.view(np.uint32)).any(1))
    assert diff.size == 0, (kind, arg, 'points differ at', diff[:8], prev[diff[:8]], p_gpu[diff[:8]], p_cpu[diff[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('name', PATTERNS)
def test_extreme_derivatives_bit_exact(ops, name, in_place):
    _compare(ops, 'extreme', name, in_place)


@pytest.mark.gpu
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('arg', EIG_CASES)
def test_eigenvalue_boundary_bit_exact(ops, arg, in_place):
    _compare(ops, 'eigen', arg, in_place)


@pytest.mark.gpu
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('n_tail', [1, 2, 3])
def test_staging_limits_bit_exact(ops, n_tail, in_place):
    _compare(ops, 'staging', n_tail, in_place)


def _scharr(I):
    P = np.pad(I.astype(np.int64), 1, mode='reflect')
    gx = 3 * (P[:-2, 2:] - P[:-2, :-2]) + 10 * (P[1:-1, 2:] - P[1:-1, :-2]) + 3 * (P[2:, 2:] - P[2:, :-2])
    gy = 3 * (P[2:, :-2] - P[:-2, :-2]) + 10 * (P[2:, 1:-1] - P[:-2, 1:-1]) + 3 * (P[2:, 2:] - P[:-2, 2:])
    return gx, gy


def test_every_class_has_members():
    """From the inputs and the oracle's outputs alone: the cases hold what their names say."""
    # extreme: all derivatives of the stripes at +-4080, a window's sum of squares above 2^31 (and below 2^32)
    inner = (slice(2, -2), slice(2, -2))
    for name in ('vstripe', 'hstripe'):
        gx, gy = _scharr(pattern(name)[0])
        g, flat = (gx, gy) if name[0] == 'v' else (gy, gx)
        assert (np.abs(g[inner]) == 4080).all() and not flat[inner].any()
        assert 2 ** 31 < (g[20:35, 20:35] ** 2).sum() == 225 * 4080 ** 2 < 2 ** 32
    gx, gy = _scharr(pattern('dstripe')[0])                               # the diagonal: both derivatives, equal, at (10 + 3 - 3) x 255
    assert (np.abs(gx[inner]) == 2550).all() and np.array_equal(gx[inner], gy[inner])
    prev = extreme_points()[0]
    fa = (prev - np.floor(prev)).astype(np.float64)
    assert np.any(fa == 0.5) and np.any(fa == 1.0 - 2.0 ** -18) and np.any(fa * 2 ** 14 % 1 == 0.5)
    assert np.any(prev - 7 < 0) and np.any(prev + 8 > SIZE - 1)
    for name in PATTERNS[4:]:                                           # the dotted stripes: still above 2^31, and tracked
        gx, gy = _scharr(pattern(name)[0])
        g = gx if name[0] == 'v' else gy
        assert max((g[y:y + 15, x:x + 15] ** 2).sum() for y in range(20, 90, 5) for x in range(20, 90, 5)) > 2 ** 31
        assert oracle('extreme', name)[1].sum() > 10, name
    # eigen: the status follows the number of pixels and flips inside the batch, for both thresholds, at different places
    flips = []
    for arg in EIG_CASES[:2]:
        st = oracle('eigen', arg)[1][:, 0]
        assert st[0] == 0 and st[-1] == 1 and 5 < (st == 0).sum() < 44, (arg, st)
        flips.append(int((st == 0).sum()))
    assert flips[0] < flips[1]
    I = eig_image('steps')[0]
    assert (I[:TILE, :TILE] == 90).all() and (I[6 * TILE:7 * TILE, 6 * TILE:7 * TILE] == 93).sum() == 48
    st = oracle('eigen', EIG_CASES[2])[1][:, 0]
    assert list(st) == [0, 0, 0, 1, 1, 1], st
    gx, gy = _scharr(eig_image('edge')[0])
    for n, y in enumerate(EDGE_YS):
        win = (slice(y - 7, y + 8), slice(EDGE_X - 7, EDGE_X + 8))
        assert (gx[win] * gy[win]).sum() == 0 and (gy[win] ** 2).sum() == 236 * n and (gx[win] ** 2).sum() > 2 ** 28
    # staging: for every level a window origin at w - 1 and one at -15, in x and in y, and the three batch sizes
    for n_tail in (1, 2, 3):
        prev = staging_points(n_tail)[0]
        assert len(prev) % 4 == n_tail
        for l, w in enumerate(LEVEL_W):
            org = np.floor(prev * np.float32(0.5 ** l) - np.float32(7.0))
            for axis in (0, 1):
                assert (org[:, axis] == w - 1).sum() >= 2 and (org[:, axis] == -15).sum() >= 2, (n_tail, l, axis)
        st = oracle('staging', n_tail)[1][:, 0]
        assert st.sum() > 20 and (st == 0).sum() > 20
