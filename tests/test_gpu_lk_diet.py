"""The 16-lane LK kernel against the CPU oracle, bit for bit, on the inputs its register arithmetic and loop control can get wrong.

lk.hip computes the W_BITS = 14 bilinear weights without a conversion instruction (x + 2^23, low half of the float's bits), tests
the window bounds with one unsigned compare per axis, zeroes lane 15's share through its weights, and runs the Newton iterations as a
loop with ONE exit that settles the exit reason (converged / oscillating / trip limit / out of the image) afterwards.  The cases:

  weight ties   fractions that make a weight an exact half-integer before rounding (odd x 2^-15 beside a zero fraction: at level 0 for
                the I weights, and as 8 n + odd x 2^-12 in the initial guess for the J weights of the first trip at the top level), the
                fractions 0, 0.5 and 1 - 2^-18, the coordinates -1e-7 and 1e-7, and window origins a few ulps below zero;
  borders       windows over every edge and corner at level 0 (the slow staging path, the derivative masks, the bounds tests), points
                that start outside, guesses far outside, tracks pushed across the border;
  exits         trip limits 1, 2 and 30; a flat region wide enough to fail the eigenvalue test at levels 0, 1 and 2;
  mixed         batches of 4 k + 1, 4 k + 2, 4 k + 3 points whose wavefront-mates come from different classes, so that the four points
                of a wavefront leave the loop on different trips and for different reasons, and the last wavefront is partly empty.

129 x 129 images: the smallest size at which the library builds four pyramid levels (129, 65, 33, 17: a level must be larger than
its 16-pixel frame, av_pyramid_layout refuses the 16 x 16 top level of a 128 x 128 image; the oracle alone would take 128).  Three
pairs: texture with a sub-pixel shift, the same with a flat region, and independent noise (steps that never settle: trip-limit and
oscillation exits).
"""
import functools

import numpy as np
import pytest

SIZE = 129
LIMITS = (1, 2, 30)
PAIRS = ('shift', 'flat', 'noise')
SHIFT = (0.6, -0.4)          # the known motion of the 'shift' pair, pixels (x, y)
FLAT_X = 88                   # the 'flat' pair is constant for x < FLAT_X: flat windows at levels 0 (15 px), 1 (30 px), 2 (60 px)


@functools.lru_cache(maxsize=None)
def images(pair):
    rng = np.random.default_rng(20)
    if pair == 'noise':
        return rng.integers(0, 256, (SIZE, SIZE), dtype=np.uint8), rng.integers(0, 256, (SIZE, SIZE), dtype=np.uint8)
    # smooth texture: coarse noise, enlarged 4 x and blurred, on a canvas large enough to cut the shifted copy from
    n = (SIZE + 16 + 3) // 4 * 4
    t = np.kron(rng.uniform(0, 255, (n // 4, n // 4)), np.ones((4, 4)))
    for ax in (0, 1):
        t = (np.roll(t, 1, ax) + 2 * t + np.roll(t, -1, ax)) / 4
        t = (np.roll(t, 2, ax) + 2 * t + np.roll(t, -2, ax)) / 4
    t = (t - t.min()) * (255 / (t.max() - t.min()))
    ys, xs = np.mgrid[0:SIZE, 0:SIZE].astype(np.float64)

    def sample(dx, dy):       # bilinear sample of the canvas at (x + 8 - dx, y + 8 - dy): the content moves by (+dx, +dy)
        x, y = xs + 8 - dx, ys + 8 - dy
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        a, b = x - x0, y - y0
        v = (t[y0, x0] * (1 - a) + t[y0, x0 + 1] * a) * (1 - b) + (t[y0 + 1, x0] * (1 - a) + t[y0 + 1, x0 + 1] * a) * b
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)

    I, J = sample(0, 0), sample(*SHIFT)
    if pair == 'flat':
        I, J = I.copy(), J.copy()
        I[:, :FLAT_X] = 90
        J[:, :FLAT_X] = 90
    return I, J


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 2))


@functools.lru_cache(maxsize=None)
def point_sets():
    rng = np.random.default_rng(21)
    sets = {}
    # ---- weight ties
    odd = [1, 3, 5, 16383, 16385, 32767]
    fr = [0.0, 0.5, 1.0 - 2.0 ** -18] + [o * 2.0 ** -15 for o in odd]
    prev, init = [], []
    for k, f in enumerate(fr):
        bx, by = 100.0 + (k % 3) * 4, 40.0 + (k // 3) * 12
        for p in ((bx + f, by), (bx, by + f), (bx + f, by + f)):
            prev.append(p)
            init.append(p)                                              # the guess is the point: ties in the I weights at level 0
            prev.append(p)
            init.append((p[0] + SHIFT[0], p[1] + SHIFT[1]))
    for k, o in enumerate(odd):                                         # ties in the J weights of the first trip (level 3: guess / 8)
        bx, by = 96.0 + (k % 3) * 8, 48.0 + (k // 3) * 16
        for g in ((bx + o * 2.0 ** -12, by), (bx, by + o * 2.0 ** -12)):
            prev.append((bx + 0.25, by + 0.25))
            init.append(g)
    for c in (-1e-7, 1e-7):
        for p in ((c, 60.0), (60.0, c), (c, c), (c, 100.5), (100.5, c)):
            prev.append(p)
            init.append(p)
    for k in (1, 2, 3):                                                 # window origin (point - 7) k ulps below zero
        c = float(np.float32(7.0) - k * np.float32(2.0 ** -21))
        for p in ((c, 60.0), (60.0, c), (c, c)):
            prev.append(p)
            init.append(p)
            prev.append((100.25, 60.5))
            init.append(p)
    sets['ties'] = (_f32(prev), _f32(init))
    # ---- borders
    edge = [-8.5, -6.0, -1.0, 0.0, 0.5, 3.0, 6.5, 7.0, 7.5]
    coords = edge + [SIZE - 1 - e for e in edge] + [64.0]
    prev = [(x, y) for x in coords for y in coords if not (x == 64.0 and y == 64.0)]
    init = [(x + dx, y + dy) for (x, y), (dx, dy) in zip(prev, rng.normal(0, 1.0, (len(prev), 2)))]
    outside = [(-20.0, 50.0), (50.0, -20.0), (150.0, 64.0), (64.0, 150.0), (-8.51, 64.0), (64.0, SIZE + 8.0), (-1e4, -1e4), (3e9, 64.0)]
    prev += outside
    init += outside
    inner = [(20.0 + 11 * k, 24.0 + 9 * k) for k in range(8)]          # good points whose guess is far outside, or pushed across
    prev += inner
    init += [(x + 300.0, y) for x, y in inner[:4]] + [(x - 60.0, y - 60.0) for x, y in inner[4:]]
    push = [(3.0, 30.0 + 8 * k) for k in range(6)] + [(SIZE - 4.0, 30.0 + 8 * k) for k in range(6)]
    prev += push
    init += [(-7.9, y) for x, y in push[:6]] + [(SIZE + 6.9, y) for x, y in push[6:]]
    sets['borders'] = (_f32(prev), _f32(init))
    sets['n_outside'] = len(outside)
    # ---- interior: ordinary points over the whole image, the flat region of the 'flat' pair included
    prev = np.stack([rng.uniform(10, SIZE - 10, 96), rng.uniform(10, SIZE - 10, 96)], 1)
    sets['interior'] = (_f32(prev), _f32(prev + rng.normal(0, 1.5, prev.shape)))
    return sets


def mixed(n_tail):
    """All classes interleaved (a fixed permutation), cut to 4 k + n_tail points."""
    s = point_sets()
    prev = np.concatenate([s[k][0] for k in ('ties', 'borders', 'interior')])
    init = np.concatenate([s[k][1] for k in ('ties', 'borders', 'interior')])
    order = np.random.default_rng(22 + n_tail).permutation(len(prev))
    n = (len(prev) - 4) // 4 * 4 + n_tail
    return prev[order][:n].copy(), init[order][:n].copy()


def _kw(limit):
    return dict(winSize=(15, 15), maxLevel=3, criteria=(3, limit, 0.01), flags=4, minEigThreshold=1e-4)


@functools.lru_cache(maxsize=None)
def oracle(pair, limit, name):
    """The reference, computed once per case and shared (read-only) among the tests."""
    from oracle import cvops
    I, J = images(pair)
    prev, init = mixed(int(name[5:])) if name.startswith('mixed') else point_sets()[name]
    p, s, _ = cvops.calc_optical_flow_pyr_lk(I, J, prev, init, **_kw(limit))
    p.setflags(write=False)
    s.setflags(write=False)
    return prev, init, p, s


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from uav_airvision_amd import ops as o
    return o


def _compare(ops, pair, limit, name):
    I, J = images(pair)
    prev, init, p_cpu, s_cpu = oracle(pair, limit, name)
    p_gpu, s_gpu, _ = ops.calc_optical_flow_pyr_lk(I, J, prev, init.copy(), **_kw(limit))
    bad = np.flatnonzero(s_gpu[:, 0] != s_cpu[:, 0])
    assert bad.size == 0, (pair, limit, name, 'status differs at', bad[:8], prev[bad[:8]], init[bad[:8]])
    diff = np.flatnonzero((p_gpu.view(np.uint32) != p_cpu.view(np.uint32)).any(1))
    assert diff.size == 0, (pair, limit, name, 'points differ at', diff[:8], prev[diff[:8]], p_gpu[diff[:8]], p_cpu[diff[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize('limit', LIMITS)
@pytest.mark.parametrize('pair', PAIRS)
@pytest.mark.parametrize('name', ['ties', 'borders', 'interior'])
def test_lk_sets_bit_exact(ops, name, pair, limit):
    _compare(ops, pair, limit, name)


@pytest.mark.gpu
@pytest.mark.parametrize('limit', LIMITS)
@pytest.mark.parametrize('pair', PAIRS)
@pytest.mark.parametrize('n_tail', [1, 2, 3])
def test_lk_mixed_wavefronts_bit_exact(ops, n_tail, pair, limit):
    _compare(ops, pair, limit, 'mixed%d' % n_tail)


def test_every_class_has_members():
    """From the oracle's outputs and the inputs alone: the sets hold what their names say."""
    assert images('shift')[0].shape == (SIZE, SIZE)
    s = point_sets()
    # ties: the fractions are exact in float32, and the half-integer products are there
    prev = s['ties'][0]
    fa = (prev - np.floor(prev)).astype(np.float64)
    assert np.any((fa * 2 ** 14 % 1 == 0.5)), 'no half-integer weight'
    assert np.any(fa == 0.5) and np.any(fa == 1.0 - 2.0 ** -18) and np.any(prev == np.float32(1e-7)) and np.any(prev == np.float32(-1e-7))
    worg = prev - np.float32(7.0)
    assert np.any((worg < 0) & (worg > -1e-6)), 'no window origin just below zero'
    g = s['ties'][1].astype(np.float64) / 8
    assert np.any(((g - np.floor(g)) * 2 ** 14 % 1 == 0.5)), 'no half-integer weight in the first trip at the top level'
    # borders: both outcomes; every point that starts outside fails, whatever the images
    for pair in PAIRS:
        prev, init, p, st = oracle(pair, 30, 'borders')
        far = (np.floor(prev - np.float32(7.0)) < -15).any(1) | (np.floor(prev - np.float32(7.0)) >= SIZE).any(1)
        assert far.sum() >= s['n_outside'] and not st[far].any()
        if pair != 'flat':
            assert st.sum() > 20 and (st == 0).sum() > s['n_outside'] + 4, (pair, int(st.sum()))
        win_over = ((prev - 7 < 0) | (prev + 8 > SIZE - 1)).any(1) & ~far
        assert win_over.sum() > 100
        if pair == 'shift':
            assert st[win_over].sum() > 20, 'no tracked point with its window over the border'
    # exits: the trip limits bind (limit 1 and 2 give other positions than 30 for points that are tracked in all three) ...
    for pair in PAIRS:
        r1, r2, r30 = (oracle(pair, k, 'interior') for k in LIMITS)
        ok = (r1[3] & r2[3] & r30[3])[:, 0] > 0
        if pair != 'flat':
            assert ok.sum() > 20
        assert np.any(r1[2][ok] != r30[2][ok]) and np.any(r2[2][ok] != r30[2][ok]) and np.any(r1[2][ok] != r2[2][ok]), pair
    # ... on the shift pair the points converge to the known motion (the convergence exit), the noise pair does not settle there
    prev, init, p, st = oracle('shift', 30, 'interior')
    good = st[:, 0] > 0
    assert good.sum() > 60 and np.median(np.abs((p - prev)[good] - np.float32(SHIFT)).max(1)) < 0.1
    # ... and the flat region fails the eigenvalue test: status 0 for every point whose level-0 window lies in it, 1 for some beside it
    prev, init, p, st = oracle('flat', 30, 'interior')
    in_flat = prev[:, 0] + 9 < FLAT_X - 1
    assert in_flat.sum() > 20 and not st[in_flat].any()
    deep = prev[:, 0] + 2 * 9 + 2 < FLAT_X - 1              # the level-1 window (30 px at level 0) is flat too
    assert deep.sum() > 10
    assert st[~in_flat].sum() > 5
    # mixed: the three sizes, and the neighbours in a wavefront differ in outcome
    for n_tail in (1, 2, 3):
        prev, init, p, st = oracle('shift', 30, 'mixed%d' % n_tail)
        assert len(prev) % 4 == n_tail
        quads = st[:len(prev) // 4 * 4, 0].reshape(-1, 4).sum(1)
        assert np.any((quads > 0) & (quads < 4)), 'no wavefront with both outcomes'
