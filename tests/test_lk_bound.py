"""av_lk_quotient_bound (uav_airvision_amd/csrc/lk_host.h): the float X that lets the 16-lane LK kernel test its eigenvalue numerator
without dividing it -- fl(x / 450) < t  <=>  x < X for every float x.  The function is compiled into a stand-alone program
(tests/native/lk_bound_harness.cpp: no GPU, no HIP, nothing loaded into Python), which checks every float within 64 ulps of X with the
host's own float division; the same floats are checked again here with numpy's float32 division, from the X the program printed.

Thresholds: three mantissas at every power of ten from 1e-14 to 1e6 (twenty orders of magnitude around the configured 1e-4, itself
included as the float the library passes), their negatives, +-0, +-inf, NaN, subnormal thresholds, the smallest and the largest
normal float, and thresholds whose bound overflows (t * 450 > FLT_MAX: the bound is +inf)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'uav_airvision_amd', 'csrc')
DEN = np.float32(450.0)
KEY_NINF, KEY_PINF = 0x007FFFFF, 0xFF800000          # ordered keys of -inf and +inf (lk_host.h, av_lk_float_key)


def configured():
    """The float the library passes for minEigThreshold = 1e-4: the smallest float >= the double."""
    up = np.float32(1e-4)
    return up if float(up) >= 1e-4 else np.nextafter(up, np.float32(np.inf))


def thresholds():
    t = [np.float32(m * 10.0 ** e) for e in range(-14, 7) for m in (1.0, 3.3333333, 9.999999)]
    t += [-x for x in t[::5]]
    t += [configured(), np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    t += [np.float32(1e-45), np.float32(1e-42), np.float32(-1e-42), np.finfo(np.float32).tiny, np.finfo(np.float32).max,
          np.float32(1e36), np.float32(8e35), np.float32(-3e38)]
    return np.array(t, np.float32)


def key_to_float(k):
    k = np.asarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k)
    return b.astype(np.uint32).view(np.float32)


def float_to_key(x):
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


@pytest.fixture(scope='module')
def bounds(tmp_path_factory):
    exe = tmp_path_factory.mktemp('lk_bound') / 'lk_bound_test'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'lk_bound_harness.cpp'), '-o', str(exe)])
    t = thresholds()
    out = subprocess.run([str(exe)] + ['%08x' % b for b in t.view(np.uint32)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    assert len(rows) == len(t)
    assert [int(r[0], 16) for r in rows] == [int(b) for b in t.view(np.uint32)]
    X = np.array([int(r[1], 16) for r in rows], np.uint32).view(np.float32)
    return t, X, np.array([int(r[2]) for r in rows]), np.array([int(r[3]) for r in rows])


def test_the_program_finds_no_mismatch_within_64_ulps(bounds):
    t, X, checked, bad = bounds
    assert (checked >= 65 + 3).all()                                 # 64 ulps to the side that exists, X itself, +-inf and NaN
    assert not bad.any(), [(float(a), float(b), int(c)) for a, b, c in zip(t, X, bad) if c]


def test_numpy_division_agrees_within_64_ulps(bounds):
    t, X, _, _ = bounds
    n_checked = 0
    with np.errstate(all='ignore'):
        for ti, Xi in zip(t, X):
            if np.isnan(Xi):
                continue
            kx = int(float_to_key(Xi))
            keys = np.arange(max(kx - 64, KEY_NINF), min(kx + 64, KEY_PINF) + 1, dtype=np.int64).astype(np.uint32)
            x = np.concatenate([key_to_float(keys), np.array([-np.inf, np.inf, np.nan], np.float32)])
            q = x / DEN
            assert q.dtype == np.float32
            assert np.array_equal(q < ti, x < Xi), (float(ti), float(Xi))
            n_checked += len(x)
    assert n_checked > 60 * 100


def test_special_thresholds(bounds):
    t, X, _, _ = bounds
    by = {int(a): b for a, b in zip(t.view(np.uint32), X)}
    f = lambda v: int(np.float32(v).view(np.uint32))
    assert np.isnan(by[f(np.nan)])                                      # NaN: x < NaN fails nothing, as fl(x / 450) < NaN does
    assert by[f(np.inf)] == np.inf and by[f(-np.inf)] == -np.inf        # everything below +inf passes; nothing is below -inf
    assert by[f(1e36)] == np.inf and by[f(np.finfo(np.float32).max)] == np.inf      # 450 t overflows: every finite x is below
    with np.errstate(all='ignore'):
        for z in (0.0, -0.0):                                           # the smallest x whose quotient rounds to -0: negative, subnormal
            Xz = by[f(z)]
            assert Xz < 0 and abs(Xz) < np.finfo(np.float32).tiny and Xz / DEN == 0 and np.nextafter(Xz, np.float32(-np.inf)) / DEN < 0
    # the configured threshold: the bound is 450 t to within a few ulps
    Xc = by[f(configured())]
    assert abs(float(Xc) - 450 * float(configured())) < 4 * np.spacing(np.float32(0.045))
