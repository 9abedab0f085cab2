"""What a batched filter with the IMU-rate odometry on (include/airvision.h, "IMU-rate odometry") holds on the device from create to
close, read through av_debug_live_resources, in the manner of tests/test_gpu_lifecycle.py: four zeros before, the counts above zero
while it steps, four zeros after close(), and a second cycle that peaks at the same counts."""
import ctypes

import pytest

import imu_rate_harness as Ih

pytestmark = pytest.mark.gpu


def live():
    from uav_airvision_amd import _native as N
    out = (ctypes.c_int64 * 4)()
    N.check(N.lib().av_debug_live_resources(ctypes.byref(out)))
    return tuple(int(v) for v in out)


def test_filter_with_the_records_on_releases_everything(cfg):
    streams = Ih.streams3(cfg, 8)[:2]
    peaks = []
    for _ in range(2):
        assert live() == (0, 0, 0, 0)
        peak = [0, 0, 0, 0]

        def check(k, bat, out, cur):
            peak[:] = [max(a, b) for a, b in zip(peak, live())]
            if k == 5:
                bat.restart([1])                              # (a restart allocates nothing)
        run = Ih.run(cfg, streams, 8, check=check, others=('odom_cov', 'landmarks', 'stats'))
        assert sum(int(n[:, 1].sum()) for _, n in run['irs']) > 20
        assert live() == (0, 0, 0, 0), 'alive after close'
        assert all(v > 0 for v in peak[:3]), peak
        peaks.append(list(peak))
    assert peaks[0] == peaks[1], peaks
