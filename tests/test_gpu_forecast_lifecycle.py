"""What a batched filter with the forecast on (include/airvision.h, "Forecast") holds on the device from create to close, read through
av_debug_live_resources, in the manner of tests/test_gpu_lifecycle.py: four zeros before, the counts above zero while it steps, four
zeros after close(), a second cycle that peaks at the same counts -- and no growth of the IMU staging over a run whose pending count
goes from nothing to two frames' worth and back: it is sized for n_streams * cap pending samples when it is first built."""
import ctypes

import pytest

import filter_harness as H
import forecast_harness as Fh

pytestmark = pytest.mark.gpu

N = 8


def live():
    from uav_airvision_amd import _native as Nat
    out = (ctypes.c_int64 * 4)()
    Nat.check(Nat.lib().av_debug_live_resources(ctypes.byref(out)))
    return tuple(int(v) for v in out)


def test_filter_with_the_forecast_on_releases_everything_and_never_grows(cfg):
    streams = Fh.streams3(cfg, N)[:2]
    rows = H.schedule(streams, N)
    # pushed ahead of step 0 .. 7: frame 0 | frames 1, 2, 3 | - | - | frames 4, 5 | - | frame 6 | frame 7
    pushed = [rows[0], rows[1] + rows[2] + rows[3], [], [], rows[4] + rows[5], [], rows[6], rows[7]]
    peaks = []
    for _ in range(2):
        assert live() == (0, 0, 0, 0)
        peak = [0, 0, 0, 0]

        def check(k, bat, out, cur):
            peak[:] = [max(a, b) for a, b in zip(peak, live())]
            if k == 5:
                bat.restart([1])                              # (a restart allocates nothing)
        run = Fh.run(cfg, streams, N, lead=0, rows=pushed, check=check, others=('odom_cov', 'landmarks', 'stats', 'imu_rate'))
        had = [int(n[0, 0]) for _, n, _ in run['fcs']]
        assert had[0] == 0 and had[1] > had[2] > had[3] == 0 and had[4] > 0 and had[5] == 0, had
        assert max(had) <= Fh.FC_CAP and run['fcs'][1][1][0].tolist() == [had[1], had[1]]
        assert run['counters']['devbuf_growths'] == 0, run['counters']
        assert live() == (0, 0, 0, 0), 'alive after close'
        assert all(v > 0 for v in peak[:3]), peak
        peaks.append(list(peak))
    assert peaks[0] == peaks[1], peaks
