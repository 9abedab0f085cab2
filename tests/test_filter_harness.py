"""tests/filter_harness.py itself, on the CPU: what `schedule`, `messages` and `arrays` hand a step, on two feature streams whose IMU
and frame rates differ."""
import numpy as np
import pytest

from filter_harness import arrays, messages, schedule

N = 12
CAP = 16


class _Thinned(object):
    """Every imu_step-th IMU sample and every frame_step-th frame of a SyntheticFeatureStream."""

    def __init__(self, base, imu_step, frame_step):
        self.base, self.frame_step = base, frame_step
        self.imu = base.imu[::imu_step]

    def frame(self, k):
        return self.base.frame(k * self.frame_step)


@pytest.fixture(scope='module')
def streams():
    """Stream 0: 20 frames and every IMU sample per second; stream 1, 7 ms later: every second frame, every third IMU sample."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticFeatureStream
    cfg = ConfigEuRoC()
    a = SyntheticFeatureStream(cfg, seed=1, n_frames=N, n_features=6)
    b = _Thinned(SyntheticFeatureStream(cfg, seed=2, n_frames=2 * N, n_features=9, t0=100.007), 3, 2)
    assert len(a.imu) > 2 * len(b.imu) > 100 and b.frame(1).timestamp - b.frame(0).timestamp > 1.5 * (a.frame(1).timestamp - a.frame(0).timestamp)
    return [a, b]


def _per_stream(rows, i):
    return [[m for j, m in row if j == i] for row in rows]


def test_schedule_delivers_every_sample_once_in_order_before_its_frame(streams):
    rows = schedule(streams, N)
    assert len(rows) == N
    for i, st in enumerate(streams):
        got = _per_stream(rows, i)
        times = [st.frame(k).timestamp for k in range(N)]
        want = [m for m in st.imu if m.timestamp <= times[-1]]
        flat = [m for row in got for m in row]
        assert len(flat) == len(want) and all(x is y for x, y in zip(flat, want)), i          # every one, once, in order
        assert len(want) < len(st.imu)                                                         # (later samples exist and stay out)
        for k, row in enumerate(got):
            for m in row:
                assert m.timestamp <= times[k] and (k == 0 or m.timestamp > times[k - 1]), (i, k)      # the first frame that is not earlier
        assert sum(bool(row) for row in got) == N, i


def test_withheld_samples_all_arrive_at_the_named_frame(streams):
    k0 = 5
    plain, held = schedule(streams, N), schedule(streams, N, withhold={1: k0})
    assert _per_stream(held, 0) == _per_stream(plain, 0)
    a, b = _per_stream(plain, 1), _per_stream(held, 1)
    assert all(not row for row in b[:k0])
    assert b[k0] == [m for row in a[:k0 + 1] for m in row] and len(b[k0]) > len(a[k0])
    assert b[k0 + 1:] == a[k0 + 1:]
    assert sum(len(r) for r in b) == sum(len(r) for r in a)


def test_arrays_gives_an_idle_stream_no_frame_and_leaves_its_neighbour_alone(streams):
    msgs = [st.frame(3) for st in streams]
    ids, uv, nf, ts = arrays(msgs, CAP)
    assert nf.tolist() == [len(m.features) for m in msgs] and min(nf) > 0 and ts.tolist() == [m.timestamp for m in msgs]
    for i, m in enumerate(msgs):
        assert ids[i, :nf[i]].tolist() == [f.id for f in m.features] and not ids[i, nf[i]:].any()
        assert uv[i, :nf[i]].tolist() == [[f.u0, f.v0, f.u1, f.v1] for f in m.features] and not uv[i, nf[i]:].any()
    for idle, other in ((0, 1), (1, 0)):
        ids2, uv2, nf2, ts2 = arrays(msgs, CAP, idle=[idle])
        assert ts2[idle] == -1.0 and nf2[idle] == 0 and not ids2[idle].any() and not uv2[idle].any()
        assert ts2[other] == ts[other] and nf2[other] == nf[other]
        assert np.array_equal(ids2[other], ids[other]) and np.array_equal(uv2[other], uv[other])
    ids3, uv3, nf3, ts3 = arrays([None, msgs[1]], CAP)                                         # (no message: no frame either)
    assert ts3.tolist() == [-1.0, ts[1]] and nf3.tolist() == [0, nf[1]] and np.array_equal(uv3[1], uv[1])


def test_messages_blanks_exactly_the_named_frames(streams):
    blank = {0: (2, 7), 1: (7,)}
    plain, got = messages(streams, N), messages(streams, N, blank=blank)
    assert len(plain) == len(got) == N
    for k in range(N):
        for i, st in enumerate(streams):
            assert plain[k][i] is st.frame(k)
            if k in blank[i]:
                assert got[k][i].timestamp == st.frame(k).timestamp and got[k][i].features == [] and st.frame(k).features
            else:
                assert got[k][i] is st.frame(k)
