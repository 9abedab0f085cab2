"""The zero-velocity detector (include/airvision.h, "Zero-velocity update": dk_zupt_detect) inside real steps of the batched filter, on
crafted IMU samples and feature messages: the counts and flags of read_zupt() after every step, exactly those of tests/zupt_ref.py.

Every crafted quantity lies a factor of two on either side of its threshold, never an ulp: displacements of dm / 2 and 2 dm, rates of
gyro_max / 2 and 2 gyro_max, an accelerometer deviation of 2 acc_dev_max.  Feature ids are unique within a message.  Both launch shapes
of the step's per-stream kernels run (AV_DK_WG, read when a batch prepares its device path: set around the batch as
tests/filter_harness.py does for every suite of the filter); the detector itself is one wavefront per stream in both."""
import numpy as np
import pytest

import filter_harness as H
import zupt_ref as Z

pytestmark = pytest.mark.gpu

G = 9.81
T0, FRAME_DT = 100.0, 0.05


class Crafted(object):
    """A stream with the interface of synth.SyntheticFeatureStream whose frames and IMU samples are listed by hand.  plan[k] =
    dict(ids=[...], moved={id: factor of dm}, imu=count, loud={sample index: ('w' | 'a')}): frame k observes `ids`; an id seen in the
    previous frame sits where it sat there, displaced along u by its factor of dm (default 1 / 2, alternating sign so nothing drifts
    far); the frame's IMU samples are quiet (|w| = gyro_max / 2 on top of a zero bias, |a| = g) except the loud ones (|w| = 2 gyro_max,
    or |a| = g + 2 acc_dev_max)."""

    def __init__(self, params, plan, seed=0):
        from uav_airvision_amd.synth import _Meas, feature_msg_t, imu_msg_t
        rng = np.random.default_rng(seed)
        dm = params['disparity_max']
        self.n_frames = len(plan)
        # 220 samples at rest before frame 0: the gyro bias they average to is exactly zero (pairs of opposite samples)
        self.imu = []
        for j in range(220):
            t = T0 - 1.2 + (j + 1) * 0.005
            w = np.array([1e-3, -2e-3, 5e-4]) * (1 if j % 2 == 0 else -1)
            self.imu.append(imu_msg_t(t, w, np.array([0.0, 0.0, G])))
        self._msgs, pos = [], {}
        for k, fr in enumerate(plan):
            t = T0 + k * FRAME_DT
            cnt = fr.get('imu', 10)
            for j in range(cnt):
                ts = t - FRAME_DT + (j + 1) * FRAME_DT / (cnt + 1)
                kind = fr.get('loud', {}).get(j)
                axis = np.array([0.6, 0.0, 0.8])
                w = axis * params['gyro_max'] * (2.0 if kind == 'w' else 0.5) * (1 if j % 2 == 0 else -1)      # (alternating: no net rotation)
                a = np.array([0.0, 0.0, G + (2.0 * params['acc_dev_max'] if kind == 'a' else 0.0)])
                if k > 0:
                    self.imu.append(imu_msg_t(ts, w, a))
            feats, new = [], {}
            for fid in fr['ids']:
                if fid in pos:
                    u, v = pos[fid]
                    u = u + dm * fr.get('moved', {}).get(fid, 0.5) * (1 if k % 2 else -1)
                else:
                    u, v = rng.uniform(-0.5, 0.5), rng.uniform(-0.35, 0.35)
                m = _Meas()
                m.id, m.u0, m.v0, m.u1, m.v1 = fid, u, v, u - 0.022, v
                feats.append(m)
                new[fid] = (u, v)
            pos = new
            self._msgs.append(feature_msg_t(t, feats))

    def frame(self, k):
        return self._msgs[k]


def _plan():
    a = list(range(10))                         # ten features that live through the whole run
    b = list(range(100, 105))
    big = list(range(1000, 1120))
    c = a[:9] + b[:1]                           # the ten that are left from frame 5 on
    return [
        dict(ids=a, imu=0),                                                   # 0  the first live frame: nothing tracked
        dict(ids=a),                                                          # 1  10 of 10 still, 10 quiet samples: detected
        dict(ids=a, moved={3: 2.0}),                                          # 2  9 of 10 still: 90 %, detected
        dict(ids=a, moved={3: 2.0, 7: 2.0}),                                  # 3  8 of 10: vision fails
        dict(ids=a[:9] + b),                                                  # 4  9 tracked = min_tracks - 1: vision fails
        dict(ids=a[:9] + b[:1]),                                              # 5  10 tracked = min_tracks: detected
        dict(ids=a[:9] + b[:1] + big, imu=70),                                # 6  130 entries, 10 of them tracked; 70 quiet samples: both loops stride
        dict(ids=a[:9] + b[:1] + big, imu=1),                                 # 7  130 tracked entries, one sample
        dict(ids=a[:9] + b[:1] + big, moved={fid: 2.0 for fid in big[60:80]}),    # 8  110 of 130 still (84 %), the moved ones past lane 63: vision fails
        dict(ids=c, loud={4: 'w'}),                                           # 9  one sample at twice the rate: IMU fails
        dict(ids=c, loud={6: 'a'}),                                           # 10 one sample at twice the accelerometer deviation
        dict(ids=c, imu=0),                                                   # 11 no sample: IMU fails
        dict(ids=c, imu=70, loud={66: 'w'}),                                  # 12 the loud sample in the loop's second trip
        dict(ids=c),                                                          # 13 detected again
    ]


WANT = {0: (0, 0, 0, False), 1: (10, 10, 10, True), 2: (10, 10, 9, True), 3: (10, 10, 8, False), 4: (10, 9, 9, False), 5: (10, 10, 10, True),
        6: (70, 10, 10, True), 7: (1, 130, 130, True), 8: (10, 130, 110, False), 9: (10, 10, 10, False), 10: (10, 10, 10, False),
        11: (0, 10, 10, False), 12: (70, 10, 10, False), 13: (10, 10, 10, True)}      # frame: n_imu, n_tracked, n_still, detected


def _same(rec, ref, where):
    """A record of read_zupt against the oracle's: integers and flags exactly, the detector's doubles to rounding."""
    for f in ('flags', 'n_imu', 'n_tracked', 'n_still', 'detected_total', 'applied_total'):
        assert int(rec[f]) == int(ref[f]), (where, f, rec, ref)
    for f in ('w_max', 'a_dev_max'):
        assert abs(rec[f] - ref[f]) <= 1e-9 * max(abs(ref[f]), 1e-3), (where, f, rec, ref)


@pytest.mark.parametrize('wg', (256, 64))
def test_counts_and_flags_on_crafted_frames(cfg, wg):
    params = Z.params_of(cfg)
    plan = _plan()
    streams = [Crafted(params, plan)]
    seen = []

    def check(k, bat, out, cur):
        rec = bat.read_zupt()[0]
        ref = cur['ref'][0]
        _same(rec, ref, (wg, k))
        seen.append((int(rec['n_imu']), int(rec['n_tracked']), int(rec['n_still']), bool(rec['flags'] & Z.DETECTED)))

    run = H.run(cfg, streams, len(plan), cap=192, oracle=Z.ZuptOracle, oracle_step=lambda o, r, reset: dict(o.record), check=check,
                env={'AV_DK_WG': '64'} if wg == 64 else {}, zupt=True)
    assert run['shape'] == [(1, wg)]
    assert all(o[0, 0] == 1.0 for o in run['outs'])
    assert dict(enumerate(seen)) == WANT
    # what fails is what was crafted to fail
    flags = [r[0]['flags'] for r in run['refs']]
    assert [bool(f & Z.IMU_OK) for f in flags] == [k not in (0, 9, 10, 11, 12) for k in range(len(plan))]
    assert [bool(f & Z.VIS_OK) for f in flags] == [k not in (0, 3, 4, 8) for k in range(len(plan))]


def test_the_frame_after_an_online_reset_tracks_nothing(cfg):
    """position_std_threshold = 0.012 makes online_reset fire (as in tests/test_gpu_msckf.py): the store is cleared, so the next frame
    has no previous observation.  Two streams, one of them not yet live in the first frames: its record is zero."""
    import copy
    from uav_airvision_amd.synth import SyntheticFeatureStream
    c = copy.copy(cfg)
    c.position_std_threshold = 0.012
    n_frames = 40
    streams = [SyntheticFeatureStream(c, seed=31, n_frames=n_frames, n_features=60), SyntheticFeatureStream(c, seed=32, n_frames=n_frames, n_features=60)]
    after_reset, idle = [], []

    def check(k, bat, out, cur):
        rec = bat.read_zupt()
        for i in range(2):
            ref, reset, live = cur['ref'][i]
            _same(rec[i], ref, (k, i))
            if not live:
                assert out[i, 0] == 0.0 and H.zero(rec[i])
                idle.append(k)
            if k > 0 and prev[i]:
                after_reset.append(int(rec[i]['n_tracked']))
            prev[i] = reset

    prev = [False, False]
    H.run(c, streams, n_frames, cap=192, oracle=Z.ZuptOracle, oracle_step=lambda o, r, reset: (dict(o.record), reset, r is not None), check=check,
          withhold={1: 6}, zupt=True)
    assert len(after_reset) >= 1 and all(n == 0 for n in after_reset) and len(idle) >= 5
