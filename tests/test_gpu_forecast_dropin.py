"""The drop-in MSCKF with config.publish_forecast (include/airvision.h, "Forecast"): `last_forecast` after every feature_callback holds
the forecast records of a one-stream BatchedMSCKF fed the same, bit for bit for T_imu_body = identity; with a T_imu_body that rotates
and shifts, p, q, v are mapped the way `publish` maps the pose and the velocity -- exactly as `last_imu_states` maps them
(tests/test_gpu_imu_rate.py) -- t and w keep their bits, and the covariance, which is not conjugated into a body frame, is withheld;
together with config.publish_covariance such a T_imu_body is refused the way publish_covariance refuses it.  vio_result is what it was."""
import os

import numpy as np
import pytest

import filter_harness as H
import forecast_harness as Fh

pytestmark = pytest.mark.gpu

N = 12


def _dropin():
    import sys
    from conftest import ROOT
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import msckf as dmsckf
    return dmsckf


def test_dropin_last_forecast_is_the_batch_forecast_mapped_by_T_imu_body(cfg):
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.msckf_ops import unpack_forecast
    dmsckf = _dropin()
    from utils import Isometry3d, to_rotation
    stream = Fh.streams3(cfg, N)[0]
    base = Fh.run(cfg, [stream], N)
    ahead = Fh.lead_rows(H.schedule([stream], N), 1)
    c = ConfigEuRoC()
    assert c.publish_forecast is False and c.forecast_cap == 32
    off = dmsckf.MSCKF(c, write_trajectory=False)
    assert off.last_forecast is None and off.last_forecast_covariance is None
    off.close()
    ang = 0.3
    T = np.identity(4)
    T[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.1, -0.2, 0.05]
    for body in (None, T):
        c = ConfigEuRoC()
        c.publish_forecast, c.forecast_cap = True, Fh.FC_CAP
        if body is not None:
            c.T_imu_body = body
        flt = dmsckf.MSCKF(c, write_trajectory=False)
        got = []
        try:
            for k in range(N):
                for _, m in ahead[k]:
                    flt.imu_callback(m)
                r = flt.feature_callback(stream.frame(k))
                assert r is None or r._fields == ('timestamp', 'pose', 'velocity', 'cam0_pose')
                got.append((flt.last_forecast.copy(), flt.last_forecast_pending, flt.last_forecast_covariance, r))
        finally:
            flt.close()
        assert sum(len(g[0]) for g in got) > 80
        for k, (g, pending, C15, r) in enumerate(got):
            want, Cw, _ = unpack_forecast(*base['fcs'][k], 0)
            assert pending == tuple(base['fcs'][k][1][0].tolist()) and len(g) == len(want), k
            if body is None:
                assert g.tobytes() == want.tobytes(), k
                assert (C15 is None) == (r is None) and (r is None or H.same(C15, Cw)), k
                continue
            assert C15 is None, k                                 # not conjugated into a body frame: withheld
            assert g['t'].tobytes() == want['t'].tobytes() and g['w'].tobytes() == want['w'].tobytes(), k
            B = Isometry3d(T[:3, :3], T[:3, 3])
            for a, b in zip(g, want):
                P = B * Isometry3d(to_rotation(b['q']).T, b['p']) * B.inverse()
                assert np.abs(a['p'] - P.t).max() <= 1e-12 and np.abs(to_rotation(a['q']).T - P.R).max() <= 1e-12 and np.abs(a['v'] - T[:3, :3] @ b['v']).max() <= 1e-12, k


def test_a_body_frame_is_refused_together_with_the_covariance():
    from uav_airvision_amd.config import ConfigEuRoC
    dmsckf = _dropin()
    c = ConfigEuRoC()
    c.publish_forecast, c.publish_covariance = True, True
    T = np.identity(4)
    T[:3, 3] = [0.1, 0.0, 0.0]
    c.T_imu_body = T
    with pytest.raises(ValueError, match='T_imu_body'):
        dmsckf.MSCKF(c, write_trajectory=False)
    c.publish_forecast = False
    with pytest.raises(ValueError, match='T_imu_body'):          # (the refusal publish_covariance has always made)
        dmsckf.MSCKF(c, write_trajectory=False)
