"""dk_cov<64> has a body of its own (csrc/msckf.hip, "dk_cov<64>'s body": independent chains, nine stored rows of F and Phi, no G, no Q,
the cross block out of registers, the augmentation a lane per column); dk_cov<256> is still propagate_body + the staged cross block +
augment_body.  The two must give the same bits: same terms, same order, same fused multiply-adds.  Everything goes through the tests-only
entry av_msckf_predict_ops_dev with the harness of tests/test_gpu_msckf_predict.py (every stream's data surrounded by NaN), ONE launch per
workgroup size for all the cases below, the whole [S, ld, ld] array compared as 64-bit patterns:

 * IMU samples per frame 0, 1, 2, 10, 11 x camera states 0 (no cross block), 1, 10 (60 columns: one partial chunk), 11 (66: a second
   chunk of two columns), 20;
 * zero patterns: gyro exactly 0 (sparser F), one sample with dt = 0 among others, every dt = 0, a fresh filter's diagonal P with zero
   cross blocks and -0.0 entries among the zeros, P entries spanning 1e-12 .. 1e6;
 * an inactive stream between active ones.

Where the samples' states are available with dk_state's own bits -- the one-sample cases -- the IMU block is also held against the
operator entry av_msckf_propagate (propagate_kernel), as tests/test_gpu_msckf_predict.py measured it equal.  Closeness to the 50-digit
reference is that file's business; it runs both workgroup sizes."""
import numpy as np
import pytest

import msckf_predict_cases as Pc
import test_gpu_msckf_predict as H

pytestmark = pytest.mark.gpu

N_IMU = (0, 1, 2, 10, 11)
N_CAM = (0, 1, 10, 11, 20)


def _fresh(case):
    """A fresh filter's covariance: diagonal IMU block, the camera blocks of the case, every other entry zero, a symmetric third of
    the zeros negative."""
    n, P0 = case['n'], case['P']
    P = np.zeros((n, n))
    P[:21, :21] = np.diag(np.diag(P0)[:21])
    for b in range(21, n, 6):
        P[b:b + 6, b:b + 6] = P0[b:b + 6, b:b + 6]
    i, j = np.indices((n, n))
    neg = (P == 0) & ((i + j) % 3 == 0)
    P[neg] = -0.0
    assert np.signbit(P).sum() > n and (P[:21, 21:] == 0).all()
    return dict(case, P=P)


def _wide(case, seed):
    """Entries from 1e-12 to 1e6: the case's matrix rescaled by 10^u, u uniform in [-6, 3] per state."""
    n, P0 = case['n'], case['P']
    d = 10.0 ** np.random.default_rng(seed).uniform(-6, 3, n)
    d[:2], s = (1e-6, 1e3), np.sqrt(np.diag(P0))
    P = (d / s)[:, None] * P0 * (d / s)
    P = (P + P.T) / 2
    assert P.diagonal().min() < 2e-12 and P.diagonal().max() > 5e5
    return dict(case, P=P)


@pytest.fixture(scope='module')
def runs(cfg):
    """-> (cases, active flags, inputs, output at wg = 64, output at wg = 256, device): one launch per workgroup size."""
    from uav_airvision_amd.msckf_ops import MsckfDevice
    cases = [dict(Pc.make_case(4000 + 10 * i + j, cfg, ncam=k, n_imu=m), name='grid imu=%d cam=%d' % (m, k))
             for i, m in enumerate(N_IMU) for j, k in enumerate(N_CAM)]
    special = [
        dict(Pc.make_case(4101, cfg, ncam=2, n_imu=3, gyro='zero'), name='zero gyro'),
        dict(Pc.make_case(4102, cfg, ncam=1, n_imu=3, dt0=1), name='one dt = 0'),
        dict(Pc.make_case(4103, cfg, ncam=1, n_imu=2, dt=0.0), name='every dt = 0'),
        dict(_fresh(Pc.make_case(4104, cfg, ncam=3, n_imu=10)), name='fresh filter, -0.0'),
        dict(_fresh(Pc.make_case(4105, cfg, ncam=11, n_imu=1, gyro='zero')), name='fresh filter, -0.0, zero gyro, two chunks'),
        dict(_wide(Pc.make_case(4106, cfg, ncam=11, n_imu=10), 4107), name='1e-12 .. 1e6'),
    ]
    idle = dict(Pc.make_case(4108, cfg, ncam=2, n_imu=2), name='inactive')
    cases = cases[:7] + [idle] + cases[7:] + special
    active = [c is not idle for c in cases]
    dev = MsckfDevice(max_cam_states=24, rows_cap=64)
    out = {}
    for wg in H.WGS:
        streams = [H._stream(c) for c in cases]
        for s, a in zip(streams, active):
            s['active'] = int(a)
        out[wg] = H._launch(dev, cases, wg, streams)
    yield cases, active, out[64][0], out[64][1], out[256][1], dev
    dev.close()


def test_wg64_has_the_bits_of_wg256(runs):
    cases, active, inp, o64, o256, _ = runs
    total = 0
    for s, c in enumerate(cases):
        a, b = o64['P'][s].view(np.uint64), o256['P'][s].view(np.uint64)
        m = c['n'] + 6
        diff, changed = int((a != b).sum()), int((a[:m, :m] != inp['P'][s].view(np.uint64)[:m, :m]).sum())
        print('CHAINS %-42s n = %3d samples = %2d: %d of %d entries differ between wg 64 and 256; %d of the (n + 6)^2 changed by the step'
              % (c['name'], c['n'], len(c['imu']), diff, a.size, changed))
        total += diff
    assert total == 0
    for s, c in enumerate(cases):
        assert H._same_stream(o64, s, o256, s), c['name']
        if active[s]:
            H._check_exact(inp, o64, s, c, c['name'])            # symmetric, finite, the camera block and the NaN around it untouched
            m = c['n'] + 6
            assert (o64['P'][s, c['n']:m, :m] != 0).any(), c['name']
        else:
            assert all(H._bits(o64[k][s], inp[k][s]) for k in ('P', 'cam_q', 'cam_p', 'cam_qn')), c['name']


def test_one_sample_imu_block_has_the_bits_of_propagate_kernel(runs):
    """One sample: the frame's accumulated transition is that sample's, and the operator can be given the state dk_state computed."""
    cases, active, inp, o64, _, dev = runs
    seen = 0
    for s, c in enumerate(cases):
        if len(c['imu']) != 1 or not active[s]:
            continue
        st, st0, g = o64['streams'][s], c['state'], c['imu'][0]
        dev.set_cov(c['P'])
        dev.propagate(g[0] - st0['ts'], g[1:4] - st0['bg'], g[4:7] - st0['ba'], st0['q'], st['q'], st0['qn'], st0['vn'], st0['pn'], st['v'], st['p'],
                      st0['gravity'], c['noise'])
        op, got = dev.get_cov()[:21, :21], o64['P'][s, :21, :21]
        diff = int((np.ascontiguousarray(op).view(np.uint64) != np.ascontiguousarray(got).view(np.uint64)).sum())
        print('CHAINS %-42s P11 against propagate_kernel: %d of 441 entries differ' % (c['name'], diff))
        assert diff == 0, c['name']
        seen += 1
    assert seen >= len(N_CAM)
