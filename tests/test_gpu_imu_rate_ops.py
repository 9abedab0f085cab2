"""The IMU-rate records (include/airvision.h, "IMU-rate odometry") through av_msckf_predict_ops_dev_rate, the tests-only entry that
launches what a step of the device-resident filter begins with when the output is on -- dk_state, dk_imu_rate, dk_cov<wg> through the
step's own helper -- against the 50-digit reference, sample by sample.

Inputs, reference and bars: tests/msckf_predict_cases.py (families samples, rate, sparsity, gap) and tests/imu_rate_ref.py.  Every
record's q (sign-aligned), p, v may be 16 e_fam off, e_fam what the fp64 oracle achieves against the reference on the same family,
floored at 4 ulp: the bars test_gpu_msckf_predict.py holds the end-of-frame state to.  Exact: t and w (the sample's stamp, NumPy's
m.w - bg), the counts, the cap rule, the NaN pre-fill around every stream's written rows, and everything the entry shares with
av_msckf_predict_ops_dev (state, camera states, covariance).  Every test prints its figures (IMU-RATE lines).

Measured on an MI355X, the same at both workgroup sizes: the largest error of any record is 0.021 of its bar in the family samples,
0.014 in rate, 0.012 in sparsity, and 0.116 in gap (v, across the 20-s sample; p 0.099)."""
import numpy as np
import pytest

import imu_rate_ref as Ir
import msckf_predict_cases as Pc

pytestmark = pytest.mark.gpu

CS, LD = Pc.CAM_STRIDE, Pc.LD
WGS = (64, 256)
CAP = 32
FAMILIES = ('samples', 'rate', 'sparsity', 'gap')
DFAIL_CAMS, DFAIL_STACK = 1, 3


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    from uav_airvision_amd.msckf_ops import MsckfDevice
    d = MsckfDevice(max_cam_states=24, rows_cap=64)
    yield d
    d.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.size == b.size and np.array_equal(a.reshape(-1).view(np.uint64), b.reshape(-1).view(np.uint64))


def _stream(case, **kw):
    st = dict(case['state'], n=case['n'], ncam=case['ncam'], t_frame=case['t_frame'], imu_cnt=len(case['imu']))
    st.update(kw)
    return st


def _launch(dev, cases, wg, cap, streams=None):
    """All `cases` as the streams of one launch, everything around a stream's own data NaN; cap = 0: av_msckf_predict_ops_dev."""
    S = len(cases)
    streams = [_stream(c) for c in cases] if streams is None else [dict(s) for s in streams]
    P = np.full((S, LD, LD), np.nan)
    cq, cp, cqn = np.full((S, CS, 4), np.nan), np.full((S, CS, 3), np.nan), np.full((S, CS, 4), np.nan)
    imu, first = [], 0
    for s, c in enumerate(cases):
        n, k = c['n'], c['ncam']
        P[s, :n, :n] = c['P']
        cq[s, :k], cp[s, :k], cqn[s, :k] = c['cam_q'], c['cam_p'], c['cam_q']
        streams[s]['imu_first'] = first
        first += len(c['imu'])
        imu.append(c['imu'])
    return dev.predict_ops_dev(streams, np.concatenate(imu), cq, cp, cqn, P, cases[0]['noise'], wg, rate_cap=cap)


def _raw(rec):
    """IMU_STATE_DTYPE[...] -> float64[..., 14] over the same bytes."""
    return np.ascontiguousarray(rec).view(np.float64).reshape(rec.shape + (14,))


def _check_stream(out, s, case, cap, where):
    """Counts, the exact fields and the pre-fill of stream s; -> its written records."""
    had = len(case['imu'])
    wr = min(had, cap)
    assert out['imu_n'][s].tolist() == [had, wr], (where, out['imu_n'][s].tolist())
    rec = out['imu_rec'][s]
    assert np.isnan(_raw(rec[wr:])).all(), where                # nothing behind the written rows, up to the next stream's
    got = rec[:wr]
    assert np.isfinite(_raw(got)).all(), where
    kept = case['imu'][had - wr:]
    assert _bits(got['t'], kept[:, 0]) and _bits(got['w'], kept[:, 1:4] - case['state']['bg']), where
    return got


def _same_core(a, b):
    from uav_airvision_amd.msckf_ops import MsckfDevice
    for sa, sb in zip(a['streams'], b['streams']):
        if not (all(_bits(sa[f], sb[f]) for f, _ in MsckfDevice.STATE_FIELDS) and all(sa[f] == sb[f] for f in MsckfDevice.STATE_INTS)):
            return False
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ('P', 'cam_q', 'cam_p', 'cam_qn'))


_REF = {}


def _ref(case):
    if case['name'] not in _REF:
        _REF[case['name']] = Ir.mp_states(case)
    return _REF[case['name']]


@pytest.mark.parametrize('name', FAMILIES)
def test_every_record_against_the_50_digit_reference(dev, cfg, name):
    """The family's cases as the streams of one launch at both workgroup sizes: every record's q, p, v within 16 e_fam of the reference,
    t and w exact, the last record the state the entry returns, and the entry's other results those of av_msckf_predict_ops_dev."""
    cases, bars = Pc.family(name, cfg), Pc.bars(name, cfg)
    assert not any(r['left_out'] for r in Pc.reference(name, cfg))
    outs = []
    for wg in WGS:
        out, plain = _launch(dev, cases, wg, CAP), _launch(dev, cases, wg, 0)
        assert _same_core(out, plain), (name, wg)
        worst = dict(q=0.0, p=0.0, v=0.0)
        for s, case in enumerate(cases):
            got, ref = _check_stream(out, s, case, CAP, (case['name'], wg)), _ref(case)
            assert len(got) == len(ref)
            for k, (g, want) in enumerate(zip(got, ref)):
                for f in ('q', 'p', 'v'):
                    e = Pc.vec_err(g[f], want[f], quaternion=f == 'q')
                    worst[f] = max(worst[f], e)
            if len(got):
                st = out['streams'][s]
                assert _bits(got[-1]['q'], st['q']) and _bits(got[-1]['p'], st['p']) and _bits(got[-1]['v'], st['v']) and got[-1]['t'] == st['ts'], (case['name'], wg)
        for f in ('q', 'p', 'v'):
            print('IMU-RATE %s dev wg=%d %s e_fam %.2e worst %.2e ratio %.3f' % (name, wg, f, bars[f], worst[f], worst[f] / (Pc.FACTOR * bars[f])))
        assert all(worst[f] <= Pc.FACTOR * bars[f] for f in worst), (name, wg, worst, bars)
        outs.append(out)
    assert outs[0]['imu_rec'].tobytes() == outs[1]['imu_rec'].tobytes() and np.array_equal(outs[0]['imu_n'], outs[1]['imu_n']), name


def test_a_repeated_stamp_still_gets_a_record(dev, cfg):
    case = Pc.family('sparsity', cfg)[2]
    out = _launch(dev, [case], 64, CAP)
    got = _check_stream(out, 0, case, CAP, 'dt0')
    assert len(got) == 4 and got[2]['t'] == got[1]['t'] and _bits(got[2]['p'], got[1]['p']) and _bits(got[2]['v'], got[1]['v'])


@pytest.mark.parametrize('wg', WGS)
def test_65_streams_cross_the_state_kernels_workgroup(dev, cfg, wg):
    """Five distinct cases replicated to 65 streams: dk_state runs 64 lanes per workgroup, stream 64 is the second workgroup's only lane.
    Every replica's rows are bit for bit its original's, and the originals meet the reference."""
    five = Pc.family('rate', cfg) + [Pc.family('sparsity', cfg)[2]]
    cases = [five[s % 5] for s in range(65)]
    out = _launch(dev, cases, wg, CAP)
    for s in range(65):
        _check_stream(out, s, cases[s], CAP, (s, wg))
        assert out['imu_rec'][s].tobytes() == out['imu_rec'][s % 5].tobytes() and np.array_equal(out['imu_n'][s], out['imu_n'][s % 5]), (s, wg)
    for s in range(5):
        bars = Pc.bars('rate' if s < 4 else 'sparsity', cfg)
        for g, want in zip(out['imu_rec'][s][:out['imu_n'][s, 1]], _ref(cases[s])):
            for f in ('q', 'p', 'v'):
                e = Pc.vec_err(g[f], want[f], quaternion=f == 'q')
                assert e <= Pc.FACTOR * bars[f], (s, f, e)


@pytest.mark.parametrize('wg', WGS)
def test_mixed_batch_idle_streams_read_zero_and_nothing_leaks(dev, cfg, wg):
    """Streams of different sample counts in one launch, among them an inactive stream, a stream that has already failed and one whose
    window is full: those three read (0, 0) and keep every pre-filled byte of their rows; every other stream has the rows it has alone,
    and the pre-fill behind its written rows."""
    small, large = Pc.family('samples', cfg), Pc.family('large', cfg)
    full = Pc.make_case(991, cfg, ncam=CS, n_imu=2)
    cases = [large[0], Pc.family('rate', cfg)[3], small[3], Pc.family('sparsity', cfg)[1], full, small[2], small[1], small[0]]
    streams = [_stream(c) for c in cases]
    streams[1]['active'] = 0
    streams[3]['failed'] = DFAIL_STACK
    out = _launch(dev, cases, wg, CAP, streams)
    assert out['streams'][4]['failed'] == DFAIL_CAMS
    for s in (1, 3, 4):
        assert out['imu_n'][s].tolist() == [0, 0], (s, wg)
        assert np.isnan(_raw(out['imu_rec'][s])).all(), (s, wg)
    for s in (0, 2, 5, 6, 7):
        _check_stream(out, s, cases[s], CAP, (s, wg))
        alone = _launch(dev, [cases[s]], wg, CAP)
        assert out['imu_rec'][s].tobytes() == alone['imu_rec'][0].tobytes() and np.array_equal(out['imu_n'][s], alone['imu_n'][0]), (s, wg)


@pytest.mark.parametrize('wg', WGS)
def test_cap_4_keeps_the_last_four_in_order(dev, cfg, wg):
    """10 and 17 samples at cap = 4: counts (10, 4) and (17, 4), the four records bit for bit the last four of the same case at cap = 32;
    one sample and none: (1, 1) and (0, 0).  The state, camera states and covariance do not depend on the cap."""
    cases = Pc.family('samples', cfg)                          # 10, 17, 0, 1 samples
    big, small = _launch(dev, cases, wg, CAP), _launch(dev, cases, wg, 4)
    assert _same_core(big, small)
    assert small['imu_n'].tolist() == [[10, 4], [17, 4], [0, 0], [1, 1]], small['imu_n'].tolist()
    assert big['imu_n'].tolist() == [[10, 10], [17, 17], [0, 0], [1, 1]]
    for s, case in enumerate(cases):
        got = _check_stream(small, s, case, 4, (s, wg))
        had = len(case['imu'])
        assert got.tobytes() == big['imu_rec'][s][had - len(got):had].tobytes(), (s, wg)


def test_arguments_are_checked(dev, cfg):
    from uav_airvision_amd import _native as N
    case = Pc.family('samples', cfg)[3]
    with pytest.raises(N.AirvisionError) as e:
        _launch(dev, [case], 64, 4097)
    assert e.value.code == N.AV_E_INVALID
