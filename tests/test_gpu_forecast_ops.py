"""The forecast's two kernels (include/airvision.h, "Forecast") through av_msckf_forecast_ops_dev, the tests-only entry that launches them
through the step's own helper, against the 50-digit reference (tests/forecast_ref.py) on the cases of tests/msckf_predict_cases.py: the
case's state is the state a step leaves, its IMU samples are the pending ones.

Bars (none from the code under test): every record's q (sign-aligned), p, v may be 16 e_fam off, e_fam what the fp64 oracle achieves
against the reference on the family, floored at 4 ulp (msckf_predict_cases.bars); the covariance record entry by entry relative to
sqrt(C_ii C_jj) of the reference's record, 16 times the oracle's own record error over the family (forecast_ref.bars).  Exact: t and w,
the counts, the rule of the cap (the FIRST cap samples), the pre-fill behind the written records and around every stream, and that
nothing the filter reads is written: P with its cross blocks and the pre-fill outside a stream's square, and the state arrays, come back
bit for bit.  Every test prints its figures (FORECAST lines).

Measured on an MI355X, the largest error of any record or covariance entry as a fraction of its bar: family samples q 0.021, p 0.017,
v 0.019, C 0.059; rate 0.014, 0.006, 0.006, 0.069; sparsity 0.012, 0.007, 0.012, 0.070; gap 0.003, 0.099 (p), 0.116 (v, across the 20-s
sample), 0.074; the cut chains C 0.006 (cap 1) and 0.032 (cap 4)."""
import numpy as np
import pytest

import forecast_ref as Fr
import msckf_predict_cases as Pc

pytestmark = pytest.mark.gpu

LD = Pc.LD
CAP = 32
DFAIL_STACK = 3


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


def _raw(rec):
    return np.ascontiguousarray(rec).view(np.float64).reshape(rec.shape + (14,))


def _launch(dev, cases, cap, **over):
    """All `cases` as the streams of one launch, everything around a stream's own covariance NaN.  over: {stream: dict of state fields}.
    -> (result, the streams and P as they went in)."""
    from uav_airvision_amd.msckf_ops import MsckfDevice
    S = len(cases)
    P = np.full((S, LD, LD), np.nan)
    streams, imu, first = [], [], 0
    for s, c in enumerate(cases):
        P[s, :c['n'], :c['n']] = c['P']
        st = dict(c['state'], n=c['n'], ncam=c['ncam'], null_aliased=0, pend_first=first, pend_cnt=len(c['imu']))
        st.update(over.get('s%d' % s, {}))
        streams.append(st)
        first += len(c['imu'])
        imu.append(c['imu'])
    out = dev.forecast_ops_dev(streams, np.concatenate(imu), P, cases[0]['noise'], cap)
    # read-only: the covariance (cross blocks, camera blocks, the pre-fill around every stream) and the state come back bit for bit
    assert np.array_equal(out['P'].view(np.uint64), P.view(np.uint64))
    for st, back in zip(streams, out['streams']):
        assert all(_bits(st[f], back[f]) for f, _ in MsckfDevice.STATE_FIELDS)
        assert all(back[f] == st.get(f, 1 if f == 'active' else 0) for f in MsckfDevice.STATE_INTS)
    return out


def _check_stream(out, s, case, cap, where):
    """Counts, the exact fields and the pre-fill of stream s; -> its written records."""
    had = len(case['imu'])
    wr = min(had, cap)
    assert out['n'][s].tolist() == [had, wr], (where, out['n'][s].tolist())
    rec = out['rec'][s]
    assert np.isnan(_raw(rec[wr:])).all(), where                # records past `written` keep their pre-fill
    got = rec[:wr]
    assert np.isfinite(_raw(got)).all() and np.isfinite(out['cov'][s]).all(), where
    kept = case['imu'][:wr]                                      # the FIRST cap samples
    assert _bits(got['t'], kept[:, 0]) and _bits(got['w'], kept[:, 1:4] - case['state']['bg']), where
    return got


def _errors(out, s, case, cap, full=None):
    from uav_airvision_amd.msckf_ops import unpack_odom_cov
    ref = Fr.mp_forecast(case, cap, full=full)
    got = out['rec'][s][:out['n'][s, 1]]
    assert len(got) == len(ref['states'])
    e = dict(q=0.0, p=0.0, v=0.0, C=Fr.rec_err(unpack_odom_cov(out['cov'][s]), ref['C']))
    for g, want in zip(got, ref['states']):
        for f in ('q', 'p', 'v'):
            e[f] = max(e[f], Pc.vec_err(g[f], want[f], quaternion=f == 'q'))
    return e


@pytest.mark.parametrize('name', Fr.FAMILIES)
def test_every_record_and_the_covariance_against_the_50_digit_reference(dev, cfg, name):
    """samples: 0, 1, 10 and 17 pending; rate: both sides of the 1e-5 rad/s branch; sparsity: a sample with dt = 0; gap: 20 s."""
    cases, bars, refs = Pc.family(name, cfg), Fr.bars(name, cfg), Pc.reference(name, cfg)
    assert not any(r['left_out'] for r in refs)
    out = _launch(dev, cases, CAP)
    worst = dict(q=0.0, p=0.0, v=0.0, C=0.0)
    for s, (case, r) in enumerate(zip(cases, refs)):
        _check_stream(out, s, case, CAP, case['name'])
        e = _errors(out, s, case, CAP, full=r['ref'])
        worst = {f: max(worst[f], e[f]) for f in worst}
    for f in worst:
        print('FORECAST %s dev %s e_fam %.2e worst %.2e ratio %.3f' % (name, f, bars[f], worst[f], worst[f] / (Pc.FACTOR * bars[f])))
    assert all(worst[f] <= Pc.FACTOR * bars[f] for f in worst), (name, worst, bars)


def test_nothing_pending_is_the_map_of_the_state_and_block_the_step_leaves(dev, cfg):
    from odom_cov_ref import odom_cov, odom_cov_bound
    from uav_airvision_amd.msckf_ops import unpack_odom_cov
    case = Pc.family('samples', cfg)[2]
    assert len(case['imu']) == 0
    out = _launch(dev, [case], CAP)
    assert out['n'][0].tolist() == [0, 0] and np.isnan(_raw(out['rec'][0])).all()
    st = case['state']
    want, bound = odom_cov(case['P'], st['q'], st['R_ic'], st['t_ci']), odom_cov_bound(case['P'], st['q'], st['R_ic'], st['t_ci'])
    assert (np.abs(unpack_odom_cov(out['cov'][0]) - want) <= 64 * Pc.EPS * bound).all()


@pytest.mark.parametrize('cap', (1, 4))
def test_the_cap_keeps_the_first_samples(dev, cfg, cap):
    """cap 1 and cap 4 against 10 pending: (10, cap), the records bit for bit the first ones of the same case at cap = 32, the
    covariance that of the cut chain (its own 50-digit reference), nothing behind the written rows."""
    case = Pc.family('samples', cfg)[0]
    big, small = _launch(dev, [case], CAP), _launch(dev, [case], cap)
    assert small['n'][0].tolist() == [10, cap] and big['n'][0].tolist() == [10, 10]
    got = _check_stream(small, 0, case, cap, cap)
    assert got.tobytes() == big['rec'][0][:cap].tobytes()
    bars, e = Fr.bars('samples', cfg), _errors(small, 0, case, cap)
    print('FORECAST cap=%d C ratio %.3f' % (cap, e['C'] / (Pc.FACTOR * bars['C'])))
    assert all(e[f] <= Pc.FACTOR * bars[f] for f in e), (cap, e, bars)
    assert not _bits(small['cov'][0], big['cov'][0])


def test_a_repeated_stamp_still_gets_a_record(dev, cfg):
    case = Pc.family('sparsity', cfg)[2]
    out = _launch(dev, [case], CAP)
    got = _check_stream(out, 0, case, CAP, 'dt0')
    assert len(got) == 4 and got[2]['t'] == got[1]['t'] and _bits(got[2]['p'], got[1]['p']) and _bits(got[2]['v'], got[1]['v'])


def test_a_full_window_of_23_cameras_is_read_and_left_alone(dev, cfg):
    """ncam = 23 (n = 159): the forecast reads the 21 x 21 block out of a covariance with 138 more rows and columns and writes none of
    it (_launch compares every bit); its result is that of the same block alone."""
    case = Pc.family('large', cfg)[2]
    assert case['ncam'] == 23
    alone = dict(case, P=case['P'][:21, :21], n=21, ncam=0, name=case['name'] + '/21')
    out, cut = _launch(dev, [case], CAP), _launch(dev, [alone], CAP)
    _check_stream(out, 0, case, CAP, 'ncam23')
    assert out['rec'].tobytes() == cut['rec'].tobytes() and _bits(out['cov'], cut['cov'])
    bars, e = Fr.bars('samples', cfg), _errors(out, 0, case, CAP)
    assert all(e[f] <= Pc.FACTOR * bars[f] for f in e), (e, bars)


def test_65_streams_cross_the_state_kernels_workgroup(dev, cfg):
    """Five distinct cases replicated to 65 streams: dk_forecast_state runs 64 lanes per workgroup, stream 64 is the second workgroup's
    only lane.  Every replica's rows are bit for bit its original's, and the originals meet the reference."""
    five = Pc.family('rate', cfg) + [Pc.family('sparsity', cfg)[2]]
    cases = [five[s % 5] for s in range(65)]
    out = _launch(dev, cases, CAP)
    for s in range(65):
        _check_stream(out, s, cases[s], CAP, s)
        assert out['rec'][s].tobytes() == out['rec'][s % 5].tobytes() and np.array_equal(out['n'][s], out['n'][s % 5]) and _bits(out['cov'][s], out['cov'][s % 5]), s
    for s in range(5):
        bars, e = Fr.bars('rate' if s < 4 else 'sparsity', cfg), _errors(out, s, cases[s], CAP)
        assert all(e[f] <= Pc.FACTOR * bars[f] for f in e), (s, e, bars)


def test_mixed_batch_idle_and_failed_streams_read_zero_and_nan(dev, cfg):
    """Streams of different pending counts in one launch, among them an inactive one and one that has failed: those two read {0, 0}, a
    NaN covariance row and keep every pre-filled byte of their records; every other stream has the rows it has alone."""
    small = Pc.family('samples', cfg)
    cases = [small[1], Pc.family('rate', cfg)[3], small[3], Pc.family('sparsity', cfg)[1], small[2], small[0]]
    out = _launch(dev, cases, CAP, s1=dict(active=0), s3=dict(failed=DFAIL_STACK))
    for s in (1, 3):
        assert out['n'][s].tolist() == [0, 0], s
        assert np.isnan(_raw(out['rec'][s])).all() and np.isnan(out['cov'][s]).all(), s
    for s in (0, 2, 4, 5):
        _check_stream(out, s, cases[s], CAP, s)
        alone = _launch(dev, [cases[s]], CAP)
        assert out['rec'][s].tobytes() == alone['rec'][0].tobytes() and np.array_equal(out['n'][s], alone['n'][0]) and _bits(out['cov'][s], alone['cov'][0]), s


def test_arguments_are_checked(dev, cfg):
    from uav_airvision_amd import _native as N
    case = Pc.family('samples', cfg)[3]
    for cap in (0, 4097):
        with pytest.raises(N.AirvisionError) as e:
            _launch(dev, [case], cap)
        assert e.value.code == N.AV_E_INVALID
    with pytest.raises(N.AirvisionError) as e:                   # pending samples outside the sample array
        _launch(dev, [case], CAP, s0=dict(pend_cnt=2))
    assert e.value.code == N.AV_E_INVALID
