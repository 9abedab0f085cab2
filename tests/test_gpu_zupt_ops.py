"""The zero-velocity update's kernel (include/airvision.h, "Zero-velocity update") through av_msckf_zupt_ops_dev, the tests-only entry that
launches it through the step's own helper, against the 50-digit reference on the cases of tests/zupt_cases.py.

Bars (none from the code under test): every injected quantity and P+ may be FACTOR = 16 times e_fam off, e_fam what the fp64 oracle
achieves against the reference over the cases, floored at 4 ulp (zupt_cases.bars).  Exact: P+ is bit-symmetric; the NaN pre-fill around
every stream's region and beyond n inside it is bit-intact; a stream that is not updated (not detected, inactive, failed, gated, bad S)
is bit for bit what went in; flags and totals.  Every test prints its figures (ZUPT lines)."""
import numpy as np
import pytest

import zupt_cases as Zc
import zupt_ref as Z

pytestmark = pytest.mark.gpu

LD = Zc.LD
CS = 24
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


def _launch(dev, cases, params=Zc.PARAMS, P_over=None, **over):
    """All `cases` as the streams of one launch at ld = 165, cam_stride = 24; everything around a stream's own n x n block, and every
    camera slot beyond its window, NaN.  over: {'s<k>': dict of stream fields}; P_over: {stream: function that edits its n x n block}.
    -> (result, the streams, cam_q, cam_p and P as they went in)."""
    S = len(cases)
    P = np.full((S, LD, LD), np.nan)
    cq, cp = np.full((S, CS, 4), np.nan), np.full((S, CS, 3), np.nan)
    streams = []
    for s, c in enumerate(cases):
        blk = c['P'].copy()
        if P_over and s in P_over:
            P_over[s](blk)
        P[s, :c['n'], :c['n']] = blk
        cq[s, :c['ncam']], cp[s, :c['ncam']] = c['cam_q'], c['cam_p']
        st = dict(c['state'], n=c['n'], ncam=c['ncam'], null_aliased=1, detected_total=3, applied_total=2)
        st.update(over.get('s%d' % s, {}))
        streams.append(st)
    out = dev.zupt_ops_dev(streams, cq, cp, P, params)
    return out, streams, cq, cp, P


def _untouched(out, s, streams, cq, cp, P):
    from uav_airvision_amd.msckf_ops import MsckfDevice
    back = out['streams'][s]
    return (all(_bits(streams[s][f], back[f]) for f, _ in MsckfDevice.STATE_FIELDS) and _bits(out['P'][s], P[s]) and
            _bits(out['cam_q'][s], cq[s]) and _bits(out['cam_p'][s], cp[s]))


def _frame_intact(out, s, n, ncam, cq, cp, P):
    """The pre-fill beyond n inside the stream's region, and the camera slots beyond its window."""
    m = np.ones((LD, LD), bool)
    m[:n, :n] = False
    return (np.array_equal(out['P'][s].view(np.uint64)[m], P[s].view(np.uint64)[m]) and np.isfinite(out['P'][s, :n, :n]).all() and
            _bits(out['cam_q'][s, ncam:], cq[s, ncam:]) and _bits(out['cam_p'][s, ncam:], cp[s, ncam:]))


def _got(out, s, c):
    st = out['streams'][s]
    return dict(q=st['q'], p=st['p'], v=st['v'], bg=st['bg'], ba=st['ba'], R_ic=st['R_ic'], t_ci=st['t_ci'],
                cam_q=out['cam_q'][s, :c['ncam']], cam_p=out['cam_p'][s, :c['ncam']], P=out['P'][s, :c['n'], :c['n']])


def _check_applied(out, s, c, cfg, streams, cq, cp, P, where):
    ref, bars = Zc.reference(c), Zc.bars(cfg)
    rec = out['rec'][s]
    assert rec['flags'] == Z.DETECTED | Z.APPLIED and rec['detected_total'] == 3 and rec['applied_total'] == 3, (where, rec)
    assert _frame_intact(out, s, c['n'], c['ncam'], cq, cp, P), where
    Pn = out['P'][s, :c['n'], :c['n']]
    assert np.array_equal(Pn.view(np.uint64), Pn.T.copy().view(np.uint64)), where          # bit-symmetric
    e = Zc.errors(_got(out, s, c), ref)
    worst = max(e[k] / (Zc.FACTOR * bars[k]) for k in e)
    print('ZUPT %s %s worst ratio %.3f' % (where, ' '.join('%s %.1e/%.1e' % (k, e[k], bars[k]) for k in Zc.QUANTITIES), worst))
    assert all(e[k] <= Zc.FACTOR * bars[k] for k in e), (where, e, bars)
    # the record's doubles: |v| before the update, gamma, |delta_x[12:15]|
    dxp = float(Zc.R.norm(ref['dx'][12:15]))
    assert abs(rec['v_norm'] - np.linalg.norm(c['state']['v'])) <= 4 * Zc.EPS * rec['v_norm']
    assert abs(rec['gamma'] - ref['gamma']) <= 1e-9 * ref['gamma'] and abs(rec['dx_pos'] - dxp) <= 1e-9 * dxp, (where, rec)
    # the null states follow the injection as the reference's aliasing makes them (null_aliased = 1): the same increments
    st, back = streams[s], out['streams'][s]
    assert _bits(back['qn'], st['qn'])
    assert np.abs((back['vn'] - st['vn']) - (back['v'] - st['v'])).max() <= 8 * Zc.EPS * np.abs(st['v']).max()
    assert np.abs((back['pn'] - st['pn']) - (back['p'] - st['p'])).max() <= 8 * Zc.EPS * np.abs(st['p']).max()


@pytest.mark.parametrize('n', Zc.DIMS)
def test_one_stream_against_the_50_digit_reference(dev, cfg, n):
    """State dimensions 21, 27, 81, 87 and 165 at ld = 165: no camera state, one, rows on both sides of the wavefront's 64 lanes, a
    full window."""
    c = Zc.case(n)
    out, streams, cq, cp, P = _launch(dev, [c])
    _check_applied(out, 0, c, cfg, streams, cq, cp, P, 'n=%d' % n)


def test_65_streams_with_every_kind_of_bystander(dev, cfg):
    """65 streams, one wavefront each: the five dimensions in rotation, and among them streams that are not detected, inactive, failed,
    gated (gamma = 2 x the gate) and with a bad S (a negative and a NaN velocity variance).  Bystanders come back bit for bit, with
    their flag; every updated stream is bit for bit the same stream alone."""
    kinds = {7: 'undetected', 13: 'inactive', 21: 'failed', 30: 'gated', 44: 'bad_neg', 52: 'bad_nan', 64: 'gated'}
    cases, over, P_over = [], {}, {}
    for s in range(65):
        n = Zc.DIMS[s % 5]
        k = kinds.get(s)
        cases.append(Zc.case(n, gamma=2 * Zc.GATE) if k == 'gated' else Zc.case(n))
        if k == 'undetected':
            over['s%d' % s] = dict(zupt_flags=Z.IMU_OK)
        elif k == 'inactive':
            over['s%d' % s] = dict(active=0)
        elif k == 'failed':
            over['s%d' % s] = dict(failed=DFAIL_STACK)
        elif k == 'bad_neg':
            P_over[s] = lambda blk: blk.__setitem__((7, 7), -1.0)
        elif k == 'bad_nan':
            P_over[s] = lambda blk: blk.__setitem__((6, 6), np.nan)
    out, streams, cq, cp, P = _launch(dev, cases, P_over=P_over, **over)
    want = dict(undetected=Z.IMU_OK, inactive=Z.DETECTED, failed=Z.DETECTED, gated=Z.DETECTED | Z.GATED, bad_neg=Z.DETECTED | Z.BAD, bad_nan=Z.DETECTED | Z.BAD)
    for s, k in kinds.items():
        rec = out['rec'][s]
        assert _untouched(out, s, streams, cq, cp, P), (s, k)
        assert rec['flags'] == want[k] and rec['detected_total'] == 3 and rec['applied_total'] == 2 and rec['dx_pos'] == 0.0, (s, k, rec)
        assert out['streams'][s]['failed'] == (DFAIL_STACK if k == 'failed' else 0), (s, k)       # a bad S does not stop the stream
        if k == 'gated':
            g = Zc.reference(cases[s])['gamma']
            assert abs(g - 2 * Zc.GATE) < 1e-6 and abs(rec['gamma'] - g) <= 1e-9 * g, (s, rec)
    alone = {}
    for s in range(65):
        if s in kinds:
            continue
        n = cases[s]['n']
        if n not in alone:
            alone[n] = _launch(dev, [cases[s]])[0]
            _check_applied(out, s, cases[s], cfg, streams, cq, cp, P, 's%d n=%d' % (s, n))
        a = alone[n]
        assert _bits(out['P'][s], a['P'][0]) and _bits(out['cam_q'][s], a['cam_q'][0]) and _bits(out['cam_p'][s], a['cam_p'][0]), s
        assert all(_bits(out['streams'][s][f], a['streams'][0][f]) for f in ('q', 'p', 'v', 'bg', 'ba', 'R_ic', 't_ci', 'qn', 'pn', 'vn')), s
        assert out['rec'][s].tobytes() == a['rec'][0].tobytes(), s


def test_the_gate_on_both_sides_with_a_margin(dev, cfg):
    """gamma = gate / 2 is applied, gamma = 2 gate is gated, and with gate = 0 the same stream is applied."""
    lo, hi = Zc.case(27), Zc.case(27, gamma=2 * Zc.GATE)
    out, streams, cq, cp, P = _launch(dev, [lo, hi])
    assert out['rec']['flags'].tolist() == [Z.DETECTED | Z.APPLIED, Z.DETECTED | Z.GATED]
    assert _untouched(out, 1, streams, cq, cp, P) and not _untouched(out, 0, streams, cq, cp, P)
    out, streams, cq, cp, P = _launch(dev, [hi], params=dict(Zc.PARAMS, gate=0.0))
    assert out['rec']['flags'].tolist() == [Z.DETECTED | Z.APPLIED]
    _check_applied(out, 0, hi, cfg, streams, cq, cp, P, 'no gate')


def test_without_aliasing_the_null_states_stay(dev, cfg):
    c = Zc.case(27)
    out, streams, cq, cp, P = _launch(dev, [c], s0=dict(null_aliased=0))
    back = out['streams'][0]
    assert out['rec'][0]['flags'] & Z.APPLIED and all(_bits(back[f], streams[0][f]) for f in ('qn', 'pn', 'vn')) and not _bits(back['v'], streams[0]['v'])


def test_arguments_are_checked(dev, cfg):
    from uav_airvision_amd import _native as N
    c = Zc.case(27)
    for bad in (dict(velocity_sigma=0.0), dict(gate=-1.0), dict(still_percent=101), dict(gyro_max=float('nan'))):
        with pytest.raises(N.AirvisionError) as e:
            _launch(dev, [c], params=dict(Zc.PARAMS, **bad))
        assert e.value.code == N.AV_E_INVALID
    with pytest.raises(N.AirvisionError) as e:                   # n does not match the camera count
        _launch(dev, [c], s0=dict(ncam=2))
    assert e.value.code == N.AV_E_INVALID
