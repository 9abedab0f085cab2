"""The batched measurement update's back end -- upd_stack_kernel (the stacking decisions), the direct pipeline on the fp64 matrix
instruction (upd_gather, upd_tt / upd_s / upd_chol / upd_fsolve / upd_p _mfma_kernel), the row compression through the bordered Gram
matrix (upd_rowmap, upd_gram_mfma, upd_gram_chol_mfma) and the information form (upd_info_kernel) -- against a 50-digit reference of
measurement_update (tests/msckf_mp_ref.py), through av_msckf_update_ops_dev: a tests-only entry that runs dev_launch_update, the helper
a phase of a filter step launches its update with, on the caller's candidates, block buffers and covariances.

Inputs, reference values and bars: tests/msckf_update_cases.py.  With e_fam the larger of what the fp64 oracle and the fp64 statement of
the path's method (tests/msckf_update_methods.py) achieve against the reference on the family, floored at 4 ulp, a kernel may be
16 e_fam off: P+ entry by entry relative to sqrt(P+_ii P+_jj), delta_x relative to sqrt(P_ii) of the prior.  Before any number is looked
at every test asserts WHICH PATH RAN, from the record the stacking kernel wrote, and that `stacked` and the touched columns are the
NumPy rule's.  Exact, bit for bit: P+ is symmetric; everything outside a stream's n x n square, every other stream's region and
delta_x beyond n keep their NaN pre-fill.  Every test prints its figures (UPDATE lines; profiles/update_parity/README.md has the table).
"""
import numpy as np
import pytest

import msckf_update_cases as Uc
import msckf_update_methods as Um

pytestmark = pytest.mark.gpu

LD, CS = Uc.LD, Uc.CAM_STRIDE
NAN_BITS = np.array([np.nan]).view(np.uint64)[0]


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


def _prefill(a):
    return bool((np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64) == NAN_BITS).all())


def _launch(dev, cases, phase, kch=0, modes=None, obs_noise=None, ld=LD, cam_stride=CS):
    """All `cases` (one hld) as the streams of one launch; everything around a stream's own data is NaN.  -> (P in, out)."""
    S, hld = len(cases), cases[0]['hld']
    assert all(c['hld'] == hld for c in cases)
    rows_cap = max(c['rows_cap'] for c in cases)
    H = np.full((S, rows_cap, hld if hld > 0 else ld), np.nan)
    r = np.full((S, rows_cap), np.nan)
    P = np.full((S, ld, ld), np.nan)
    streams = []
    for s, c in enumerate(cases):
        H[s, :c['rows_cap']], r[s, :c['rows_cap']] = c['H'][:, :H.shape[2]], c['r']
        k = min(len(c['P']), ld)
        P[s, :k, :k] = c['P'][:k, :k]
        streams.append(dict(n=c['n'], mode=1 if modes is None else modes[s], feats=c['feats']))
    out = dev.update_ops_dev(streams, H, r, P, cases[0]['obs_noise'] if obs_noise is None else obs_noise, phase, kch=kch, hld=hld, cam_stride=cam_stride)
    return P, out


def _check_path(out, s, case, phase, path, kch=Um.KCH, mode=1):
    """Which path ran, from the stacking kernel's record; `stacked` and the touched columns are the NumPy rule's."""
    rule, rec = Um.stack_rule(case['feats'], phase, mode=mode, kch=kch), out['rec'][s]
    label = (case['name'], rec, int(out['stacked'][s]))
    assert rule['path'] == path, (label, rule['path'])
    assert int(out['stacked'][s]) == rule['stacked'], label
    assert np.array_equal(out['cols'][s], rule['cols']), label
    assert (rec['m'], rec['nc'], rec['n_blk']) == (rule['m'], rule['nc'], len(rule['taken'])), label
    if path is not None:
        assert (rec['mode'], rec['kdir']) == (rule['mode'], rule['kdir']), label
        assert {'info': rec['mode'] == 1, 'direct': rec['mode'] == 0 and rec['kdir'] == rec['m'] <= kch,
                'compress': rec['mode'] == 0 and rec['kdir'] == 0 and rec['m'] > kch}[path], label
    return rule


def _check_exact(Pin, out, s, n, updated):
    """What must hold bit for bit about stream s of a launch."""
    P, dx = out['P'][s], out['dx'][s]
    assert _prefill(P[n:, :]) and _prefill(P[:, n:]) and _prefill(dx[n:]), s
    if updated:
        assert np.isfinite(P[:n, :n]).all() and np.isfinite(dx[:n]).all(), s
        assert _bits(P[:n, :n], P[:n, :n].T), s
    else:
        assert _bits(P, Pin[s]) and _prefill(dx), s


def _judge(name, path, errs, bars, left=0):
    bad = []
    for k, worst in sorted(errs.items()):
        print('UPDATE %s %s %s e_fam %.2e kernel worst %.2e ratio %.3f left_out %d' % (name, path, k, bars[k], worst, worst / (Uc.FACTOR * bars[k]), left))
        assert Uc.FACTOR * bars[k] <= Uc.OLD_BAR, (name, path, k, bars[k])      # a looser bar than the suite already enforces is not asserted: the inputs would be outside the method
        if not worst <= Uc.FACTOR * bars[k]:
            bad.append((name, path, k, worst, bars[k]))
    assert left == 0
    return bad


@pytest.mark.parametrize('name', sorted(Uc.FAMILIES))
def test_update_family(dev, cfg, name):
    """One family through its path, all its cases as the streams of one launch (one launch per row layout)."""
    fam = Uc.FAMILIES[name]
    phase, path = fam['phase'], fam['path']
    cases, ferr, bars = Uc.family(name, cfg), Uc.family_errors(name, cfg), Uc.bars(name, cfg)
    worst = {}
    for hld in sorted({c['hld'] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c['hld'] == hld]
        Pin, out = _launch(dev, [cases[i] for i in idx], phase)
        for s, i in enumerate(idx):
            case, ref = cases[i], ferr[i]['ref']
            _check_path(out, s, case, phase, path)
            _check_exact(Pin, out, s, case['n'], True)
            e = Uc.errors(out['dx'][s], out['P'][s], ref, case['P'])
            print('UPDATE %s %s n %d nc %d m %d %s ref %s: oracle P %.2e dx %.2e | method P %.2e dx %.2e | kernel P %.2e dx %.2e' % (
                name, case['name'], case['n'], out['rec'][s]['nc'], out['rec'][s]['m'], case['kind'], ref['form'], ferr[i]['oracle']['P'], ferr[i]['oracle']['dx'],
                ferr[i]['method']['P'], ferr[i]['method']['dx'], e['P'], e['dx']))
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert not _judge(name, path, worst, bars, sum(f['left_out'] for f in ferr))


def test_three_ways(dev, cfg):
    """One problem (n = 45, nc = 12, m = 40, geometric blocks) through the direct pipeline, the compression (kch = 12) and the
    information form, each within its own bar of the ONE 50-digit answer; the differences between the paths are reported."""
    case = Uc.family('three_ways', cfg)[0]
    got, bad = {}, []
    for path, phase, kch in (('direct', 0, 0), ('compress', 0, 12), ('info', 1, 0)):
        Pin, out = _launch(dev, [case], phase, kch=kch)
        _check_path(out, 0, case, phase, path, kch=kch if kch else Um.KCH)
        _check_exact(Pin, out, 0, case['n'], True)
        ferr = Uc.family_errors('three_ways', cfg, path, phase)[0]
        e = Uc.errors(out['dx'][0], out['P'][0], ferr['ref'], case['P'])
        print('UPDATE three_ways %s: oracle P %.2e dx %.2e | method P %.2e dx %.2e' % (path, ferr['oracle']['P'], ferr['oracle']['dx'], ferr['method']['P'], ferr['method']['dx']))
        bad += _judge('three_ways', path, e, Uc.bars('three_ways', cfg, path, phase))
        got[path] = out
    n = case['n']
    sd = np.sqrt(np.diag(case['P']))
    for a, b in (('direct', 'compress'), ('direct', 'info'), ('compress', 'info')):
        dP = np.abs(got[a]['P'][0, :n, :n] - got[b]['P'][0, :n, :n]) / np.sqrt(np.outer(np.diag(got[a]['P'][0, :n, :n]), np.diag(got[a]['P'][0, :n, :n])))
        print('UPDATE three_ways %s against %s: P %.2e dx %.2e (reported, not asserted)' % (a, b, dP.max(), (np.abs(got[a]['dx'][0, :n] - got[b]['dx'][0, :n]) / sd).max()))
    assert not bad


# ---- launch shapes ----------------------------------------------------------------------------------------------------------
def _shape_streams(cfg):
    """17 streams of one phase-1 launch with full-width rows: all three paths, different n, nc and m, a stream with no passing feature,
    a stopped one (mode 2), one with more than STACK_LDS_BLOCKS passing one-row blocks.  -> [(case, mode, path)]."""
    d, c, i = ({x['name']: x for x in Uc.family(f, cfg)} for f in ('direct', 'compress', 'info'))
    none = dict(d['m17'], name='no_pass', feats=[dict(f, ok=0) for f in d['m17']['feats']])
    none2 = dict(d['m33'], name='no_pass2', feats=[dict(f, ok=0) for f in d['m33']['feats']])
    over = dict(d['k1'], name='over_blocks', feats=[dict(d['k1']['feats'][0], ok=1) for _ in range(Um.STACK_BLOCKS + 1)])
    three = Uc.family('three_ways', cfg)[0]
    return [(i['w_nc24'], 1, 'info'), (d['n69_m65'], 1, 'direct'), (c['m137'], 1, 'compress'), (none, 1, None), (i['w_nc6'], 2, None), (over, 1, None),
            (i['w_nc6'], 1, 'info'), (d['m5'], 1, 'info'), (three, 1, 'info'), (c['m300'], 1, 'compress'), (d['full_window'], 1, 'info'), (d['m33'], 1, 'info'),
            (none2, 1, None), (d['n69_m65'], 1, 'direct'), (c['m137'], 1, 'compress'), (c['m513'], 1, 'info'), (d['m136'], 1, 'info')]


_alone = {}


@pytest.mark.parametrize('S', [1, 8, 9, 17])
def test_launch_shapes(dev, cfg, S):
    """1, 8, 9 and 17 streams (the task map puts stream (t / parts) * 8 + (id & 7) on workgroup id): the streams that must not be
    updated are untouched, every stream that updates has the bits it has in a launch of its own."""
    streams = _shape_streams(cfg)[:S]
    cases, modes = [c for c, _, _ in streams], [m for _, m, _ in streams]
    Pin, out = _launch(dev, cases, 1, modes=modes)
    differ = []
    for s, (case, mode, path) in enumerate(streams):
        rule = _check_path(out, s, case, 1, path, mode=mode)
        _check_exact(Pin, out, s, case['n'], path is not None)
        if path is None:
            want = -1 if (mode == 2 or case['name'] == 'over_blocks') else 0
            assert int(out['stacked'][s]) == want == rule['stacked'], (case['name'], out['stacked'][s])
            continue
        if case['name'] not in _alone:
            _, o1 = _launch(dev, [case], 1)
            _check_path(o1, 0, case, 1, path)
            _alone[case['name']] = (o1['P'][0].copy(), o1['dx'][0].copy())
        P1, dx1 = _alone[case['name']]
        if not (_bits(out['P'][s], P1) and _bits(out['dx'][s], dx1)):
            differ.append((s, case['name'], path))
    print('UPDATE launch_shapes S = %d: %d updating streams, %d differ from a launch of their own %s' % (S, sum(p is not None for _, _, p in streams), len(differ), differ))
    assert not differ


# ---- the documented pivot rule ------------------------------------------------------------------------------------------------
def test_indefinite_s_is_flagged_and_the_update_is_a_no_op(dev, cfg):
    """A symmetric P with one negative eigenvalue in the touched block, large enough that S = H P H^T + s^2 I is indefinite: the factor
    kernel writes UPD_BAD_PIVOT, delta_x is zero and P keeps its bits.  No NaN or Inf is fed: the comment promises no no-op for them.
    The compression's factor cannot be brought to a bad pivot with finite values -- A + E is a Gram matrix plus a positive diagonal and
    the border pivot is at least rho + 1 -- short of sums that overflow, so it has no such test."""
    case = dict(Uc.make_case(Uc.C('pivot', 45, [0, 1, 2, 3], 20, 'dense'), Uc.SEEDS['pivot'], cfg.observation_noise, cfg))
    rule, Hc, r = Uc.stacked_problem(case, 0)
    cols, P = rule['cols'], case['P'].copy()
    w, V = np.linalg.eigh(P[np.ix_(cols, cols)])
    u = np.zeros(case['n'])
    u[cols] = V[:, -1]
    P -= 10 * w[-1] * np.outer(u, u)
    P = (P + P.T) / 2
    S = Hc @ P[np.ix_(cols, cols)] @ Hc.T + case['obs_noise'] * np.eye(len(Hc))
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(S).min() < -1e-3 and np.isfinite(P).all()
    case['P'] = P
    Pin, out = _launch(dev, [case], 0)
    n = case['n']
    print('UPDATE pivot: stacked %d, largest |dx| %.3e' % (out['stacked'][0], np.abs(out['dx'][0, :n]).max()))
    assert int(out['stacked'][0]) == Um.BAD_PIVOT and out['rec'][0]['kdir'] == 20 and out['rec'][0]['mode'] == 0
    assert _bits(out['P'][0], Pin[0])
    assert (out['dx'][0, :n] == 0.0).all() and _prefill(out['dx'][0, n:])


# ---- refused arguments --------------------------------------------------------------------------------------------------------
def test_arguments_that_would_leave_a_buffer_are_refused(dev, cfg):
    from uav_airvision_amd import _native as N
    base = Uc.family('direct', cfg)[1]                       # n = 33, two cameras, one passing block of 5 rows
    INV, CAP = N.AV_E_INVALID, N.AV_E_CAPACITY

    def run(case=base, phase=0, want=None, label='', **kw):
        with pytest.raises(N.AirvisionError) as e:
            _launch(dev, [case], phase, **kw)
        assert e.value.code == want, (label, e.value.code, str(e.value))

    feats = base['feats']
    first = next(k for k, f in enumerate(feats) if f['ok'])

    def with_feat(**ch):
        return dict(base, feats=[dict(f, **ch) if k == first else f for k, f in enumerate(feats)])

    run(dict(base, n=LD + 6), want=CAP, label='n > ld')
    run(dict(base, n=34), want=INV, label='n != 21 + 6 ncam')
    run(base, cam_stride=65, want=INV, label='cam_stride > 64')
    run(base, cam_stride=1, want=CAP, label='more camera states than cam_stride')
    run(with_feat(cams=[0, CS]), want=INV, label='camera slot = cam_stride')
    run(with_feat(cams=[0, 2]), want=INV, label='camera slot outside the window of two')
    run(with_feat(cams=[]), want=INV, label='a passing feature without an observation')
    run(with_feat(row=base['rows_cap'] - 2), want=CAP, label='rows outside the block buffer')
    run(dict(base, feats=feats + [dict(feats[first])] * (base['rows_cap'] // 5 + 1)), want=CAP, label='m > ldt (blocks that share rows)')
    run(base, phase=2, want=INV, label='phase')
    run(base, kch=137, want=INV, label='kch beyond one pass')
    run(base, modes=[3], want=INV, label='mode')
    run(base, obs_noise=0.0, want=INV, label='observation noise')
    run(dict(base, hld=12, H=base['H'][:, :12].copy()), phase=0, want=INV, label='compact rows in phase 0')
    run(dict(base, hld=6, H=base['H'][:, :6].copy()), phase=1, want=INV, label='hld < nc')
    with pytest.raises(N.AirvisionError) as e:              # more candidates than fs_stride
        dev.update_ops_dev([dict(n=33, feats=feats)], np.zeros((1, base['rows_cap'], LD)), np.zeros((1, base['rows_cap'])), np.zeros((1, LD, LD)),
                           base['obs_noise'], 0, fs_stride=len(feats) - 1)
    assert e.value.code == CAP
    # rows kept by one pass beyond ld: 33 stacked rows, a covariance of 27
    small = dict(Uc.family('direct', cfg)[0])
    small.update(feats=[dict(cams=[0], ok=1, row=1)] * 33, H=np.zeros((40, 27)), r=np.zeros(40), rows_cap=40)
    run(small, ld=27, cam_stride=1, kch=Um.KCH, want=CAP, label='k > ld')
    # ... and with kch = 0 the entry takes the step's own min(136, ld): the same stream is compressed to its six columns' worth and runs
    Pin, out = _launch(dev, [small], 0, ld=27, cam_stride=1)
    assert int(out['stacked'][0]) == 33 and out['rec'][0]['kdir'] == 0 and out['rec'][0]['mode'] == 0 and np.isfinite(out['P'][0]).all()
    # more than MFMA_MAXCOLS touched columns: 43 cameras
    ncam = 43
    n = 21 + 6 * ncam
    wide = dict(base, n=n, P=np.eye(n), feats=[dict(cams=list(range(ncam)), ok=1, row=0)], H=np.zeros((4 * ncam, n)), r=np.zeros(4 * ncam), rows_cap=4 * ncam)
    run(wide, ld=n, cam_stride=ncam, want=CAP, label='nc > 256')
    # the information form's LDS: 24 columns of a state of 405
    n = 21 + 6 * 64
    big = dict(base, n=n, P=np.eye(n), feats=[dict(cams=[0, 1, 2, 3], ok=1, row=0)], H=np.zeros((16, n)), r=np.zeros(16), rows_cap=16)
    run(big, phase=1, ld=n, cam_stride=64, want=CAP, label='information-form LDS')
