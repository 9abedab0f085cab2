"""The part of a filter step that runs before any feature is looked at -- dev_predict_new_state (RK4), propagate_body (F, G, Phi to third
order, the observability patches, Q, P11), the cross block with the frame's accumulated transition (dk_cov<64> / <256>), augment_body,
remove_cam_body / remove_two_cams_body, dev_find_redundant -- against a 50-digit reference (tests/msckf_mp_ref.py), through both launchers:

 * the operator entries av_msckf_propagate / _augment / _remove_cam: sample by sample, the per-sample cross block in chunks of 21
   columns, covariance only (the state they are given is the oracle's);
 * av_msckf_predict_ops_dev (a tests-only entry), which launches what a step of the device-resident filter launches -- dk_state, then
   dk_cov<wg> through the step's own helper -- at wg = 64 and 256, many streams per launch.

Inputs, reference values and bars: tests/msckf_predict_cases.py.  With e_fam what the fp64 oracle achieves against the reference on the
same family (floored at 4 ulp) a kernel may be 16 e_fam off, in q, p, v, the new camera state and every entry of the covariance
(relative to sqrt(P_ii P_jj)).  Exact: the fields the prediction must not touch, the null states handed over, symmetry, the
camera-camera block, the NaN pre-fill around every stream's matrix and camera window, removal (numpy.delete, in place), the
redundancy rule (the 50-digit decision).  Every test prints its figures (PARITY lines; profiles/predict_parity/README.md has the table).
"""
import numpy as np
import pytest

import msckf_predict_cases as Pc

pytestmark = pytest.mark.gpu

CS, LD = Pc.CAM_STRIDE, Pc.LD
WGS = (64, 256)
UNTOUCHED = ('bg', 'ba', 'R_ic', 't_ci', 'gravity', 'tracking_rate')
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


# ---- the device-resident launcher -----------------------------------------------------------------------
def _stream(case, **kw):
    st = dict(case['state'], n=case['n'], ncam=case['ncam'], t_frame=case['t_frame'], imu_cnt=len(case['imu']))
    st.update(kw)
    return st


def _launch(dev, cases, wg, streams=None):
    """All `cases` as the streams of one launch; everything around a stream's own data is NaN.  -> (inputs, outputs)."""
    S = len(cases)
    streams = [_stream(c) for c in cases] if streams is None else streams
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
    imu = np.concatenate(imu) if imu else np.zeros((0, 7))
    out = dev.predict_ops_dev(streams, imu, cq, cp, cqn, P, cases[0]['noise'], wg)
    return dict(P=P, cam_q=cq, cam_p=cp, cam_qn=cqn, streams=streams), out


def _result(out, s, case):
    """Stream s of a launch as the dict msckf_predict_cases.errors reads."""
    st, n, k = out['streams'][s], case['n'], case['ncam']
    return dict(q=st['q'], p=st['p'], v=st['v'], cam_q=out['cam_q'][s, k], cam_p=out['cam_p'][s, k], P=out['P'][s, :n + 6, :n + 6])


def _check_exact(inp, out, s, case, label):
    """Everything about stream s of a launch that must hold bit for bit."""
    st, st0, n, k, ni = out['streams'][s], inp['streams'][s], case['n'], case['ncam'], len(case['imu'])
    assert (st['n'], st['ncam'], st['failed'], st['active'], st['first_img']) == (n + 6, k + 1, 0, 1, 0), label
    for f in UNTOUCHED:
        assert _bits(st[f], st0[f]), (label, f)
    if ni:                                               # the null states are handed over after every sample
        assert st['ts'] == case['imu'][-1, 0] and st['null_aliased'] == 1, label
        assert _bits(st['qn'], st['q']) and _bits(st['pn'], st['p']) and _bits(st['vn'], st['v']), label
    else:
        assert st['ts'] == st0['ts'] and st['null_aliased'] == 0, label
        for f in ('q', 'p', 'v', 'qn', 'pn', 'vn'):
            assert _bits(st[f], st0[f]), (label, f)
    # camera window: the old states keep their bits, the new one's null orientation is its orientation, the rest keeps the pre-fill
    assert _bits(out['cam_q'][s, :k], inp['cam_q'][s, :k]) and _bits(out['cam_p'][s, :k], inp['cam_p'][s, :k]) and _bits(out['cam_qn'][s, :k], inp['cam_qn'][s, :k]), label
    assert _bits(out['cam_qn'][s, k], out['cam_q'][s, k]) and np.isfinite(out['cam_q'][s, k]).all() and np.isfinite(out['cam_p'][s, k]).all(), label
    assert np.isnan(out['cam_q'][s, k + 1:]).all() and np.isnan(out['cam_p'][s, k + 1:]).all() and np.isnan(out['cam_qn'][s, k + 1:]).all(), label
    # covariance: exactly symmetric, the camera-camera block keeps the input's bits, nothing outside the n + 6 square is written
    P = out['P'][s]
    m = n + 6
    assert np.isfinite(P[:m, :m]).all() and _bits(P[:m, :m], P[:m, :m].T), label
    assert _bits(P[21:n, 21:n], inp['P'][s, 21:n, 21:n]), label
    assert np.isnan(P[m:, :]).all() and np.isnan(P[:, m:]).all(), label


def _judge(name, launcher, errs, bars, refs):
    """Prints the launcher's figures; -> the quantities beyond 16 e_fam (the caller asserts once every launcher has been through)."""
    left = sum(r['left_out'] for r in refs)
    for k, worst in sorted(errs.items()):
        print('PARITY %s %s %s e_fam %.2e worst %.2e ratio %.3f left_out %d' % (name, launcher, k, bars[k], worst, worst / (Pc.FACTOR * bars[k]), left))
    assert left == 0
    return [(name, launcher, k, worst, bars[k]) for k, worst in errs.items() if not worst <= Pc.FACTOR * bars[k]]


def _worst(acc, e):
    for k, v in e.items():
        acc[k] = max(acc.get(k, 0.0), v)


# ---- the operator launcher ------------------------------------------------------------------------------
def _operator(dev, case, ora):
    """The covariance of a case through av_msckf_propagate per sample and av_msckf_augment, given the oracle's state per sample."""
    g = case['state']['gravity']
    dev.set_cov(case['P'])
    for a in ora['samples']:
        dev.propagate(a['dt'], a['gyro'], a['acc'], a['q_old'], a['q_new'], a['q_null'], a['v_null'], a['p_null'], a['v_new'], a['p_new'], g, case['noise'])
    before = dev.get_cov()
    dev.augment(ora['aug']['R_ic'], ora['aug']['sk'])
    return before, dev.get_cov()


@pytest.mark.parametrize('name', list(Pc.FAMILIES))
def test_prediction_family(dev, cfg, name):
    """The family's cases through the operator entries and as the streams of one launch of the device-resident shapes at both
    workgroup sizes."""
    cases, refs, bars = Pc.family(name, cfg), Pc.reference(name, cfg), Pc.bars(name, cfg)
    # operator entries: covariance only
    worst = {}
    for case, r in zip(cases, refs):
        n = case['n']
        before, after = _operator(dev, case, r['oracle'])
        assert _bits(after, after.T) and _bits(before, before.T), case['name']
        assert _bits(before[21:, 21:], case['P'][21:, 21:]) and _bits(after[:n, :n], before), case['name']
        _worst(worst, dict(P=Pc.cov_err(after, r['ref']['P']), P_prop=Pc.cov_err(before, r['ref']['P_prop'])))
    beyond = _judge(name, 'operator', worst, dict(bars, P_prop=bars['P']), refs)
    # device-resident shapes
    for wg in WGS:
        inp, out = _launch(dev, cases, wg)
        worst = {}
        for s, (case, r) in enumerate(zip(cases, refs)):
            _check_exact(inp, out, s, case, (case['name'], wg))
            _worst(worst, Pc.errors(_result(out, s, case), r['ref']))
        beyond += _judge(name, 'dev wg=%d' % wg, worst, bars, refs)
    assert not beyond, beyond


def test_rate_branch_margins(cfg):
    """The `> 1e-5` decision of every sample of every case, in 50 digits: none within 1e-9 relative of the threshold, both sides taken."""
    margins = [float(r['ref']['rate_margin']) for name in Pc.FAMILIES for r in Pc.reference(name, cfg)]
    print('PARITY rate branch: smallest margin %.3g' % min(margins))
    assert min(margins) >= Pc.MARGIN_MIN


# ---- removal ----------------------------------------------------------------------------------------------
def _removal_streams(pairs):
    """Inactive streams (the prediction leaves them alone) that only ask for the removal of a pair of camera states."""
    base = Pc.make_state(np.random.default_rng(1))
    return [dict(base, n=21 + 6 * K, ncam=K, active=0, remove=pr) for K, pr in pairs]


@pytest.mark.parametrize('K', [2, 11, 24])
def test_removal_is_numpy_delete_in_place(dev, K):
    """Both launchers on every pair of positions of the window: the matrix equals numpy.delete of the input bit for bit, in place, the
    untouched top-left block left untouched, everything else as it was (the NaN pre-fill included)."""
    pairs = [(k, pr) for k, pr in Pc.REMOVALS if k == K]
    P0 = Pc.removal_case(K)
    n, m = 21 + 6 * K, 21 + 6 * K - 12
    want = []
    for _, (i0, i1) in pairs:
        rows = np.r_[21 + 6 * i0:27 + 6 * i0, 21 + 6 * i1:27 + 6 * i1]
        want.append(np.delete(np.delete(P0, rows, axis=0), rows, axis=1))
        assert _bits(want[-1], Pc.R.remove_cam_states(P0, (i0, i1)))          # (the reference's one-after-the-other loop is the same selection)
    for w, (_, (i0, i1)) in zip(want, pairs):                                    # operator entry: one camera state per call
        dev.set_cov(P0)
        dev.remove_cam(i0)
        dev.remove_cam(i1 - 1)
        assert _bits(dev.get_cov(), w), (K, i0, i1)
    streams = _removal_streams(pairs)
    S = len(pairs)
    for wg in WGS:
        P = np.full((S, LD, LD), np.nan)
        P[:, :n, :n] = P0
        cams = np.full((S, CS, 4), np.nan)
        out = dev.predict_ops_dev([dict(s) for s in streams], np.zeros((0, 7)), cams, cams[:, :, :3], cams, P, np.zeros(4), wg)
        for s, (w, (_, (i0, i1))) in enumerate(zip(want, pairs)):
            got = out['P'][s]
            assert _bits(got[:m, :m], w), (K, wg, i0, i1)
            rest = np.ones((LD, LD), bool)
            rest[:m, :m] = False
            assert _bits(got[rest], P[s][rest]), (K, wg, i0, i1)
            assert out['streams'][s]['n'] == n and out['streams'][s]['active'] == 0
    print('PARITY removal K=%d: %d position pairs, operator and wg=64/256, bit for bit' % (K, len(pairs)))


def test_removal_and_redundancy_arguments_are_checked(dev):
    """Positions outside the window, not ascending, a window too small for the rule, samples outside their array, a bad workgroup size,
    a window beyond the stride: refused on the host before any launch."""
    from uav_airvision_amd import _native as N
    base = _removal_streams([(6, (0, 1))])[0]
    P, cams = np.full((1, LD, LD), np.nan), np.full((1, CS, 4), np.nan)

    def run(st, wg=64):
        return dev.predict_ops_dev([st], np.zeros((0, 7)), cams, cams[:, :, :3], cams, P, np.zeros(4), wg)
    for bad in (dict(remove=(1, 1)), dict(remove=(3, 2)), dict(remove=(0, 6)), dict(remove=(-1, 2)), dict(ncam=3, n=39, find_redundant=True, remove=None),
                dict(imu_cnt=1), dict(n=28)):
        with pytest.raises(N.AirvisionError) as e:
            run(dict(base, **bad))
        assert e.value.code == N.AV_E_INVALID, bad
    with pytest.raises(N.AirvisionError) as e:
        run(base, wg=128)
    assert e.value.code == N.AV_E_INVALID
    with pytest.raises(N.AirvisionError) as e:
        run(dict(base, ncam=25, n=171, remove=None))
    assert e.value.code == N.AV_E_CAPACITY


# ---- the redundancy rule ----------------------------------------------------------------------------------
def test_redundancy_rule_takes_the_reference_decision(dev, cfg):
    refs = [Pc.redundant_reference(spec) for spec in Pc.REDUNDANT]
    print('PARITY redundancy rule: smallest decision margin %.3g, left out %d' % (min(float(r['margin']) for r in refs), sum(r['left_out'] for r in refs)))
    assert not any(r['left_out'] for r in refs)
    assert [r['pos'] for r in refs] == [spec['want'] for spec in Pc.REDUNDANT]
    base = _removal_streams([(6, (0, 1))])[0]
    streams, S = [], len(Pc.REDUNDANT)
    cq, cp = np.full((S, CS, 4), np.nan), np.full((S, CS, 3), np.nan)
    for s, spec in enumerate(Pc.REDUNDANT):
        q, p, rate = Pc.redundant_case(spec)
        cq[s, :len(q)], cp[s, :len(q)] = q, p
        streams.append(dict(base, n=21 + 6 * len(q), ncam=len(q), active=0, remove=None, find_redundant=True, tracking_rate=rate))
    P = np.full((S, LD, LD), np.nan)
    for wg in WGS:
        out = dev.predict_ops_dev([dict(s) for s in streams], np.zeros((0, 7)), cq, cp, cq, P, np.zeros(4), wg)
        assert [st['redundant'] for st in out['streams']] == [r['pos'] for r in refs], wg
        assert _bits(out['cam_q'], cq) and _bits(out['cam_p'], cp) and np.isnan(out['P']).all()


# ---- launch shapes ----------------------------------------------------------------------------------------
def _same_stream(out_a, a, out_b, b):
    from uav_airvision_amd.msckf_ops import MsckfDevice
    sa, sb = out_a['streams'][a], out_b['streams'][b]
    return (all(_bits(sa[f], sb[f]) for f, _ in MsckfDevice.STATE_FIELDS) and all(sa[f] == sb[f] for f in MsckfDevice.STATE_INTS)
            and all(_bits(out_a[k][a], out_b[k][b]) for k in ('P', 'cam_q', 'cam_p', 'cam_qn')))


@pytest.mark.parametrize('wg', WGS)
def test_65_streams_cross_the_state_kernels_workgroup(dev, cfg, wg):
    """Five distinct cases replicated to 65 streams: dk_state runs 64 lanes per workgroup, stream 64 is the second workgroup's only lane.
    Every replica is bit for bit its original, and the originals meet the reference."""
    five = Pc.family('rate', cfg) + [Pc.family('sparsity', cfg)[2]]
    refs = Pc.reference('rate', cfg) + [Pc.reference('sparsity', cfg)[2]]
    cases = [five[s % 5] for s in range(65)]
    inp, out = _launch(dev, cases, wg)
    for s in range(65):
        _check_exact(inp, out, s, cases[s], (s, wg))
        assert _same_stream(out, s, out, s % 5), (s, wg)
    for s in range(5):
        name = 'rate' if s < 4 else 'sparsity'
        e, bars = Pc.errors(_result(out, s, cases[s]), refs[s]['ref']), Pc.bars(name, cfg)
        for k, v in e.items():
            assert v <= Pc.FACTOR * bars[k], (s, k, v)


@pytest.mark.parametrize('wg', WGS)
def test_mixed_batch_streams_do_not_see_their_neighbours(dev, cfg, wg):
    """Streams of different n and sample counts in one launch, among them an inactive stream, a stream that has already failed and one
    whose window is full: the full window gives DFAIL_CAMS, those three keep every bit, and every other stream has the bits it has alone."""
    small, large = Pc.family('samples', cfg), Pc.family('large', cfg)
    full = Pc.make_case(991, cfg, ncam=CS, n_imu=2)
    cases = [large[0], Pc.family('rate', cfg)[3], small[3], Pc.family('sparsity', cfg)[1], full, small[2], large[2]]
    streams = [_stream(c) for c in cases]
    streams[1]['active'] = 0
    streams[3]['failed'] = DFAIL_STACK
    inp, out = _launch(dev, cases, wg, streams)
    for s, code in ((1, 0), (3, DFAIL_STACK), (4, DFAIL_CAMS)):
        st, st0 = out['streams'][s], inp['streams'][s]
        assert (st['failed'], st['active'], st['n'], st['ncam'], st['null_aliased']) == (code, 0, cases[s]['n'], cases[s]['ncam'], 0), s
        for f, _ in dev.STATE_FIELDS:
            assert _bits(st[f], st0[f]), (s, f)
        for k in ('P', 'cam_q', 'cam_p', 'cam_qn'):
            assert _bits(out[k][s], inp[k][s]), (s, k)
    for s in (0, 2, 5, 6):
        _check_exact(inp, out, s, cases[s], (s, wg))
        _, alone = _launch(dev, [cases[s]], wg)
        assert _same_stream(out, s, alone, 0), (s, wg)


def test_workgroup_sizes_64_and_256_against_each_other(dev, cfg):
    """dk_state is one kernel whatever wg is: the state and the new camera state have the same bits.  The covariance comes from two
    instantiations of dk_cov: propagate_body's sums run over the same masks in the same order, the cross block sums the same 21 terms
    in the same order, the augmentation is a sum per entry -- the bits were measured equal for every entry of every family (unlike the
    8-lane / 16-lane gate kernels, no contraction difference between the two), so they are held equal; each shape is held to the
    reference on its own in test_prediction_family.  The operator entries against them, where the comparison is clean (one IMU sample:
    the accumulated transition is that sample's, and the operator is given the state dk_state computed), is reported, not asserted:
    measured, the propagated matrix has the same bits (propagate_kernel sums the cross block over the non-zeros of Phi, dk_cov over all
    21 terms: the skipped terms are exact zeros), and at n = 87 six entries of the new camera state's rows differ by one unit in the
    last place -- augment_kernel and the augment_body inlined into dk_cov are contracted into fused multiply-adds differently; built
    with -ffp-contract=off there was no difference (profiles/predict_parity/README.md)."""
    differing, total = 0, 0
    for name in Pc.FAMILIES:
        cases = Pc.family(name, cfg)
        outs = [_launch(dev, cases, wg)[1] for wg in WGS]
        for s, c in enumerate(cases):
            m = c['n'] + 6
            assert _same_stream(outs[0], s, outs[1], s), (name, s)
            a, b = outs[0]['P'][s, :m, :m], outs[1]['P'][s, :m, :m]
            differing += int((a.view(np.uint64) != b.view(np.uint64)).sum())
            total += a.size
            if len(c['imu']) == 1:
                st, st0, g = outs[0]['streams'][s], c['state'], c['imu'][0]
                dev.set_cov(c['P'])
                dev.propagate(g[0] - st0['ts'], g[1:4] - st0['bg'], g[4:7] - st0['ba'], st0['q'], st['q'], st0['qn'], st0['vn'], st0['pn'], st['v'], st['p'],
                              st0['gravity'], c['noise'])
                Rwi = Pc.O.to_rotation(st['q'])
                dev.augment(st0['R_ic'], Pc.O.skew(Rwi.T @ st0['t_ci']))
                op = dev.get_cov()
                where = np.argwhere(op.view(np.uint64) != a.view(np.uint64))
                print('PARITY operator against dev, %s (one sample, n = %d): %d of %d covariance entries differ in their bits, largest difference %.2e of sqrt(P_ii P_jj)%s'
                      % (c['name'], c['n'], len(where), a.size, (np.abs(op - a) / np.sqrt(np.outer(np.diag(a), np.diag(a)))).max(),
                         ', at ' + ' '.join('(%d,%d)' % (i, j) for i, j in where[:12]) if len(where) else ''))
    print('PARITY wg 64 against 256: %d of %d covariance entries differ in their bits' % (differing, total))
    assert differing == 0
