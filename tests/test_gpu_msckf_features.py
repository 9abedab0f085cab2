"""The filter's per-feature kernels (csrc/msckf.hip: triangulate_kernel / triangulate_one, feature_one: measurement Jacobian with the
observability projection, null-space projection by three Householder reflectors, chi^2 gate) against a 50-digit reference
(tests/msckf_mp_ref.py), in every launch shape the library uses:

 * the operator entries av_msckf_triangulate / av_msckf_feature_blocks: dense grids, four-wavefront workgroups, feature_kernel<16> for
   two-observation features, <64> as four-team workgroups up to 4 observations, <256> beyond;
 * av_msckf_feature_ops_dev, which launches what the device-resident filter's update phases launch: triangulate_kernel in list form with
   one wavefront per workgroup, feature_kernel8 with compact 12-double rows, <64> as single-wavefront workgroups, <256>, lists with a
   device-side count, valid[] flags, grids that stride over their list (with the team_sync between features), two streams (fs_stride).

Inputs, reference values and bars: tests/msckf_feature_cases.py.  In short, with e_fam what the fp64 oracle achieves against the
reference on the same family (floored at 4 ulp): triangulation flags equal, position within 16 e_fam + und * d * max(1, d); the rows
through H_o^T H_o, H_o^T r_o, r_o^T r_o (a null-space basis is not unique) within 16 e_fam each, K = 4M - 3 of them, zero outside the
feature's own camera columns; gamma within 16 e_fam, pass equal, both outcomes in every family.  The two launchers give the same bits.
Every test prints its figures (PARITY lines; profiles/feature_parity/README.md has the table).

A one-observation feature (stereo pair only) is triangulated but has no rows: the filter never gates one, and the two-observation
kernels evaluate two-observation features only.  The 32-observation family (the 64-view limit of a wavefront) is triangulation only:
a filter holds at most 25 camera states.
"""
import numpy as np
import pytest

import msckf_feature_cases as Cs
import msckf_mp_ref as R

pytestmark = pytest.mark.gpu

FS = 40                         # feature slots per stream in the list launches: 2 streams x 40 slots hold a list of 65
LISTS = (1, 7, 65)
GRIDS = (1, 3)                  # workgroups


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    from uav_airvision_amd.msckf_ops import MsckfDevice
    d = MsckfDevice(max_cam_states=24, rows_cap=4096)
    yield d
    d.close()


def _batch(dev, obs):
    from uav_airvision_amd.msckf_ops import FeatureBatch
    return FeatureBatch([[c for c, _ in o] for o in obs], [[z for _, z in o] for o in obs], dev.device)


def _op_triangulate(dev, fam):
    return dev.triangulate(_batch(dev, fam['obs']), fam['cam_q'], fam['cam_p'], fam['T01'], fam['opt'])


def _op_gate(dev, fam, cfg, obs, pos, P):
    """av_msckf_feature_blocks on (obs, pos) with covariance P -> per feature (gamma, pass, rows [K, ld], r [K])."""
    dev.set_cov(P)
    b = _batch(dev, obs)
    dofs = [Cs.dof_of(len(o)) for o in obs]
    row_off, rows, gamma, ok = dev.feature_blocks(b, pos, dofs, fam['cam_q'], fam['cam_p'], fam['cam_qn'], fam['cam_pn'], fam['T01'], Cs.GRAVITY, cfg.observation_noise)
    H, r = dev.read_blocks(0, int(rows.sum()))
    return [(gamma[i], bool(ok[i]), H[row_off[i]:row_off[i] + rows[i]], r[row_off[i]:row_off[i] + rows[i]]) for i in range(len(obs))]


def _teams(M, workgroups):
    return workgroups * (8 if M == 2 else 1)          # teams of 8 lanes (two-observation features) come eight to a workgroup


def _perm(n_slots, seed):
    return np.random.default_rng(seed).permutation(n_slots).astype(np.int32)


def _two_streams(fams, what):
    return np.concatenate([f[what] for f in fams])


def _ops_dev(dev, cfg, fams, slot_obs, P2, max_obs, teams, **kw):
    n = 21 + 6 * len(fams[0]['cam_q'])
    if P2 is None:
        P2 = np.tile(np.eye(n), (2, 1, 1))
    grav = np.array([Cs.GRAVITY, Cs.GRAVITY])
    dofs = [Cs.dof_of(len(o)) if len(o) > 1 else 1 for o in slot_obs]
    return dev.feature_ops_dev([[c for c, _ in o] for o in slot_obs], [[z for _, z in o] for o in slot_obs], FS,
                               _two_streams(fams, 'cam_q'), _two_streams(fams, 'cam_p'), _two_streams(fams, 'cam_qn'), _two_streams(fams, 'cam_pn'),
                               P2, grav, fams[0]['T01'], fams[0]['opt'], cfg.observation_noise, dofs, max_obs, teams, **kw)


def _check_triangulation(fam, ref, pos, valid, label):
    """Flags and positions of one launcher against the reference."""
    e_fam = Cs.tri_bar(fam)
    worst, decided, ratio, left = 0.0, 0.0, 0.0, 0
    for i, t in enumerate(ref):
        if t['left_out']:
            left += 1
            continue
        assert bool(valid[i]) == t['valid'], (label, i)
        if not t['valid']:
            continue                                    # (the position of a feature that failed the depth check is not used by anything)
        e = Cs.pos_err(pos[i], t)
        bar = Cs.FACTOR * e_fam + t['slack']
        worst, ratio = max(worst, e), max(ratio, e / bar)
        if t['und'] == 0:
            decided = max(decided, e)
        assert e <= bar, (label, i, e, bar, e_fam, t['slack'])
    assert left <= 0.02 * len(ref)
    print('PARITY %s %s position e_fam %.2e worst %.2e ratio %.3f left_out %d (decided cases: %d of %d, worst %.2e)'
          % (fam['name'], label, e_fam, worst, ratio, left, sum(t['und'] == 0 for t in ref), len(ref), decided))


def _tri_family(dev, cfg, fam, fam1):
    """Triangulation of a family through both launchers: the operator entry against the reference, the list launches against the
    operator entry bit for bit (both streams), unlisted slots untouched."""
    ref = Cs.tri_reference(fam)
    fams = (fam, fam1)
    op = [_op_triangulate(dev, f) for f in fams]
    _check_triangulation(fam, ref, op[0][0], op[0][1], 'operator')
    n = len(fam['obs'])
    slot_obs = [fams[s]['obs'][(s * FS + k) % n] for s in range(2) for k in range(FS)]
    perm = _perm(2 * FS, fam.get('seed', 1))
    M = fam['M']
    for wg in GRIDS:
        for L in LISTS:
            out = _ops_dev(dev, cfg, fams, slot_obs, None, M, _teams(M, wg), tri_list=perm[:L],
                           positions=np.full((2 * FS, 3), np.nan), valid=np.full(2 * FS, -7))
            listed = set(int(v) for v in perm[:L])
            for f in range(2 * FS):
                s, k = divmod(f, FS)
                if f in listed:
                    assert np.array_equal(out['pos'][f], op[s][0][f % n], equal_nan=True) and bool(out['valid'][f]) == bool(op[s][1][f % n]) and out['valid'][f] in (0, 1), (wg, L, f)
                else:
                    assert np.isnan(out['pos'][f]).all() and out['valid'][f] == -7, (wg, L, f)
    return op


@pytest.mark.parametrize('name', list(Cs.FAMILIES))
def test_triangulation_family(dev, cfg, name):
    fam, fam1 = Cs.make_family(name, cfg), Cs.make_family(name, cfg, variant=1)
    ref = Cs.tri_reference(fam)
    assert sum(t['valid'] for t in ref) >= len(ref) - 2
    _tri_family(dev, cfg, fam, fam1)
    if name == 'm9_huber':                              # the Huber branch is taken and all five outer iterations run
        assert all(t['n_huber'] > 0 and t['outer'] == 5 for t in ref)


def test_triangulation_recorded_cases(dev, cfg):
    """The 60 recorded cases (tracks of 3 .. 24 observations) through both launchers."""
    fam = Cs.make_recorded(cfg)
    fam['seed'] = 60
    op = _tri_family(dev, cfg, fam, fam)
    for i in range(60):                                 # and the reference filter's own results, at the bar they have always had
        assert bool(op[0][1][i]) == bool(fam['ref_ok'][i])
        assert np.allclose(op[0][0][i], fam['ref_pos'][i], rtol=1e-8, atol=1e-9)


def test_invalid_features_stay_invalid_and_are_not_gated(dev, cfg):
    """A feature behind its cameras and one with zero parallax: invalid in the reference, the oracle and both launchers; in the chained
    launch the gate reads the flag the triangulation wrote: gamma = 0, pass = 0, no rows."""
    for fam in Cs.make_special(cfg):
        t = Cs.tri_reference(fam)[0]
        assert not t['valid'] and not t['oracle_valid']
        pos, valid = _op_triangulate(dev, fam)
        assert not valid[0], fam['name']
        slot_obs = [fam['obs'][0] for _ in range(2 * FS)]
        lst = np.array([3, FS + 1], np.int32)
        out = _ops_dev(dev, cfg, (fam, fam), slot_obs, None, 3, 1, tri_list=lst, feat_list=lst, valid=np.full(2 * FS, -7), zero_fill=1)
        for f in lst:
            assert out['valid'][f] == 0 and out['gamma'][f] == 0.0 and out['ok'][f] == 0, (fam['name'], f)
        assert np.isnan(out['H']).all() and np.isnan(out['r']).all()


def test_more_than_32_observations_are_refused(dev, cfg):
    """triangulate_one gives every view a lane of one wavefront: a 33-observation track is refused on the host, before any launch."""
    from uav_airvision_amd import _native as N
    rng = np.random.default_rng(3)
    obs = [[(c, rng.normal(0, 0.1, 4)) for c in range(33)]]
    q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (33, 1))
    p = rng.normal(0, 1, (33, 3))
    with pytest.raises(N.AirvisionError) as e:
        dev.triangulate(_batch(dev, obs), q, p, np.eye(4), cfg.optimization_config)
    assert e.value.code == N.AV_E_CAPACITY
    fam = dict(cam_q=q, cam_p=p, cam_qn=q, cam_pn=p, T01=np.eye(4), opt=cfg.optimization_config)
    slot_obs = [obs[0] for _ in range(2 * FS)]
    with pytest.raises(N.AirvisionError) as e:
        _ops_dev(dev, cfg, (fam, fam), slot_obs, None, 33, 1, tri_list=np.array([0], np.int32))
    assert e.value.code == N.AV_E_CAPACITY


def _own(H_full, obs):
    return H_full[:, R.own_columns(obs)]


def _check_rows_shape(H_full, obs, n_state, label):
    """K = 4M - 3 rows; every IMU column and every column of a camera the feature was not seen from is exactly zero."""
    assert H_full.shape[0] == 4 * len(obs) - 3
    other = np.setdiff1d(np.arange(n_state), R.own_columns(obs))
    assert np.isfinite(H_full[:, :n_state]).all(), label
    assert not H_full[:, other].any(), label


GATED = [n for n, s in Cs.FAMILIES.items() if s['gate']]


def _against_reference(g, bars, gam, ok, Ho_own, r, label, worst=None):
    """gamma, pass and the rows of one feature from one launcher against its reference entry g of gate_reference."""
    e = dict(zip(('HtH', 'Htr', 'rtr'), Cs.rows_errors(Ho_own, r, g['rows'])))
    e['gamma'] = float(abs(R.mpf(float(gam)) - g['gamma']) / abs(g['gamma']))
    for k, v in e.items():
        if worst is not None:
            worst[k] = max(worst[k], v)
        assert v <= Cs.FACTOR * bars[k], (label, k, v, bars[k])
    assert g['left_out'] or bool(ok) == g['ok'], (label, gam, float(g['gamma']))


@pytest.mark.parametrize('name', GATED)
def test_rows_and_gate_family(dev, cfg, name):
    fam, fam1 = Cs.make_family(name, cfg), Cs.make_family(name, cfg, variant=1)
    fams = (fam, fam1)
    M, ng = fam['M'], fam['n_gate']
    n_state = 21 + 6 * len(fam['cam_q'])
    pos0, gobs0, P0 = Cs.gate_inputs(fam, cfg)
    refs, bars = [Cs.gate_reference(fam, cfg)], [Cs.gate_bars(fam, cfg)]
    # Two-observation features: the list launches run the 8-lane kernel, the operator entry the 16-lane one.  They are two instantiations
    # of one template, same arithmetic per element, and the compiler contracts them into fused multiply-adds differently (msckf.hip is
    # built with -ffp-contract=fast): gamma differed by up to 5e-14 relative; built with -ffp-contract=off the two gave the same bits
    # for every feature, list and grid of this test.  So the 8-lane kernel is held to the reference itself, in both streams, and to its
    # own bits across lists and grids.  Longer tracks run one instantiation (<64>, <256>) in both launchers: the same bits.
    exact = M != 2
    if exact:       # the second stream has no reference: the same family from another seed, positions from the GPU triangulation of its own gate measurements
        gobs1 = Cs.gate_obs(fam1)
        pos1 = _op_triangulate(dev, dict(fam1, obs=gobs1))[0]
        P1 = Cs.make_cov(fam1, cfg, pos1[0])
    else:
        pos1, gobs1, P1 = Cs.gate_inputs(fam1, cfg)
        refs.append(Cs.gate_reference(fam1, cfg))
        bars.append(Cs.gate_bars(fam1, cfg))
    gobs, pos, P = (gobs0, gobs1), (pos0, pos1), (P0, P1)

    # ---- the operator entry against the reference
    op = [_op_gate(dev, fams[s], cfg, gobs[s], pos[s], P[s]) for s in range(2)]
    worst = dict(HtH=0.0, Htr=0.0, rtr=0.0, gamma=0.0)
    for s in range(len(refs)):
        for i, g in enumerate(refs[s]):
            gam, ok, H, r = op[s][i]
            _check_rows_shape(H, gobs[s][i], n_state, (name, s, i))
            _against_reference(g, bars[s], gam, ok, _own(H, gobs[s][i]), r, (name, 'operator', s, i), worst if s == 0 else None)
    left = sum(g['left_out'] for g in refs[0])
    assert left == 0
    assert {g['ok'] for g in refs[0]} == {True, False} and {o[1] for o in op[0]} == {True, False}
    for k in ('HtH', 'Htr', 'rtr', 'gamma'):
        print('PARITY %s operator %s e_fam %.2e worst %.2e ratio %.3f left_out %d' % (name, k, bars[0][k], worst[k], worst[k] / (Cs.FACTOR * bars[0][k]), left))

    # ---- the list launches
    compact = 12 if M == 2 else 0
    slot_obs = [gobs[s][k % ng] for s in range(2) for k in range(FS)]
    slot_pos = np.array([pos[s][k % ng] for s in range(2) for k in range(FS)])
    perm = _perm(2 * FS, fam['seed'] + 7)
    first = {}                                          # (stream, feature) -> what the first list launch gave
    worst8 = dict(HtH=0.0, Htr=0.0, rtr=0.0, gamma=0.0)
    for wg in GRIDS:
        for L in LISTS:
            valid = np.ones(2 * FS, np.int32)
            valid[perm[2::5]] = 0                       # holes: every fifth listed slot, from the third
            out = _ops_dev(dev, cfg, fams, slot_obs, np.array(P), M, _teams(M, wg), feat_list=perm[:L], positions=slot_pos, valid=valid,
                           compact=compact, zero_fill=0 if compact else 1)
            listed = set(int(v) for v in perm[:L])
            touched = np.zeros(out['H'].shape[:2], bool)
            for f in range(2 * FS):
                s, k = divmod(f, FS)
                if f not in listed:
                    assert np.isnan(out['gamma'][f]) and out['ok'][f] == -1, (wg, L, f)
                    continue
                if not valid[f]:
                    assert out['gamma'][f] == 0.0 and out['ok'][f] == 0, (wg, L, f)
                    continue
                r0, K = out['row_off'][f], out['rows'][f]
                assert K == 4 * M - 3 and out['ok'][f] in (0, 1)
                touched[s, r0:r0 + K] = True
                got = (out['gamma'][f], bool(out['ok'][f]), out['H'][s, r0:r0 + K], out['r'][s, r0:r0 + K])
                if exact:                               # full-width rows, cleared first: the operator entry's rows, zeros included
                    gam, ok, H, r = op[s][k % ng]
                    assert got[0] == gam and got[1] == ok and np.array_equal(got[3], r) and np.array_equal(got[2][:, :n_state], H[:, :n_state]), (wg, L, f, got[0], gam)
                elif (s, k % ng) in first:
                    was = first[(s, k % ng)]
                    assert got[0] == was[0] and got[1] == was[1] and np.array_equal(got[2], was[2]) and np.array_equal(got[3], was[3]), (wg, L, f)
                else:                                   # a row's 12 doubles are the two cameras' columns in observation order: the reference's order
                    first[(s, k % ng)] = got
                    _against_reference(refs[s][k % ng], bars[s], got[0], got[1], got[2], got[3], (name, 'list', wg, L, f), worst8 if s == 0 else None)
            assert np.isnan(out['H'][~touched]).all() and np.isnan(out['r'][~touched]).all(), (wg, L)
    if not exact:
        assert len(first) >= 2 * ng - 2
        for k in ('HtH', 'Htr', 'rtr', 'gamma'):
            print('PARITY %s list %s e_fam %.2e worst %.2e ratio %.3f left_out %d' % (name, k, bars[0][k], worst8[k], worst8[k] / (Cs.FACTOR * bars[0][k]), left))

    # ---- chained: the gate reads the position and the flag the triangulation ahead of it wrote
    kw = dict(compact=compact, zero_fill=0 if compact else 1)
    out = _ops_dev(dev, cfg, fams, slot_obs, np.array(P), M, _teams(M, 3), tri_list=perm[:65], feat_list=perm[:65], valid=np.full(2 * FS, -7), **kw)
    tri = [_op_triangulate(dev, dict(fams[s], obs=gobs[s])) for s in range(2)]
    if exact:
        chained = [_op_gate(dev, fams[s], cfg, gobs[s], tri[s][0], P[s]) for s in range(2)]
    else:           # (the 8-lane kernel again, given what the triangulation gave)
        two = _ops_dev(dev, cfg, fams, slot_obs, np.array(P), M, _teams(M, 1), feat_list=perm[:65], positions=out['pos'], valid=out['valid'], **kw)
    for f in perm[:65]:
        s, k = divmod(int(f), FS)
        assert np.array_equal(out['pos'][f], tri[s][0][k % ng]) and bool(out['valid'][f]) == bool(tri[s][1][k % ng])
        if not out['valid'][f]:
            assert out['gamma'][f] == 0.0 and out['ok'][f] == 0
            continue
        r0, K = out['row_off'][f], out['rows'][f]
        if exact:
            gam, ok, H, r = chained[s][k % ng]
            assert out['gamma'][f] == gam and bool(out['ok'][f]) == ok and np.array_equal(out['H'][s, r0:r0 + K], H[:, :n_state])
        else:
            assert out['gamma'][f] == two['gamma'][f] and out['ok'][f] == two['ok'][f] and np.array_equal(out['H'][s, r0:r0 + K], two['H'][s, r0:r0 + K])


@pytest.mark.parametrize('name', ['m2_5m', 'm3_5m'])
def test_short_tracks_in_a_longer_batch(dev, cfg, name):
    """A batch that also holds a four-observation feature goes through feature_kernel<64> with a per-feature track length (four teams
    per workgroup in the operator entry, one wavefront per workgroup in the list launch, there with full-width rows that are NOT cleared
    first, as the pruning phase writes them when its update needs the Cholesky back end): two-observation features against the
    reference once more (another kernel than <16> / the 8-lane one), three-observation features the same bits as on their own."""
    fam = Cs.make_family(name, cfg)
    pos, gobs, P = Cs.gate_inputs(fam, cfg)
    ref, bars = Cs.gate_reference(fam, cfg), Cs.gate_bars(fam, cfg)
    n_state = 21 + 6 * len(fam['cam_q'])
    long_one = [(c, Cs._project(fam['cam_q'][c], fam['cam_p'][c], fam['T01'], fam['pts'][0])) for c in range(4)]
    obs, posx = gobs + [long_one], np.vstack([pos, fam['pts'][0]])
    alone = _op_gate(dev, fam, cfg, gobs, pos, P)
    mixed = _op_gate(dev, fam, cfg, obs, posx, P)
    for i, g in enumerate(ref):
        gam, ok, H, r = mixed[i]
        _check_rows_shape(H, gobs[i], n_state, (name, i))
        _against_reference(g, bars, gam, ok, _own(H, gobs[i]), r, (name, 'mixed', i))
        if fam['M'] > 2:
            assert gam == alone[i][0] and np.array_equal(H, alone[i][2]) and np.array_equal(r, alone[i][3])
    n = len(obs)
    slot_obs = [obs[(s * FS + k) % n] for s in range(2) for k in range(FS)]
    slot_pos = np.array([posx[(s * FS + k) % n] for s in range(2) for k in range(FS)])
    lst = _perm(2 * FS, 5)[:33]
    out = _ops_dev(dev, cfg, (fam, fam), slot_obs, np.array([P, P]), 4, 3, feat_list=lst, positions=slot_pos, valid=np.ones(2 * FS), zero_fill=0)
    for f in lst:
        s, i = divmod(int(f), FS)[0], int(f) % n
        gam, ok, H, r = mixed[i]
        r0, K = out['row_off'][f], out['rows'][f]
        own = R.own_columns(obs[i])
        rows = out['H'][s, r0:r0 + K]
        assert out['gamma'][f] == gam and bool(out['ok'][f]) == ok and np.array_equal(out['r'][s, r0:r0 + K], r)
        assert np.array_equal(rows[:, own], H[:, own]) and np.isnan(np.delete(rows, own, axis=1)).all()
