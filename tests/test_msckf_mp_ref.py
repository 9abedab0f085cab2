"""The 50-digit reference of the per-feature chain (tests/msckf_mp_ref.py) held to the fp64 oracle (oracle/msckf_np.py) and to the
vectors the reference filter itself recorded (tests/golden/msckf_units.npz), on the CPU.

What fp64 achieves against 50 digits here is the yardstick of tests/test_gpu_msckf_features.py.  Measured (the oracle on this
suite's inputs; position errors as msckf_feature_cases.pos_err, the others relative to the quantity's largest entry):

 * the 60 recorded triangulations: the reference's validity flags equal the recorded ones; 37 cases are decided (no Levenberg-
   Marquardt step whose cost comparison is closer than 1e-12) and the recorded positions are within 4.3e-15 of the reference there,
   the median 8e-16; 23 have an undecided step, of which 21 still agree to 2.3e-13 and two differ by 8.1e-10 and 5.6e-9, 0.43 and
   0.19 of what the undecided steps allow (und * d * max(1, d));
 * seeded families (2 .. 9 observations, 5 .. 100 m): triangulation 5e-15 .. 1e-14 at 5 .. 10 m, 1e-13 .. 4.5e-13 at 40 m with a
   2 cm baseline and at 100 m; H_o^T H_o 9e-16 .. 1.3e-14, H_o^T r_o 8e-15 .. 1e-13, r_o^T r_o 9e-16 .. 5e-14, gamma 9e-15 .. 7e-12.
"""
import numpy as np
import pytest

import msckf_feature_cases as Cs
import msckf_mp_ref as R


def test_reference_reproduces_the_recorded_triangulations(cfg):
    """Flags equal; position within 1e-13 + und * d * max(1, d) of the recorded one (pos_err), for the reference filter's own recorded
    results and for the oracle."""
    fam = Cs.make_recorded(cfg)
    ref = Cs.tri_reference(fam)
    assert len(ref) == 60
    worst, decided = 0.0, []
    for i, t in enumerate(ref):
        assert not t['left_out'], (i, float(t['huber_margin']), float(t['stop_margin']))
        assert t['valid'] == bool(fam['ref_ok'][i]) == t['oracle_valid'], i
        for name, p in (('recorded', fam['ref_pos'][i]), ('oracle', t['oracle_pos'])):
            e = Cs.pos_err(p, t)
            bound = 1e-13 + t['slack']
            assert e <= bound, (i, name, e, bound)
            worst = max(worst, e / bound)
        if t['und'] == 0:
            decided.append(Cs.pos_err(fam['ref_pos'][i], t))
    print('recorded triangulations: decided %d, worst decided error %.2e, median %.2e, largest ratio to the bound %.2f, smallest Huber / stop margin %.2e / %.2e'
          % (len(decided), max(decided), np.median(decided), worst, min(float(t['huber_margin']) for t in ref), min(float(t['stop_margin']) for t in ref)))
    assert len(decided) >= 37 and max(decided) <= 1e-14


def test_special_cases_are_invalid_in_reference_and_oracle(cfg):
    for fam in Cs.make_special(cfg):
        t = Cs.tri_reference(fam)[0]
        assert t['valid'] is False and t['oracle_valid'] is False, fam['name']
        assert t['degenerate'] == (fam['name'] == 'zero_parallax')


# Why these bars (they hold the ORACLE, the kernels' bars come from what the oracle measures): the projected rows are orthogonal
# transforms of H_x and r, so H_o^T H_o carries a few ulp per row of the basis, amplified by the conditioning of H_f^T H_f where the
# parallax is low (measured 1.3e-14 at 40 m with a 2 cm baseline); r = z - h(p) cancels |z| ~ 0.3 down to |r| ~ 2e-3 .. 3e-2, two orders;
# the gate matrix has a condition number of at most 1e3 + 1 by construction of P, and gamma inherits r's cancellation twice.
ORACLE_BARS = dict(HtH=1e-12, Htr=1e-11, rtr=1e-11, gamma=1e-9)


@pytest.mark.parametrize('name', ['m2_5m', 'm4_40m_lowpar', 'm5_5m', 'm9_huber'])
def test_oracle_rows_and_gamma_agree_with_the_reference(cfg, name):
    """A = U[:, 3:] of the oracle's SVD put through the three invariants agrees with the projector form, gating_test's gamma with the
    reference's, the decisions are equal and both occur."""
    fam = Cs.make_family(name, cfg)
    tri = Cs.tri_reference(fam)
    assert all(t['valid'] == t['oracle_valid'] for t in tri if not t['left_out'])
    e_fam = Cs.tri_bar(fam)
    for i, t in enumerate(tri):
        if t['valid'] and not t['left_out']:
            assert t['oracle_err'] <= e_fam + t['slack'], (i, t['oracle_err'])
    gate = Cs.gate_reference(fam, cfg)
    bars = Cs.gate_bars(fam, cfg)
    print(name, 'oracle against the reference: triangulation %.2e' % e_fam, ' '.join('%s %.2e' % kv for kv in sorted(bars.items())))
    for k, v in bars.items():
        assert v <= ORACLE_BARS[k], (k, v)
    for i, g in enumerate(gate):
        assert g['margin'] > Cs.MARGIN_MIN
        assert (g['oracle_gamma'] < Cs.CHI2[g['dof']]) == g['ok'], i
    assert {g['ok'] for g in gate} == {True, False}


def test_gamma_without_a_basis_is_gamma_with_one(cfg):
    fam = Cs.make_family('m5_5m', cfg)
    pos, gobs, P = Cs.gate_inputs(fam, cfg)
    for i in (0, 1):
        rows = R.feature_rows(gobs[i], pos[i], fam['cam_q'], fam['cam_p'], fam['cam_qn'], fam['cam_pn'], fam['T01'], Cs.GRAVITY)
        own = R.own_columns(gobs[i])
        a, b = R.gamma_basis(rows, P[np.ix_(own, own)], cfg.observation_noise), R.gamma(rows, P[np.ix_(own, own)], cfg.observation_noise)
        assert abs(a - b) <= R.mpf('1e-40') * a
        A = R.null_basis(rows['Hf'])
        assert max(abs(v) for v in (A.T.dot(A) - R.eye(A.shape[1])).reshape(-1)) < R.mpf('1e-45')
        assert max(abs(v) for v in A.T.dot(rows['Hf']).reshape(-1)) < R.mpf('1e-45')


def test_long_double_invariants_match_the_50_digit_ones(cfg):
    """rows_errors forms H_o^T H_o of long tracks in long double: on a track both paths can afford they agree far below the bars."""
    fam = Cs.make_family('m9_huber', cfg)
    pos, gobs, P = Cs.gate_inputs(fam, cfg)
    flt = Cs.oracle_filter(fam, P, cfg)
    Ho, ro, _, _ = Cs.oracle_rows(flt, fam, 0, pos[0], gobs[0])
    H, r = np.asarray(Ho, dtype=np.longdouble), np.asarray(ro, dtype=np.longdouble)
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('long double is fp64 on this platform: rows_errors uses the 50-digit path throughout')
    HtH, Htr, rtr = R.rows_invariants(Ho, ro)
    assert Cs.rel_err(Cs._ld_to_mp(H.T @ H), HtH) < 1e-17 and Cs.rel_err(Cs._ld_to_mp(H.T @ r), Htr) < 1e-17 and Cs.rel_err(Cs._ld_to_mp([r @ r]), [rtr]) < 1e-17
