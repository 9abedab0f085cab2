"""The NumPy statement of the IMU-rate odometry's contract (tests/imu_rate_ref.py) held, on the CPU, to the 50-digit predict_new_state
(tests/msckf_mp_ref.py) on the cases the GPU suite uses (tests/msckf_predict_cases.py: families samples, rate, sparsity, gap), sample by
sample.  The bars are the ones msckf_predict_cases.bars gives for q, p, v -- the fp64 oracle's own end-of-frame error over the family,
floored at 4 ulp -- times the project's FACTOR of 16, the bar the kernels get; t and w are exact."""
import numpy as np
import pytest

import imu_rate_ref as Ir
import msckf_predict_cases as Pc

FAMILIES = ('samples', 'rate', 'sparsity', 'gap')


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('name', FAMILIES)
def test_recording_oracle_against_the_50_digit_reference(cfg, name):
    bars = Pc.bars(name, cfg)
    worst = dict(q=0.0, p=0.0, v=0.0)
    for case, r in zip(Pc.family(name, cfg), Pc.reference(name, cfg)):
        got, ref = Ir.predict_case(case, cfg), Ir.mp_states(case)
        assert len(got) == len(ref) == len(case['imu']), case['name']
        for k, (g, m, want) in enumerate(zip(got, case['imu'], ref)):
            assert g['t'] == m[0] and _bits(g['w'], m[1:4] - case['state']['bg']), (case['name'], k)
            for f in ('q', 'p', 'v'):
                e = Pc.vec_err(g[f], want[f], quaternion=f == 'q')
                worst[f] = max(worst[f], e)
                assert e <= Pc.FACTOR * bars[f], (case['name'], k, f, e, bars[f])
        if got:                                               # the last record is the state the frame's prediction ends with
            ora = r['oracle']
            assert _bits(got[-1]['q'], ora['q']) and _bits(got[-1]['p'], ora['p']) and _bits(got[-1]['v'], ora['v']), case['name']
    print('IMU-RATE ref %s: worst / (16 e_fam)  q %.3f  p %.3f  v %.3f' % ((name,) + tuple(worst[f] / (Pc.FACTOR * bars[f]) for f in ('q', 'p', 'v'))))


def test_the_families_hold_what_the_contract_names(cfg):
    """0, 1, 10 and 17 samples; both sides of the 1e-5 rad/s branch; a sample that repeats its predecessor's stamp, which still gets a
    record of its own."""
    assert sorted(len(c['imu']) for c in Pc.family('samples', cfg)) == [0, 1, 10, 17]
    margins = [np.linalg.norm(m[1:4] - c['state']['bg']) > 1e-5 for c in Pc.family('rate', cfg) for m in c['imu']]
    assert any(margins) and not all(margins)
    case = Pc.family('sparsity', cfg)[2]
    assert case['imu'][2, 0] == case['imu'][1, 0]
    got = Ir.predict_case(case, cfg)
    assert len(got) == 4 and got[2]['t'] == got[1]['t']
    assert _bits(got[2]['p'], got[1]['p']) and _bits(got[2]['v'], got[1]['v'])      # dt = 0 moves nothing


def test_cap_rule_keeps_the_last_samples_in_order():
    states = [dict(t=float(k)) for k in range(10)]
    assert Ir.capped(states, 32) == (10, 10, states)
    had, wr, kept = Ir.capped(states, 4)
    assert (had, wr) == (10, 4) and [s['t'] for s in kept] == [6.0, 7.0, 8.0, 9.0]
    assert Ir.capped([], 4) == (0, 0, [])
    assert Ir.capped(states[:4], 4) == (4, 4, states[:4])


def test_synthetic_streams_overflow_cap_4_and_not_cap_32(cfg):
    """The three streams of tests/test_gpu_imu_rate.py give about 10 samples per frame: cap = 4 overflows, cap = 32 does not."""
    import imu_rate_harness as Ih
    streams = Ih.streams3(cfg)
    rows = Ih.H.schedule(streams, Ih.N_FRAMES)
    oras = [Ir.ImuRateOracle(cfg) for _ in streams]
    most, live = 0, 0
    for k in range(Ih.N_FRAMES):
        for i, m in rows[k]:
            oras[i].imu_callback(m)
        for i, st in enumerate(streams):
            oras[i].feature_callback(st.frame(k))
            n = len(oras[i].imu_states)
            most, live = max(most, n), live + (n > 0)
    assert 4 < most <= 32 and live > 2 * Ih.N_FRAMES, (most, live)
