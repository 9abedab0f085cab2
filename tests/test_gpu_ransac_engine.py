"""The front-end engine with config.use_ransac against the CPU oracle front-end with the NumPy reference of tests/ransac_ref.py
inserted where the engine runs its stage; the switch off; placement independence in a batch."""
import numpy as np
import pytest

import ransac_ref as rr
from fe_harness import Frames, against_oracle, bare_cfg, make_cfg as _cfg, read_ransac_counts, run_engine, same as _same
from ransac_helpers import REGION, STREAM, check_ransac_counts, run_ransac_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def moving():
    from uav_airvision_amd.synth import SyntheticStream
    cfg = _cfg(use_ransac=True)
    st = Frames.cached(SyntheticStream(cfg, **STREAM))
    return cfg, st, run_ransac_oracle(cfg, st)


def test_engine_with_ransac_matches_the_oracle_on_a_stream_with_a_moving_region(moving):
    """26 frames of a stream whose central rectangle moves on its own: published ids and coordinates bit-identical to the oracle
    with the reference stage on every frame, read_ransac_counts equal to the oracle's, in both level-0 modes, through step_host and
    through the frame store.  The preconditions are asserted here so that the comparison cannot pass vacuously.  The stream's seed
    was picked on the CPU oracle among 11 .. 14 for the largest decision margin: seed 13 has 5.1e-4 as its smallest margin, features
    rejected on 18 of 26 frames, 81 rejected in all, 73 of them (90 %) inside the moving rectangle.  (Seed 11 has a hypothesis that
    gathers exactly 0.2 n pairs, seed 12 only 78 % of its rejections inside.)"""
    cfg, st, ref = moving
    n = len(ref)
    assert n >= 25
    # preconditions on the oracle's own run
    assert all(r['margin'] >= 1e-9 for r in ref), [(k, r['margin']) for k, r in enumerate(ref) if r['margin'] < 1e-9]
    rej_frames = [k for k, r in enumerate(ref) if k > 0 and r['nf']['after_ransac'] < r['nf']['after_matching']]
    assert len(rej_frames) * 3 >= n, (len(rej_frames), n)
    rejected = [p for r in ref for p in r['rejected']]
    inside = sum(st.in_moving_region(float(p[0]), float(p[1])) for p in rejected)
    print('frames with rejections %d of %d, rejected %d, inside the moving region %d' % (len(rej_frames), n, len(rejected), inside))
    assert len(rejected) >= 20 and inside >= 0.8 * len(rejected), (inside, len(rejected))
    assert any((r['counts'][3] & 15) == rr.PATH_MODEL for r in ref)
    for tag, mode in (('copy', 'step'), ('in place', 'persist'), ('host', 'host'), ('frames', 'frames')):
        got = run_engine(cfg, [st], mode=mode, read=read_ransac_counts)[0]
        against_oracle(ref, got, tag)
        check_ransac_counts(ref, got, tag)


def test_off_is_off(moving):
    """use_ransac = False is bit-identical to a config object without the attribute, with the same number of timing spans per step;
    the switch on shows exactly one span more, in the glue class; and it changes what is published."""
    _cfg_on, st, _ref = moving
    from uav_airvision_amd.synth import SyntheticStream
    short = Frames.cached(SyntheticStream(_cfg(), **dict(STREAM, n_frames=8)))

    bare = bare_cfg(lambda k: k.startswith('ransac_') or k == 'use_ransac')
    assert not hasattr(bare, 'use_ransac')
    off, sp_off = run_engine(_cfg(use_ransac=False), [short], timing=True, read=read_ransac_counts)
    none, sp_none = run_engine(bare, [short], timing=True, read=read_ransac_counts)
    on, sp_on = run_engine(_cfg(use_ransac=True), [short], timing=True, read=read_ransac_counts)
    assert all(_same(a, b) for a, b in zip(off[0], none[0]))
    assert sp_off == sp_none
    assert all(g[3] == dict(after_ransac=0, cam0_set=0, cam1_set=0, path=0) for g in off[0])
    assert [(s['glue'] + 1, sum(s.values()) + 1) for s in sp_off] == [(s['glue'], sum(s.values())) for s in sp_on], (sp_off, sp_on)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(off[0], on[0]))


def test_a_stream_gives_the_same_result_anywhere_in_a_batch():
    """One stream alone = the same stream as entry 0, 17 and 63 of a 64-stream batch of different streams, RANSAC on."""
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    cfg = _cfg(use_ransac=True)
    nf = 5
    tex = make_texture(0xA1B0 + 3)
    probe = Frames.cached(SyntheticStream(cfg, **dict(STREAM, n_frames=nf)))
    alone = run_engine(cfg, [probe], read=read_ransac_counts)[0]
    assert any(g[3]['after_ransac'] < g[2]['after_matching'] for g in alone)
    # the other 61 entries replay six other streams (rendering 61 would take minutes): what matters is that they are not the probe
    pool = [Frames.cached(SyntheticStream(cfg, seed=100 + i, n_frames=nf, motion_scale=1.0 + 0.4 * i, texture=tex, tex_offset=(37.0 * i, 11.0 * i),
                                   moving_region=REGION if i % 2 else None)) for i in range(6)]
    others = [pool[i % 6] for i in range(61)]
    batch = list(others)
    for pos in (0, 17, 63):
        batch.insert(pos, probe)
    assert len(batch) == 64 and all(batch[p] is probe for p in (0, 17, 63))
    got = run_engine(cfg, batch, read=read_ransac_counts)
    for pos in (0, 17, 63):
        assert all(_same(a, b) for a, b in zip(alone, got[pos])), pos
    assert not all(_same(a, b) for a, b in zip(alone, got[1]))
