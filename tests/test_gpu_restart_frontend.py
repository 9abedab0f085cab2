"""Stream restart of the front-end engine (include/airvision.h, "Stream restart"; FrontendEngine.restart): two rendered streams for 8
frames, then `restart([1])` and stream 1 is fed ANOTHER rendered stream from its frame 0 (and its first IMU sample) for 8 more frames.
  * stream 0 -- ids, coordinates as bit patterns, counters, grid -- equals the run in which nothing was restarted, on all 16 frames;
  * stream 1 after the restart equals a fresh engine on the new life frame by frame, and a fresh OracleFrontend: ids begin again at 0
    and the first frame is an initialisation;
on the entry paths `step`, `step_host`, inputs_persist + `prestage` with the restart BETWEEN the prestage and the step, and the frame
store (`step_frames`); once more with RANSAC and CLAHE on (the draws hash the stream's frame number; the stage owns the per-stream mask)
engine against engine; and with a feature read-back pending across the restart, which still delivers the old life's features."""
import numpy as np
import pytest

import fe_harness as H

pytestmark = pytest.mark.gpu

N1, N2 = 8, 8               # frames before the restart, frames of the new life
MODES = ('step', 'host', 'prestage', 'frames')

_STREAMS = {}


def _streams(cfg):
    """Rendered once: stream 0 (16 frames), stream 1's first life (16 frames, of which the restarted run uses 8), its second life (8)."""
    if 'all' not in _STREAMS:
        from uav_airvision_amd.synth import SyntheticStream
        _STREAMS['all'] = (H.Frames.cached(SyntheticStream(cfg, seed=11, n_frames=N1 + N2)), H.Frames.cached(SyntheticStream(cfg, seed=12, n_frames=N1 + N2)),
                           H.Frames.cached(SyntheticStream(cfg, seed=13, n_frames=N2)))
    return _STREAMS['all']


def _grid_same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _run(cfg, plan, n_steps, mode, pending=False):
    """One FrontendEngine, a slot per entry of plan = [(first step, Frames, frames), ...]: every slot has exactly one frame in every
    step.  A life that does not begin at step 0 is preceded by restart([slot]); its IMU samples are pushed after that.  Per slot and step
    (ids, uv, counters) and the grid.  pending: a read-back is begun ahead of every restart and ended after the step that follows;
    run['pending'] = [(what it delivered, the features of the step before)]."""
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    S = len(plan)
    eng = FrontendEngine(cfg, n_streams=S, inputs_persist=mode == 'prestage')
    try:
        if mode == 'frames':
            eng.frames_reserve(2 * S + 1)
        imu = {}
        out, grids, pend_out, gens = [[] for _ in plan], [[] for _ in plan], [], []

        def life(i, k):
            for first, fr, n in plan[i]:
                if first <= k < first + n:
                    return first, fr
            raise AssertionError('slot %d has no frame at step %d' % (i, k))

        def arrays(k):
            ms = [life(i, k)[1].frame(k - life(i, k)[0]) for i in range(S)]
            return np.stack([m.cam0_image for m in ms]), np.stack([m.cam1_image for m in ms]), [m.timestamp for m in ms]
        dev, last = {}, None
        for k in range(n_steps):
            begin = [i for i in range(S) if life(i, k)[0] == k and k > 0]
            if begin:
                if pending:
                    eng.read_features_begin(1)
                eng.restart(begin)                           # (prestage mode: the pyramids of this step's images are already built)
            a0, a1, ts = arrays(k)
            for i in range(S):
                first, fr = life(i, k)
                if (i, first) not in imu:
                    it = iter(fr.imu)
                    imu[i, first] = [it, next(it, None)]
                st = imu[i, first]
                while st[1] is not None and st[1].timestamp <= ts[i]:
                    eng.push_imu(i, st[1].timestamp, st[1].angular_velocity)
                    st[1] = next(st[0], None)
            if mode in ('step', 'prestage'):
                if k not in dev:
                    dev[k] = (torch.from_numpy(a0).cuda(), torch.from_numpy(a1).cuda())
                eng.step(dev[k][0], dev[k][1], ts)
            elif mode == 'host':
                eng.step_host(a0.copy(), a1.copy(), ts)
            else:
                slots = (np.arange(S, dtype=np.int32)[::-1] + 1 + (k & 1) * S).astype(np.int32)
                eng.frames_upload(slots, a0.copy(), a1.copy())
                eng.step_frames(slots, ts)
            if begin and pending:
                ids, uv, n = eng.read_features_end(1)
                pend_out.append(([(ids[s, :n[s]].copy(), uv[s, :n[s]].copy()) for s in range(S)], last))
            feats = eng.read_features()
            last = feats
            for i in range(S):
                out[i].append((feats[i][0], feats[i][1], eng.read_counters(i)))
                grids[i].append(eng.read_grid(i))
            if mode == 'prestage' and k + 1 < n_steps:
                b0, b1, _ = arrays(k + 1)
                dev[k + 1] = (torch.from_numpy(b0).cuda(), torch.from_numpy(b1).cuda())
                eng.prestage(*dev[k + 1])
            dev.pop(k - 1, None)
            gens.append(eng.generation.tolist())
        return dict(out=out, grids=grids, pending=pend_out, generation=gens)
    finally:
        eng.close()


_RUNS = {}


def _abc(cfg, tag, mode):
    """A: nothing restarted; B: stream 1 restarted ahead of step 8 and given the new life; C: a fresh engine on the new life alone."""
    key = (tag, mode)
    if key not in _RUNS:
        s0, s1, s2 = _streams(cfg)
        n = N1 + N2
        a = _run(cfg, [[(0, s0, n)], [(0, s1, n)]], n, mode)
        b = _run(cfg, [[(0, s0, n)], [(0, s1, N1), (N1, s2, N2)]], n, mode, pending=mode == 'step')
        c = _run(cfg, [[(0, s2, N2)]], N2, mode)
        _RUNS[key] = (a, b, c)
    return _RUNS[key]


def _check(a, b, c, where):
    for k in range(N1 + N2):
        assert H.same(b['out'][0][k], a['out'][0][k]) and _grid_same(b['grids'][0][k], a['grids'][0][k]), '%s: stream 0 differs at frame %d' % (where, k)
        if k < N1:
            assert H.same(b['out'][1][k], a['out'][1][k]) and _grid_same(b['grids'][1][k], a['grids'][1][k]), '%s: stream 1 differs before the restart, frame %d' % (where, k)
    for j in range(N2):
        assert H.same(b['out'][1][N1 + j], c['out'][0][j]), '%s: second life differs from a fresh engine at frame %d' % (where, j)
        assert _grid_same(b['grids'][1][N1 + j], c['grids'][0][j]), '%s: second life, grid at frame %d' % (where, j)
    first = b['out'][1][N1]
    assert len(first[0]) > 20 and first[0].min() == 0 and first[2]['before_tracking'] == 0, (where, first[2])      # ids begin again at 0; an initialisation
    assert b['grids'][1][N1]['lifetime'].max() == 1 and sorted(first[0].tolist()) == list(range(len(first[0])))
    assert b['generation'][N1 - 1] == [0, 0] and b['generation'][N1] == [0, 1] and b['generation'][-1] == [0, 1]


@pytest.mark.parametrize('mode', MODES)
def test_restart_on_every_entry_path(cfg, mode):
    a, b, c = _abc(cfg, 'plain', mode)
    _check(a, b, c, mode)


def test_second_life_equals_a_fresh_oracle(cfg):
    _, b, _ = _abc(cfg, 'plain', 'step')
    ref = H.run_oracle(cfg, _streams(cfg)[2], N2)
    H.against_oracle(ref, b['out'][1][N1:], 'second life', min_features=20)
    assert ref[0]['ids'].min() == 0


def test_a_pending_read_back_delivers_the_old_life(cfg):
    _, b, _ = _abc(cfg, 'plain', 'step')
    assert len(b['pending']) == 1
    got, want = b['pending'][0]
    for s in range(2):
        assert np.array_equal(got[s][0], want[s][0]) and np.array_equal(got[s][1].view(np.uint64), want[s][1].view(np.uint64)), s
    assert len(want[1][0]) > 20 and not np.array_equal(got[1][0], b['out'][1][N1][0])      # stream 1's old features, not the new life's


def test_restart_with_ransac_and_clahe(cfg):
    """The RANSAC draws hash the stream's frame number and the stage builds the per-stream mask: both start over with the stream."""
    rc = H.make_cfg(use_ransac=True, use_clahe=True)
    a, b, c = _abc(rc, 'ransac+clahe', 'step')
    _check(a, b, c, 'ransac+clahe')
    a, b, c = _abc(rc, 'ransac+clahe', 'frames')
    _check(a, b, c, 'ransac+clahe, frame store')


def test_edges(cfg):
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    eng = FrontendEngine(cfg, n_streams=3)
    try:
        eng.restart([])
        assert eng.generation.tolist() == [0, 0, 0]
        for bad in ([3], [-1], [0, 9]):
            with pytest.raises(N.AirvisionError) as err:
                eng.restart(bad)
            assert err.value.code == N.AV_E_INVALID and 'out of range' in str(err.value)
        assert eng.generation.tolist() == [0, 0, 0]
        eng.restart([2, 2, 0])                               # before the first step; an index listed twice counts once
        assert eng.generation.tolist() == [1, 0, 1]
        assert eng.read_counters(2)['n_published'] == 0 and eng.read_grid(2)['next_feature_id'] == 0
    finally:
        eng.close()
