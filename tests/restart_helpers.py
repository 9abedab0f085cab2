"""Driver of the stream-restart tests (include/airvision.h, "Stream restart"): a BatchedMSCKF whose slots are fed LIVES -- a synthetic
feature stream from its first IMU sample and frame, starting at some step of the batch -- with a restart of the slot between two of them.
The comparisons, the step arrays and the environment handling are those of tests/filter_harness.py; the lives are its own.

A plan is, per slot, a list of (first step, stream, frames): the slot gets frame j of the stream at step first + j for j < frames and no
frame (timestamp -1) at every other step.  A life that does not begin at step 0 is preceded by `restart([slot])`; the IMU samples of a life
are pushed after that restart, each before the first frame that is not older than it (synth.replay's rule)."""
import numpy as np

from filter_harness import CAP, ENV_KEYS, LM_CAP, arrays, clean_env, push, same, same_bytes, same_lm      # noqa: F401 (the restart suites take them from here)


def same_step(a, ka, sa, b, kb, sb):
    """All four outputs of stream sa in step ka of run a against stream sb in step kb of run b, bit for bit; the name of the first that
    differs, or None."""
    if not same(a['outs'][ka][sa], b['outs'][kb][sb]):
        return 'pose'
    if not same(a['covs'][ka][sa], b['covs'][kb][sb]):
        return 'covariance'
    if not same_lm(a['lms'][ka], b['lms'][kb], sa, sb):
        return 'landmarks'
    if not same_bytes(a['sts'][ka][sa], b['sts'][kb][sb]):
        return 'statistics'
    return None


class Life(object):
    """One stream fed to a slot from step `first` on, `frames` frames of it; blank: frames whose message is replaced by an empty one."""

    def __init__(self, first, stream, frames, blank=()):
        self.first, self.stream, self.frames, self.blank = int(first), stream, int(frames), tuple(blank)
        self._it = iter(stream.imu)
        self._pend = next(self._it, None)

    def imu_before(self, j):
        """The IMU messages that arrive before frame j (each once)."""
        t = self.stream.frame(j).timestamp
        out = []
        while self._pend is not None and self._pend.timestamp <= t:
            out.append(self._pend)
            self._pend = next(self._it, None)
        return out

    def message(self, j):
        from uav_airvision_amd.synth import feature_msg_t
        m = self.stream.frame(j)
        return feature_msg_t(m.timestamp, []) if j in self.blank else m


def run_lives(cfg, plan, n_steps, env=None, cap=CAP, queued=(), before=None, after_restart=None, oracles=None, outputs=True, **kw):
    """Drives a BatchedMSCKF with len(plan) slots over n_steps steps.  queued: the steps that are `submit`ted and left in the queue (every
    other step is a synchronous `step`, which drains it).  before(k, bat, run): called ahead of step k's restarts; after_restart(k, bat,
    run): right after them.  oracles: {slot: {index of the life in the slot's list: an oracle}}: fed the life's IMU messages and frames
    alongside, run['refs'][k][slot] = its landmark list after step k.  Returns per-step outputs, covariance, landmark and statistics arrays, the final state of every slot, the
    status of every slot after every step."""
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    with clean_env(env):
        bat = None
        try:
            S = len(plan)
            bat = BatchedMSCKF(cfg, S, odom_cov=outputs, landmarks=outputs, landmark_cap=LM_CAP, stats=outputs, **kw)
            assert bat.device_resident()
            run = dict(outs=[], covs=[], lms=[], sts=[], refs=[], status=[], restarts=[])
            for k in range(n_steps):
                if before is not None:
                    before(k, bat, run)
                begin = [i for i in range(S) if any(L.first == k and L.first > 0 for L in plan[i])]
                if begin:
                    bat.restart(begin)                           # (no wait ahead of it: the call drains)
                    run['restarts'].append((k, begin))
                    if after_restart is not None:
                        after_restart(k, bat, run)
                msgs, pushed = [None] * S, []
                for i in range(S):
                    for li, L in enumerate(plan[i]):
                        j = k - L.first
                        if 0 <= j < L.frames:
                            imu = L.imu_before(j)
                            pushed += [(i, m) for m in imu]
                            msgs[i] = L.message(j)
                            ora = (oracles or {}).get(i, {}).get(li)
                            if ora is not None:
                                for m in imu:
                                    ora.imu_callback(m)
                                ora.feature_callback(msgs[i])
                push(bat, pushed)
                ids, uv, nf, ts = arrays(msgs, cap)
                args = dict(cov=True, landmarks=True, stats=True) if outputs else {}
                out = (bat.submit if k in queued else bat.step)(ids, uv, nf, ts, **args)
                run['outs'].append(out); run['covs'].append(bat.last_cov); run['lms'].append(bat.last_landmarks); run['sts'].append(bat.last_stats)
                run['refs'].append({i: list(o.landmarks) for i, d in (oracles or {}).items() for o in d.values()})
                if k not in queued:
                    run['status'].append([bat.stream_status(i) for i in range(S)])
                else:
                    run['status'].append(None)
            bat.wait(0)
            run['state'] = [bat.get_state(i) for i in range(S)]
            run['cov'] = [bat.get_cov(i) for i in range(S)]
            run['sizes'] = [bat.sizes(i) for i in range(S)]
            run['generation'] = bat.generation.copy()
            run['counters'] = bat.counters()
            run['shape'] = bat.launch_shape()
            return run
        finally:
            if bat is not None:
                bat.close()


def same_state(a, b):
    """Two get_state dicts, bit for bit."""
    return sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and
                                          same(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)) for k in a)


def against_landmark_ref(rec, n, s, ref, lm_cap, where):
    """Stream s's landmark records of one step against a LandmarkOracle's list, with the comparison and the bar of
    tests/test_gpu_landmarks.py: ids, flags and n_obs exactly, positions within 1e-6 * max(1, z^2 / b) metres.  Returns the largest
    position error / bar."""
    from uav_airvision_amd.msckf_ops import unpack_landmarks
    assert int(n[s, 0]) == len(ref) and int(n[s, 1]) == min(len(ref), lm_cap), (where, n[s].tolist(), len(ref))
    got = unpack_landmarks(rec, n, s)
    ref = ref[:lm_cap]
    assert got['id'].tolist() == [r['id'] for r in ref], where
    assert got['flags'].tolist() == [r['flags'] for r in ref], (where, got['flags'].tolist(), [r['flags'] for r in ref])
    assert got['n_obs'].tolist() == [r['n_obs'] for r in ref], where
    worst = 0.0
    for g, r in zip(got, ref):
        err, bar = float(np.linalg.norm(g['p'] - r['p'])), 1e-6 * max(1.0, r['z'] ** 2 / r['b'])
        assert err <= bar, (where, r['id'], err, bar)
        worst = max(worst, err / bar)
    return worst
