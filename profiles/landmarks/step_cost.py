#!/usr/bin/env python3
"""step_cost.py [--rounds N] [--streams S ...] [--cases CASE ...] -- what the landmark map costs a filter step (needs an MI355X; run from the repository root).

The batched filter alone, fed replicas of one synthetic feature stream (100 features per frame, 80 frames), alternating cases, N rounds each:
  * 2,048 streams (two groups, one wavefront per stream), submit + wait(1) as bench.py's queued path: ms per step over frames 25 .. 79;
  * one stream, synchronous step: ms per step over the same frames.
Cases: off; on64 / on256 = BatchedMSCKF(landmarks=True, landmark_cap=64 / 256), the records going to three pairs of arrays allocated once
and handed over in turn; drop64 = the map is on and no step has a destination (the kernels write the records, the copies bring them to the
pinned buffers, nothing is handed out).
Prints one JSON line: per case the per-round values, min / median / max, the read-back bytes per step and the records a step had."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

F, FIRST, CAP = 80, 25, 128
CASES = {'off': 0, 'on64': 64, 'on256': 256, 'drop64': 64}


def inputs(cfg, S):
    from uav_airvision_amd.synth import SyntheticFeatureStream
    st = SyntheticFeatureStream(cfg, seed=0, n_frames=F, n_features=100)
    T = np.array([m.timestamp for m in st.imu]); W = np.array([m.angular_velocity for m in st.imu]); A = np.array([m.linear_acceleration for m in st.imu])
    rows, prev = [], -np.inf
    for k in range(F):
        m = st.frame(k)
        sel = (T <= m.timestamp) & (T > prev)
        prev = m.timestamp
        n = int(sel.sum())
        ids = np.zeros((1, CAP), np.int64); uv = np.zeros((1, CAP, 4)); nf = len(m.features)
        ids[0, :nf] = [f.id for f in m.features]
        uv[0, :nf] = [(f.u0, f.v0, f.u1, f.v1) for f in m.features]
        rows.append(dict(idx=np.repeat(np.arange(S, dtype=np.int32), n), t=np.tile(T[sel], S), w=np.tile(W[sel], (S, 1)), a=np.tile(A[sel], (S, 1)),
                         ids=np.repeat(ids, S, 0), uv=np.repeat(uv, S, 0), nf=np.full(S, nf, np.int32), ts=np.full(S, m.timestamp)))
    return rows


def one(cfg, S, rows, case):
    from uav_airvision_amd.msckf_ops import LANDMARK_DTYPE, BatchedMSCKF
    lc = CASES[case]
    flt = BatchedMSCKF(cfg, S, max_features=CAP, landmarks=lc > 0, landmark_cap=max(lc, 1))
    ring = [(np.zeros((S, lc), LANDMARK_DTYPE), np.zeros((S, 2), np.int32)) for _ in range(3)] if case.startswith('on') else None
    had = []
    try:
        t0 = None
        for k, r in enumerate(rows):
            if k == FIRST:
                flt.wait(0)
                t0 = time.perf_counter()
            flt.push_imu(r['idx'], r['t'], r['w'], r['a'])
            lm = ring[k % 3] if ring else None
            if S == 1:
                out = flt.step(r['ids'], r['uv'], r['nf'], r['ts'], landmarks=lm)
            else:
                out = flt.submit(r['ids'], r['uv'], r['nf'], r['ts'], landmarks=lm)
                flt.wait(1)
            if ring and k >= 3:
                had.append(int(ring[(k - 2) % 3][1][0, 0]))     # (a step that has retired)
        flt.wait(0)
        ms = (time.perf_counter() - t0) * 1e3 / (F - FIRST)
        assert out[:, 0].min() == 1.0
        return ms, had
    finally:
        flt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--streams', type=int, nargs='+', default=[2048, 1])
    ap.add_argument('--cases', nargs='+', default=['off', 'on64', 'on256'], choices=sorted(CASES))
    args = ap.parse_args()
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    res = {}
    for S in args.streams:
        rows = inputs(cfg, S)
        one(cfg, S, rows, 'off')                       # (the first run of a size also pays for the allocator and the code objects)
        vals, had = {c: [] for c in args.cases}, {}
        for _ in range(args.rounds):
            for c in args.cases:
                ms, h = one(cfg, S, rows, c)
                vals[c].append(ms); had[c] = h
        for c in args.cases:
            v = sorted(vals[c])
            res['S=%d,%s' % (S, c)] = dict(ms_per_step=vals[c], min=v[0], median=float(np.median(v)), max=v[-1],
                                           readback_bytes=S * (12 * 8 + CASES[c] * 40 + (8 if CASES[c] else 0)) + 64,
                                           records_per_step_stream0=dict(mean=float(np.mean(had[c])), max=int(np.max(had[c]))) if had.get(c) else None)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
