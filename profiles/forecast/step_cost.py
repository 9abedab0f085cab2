#!/usr/bin/env python3
"""step_cost.py [--rounds N] [--streams S ...] [--cap N] [--tree DIR --cases off] -- what the forecast costs a filter step (needs an MI355X).

The batched filter alone, fed replicas of one synthetic feature stream (100 features and 10 IMU samples per frame, 80 frames) with the
IMU pushed ONE FRAME AHEAD of the frame that consumes it, so that every step has a frame's worth of pending samples (in the `off` case
too: the pushes are the same), alternating cases, N rounds each, as profiles/imu_rate/step_cost.py times the IMU-rate records:
  * 2,048 streams (two groups, one wavefront per stream), submit + wait(1) as bench.py's queued path: ms per step over frames 25 .. 78;
  * one stream, synchronous step: ms per step over the same frames.
Cases: off; on = BatchedMSCKF(forecast=True, forecast_cap=cap), the arrays going to three triples allocated once and handed over in turn.
--tree DIR: import the package from DIR instead of this checkout (a build of the parent commit), with --cases off.
Prints one JSON line: per case the per-round values, min / median / max, the read-back bytes per step and the pending samples of stream 0."""
import argparse
import json
import os
import sys
import time

import numpy as np

F, FIRST, CAP = 80, 25, 128


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


def one(cfg, S, rows, case, cap):
    from uav_airvision_amd import msckf_ops
    on = case == 'on'
    flt = msckf_ops.BatchedMSCKF(cfg, S, max_features=CAP, **({'forecast': True, 'forecast_cap': cap} if on else {}))
    ring = [(np.zeros((S, cap), msckf_ops.IMU_STATE_DTYPE), np.zeros((S, 2), np.int32), np.zeros((S, 120))) for _ in range(3)] if on else None
    had = []
    push = lambda r: flt.push_imu(r['idx'], r['t'], r['w'], r['a'])
    try:
        t0 = None
        push(rows[0])
        for k, r in enumerate(rows[:-1]):
            if k == FIRST:
                flt.wait(0)
                t0 = time.perf_counter()
            push(rows[k + 1])                                 # one frame ahead
            kw = {'forecast': ring[k % 3]} if ring else {}
            if S == 1:
                out = flt.step(r['ids'], r['uv'], r['nf'], r['ts'], **kw)
            else:
                out = flt.submit(r['ids'], r['uv'], r['nf'], r['ts'], **kw)
                flt.wait(1)
            if ring and k >= 3:
                had.append(int(ring[(k - 2) % 3][1][0, 0]))       # (a step that has retired)
        flt.wait(0)
        ms = (time.perf_counter() - t0) * 1e3 / (F - 1 - FIRST)
        assert out[:, 0].min() == 1.0
        return ms, had
    finally:
        flt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--streams', type=int, nargs='+', default=[2048, 1])
    ap.add_argument('--cap', type=int, default=32)
    ap.add_argument('--cases', nargs='+', default=['off', 'on'])
    ap.add_argument('--tree', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    res = {}
    for S in args.streams:
        rows = inputs(cfg, S)
        one(cfg, S, rows, 'off', args.cap)             # (the first run of a size also pays for the allocator and the code objects)
        vals, had = {c: [] for c in args.cases}, {}
        for _ in range(args.rounds):
            for c in args.cases:
                ms, h = one(cfg, S, rows, c, args.cap)
                vals[c].append(ms); had[c] = h
        for c in args.cases:
            v = sorted(vals[c])
            res['S=%d,%s' % (S, c)] = dict(ms_per_step=vals[c], min=v[0], median=float(np.median(v)), max=v[-1],
                                           readback_bytes=S * (12 * 8 + (args.cap * 112 + 8 + 960 if c == 'on' else 0)) + 64,
                                           pending_per_step_stream0=dict(mean=float(np.mean(had[c])), max=int(np.max(had[c]))) if had.get(c) else None)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
