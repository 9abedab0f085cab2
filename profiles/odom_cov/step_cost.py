#!/usr/bin/env python3
"""step_cost.py [--rounds N] [--streams S ...] [--cases CASE ...] -- what the odometry covariance costs a filter step (needs an MI355X; run from the repository root).

The batched filter alone, fed replicas of one synthetic feature stream (100 features per frame, 80 frames), with BatchedMSCKF(odom_cov=
False) and (odom_cov=True, every step given a records array), alternating, N rounds each:
  * 2,048 streams (two groups, one wavefront per stream), submit + wait(1) as bench.py's queued path: ms per step over frames 25 .. 79;
  * one stream, synchronous step: ms per step over the same frames.
Cases: off; on = every step is given a fresh records array (cov=True); on-reuse = the records go to three arrays allocated once and
handed over in turn (no allocation and no first touch of fresh pages inside the loop); on-drop = the feature is on and no step has a
destination (the kernel writes the records, the copy brings them to the pinned buffer, nothing is handed out).
Prints one JSON line: per case the per-round values, min / median / max, and the read-back bytes per step."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

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


def one(cfg, S, rows, case):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    on = case != 'off'
    flt = BatchedMSCKF(cfg, S, max_features=CAP, odom_cov=on)
    ring = [np.full((S, 120), np.nan) for _ in range(3)] if case == 'on-reuse' else None
    try:
        t0 = None
        for k, r in enumerate(rows):
            if k == FIRST:
                flt.wait(0)
                t0 = time.perf_counter()
            flt.push_imu(r['idx'], r['t'], r['w'], r['a'])
            cov = {'off': None, 'on': True, 'on-drop': None}.get(case, ring[k % 3] if ring else None)
            if S == 1:
                out = flt.step(r['ids'], r['uv'], r['nf'], r['ts'], cov=cov)
            else:
                out = flt.submit(r['ids'], r['uv'], r['nf'], r['ts'], cov=cov)
                flt.wait(1)
        flt.wait(0)
        ms = (time.perf_counter() - t0) * 1e3 / (F - FIRST)
        assert out[:, 0].min() == 1.0 and (case in ('off', 'on-drop') or np.isfinite(flt.last_cov).all())
        return ms
    finally:
        flt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--streams', type=int, nargs='+', default=[2048, 1])
    ap.add_argument('--cases', nargs='+', default=['off', 'on'], choices=['off', 'on', 'on-reuse', 'on-drop'])
    args = ap.parse_args()
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    res = {}
    for S in args.streams:
        rows = inputs(cfg, S)
        one(cfg, S, rows, 'off')                       # (the first run of a size also pays for the allocator and the code objects)
        vals = {c: [] for c in args.cases}
        for _ in range(args.rounds):
            for c in args.cases:
                vals[c].append(one(cfg, S, rows, c))
        for c in args.cases:
            v = sorted(vals[c])
            res['S=%d,%s' % (S, c)] = dict(ms_per_step=vals[c], min=v[0], median=float(np.median(v)), max=v[-1],
                                           readback_bytes=S * (12 + (0 if c == 'off' else 120)) * 8 + 64)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
