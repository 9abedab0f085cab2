#!/usr/bin/env python3
"""step_cost.py [--rounds N] [--streams S ...] [--tree DIR --cases off] -- what the zero-velocity update costs a filter step, and what it
does to a resting stream (needs an MI355X).

The batched filter alone, fed replicas of one synthetic feature stream (40 features and 10 IMU samples per frame, 80 frames, pixel
sigma 0.05), alternating cases, N rounds each, as profiles/forecast/step_cost.py times the forecast:
  * 2,048 streams (two groups, one wavefront per stream), submit + wait(1) as bench.py's queued path: ms per step over frames 25 .. 78;
  * one stream, synchronous step: ms per step over the same frames.
Cases: off; on = BatchedMSCKF(zupt=True) with the config's defaults.  Streams: `rest` (motion_scale = 0: every stream is detected and
updated in every step) and `moving` (motion_scale = 1: the detector runs, the update returns at once).
--tree DIR: import the package from DIR instead of this checkout (a build of the parent commit), with --cases off.
--drift: instead, one resting stream of 60 frames, off and on: |v| and |p - p(frame 0)| after the last frame.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

F, FIRST, CAP = 80, 25, 64


def inputs(cfg, S, motion_scale, frames=F):
    from uav_airvision_amd.synth import SyntheticFeatureStream
    st = SyntheticFeatureStream(cfg, seed=0, n_frames=frames, n_features=40, pixel_sigma=0.05, motion_scale=motion_scale)
    T = np.array([m.timestamp for m in st.imu]); W = np.array([m.angular_velocity for m in st.imu]); A = np.array([m.linear_acceleration for m in st.imu])
    rows, prev = [], -np.inf
    for k in range(frames):
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
    from uav_airvision_amd import msckf_ops
    on = case == 'on'
    flt = msckf_ops.BatchedMSCKF(cfg, S, max_features=CAP, **({'zupt': True} if on else {}))
    try:
        t0 = None
        for k, r in enumerate(rows):
            if k == FIRST:
                flt.wait(0)
                t0 = time.perf_counter()
            flt.push_imu(r['idx'], r['t'], r['w'], r['a'])
            if S == 1:
                out = flt.step(r['ids'], r['uv'], r['nf'], r['ts'])
            else:
                out = flt.submit(r['ids'], r['uv'], r['nf'], r['ts'])
                flt.wait(1)
        flt.wait(0)
        ms = (time.perf_counter() - t0) * 1e3 / (len(rows) - FIRST)
        assert out[:, 0].min() == 1.0
        z = flt.read_zupt()[0] if on else None
        gs = flt.get_state(0)
        return ms, (None if z is None else (int(z['detected_total']), int(z['applied_total']))), gs
    finally:
        flt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--streams', type=int, nargs='+', default=[2048, 1])
    ap.add_argument('--cases', nargs='+', default=['off', 'on'])
    ap.add_argument('--drift', action='store_true')
    ap.add_argument('--tree', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    res = {}
    if args.drift:
        rows = inputs(cfg, 1, 0.0, frames=60)
        for c in args.cases:
            _, tot, gs = one(cfg, 1, rows, c)
            res['drift,' + c] = dict(v_norm=float(np.linalg.norm(gs['v'])), p_drift=float(np.linalg.norm(gs['p'])), ba_norm=float(np.linalg.norm(gs['ba'])), totals=tot)
        print(json.dumps(res))
        return
    for S in args.streams:
        for name, scale in (('rest', 0.0), ('moving', 1.0)):
            rows = inputs(cfg, S, scale)
            one(cfg, S, rows, 'off')                      # (the first run of a size also pays for the allocator and the code objects)
            vals, tots = {c: [] for c in args.cases}, {}
            for _ in range(args.rounds):
                for c in args.cases:
                    ms, tot, _ = one(cfg, S, rows, c)
                    vals[c].append(ms); tots[c] = tot
            for c in args.cases:
                v = sorted(vals[c])
                res['S=%d,%s,%s' % (S, name, c)] = dict(ms_per_step=vals[c], min=v[0], median=float(np.median(v)), max=v[-1], totals_stream0=tots[c])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
