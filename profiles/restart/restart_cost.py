#!/usr/bin/env python3
"""restart_cost.py [--rounds N] [--streams S] -- what one stream-restart call takes (needs an MI355X).

Filter: a BatchedMSCKF of S streams (default 2,048: two groups) fed replicas of one synthetic feature stream (100 features per frame, message
capacity 128) for 30 frames, so that every stream holds a full window and a populated store; then, N times each, `restart([0])` and
`restart(range(S))` with the queue empty: wall clock around the call, which returns when the device state is reset.  The streams are not
fed again: a restart of a stream that has just been restarted does the same work.  Once more with the three optional outputs on.
Front-end: a FrontendEngine of S streams (752 x 480) after two steps on one rendered frame pair; `restart([0])` and `restart(range(S))`
followed by a synchronisation of the stream, against the synchronisation alone.
Prints one JSON line: per case the values in microseconds, min / median / max."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
F, CAP = 30, 128


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


def stats(v):
    v = sorted(v)
    return dict(us=[round(x, 1) for x in v], min=round(v[0], 1), median=round(float(np.median(v)), 1), max=round(v[-1], 1))


def filter_cases(cfg, S, rows, rounds, outputs):
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    kw = dict(odom_cov=True, landmarks=True, landmark_cap=64, stats=True) if outputs else {}
    flt = BatchedMSCKF(cfg, S, max_features=CAP, **kw)
    try:
        for r in rows:
            flt.push_imu(r['idx'], r['t'], r['w'], r['a'])
            out = flt.submit(r['ids'], r['uv'], r['nf'], r['ts'])
            flt.wait(1)
        flt.wait(0)
        assert out[:, 0].min() == 1.0 and flt.sizes(0)[1] >= 18, flt.sizes(0)
        shape = flt.launch_shape()
        one, every = [], []
        everyone = np.arange(S, dtype=np.int32)
        flt.restart([S - 1])                                 # (the first call also pays for the kernel's code object)
        for _ in range(rounds):
            t0 = time.perf_counter(); flt.restart([0]); one.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); flt.restart(everyone); every.append((time.perf_counter() - t0) * 1e6)
        assert flt.sizes(0) == (21, 0, 0) and flt.sizes(S - 1) == (21, 0, 0)
        return dict(shape=shape, one_stream=stats(one), all_streams=stats(every))
    finally:
        flt.close()


def frontend_cases(cfg, S, rounds):
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream
    m = SyntheticStream(cfg, seed=0, n_frames=2).frame(0)
    a0 = torch.from_numpy(np.repeat(m.cam0_image[None], S, 0)).cuda(); a1 = torch.from_numpy(np.repeat(m.cam1_image[None], S, 0)).cuda()
    eng = FrontendEngine(cfg, n_streams=S)
    try:
        for k in range(2):
            eng.step(a0, a1, [m.timestamp + 0.05 * k] * S)
        torch.cuda.synchronize()
        assert eng.read_counters(0)['n_published'] > 20
        one, every, sync, call = [], [], [], []
        everyone = np.arange(S, dtype=np.int32)
        eng.restart([S - 1]); torch.cuda.synchronize()
        for _ in range(rounds):
            t0 = time.perf_counter(); torch.cuda.synchronize(); sync.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); eng.restart([0]); call.append((time.perf_counter() - t0) * 1e6); torch.cuda.synchronize(); one.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); eng.restart(everyone); torch.cuda.synchronize(); every.append((time.perf_counter() - t0) * 1e6)
        assert eng.read_grid(0)['next_feature_id'] == 0
        return dict(one_stream_call_only=stats(call), one_stream=stats(one), all_streams=stats(every), synchronise_alone=stats(sync))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--streams', type=int, default=2048)
    args = ap.parse_args()
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    rows = inputs(cfg, args.streams)
    res = dict(streams=args.streams, rounds=args.rounds)
    res['filter'] = filter_cases(cfg, args.streams, rows, args.rounds, False)
    res['filter_outputs_on'] = filter_cases(cfg, args.streams, rows, args.rounds, True)
    res['frontend'] = frontend_cases(cfg, args.streams, args.rounds)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
