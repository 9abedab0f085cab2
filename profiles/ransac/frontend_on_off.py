"""Cost of config.use_ransac in the front-end: a front-end-only loop at 2,048 streams x 300 features (grid 4 x 5 x 15), HIP-event
spans per kernel class (FrontendEngine.enable_timing), switch off against switch on, same frames.

    python profiles/ransac/frontend_on_off.py [--streams 2048] [--steps 12] [--warmup 4] [--only on|off]   -> one JSON line

16 distinct synthetic streams (rendered on the GPU, a moving rectangle in every second one) are replayed by streams/16 replicas
each: the kernels' work per stream is what a distinct stream would give, only the rendering is shared.  For the stage kernel's own
time per launch run the `--only on` form under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=2048)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--only', choices=('on', 'off'), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    D = 16
    S = args.streams - args.streams % D
    n_frames = args.warmup + args.steps
    dev = torch.device('cuda', 0)
    base = ConfigEuRoC(grid_max_feature_num=15, grid_min_feature_num=8)
    tex = make_texture(0xA1B0)
    streams = [SyntheticStream(base, seed=i, n_frames=n_frames, motion_scale=1.5 + 0.1 * i, texture=tex, tex_offset=(53.0 * i, 29.0 * i),
                               moving_region=(250, 150, 500, 330) if i % 2 else None, moving_amplitude=0.3) for i in range(D)]
    state = streams[0].torch_state(dev)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    frames = []
    for k in range(n_frames):
        a0, a1 = [], []
        for st in streams:
            i0, i1 = st.frame_torch(k, state, gen)
            if st.moving_region is not None:               # the rectangle from the shifted pose (SyntheticStream.frame does the same)
                x0, y0, x1, y1 = st.moving_region
                keep = st.position
                st.position = lambda t, st=st, keep=keep: keep(t) + st.region_offset(t)
                j0, j1 = st.frame_torch(k, state, gen)
                st.position = keep
                i0[y0:y1, x0:x1] = j0[y0:y1, x0:x1]; i1[y0:y1, x0:x1] = j1[y0:y1, x0:x1]
            a0.append(i0); a1.append(i1)
        frames.append((torch.stack(a0), torch.stack(a1)))
    rep = S // D
    result = dict(streams=S, features=base.grid_num * base.grid_max_feature_num, steps=args.steps, warmup=args.warmup)
    for tag in ('off', 'on'):
        if args.only and args.only != tag:
            continue
        cfg = ConfigEuRoC(grid_max_feature_num=15, grid_min_feature_num=8)
        cfg.use_ransac = tag == 'on'
        eng = FrontendEngine(cfg, n_streams=S)
        its = [iter(st.imu) for st in streams]
        pend = [next(it, None) for it in its]
        wall = 0.0
        counts = []
        for k in range(n_frames):
            t = streams[0].frame_time(k)
            for d in range(D):
                while pend[d] is not None and pend[d].timestamp <= t:
                    ids = np.arange(d, S, D, dtype=np.int32)
                    eng.push_imu_batch(ids, np.full(len(ids), pend[d].timestamp), np.tile(pend[d].angular_velocity, (len(ids), 1)))
                    pend[d] = next(its[d], None)
            img0 = frames[k][0].repeat(rep, 1, 1).contiguous(); img1 = frames[k][1].repeat(rep, 1, 1).contiguous()      # stream s = distinct s % D
            if k == args.warmup:
                torch.cuda.synchronize()
                eng.enable_timing(64 * args.steps)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eng.step(img0, img1, [t] * S)
            torch.cuda.synchronize()
            if k >= args.warmup:
                wall += time.perf_counter() - t1
                c, r = eng.read_counters(1), eng.read_ransac_counts(1)
                counts.append((c['after_matching'], r['after_ransac']))
        tm = eng.read_timing()
        eng.close()
        result[tag] = dict(ms_per_step={k: v[0] / args.steps for k, v in tm.items()}, spans_per_step={k: v[1] / args.steps for k, v in tm.items()},
                           wall_ms_per_step=1e3 * wall / args.steps, stream1_after_matching_after_ransac=counts)
    if 'on' in result and 'off' in result:
        result['glue_on_minus_off_ms'] = result['on']['ms_per_step']['glue'] - result['off']['ms_per_step']['glue']
        result['wall_on_over_off'] = result['on']['wall_ms_per_step'] / result['off']['wall_ms_per_step']
    print(json.dumps(result))


if __name__ == '__main__':
    main()
