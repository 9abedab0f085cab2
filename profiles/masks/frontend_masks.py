"""What static masks cost or save in the front-end at 64 streams.

    timeout -k 10 240 python profiles/masks/frontend_masks.py [--streams 64] [--steps 20] [--warmup 5]      -> one JSON line

`streams` streams of 752 x 480 frames (16 distinct synthetic scenes, repeated) stepped without masks, with both cameras behind a
fisheye image circle (radius 300 around the image centre) and with the comb masks of the tests (a quarter of every image masked):
wall-clock time per step (host clock around step + synchronize), stream-frames/s, HIP-event time per kernel class and step, and the
corners and published features per frame of stream 1."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 752, 480


def comb(phase):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from mask_ref import comb_mask                      # the tests' own definition
    return comb_mask(W, H, 96, 24, phase)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine, circle_mask
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    D = 16
    S = args.streams - args.streams % D
    n_frames = args.warmup + args.steps
    dev = torch.device('cuda', 0)
    tex = make_texture(0xA1B0)
    streams = [SyntheticStream(ConfigEuRoC(), seed=i, n_frames=n_frames, motion_scale=1.5 + 0.1 * i, texture=tex, tex_offset=(53.0 * i, 29.0 * i)) for i in range(D)]
    state = streams[0].torch_state(dev)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    frames = []
    for k in range(n_frames):
        pairs = [st.frame_torch(k, state, gen) for st in streams]
        frames.append((torch.stack([p[0] for p in pairs]).repeat(S // D, 1, 1).contiguous(), torch.stack([p[1] for p in pairs]).repeat(S // D, 1, 1).contiguous()))
    circle = circle_mask(W, H, 376, 240, 300)
    cases = (('none', None, None), ('circle', circle, circle), ('comb', comb(0), comb(48)))
    result = dict(streams=S, steps=args.steps, warmup=args.warmup, size=[W, H], masked_share={n: (None if a is None else float(1.0 - a.mean())) for n, a, _b in cases})
    for rnd in range(2):                                   # every case twice, alternating: the spread is part of the record
        for name, a, b in cases:
            cfg = ConfigEuRoC()
            cfg.cam0_mask, cfg.cam1_mask = a, b
            eng = FrontendEngine(cfg, n_streams=S)
            its = [iter(st.imu) for st in streams]
            pend = [next(it, None) for it in its]
            wall, fast, published = 0.0, [], []
            for k in range(n_frames):
                t = streams[0].frame_time(k)
                for d in range(D):
                    while pend[d] is not None and pend[d].timestamp <= t:
                        ids = np.arange(d, S, D, dtype=np.int32)
                        eng.push_imu_batch(ids, np.full(len(ids), pend[d].timestamp), np.tile(pend[d].angular_velocity, (len(ids), 1)))
                        pend[d] = next(its[d], None)
                if k == args.warmup:
                    torch.cuda.synchronize()
                    eng.enable_timing(64 * args.steps)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.step(frames[k][0], frames[k][1], [t] * S)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    wall += time.perf_counter() - t1
                    c = eng.read_counters(1)
                    fast.append(c['n_fast']); published.append(c['n_published'])
            tm = eng.read_timing()
            eng.close()
            result.setdefault(name, []).append(dict(wall_ms_per_step=1e3 * wall / args.steps, frames_per_s=S * args.steps / wall,
                                                    ms_per_step={k: v[0] / args.steps for k, v in tm.items()},
                                                    stream1_n_fast_mean=float(np.mean(fast)), stream1_published_mean=float(np.mean(published))))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
