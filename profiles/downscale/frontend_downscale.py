"""What config.image_downscale buys at 1920 x 1200.

    python profiles/downscale/frontend_downscale.py [--streams 64] [--steps 10] [--warmup 3] [--frames 60]      -> one JSON line

Part 1, front-end only: `streams` streams of 1920 x 1200 frames (16 distinct synthetic scenes, repeated) stepped with f = 1, 2 and 4:
stream-frames/s over the timed steps (wall clock around step + synchronize), HIP-event time per kernel class and step, published
features per frame of stream 1.
Part 2, trajectories: one synthetic stream of `frames` frames through the front-end (step_host) and the batched filter with f = 1, 2
and 4; the RMS and the largest distance between the positions of the f = 2 / 4 trajectory and the f = 1 trajectory on the frames
both publish, and each one's RMS distance to the stream's true positions (no alignment: all three start from the same state)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1920, 1200


def throughput(args):
    import numpy as np
    import torch
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream, make_texture, scaled_config
    D = 16
    S = args.streams - args.streams % D
    n_frames = args.warmup + args.steps
    dev = torch.device('cuda', 0)
    base = scaled_config(ConfigEuRoC(), W, H)
    tex = make_texture(0xA1B0)
    streams = [SyntheticStream(base, seed=i, n_frames=n_frames, motion_scale=1.5 + 0.1 * i, texture=tex, tex_offset=(53.0 * i, 29.0 * i)) for i in range(D)]
    state = streams[0].torch_state(dev)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    frames = []
    for k in range(n_frames):
        pairs = [st.frame_torch(k, state, gen) for st in streams]
        frames.append((torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])))
    rep = S // D
    result = dict(streams=S, steps=args.steps, warmup=args.warmup, size=[W, H])
    for f in (1, 2, 4):
        cfg = scaled_config(ConfigEuRoC(), W, H)
        cfg.image_downscale = f
        eng = FrontendEngine(cfg, n_streams=S)
        its = [iter(st.imu) for st in streams]
        pend = [next(it, None) for it in its]
        wall, published = 0.0, []
        for k in range(n_frames):
            t = streams[0].frame_time(k)
            for d in range(D):
                while pend[d] is not None and pend[d].timestamp <= t:
                    ids = np.arange(d, S, D, dtype=np.int32)
                    eng.push_imu_batch(ids, np.full(len(ids), pend[d].timestamp), np.tile(pend[d].angular_velocity, (len(ids), 1)))
                    pend[d] = next(its[d], None)
            img0 = frames[k][0].repeat(rep, 1, 1).contiguous(); img1 = frames[k][1].repeat(rep, 1, 1).contiguous()
            if k == args.warmup:
                torch.cuda.synchronize()
                eng.enable_timing(64 * args.steps)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eng.step(img0, img1, [t] * S)
            torch.cuda.synchronize()
            if k >= args.warmup:
                wall += time.perf_counter() - t1
                published.append(eng.read_counters(1)['n_published'])
            del img0, img1
        tm = eng.read_timing()
        eng.close()
        result['f%d' % f] = dict(processed=[W // f, H // f], ms_per_step={k: v[0] / args.steps for k, v in tm.items()}, wall_ms_per_step=1e3 * wall / args.steps,
                                 frames_per_s=S * args.steps / wall, stream1_published=published)
    return result


def trajectories(args):
    import numpy as np
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream, scaled_config
    base = scaled_config(ConfigEuRoC(), W, H)
    st = SyntheticStream(base, seed=5, n_frames=args.frames, motion_scale=1.5)
    rendered = [st.frame(k) for k in range(args.frames)]
    traj, feats = {}, {}
    for f in (1, 2, 4):
        cfg = scaled_config(ConfigEuRoC(), W, H)
        cfg.image_downscale = f
        eng = FrontendEngine(cfg, n_streams=1)
        flt = BatchedMSCKF(cfg, 1, device=0, max_features=eng.max_features)
        it = iter(st.imu); pend = next(it, None)
        rows, nf = {}, []
        for k, m in enumerate(rendered):
            while pend is not None and pend.timestamp <= m.timestamp:
                eng.push_imu(0, pend.timestamp, pend.angular_velocity)
                flt.push_imu([0], [pend.timestamp], [pend.angular_velocity], [pend.linear_acceleration])
                pend = next(it, None)
            eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
            ids, uv, n = eng.read_features_raw()
            nf.append(int(n[0]))
            out = flt.step(ids, uv, n, [m.timestamp])
            if out[0, 0] > 0.5:
                rows[k] = out[0, 2:5].copy()
        eng.close(); flt.close()
        traj[f], feats[f] = rows, nf
    res = dict(frames=args.frames, published_per_frame={('f%d' % f): feats[f] for f in feats}, frames_with_pose={('f%d' % f): len(traj[f]) for f in traj})
    truth = {k: st.position(rendered[k].timestamp) for k in range(args.frames)}
    for f in (1, 2, 4):
        ks = sorted(traj[f])
        if ks:
            d = np.array([np.linalg.norm(traj[f][k] - truth[k]) for k in ks])
            res['f%d_vs_truth_rmse_m' % f] = float(np.sqrt((d ** 2).mean()))
    for f in (2, 4):
        ks = sorted(set(traj[f]) & set(traj[1]))
        if ks:
            d = np.array([np.linalg.norm(traj[f][k] - traj[1][k]) for k in ks])
            res['f%d_vs_f1' % f] = dict(frames=len(ks), rmse_m=float(np.sqrt((d ** 2).mean())), max_m=float(d.max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=64)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=60)
    args = ap.parse_args()
    print(json.dumps(dict(throughput=throughput(args), trajectories=trajectories(args))))


if __name__ == '__main__':
    main()
