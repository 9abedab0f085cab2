"""Cost of config.use_clahe in the front-end: a front-end-only loop at 2,048 streams (default grid), HIP-event spans per kernel class
(FrontendEngine.enable_timing), switch off against switch on, same frames; then ops.clahe alone on the same 2 x 2,048 images.

    python profiles/clahe/frontend_on_off.py [--streams 2048] [--steps 10] [--warmup 3] [--only on|off] [--kernel-stats FILE]   -> one JSON line

16 distinct synthetic streams (rendered on the GPU) are replayed by streams/16 replicas each: the kernels' work per stream is what a
distinct stream would give, only the rendering is shared.  For the two kernels' own time per launch run the `--only on` form under
`rocprofv3 --kernel-trace --stats -- python ...` and hand the kernel_stats.csv it wrote to `--kernel-stats`: the JSON line then
carries per-launch times and the achieved fraction of HBM bandwidth (algorithmic bytes per image: one read for the histogram, one read
and one write for the apply pass; peak taken as 8 TB/s)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def kernel_stats(path, n_img, hw):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '')
            for key, nbytes in (('clahe_lut_kernel', hw), ('clahe_apply_kernel', 2 * hw), ('pyr_l0l1_kernel', None)):
                if key in name:
                    ns = float(row['AverageNs'])
                    out[key] = dict(calls=int(row['Calls']), ms_per_launch=ns * 1e-6)
                    if nbytes:
                        out[key]['bytes_per_launch'] = n_img * nbytes
                        out[key]['fraction_of_hbm_peak'] = n_img * nbytes / (ns * 1e-9) / HBM_PEAK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=2048)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=('on', 'off'), default=None)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    D = 16
    S = args.streams - args.streams % D
    if args.kernel_stats is not None:
        print(json.dumps(dict(streams=S, kernels=kernel_stats(args.kernel_stats, 2 * S, 752 * 480))))
        return
    import numpy as np
    import torch
    from uav_airvision_amd import ops
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    n_frames = args.warmup + args.steps
    dev = torch.device('cuda', 0)
    base = ConfigEuRoC()
    tex = make_texture(0xA1B0)
    streams = [SyntheticStream(base, seed=i, n_frames=n_frames, motion_scale=1.5 + 0.1 * i, texture=tex, tex_offset=(53.0 * i, 29.0 * i)) for i in range(D)]
    state = streams[0].torch_state(dev)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    frames = []
    for k in range(n_frames):
        pairs = [st.frame_torch(k, state, gen) for st in streams]
        frames.append((torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])))
    rep = S // D
    result = dict(streams=S, steps=args.steps, warmup=args.warmup)
    for tag in ('off', 'on'):
        if args.only and args.only != tag:
            continue
        cfg = ConfigEuRoC()
        cfg.use_clahe = tag == 'on'
        eng = FrontendEngine(cfg, n_streams=S)
        its = [iter(st.imu) for st in streams]
        pend = [next(it, None) for it in its]
        wall = 0.0
        published = []
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
                published.append(eng.read_counters(1)['n_published'])
        tm = eng.read_timing()
        eng.close()
        result[tag] = dict(ms_per_step={k: v[0] / args.steps for k, v in tm.items()}, spans_per_step={k: v[1] / args.steps for k, v in tm.items()},
                           wall_ms_per_step=1e3 * wall / args.steps, stream1_published=published)
    if 'on' in result and 'off' in result:
        result['pyramid_on_minus_off_ms'] = result['on']['ms_per_step']['pyramid'] - result['off']['ms_per_step']['pyramid']
        result['wall_on_over_off'] = result['on']['wall_ms_per_step'] / result['off']['wall_ms_per_step']
    if not args.only:
        # the operator alone on one step's images (both kernels, event-timed over ten launches)
        img = torch.cat([frames[0][0].repeat(rep, 1, 1), frames[0][1].repeat(rep, 1, 1)]).contiguous()
        out = torch.empty_like(img)
        ops.clahe(img, out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.clahe(img, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        result['ops_clahe'] = dict(images=int(img.shape[0]), ms=ms, fraction_of_hbm_peak_3_passes=3 * img.numel() / (ms * 1e-3) / HBM_PEAK)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
