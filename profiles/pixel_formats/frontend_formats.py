"""Cost of config.image_format in the front-end: a front-end-only loop at 2,048 streams (default grid) with gray8, gray16, bgr8 and
rgba8 frames of the same scenes (g << 8, equal channels: every format publishes the same features), then the conversion kernel alone
on one step's 2 x 2,048 images next to a device-to-device hipMemcpyAsync in the same process.

    python profiles/pixel_formats/frontend_formats.py [--streams 2048] [--steps 10] [--warmup 3] [--only FORMAT] [--kernel-stats FILE]   -> one JSON line

For the kernel's own time per launch run the `--only FORMAT` form under `rocprofv3 --kernel-trace --stats -- python ...` and hand the
kernel_stats.csv it wrote to `--kernel-stats`.  Bytes of a launch = input + output; the copy used as the yardstick moves half that
many bytes, i.e. it also reads and writes that total."""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
FORMATS = ('gray8', 'gray16', 'bgr8', 'rgba8')
BYTES = dict(gray8=1, gray16=2, bgr8=3, rgba8=4)


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if 'PixOp' in row.get('Name', ''):                  # stream_pass_kernel<PixOp<format>>
                out[row['Name']] = dict(calls=int(row['Calls']), ms_per_launch=float(row['AverageNs']) * 1e-6)
    return out


def encode(g, fmt):
    import torch
    if fmt == 'gray8':
        return g
    if fmt == 'gray16':
        return (g.to(torch.int32) << 8).to(torch.uint16)
    return g.unsqueeze(-1).expand(*g.shape, BYTES[fmt]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=2048)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=FORMATS, default=None)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats is not None:
        print(json.dumps(dict(kernels=kernel_stats(args.kernel_stats))))
        return
    D = 16
    S = args.streams - args.streams % D
    import numpy as np
    import torch
    from uav_airvision_amd import _native as N, ops
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
    for fmt in FORMATS:
        if args.only and args.only != fmt:
            continue
        cfg = ConfigEuRoC()
        cfg.image_format = fmt
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
            img0 = encode(frames[k][0].repeat(rep, 1, 1).contiguous(), fmt); img1 = encode(frames[k][1].repeat(rep, 1, 1).contiguous(), fmt)
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
        result[fmt] = dict(ms_per_step={k: v[0] / args.steps for k, v in tm.items()}, spans_per_step={k: v[1] / args.steps for k, v in tm.items()},
                           wall_ms_per_step=1e3 * wall / args.steps, frames_per_s=S * args.steps / wall, stream1_published=published)
    if not args.only:
        # the kernel alone on one step's images (2 S of them), event-timed over ten launches, next to hipMemcpyAsync device to device
        hip = ctypes.CDLL('libamdhip64.so')
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        g = torch.cat([frames[0][0].repeat(rep, 1, 1), frames[0][1].repeat(rep, 1, 1)]).contiguous()
        out = torch.empty_like(g)
        result['kernel_alone'] = {}
        for fmt in FORMATS[1:]:
            img = encode(g, fmt)
            total = img.numel() * img.element_size() + out.numel()
            src = torch.empty(total // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)

            def timed(fn):
                fn(); torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / 10
            ms_k = timed(lambda: ops.to_gray8(img, fmt, out=out))
            ms_c = timed(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, N.current_stream()))
            # the byte-wise path: the same images one pixel into a larger buffer
            flat = torch.empty(img.numel() + img[0, 0, 0].numel(), dtype=img.dtype, device=dev)
            un = flat[img[0, 0, 0].numel():].view(img.shape)
            un.copy_(img)
            ms_u = timed(lambda: ops.to_gray8(un, fmt, out=out))
            result['kernel_alone'][fmt] = dict(images=int(img.shape[0]), bytes_in_plus_out=total, ms=ms_k, TB_per_s=total / (ms_k * 1e-3) / 1e12,
                                               memcpy_ms=ms_c, memcpy_TB_per_s=total / (ms_c * 1e-3) / 1e12, kernel_over_memcpy_rate=ms_c / ms_k,
                                               unaligned_ms=ms_u, unaligned_TB_per_s=total / (ms_u * 1e-3) / 1e12)
            del img, src, dst, flat, un
    print(json.dumps(result))


if __name__ == '__main__':
    main()
