"""Cost of the Bayer formats (config.image_format = 'bayer_*').

    python profiles/bayer/bayer_formats.py --kernels [--images 4096]          -> one JSON line
    python profiles/bayer/bayer_formats.py --engine [--streams 2048] [--steps 10] [--warmup 3] [--only FORMAT]   -> one JSON line
    python profiles/bayer/bayer_formats.py --kernel-stats kernel_stats.csv    -> one JSON line

--kernels: ops.to_gray8 on 4,096 images of 752 x 480, HIP-event-timed over ten launches: the Bayer kernel on 8- and 16-bit samples on
the vector path and (the same images one sample into a larger buffer) on the generic path, to_gray8_kernel<GRAY16> on 16-bit grey
frames, and next to each a device-to-device hipMemcpyAsync that reads and writes the same total (it copies half the kernel's input +
output bytes).  Run the same command under `rocprofv3 --kernel-trace --stats --output-format csv -- python ...` and hand the
kernel_stats.csv to --kernel-stats for the kernels' own time per launch.
--engine: a front-end-only loop at 2,048 streams with gray8 frames and with the rggb mosaics of the same scenes (gains 0.8, 1.0,
0.6), HIP-event spans per kernel class."""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GAINS = (0.8, 1.0, 0.6)


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if 'to_gray8' in row.get('Name', ''):
                out[row['Name']] = dict(calls=int(row['Calls']), ms_per_launch=float(row['AverageNs']) * 1e-6)
    return out


def mosaic(g, wide=False, shift=4):
    """uint8 cuda [n, h, w] -> the rggb mosaic of a scene with R, G, B = g x GAINS (uint8, or uint16 << shift)."""
    import torch
    gain = torch.tensor([[GAINS[0], GAINS[1]], [GAINS[1], GAINS[2]]], device=g.device).repeat(g.shape[-2] // 2, g.shape[-1] // 2)
    m = torch.clamp(torch.round(g.to(torch.float32) * gain), 0, 255)
    return (m.to(torch.int32) << shift).to(torch.uint16) if wide else m.to(torch.uint8)


def timed(fn):
    import torch
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 10


def kernels(n_img):
    import torch
    from uav_airvision_amd import _native as N, ops
    dev = torch.device('cuda', 0)
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    g = torch.randint(0, 256, (n_img, 480, 752), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.empty_like(g)
    result = dict(images=n_img, size=[752, 480])
    for name, fmt, wide in (('bayer_rggb8', 'bayer_rggb8', False), ('bayer_rggb16', 'bayer_rggb16', True), ('gray16', 'gray16', True)):
        img = mosaic(g, wide) if fmt != 'gray16' else (g.to(torch.int32) << 4).to(torch.uint16)
        total = img.numel() * img.element_size() + out.numel()
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        ms_k = timed(lambda: ops.to_gray8(img, fmt, shift=4, out=out))
        ms_c = timed(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, N.current_stream()))
        flat = torch.empty(img.numel() + 1, dtype=img.dtype, device=dev)      # the generic / byte-wise path: the same images one sample into a larger buffer
        un = flat[1:].view(img.shape)
        un.copy_(img)
        ms_u = timed(lambda: ops.to_gray8(un, fmt, shift=4, out=out))
        result[name] = dict(bytes_in_plus_out=total, ms=ms_k, TB_per_s=total / (ms_k * 1e-3) / 1e12, memcpy_ms=ms_c, memcpy_TB_per_s=total / (ms_c * 1e-3) / 1e12,
                            kernel_over_memcpy_rate=ms_c / ms_k, unaligned_ms=ms_u, unaligned_TB_per_s=total / (ms_u * 1e-3) / 1e12, unaligned_over_memcpy_rate=ms_c / ms_u)
        del img, src, dst, flat, un
    return result


def engine(args):
    import numpy as np
    import torch
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    D = 16
    S = args.streams - args.streams % D
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
    for fmt in ('gray8', 'bayer_rggb8', 'bayer_rggb16'):
        if args.only and args.only != fmt:
            continue
        cfg = ConfigEuRoC()
        cfg.image_format, cfg.gray16_shift = fmt, 4
        enc = (lambda g: g) if fmt == 'gray8' else (lambda g: mosaic(g, fmt.endswith('16')))
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
            img0 = enc(frames[k][0].repeat(rep, 1, 1).contiguous()); img1 = enc(frames[k][1].repeat(rep, 1, 1).contiguous())
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
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--engine', action='store_true')
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--streams', type=int, default=2048)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats is not None:
        print(json.dumps(dict(kernels=kernel_stats(args.kernel_stats))))
    elif args.kernels:
        print(json.dumps(kernels(args.images)))
    elif args.engine:
        print(json.dumps(engine(args)))
    else:
        ap.error('one of --kernels, --engine, --kernel-stats')


if __name__ == '__main__':
    main()
