"""Cost of the packed 10 / 12-bit transports (config.image_format = 'gray12p', 'bayer_rggb12p', ..).

    python profiles/packed/packed_formats.py --kernels [--images 4096]                         -> one JSON line
    python profiles/packed/packed_formats.py --host-fed [--streams 128] [--steps 10] [--warmup 3] [--rounds 2]   -> one JSON line

--kernels: ops.to_gray8 on 4,096 images of 752 x 480, HIP-event-timed over ten launches after one: each of the four grey packings on
the aligned body and (the same bytes one byte into a larger buffer) on the group-wise path, to_gray8_kernel<GRAY16> on unpacked frames of
the same size, and next to each a device-to-device hipMemcpyAsync that reads and writes the same total (it copies half the kernel's
input + output bytes), all in one process.  Random bytes are valid packed frames, so nothing is packed here.  Then the two passes of a
packed mosaic -- the unpack kernel of its packing, and bayer_to_gray8_kernel<uint8> on the 8-bit mosaic -- each timed alone, beside the
one pass of bayer_rggb16.
--host-fed: FrontendEngine.step_host at 128 streams with gray8, gray16, gray12p and gray10p frames of the same scenes (16 distinct
synthetic streams, each eight times): wall ms per step (host clock around step_host and a device synchronise) over 10 steps after 3,
every format `rounds` times in rotating order."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 752, 480


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
    out = torch.empty((n_img, H, W), dtype=torch.uint8, device=dev)
    result = dict(images=n_img, size=[W, H], launches_timed=10)

    def entry(img, fmt, unaligned=True):
        total = img.numel() * img.element_size() + out.numel()
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        ms_k = timed(lambda: ops.to_gray8(img, fmt, shift=4, out=out))
        ms_c = timed(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel(), 3, N.current_stream()))
        e = dict(bytes_in_plus_out=total, bytes_per_pixel_moved=total / out.numel(), ms=ms_k, TB_per_s=total / (ms_k * 1e-3) / 1e12, memcpy_ms=ms_c,
                 memcpy_TB_per_s=total / (ms_c * 1e-3) / 1e12, kernel_over_memcpy_rate=ms_c / ms_k)
        if unaligned:                                       # the group-wise / byte-wise path: the same frames one element into a larger buffer
            flat = torch.empty(img.numel() + 1, dtype=img.dtype, device=dev)
            un = flat[1:].view(img.shape)
            un.copy_(img)
            ms_u = timed(lambda: ops.to_gray8(un, fmt, shift=4, out=out))
            e.update(unaligned_ms=ms_u, unaligned_TB_per_s=total / (ms_u * 1e-3) / 1e12, unaligned_over_memcpy_rate=ms_c / ms_u)
        return e
    g16 = torch.randint(0, 65536, (n_img, H, W), dtype=torch.int32, device=dev, generator=gen).to(torch.uint16)
    result['gray16'] = entry(g16, 'gray16')
    result['bayer_rggb16'] = entry(g16, 'bayer_rggb16', unaligned=False)
    del g16
    for fmt in ('gray10p', 'gray12p', 'gray10_csi2', 'gray12_csi2'):
        raw = torch.randint(0, 256, (n_img, H, N.frame_bytes(N.PACKED_FORMATS[fmt], W, 1)), dtype=torch.uint8, device=dev, generator=gen)
        result[fmt] = entry(raw, fmt)
        result[fmt]['ms_over_gray16_ms'] = result[fmt]['ms'] / result['gray16']['ms']
        del raw
    m8 = torch.randint(0, 256, (n_img, H, W), dtype=torch.uint8, device=dev, generator=gen)
    result['bayer_rggb8_second_pass'] = entry(m8, 'bayer_rggb8', unaligned=False)
    for k in ('10p', '12p', '10_csi2', '12_csi2'):
        two = result['gray' + k]['ms'] + result['bayer_rggb8_second_pass']['ms']
        result['bayer_rggb%s_two_passes' % k] = dict(ms=two, unpack_ms=result['gray' + k]['ms'], demosaic_ms=result['bayer_rggb8_second_pass']['ms'],
                                                      ms_over_bayer_rggb16_ms=two / result['bayer_rggb16']['ms'])
    return result


def host_fed(args):
    import numpy as np
    import torch
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine, pack_frames
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    D = 16
    S = args.streams - args.streams % D
    rep = S // D
    n_frames = args.warmup + args.steps
    dev = torch.device('cuda', 0)
    base = ConfigEuRoC()
    tex = make_texture(0xA1B0)
    streams = [SyntheticStream(base, seed=i, n_frames=n_frames, motion_scale=1.5 + 0.1 * i, texture=tex, tex_offset=(53.0 * i, 29.0 * i)) for i in range(D)]
    state = streams[0].torch_state(dev)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    grey = []
    for k in range(n_frames):
        pairs = [st.frame_torch(k, state, gen) for st in streams]
        grey.append((torch.stack([p[0] for p in pairs]).cpu().numpy(), torch.stack([p[1] for p in pairs]).cpu().numpy()))
    encoders = dict(gray8=lambda g: g, gray16=lambda g: g.astype(np.uint16) << 8,
                    gray12p=lambda g: pack_frames(g.astype(np.uint16) << 4, 'gray12p'), gray10p=lambda g: pack_frames(g.astype(np.uint16) << 2, 'gray10p'))
    formats = list(encoders)
    result = dict(streams=S, steps=args.steps, warmup=args.warmup, rounds=args.rounds, size=[W, H], order=[])
    for fmt in formats:
        result[fmt] = dict(wall_ms_per_step=[], stream1_published=None, frame_bytes=None)
    for r in range(args.rounds):
        order = formats[r % len(formats):] + formats[:r % len(formats)]
        result['order'].append(order)
        for fmt in order:
            enc = [(encoders[fmt](a), encoders[fmt](b)) for a, b in grey]
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
                a0 = np.tile(enc[k][0], (rep, 1, 1)); a1 = np.tile(enc[k][1], (rep, 1, 1))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.step_host(a0, a1, [t] * S)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    wall += time.perf_counter() - t1
                    published.append(eng.read_counters(1)['n_published'])
            result[fmt]['wall_ms_per_step'].append(1e3 * wall / args.steps)
            result[fmt]['frame_bytes'] = eng._frame_bytes
            if result[fmt]['stream1_published'] is None:
                result[fmt]['stream1_published'] = published
            else:
                assert result[fmt]['stream1_published'] == published
            eng.close()
            del enc
    for fmt in formats:
        ms = result[fmt]['wall_ms_per_step']
        result[fmt]['frames_per_s'] = [S / (m * 1e-3) for m in ms]
        result[fmt]['h2d_MB_per_step'] = 2 * S * result[fmt]['frame_bytes'] / 1e6
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--host-fed', action='store_true')
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--streams', type=int, default=128)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    if args.kernels:
        print(json.dumps(kernels(args.images)))
    elif args.host_fed:
        print(json.dumps(host_fed(args)))
    else:
        ap.error('one of --kernels, --host-fed')


if __name__ == '__main__':
    main()
