"""Cost and effect of the exposure-time normalisation (config.exposure_reference; the HAS_EXPOSURE instances of csrc/photometric.hip).

    python profiles/exposure/exposure_cost.py --kernels                                            -> one JSON line
    python profiles/exposure/exposure_cost.py --frontend [--streams 64] [--steps 20] [--warmup 5]  -> one JSON line
    python profiles/exposure/exposure_cost.py --table                                              -> one JSON line

--kernels: av_photometric (PhOp<true, true, false>: instruction for instruction the parent commit's PhOp<true, true>,
device_code_compare.txt) and av_photometric_exposure (PhOp<true, true, true>, a factor of its own for every image) out of place on the
same 128 images of 752 x 480 and of 1920 x 1200, HIP-event-timed over ten launches after one, five rounds alternating, next to a
device-to-device hipMemcpyAsync of the same bytes in + out.  Both calls read the 512-byte response table back and wait for the stream
before they launch; the same call on ONE 64 x 4 image is timed the same way and subtracted (`fixed_ms`), as profiles/photometric does.
--frontend: 64 streams of 752 x 480 (16 distinct synthetic scenes, repeated), `step` on resident frames, with the stage off (`off`), on
without exposure (`on`), on with every exposure at the reference (`on_exposure_reference`: k = 4096, the images downstream are those of
`on`, so the difference is the stage's own) and on with every stream and frame recorded at an exposure of its own, 0.6 .. 1.5 of the
reference, and normalised back (`on_exposure_varying`: the tracker then works on requantised images), every case three times,
alternating: wall ms per step and the HIP-event time per kernel class.
--table: the two synthetic streams and exposure ratios of tests/exposure_ref.py, 4 frames, as an auto-exposing rig records them --
alone, and behind gamma + vignette -- through the engine with the normalisation off and on: after_matching and published per frame."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
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


def kernels():
    import numpy as np
    import torch
    import photometric_ref as pr
    from uav_airvision_amd import _native as N
    dev = torch.device('cuda', 0)
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L = N.lib()
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    result = dict(launches_timed=10, rounds=5, cases=[])
    tiny = torch.zeros((1, 4, 64), dtype=torch.uint8, device=dev)
    tiny_out = torch.empty_like(tiny)
    for w, h, n in ((752, 480, 128), (1920, 1200, 128)):
        img = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)
        out = torch.empty_like(img)
        resp = torch.from_numpy(pr.quantise_response(pr.gamma_inverse_response(2.2)).view(np.int16)).cuda()
        gain = torch.from_numpy(pr.quantise_vignette(pr.radial_vignette(w, h, 0.35)).view(np.int16)).cuda()
        k = torch.from_numpy(np.random.default_rng(2).integers(2048, 9000, n).astype(np.uint16).view(np.int16)).cuda()
        tiny_gain = gain.view(-1)[:256].view(4, 64).contiguous()
        st = N.current_stream()

        def plain(i=img, o=out, nn=n, ww=w, hh=h, g=gain):
            N.check(L.av_photometric(p(i), p(o), nn, ww, hh, ww * hh, ww * hh, p(resp), p(g), st))

        def expo(i=img, o=out, nn=n, ww=w, hh=h, g=gain):
            N.check(L.av_photometric_exposure(p(i), p(o), nn, ww, hh, ww * hh, ww * hh, p(resp), p(g), p(k), st))
        total = 2 * img.numel()
        rows = dict(memcpy_ms=[], plain_ms=[], exposure_ms=[], plain_fixed_ms=[], exposure_fixed_ms=[])
        for _ in range(5):
            rows['memcpy_ms'].append(timed(lambda: hip.hipMemcpyAsync(out.data_ptr(), img.data_ptr(), img.numel(), 3, st)))
            rows['plain_ms'].append(timed(plain))
            rows['exposure_ms'].append(timed(expo))
            rows['plain_fixed_ms'].append(timed(lambda: plain(tiny, tiny_out, 1, 64, 4, tiny_gain)))
            rows['exposure_fixed_ms'].append(timed(lambda: expo(tiny, tiny_out, 1, 64, 4, tiny_gain)))
        kp = [a - b for a, b in zip(rows['plain_ms'], rows['plain_fixed_ms'])]
        ke = [a - b for a, b in zip(rows['exposure_ms'], rows['exposure_fixed_ms'])]
        med = lambda v: float(np.median(v))      # noqa: E731
        result['cases'].append(dict(size=[w, h], images=n, bytes_in_plus_out=total, gain_map_bytes=2 * w * h, rounds=rows,
                                    plain_kernel_ms=dict(min=min(kp), median=med(kp), max=max(kp)), exposure_kernel_ms=dict(min=min(ke), median=med(ke), max=max(ke)),
                                    memcpy_ms=dict(min=min(rows['memcpy_ms']), median=med(rows['memcpy_ms']), max=max(rows['memcpy_ms'])),
                                    plain_over_memcpy_rate=med(rows['memcpy_ms']) / med(kp), exposure_over_memcpy_rate=med(rows['memcpy_ms']) / med(ke),
                                    plain_TB_per_s=total / (med(kp) * 1e-3) / 1e12, exposure_TB_per_s=total / (med(ke) * 1e-3) / 1e12))
        del img, out
    return result


def frontend(args):
    import numpy as np
    import torch
    import photometric_ref as pr
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
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
        frames.append((torch.stack([q[0] for q in pairs]).repeat(S // D, 1, 1).contiguous(), torch.stack([q[1] for q in pairs]).repeat(S // D, 1, 1).contiguous()))
    u, v = pr.gamma_inverse_response(2.2), pr.radial_vignette(W, H, 0.35)
    rng = np.random.default_rng(4)
    ratio = rng.uniform(0.6, 1.5, (n_frames, 2, S))                 # t / t_ref of every frame, camera and stream
    recorded = [tuple(torch.clamp(torch.floor(frames[k][c].float() * torch.from_numpy(ratio[k, c]).float().to(dev)[:, None, None] + 0.5), 0, 255).to(torch.uint8)
                      for c in (0, 1)) for k in range(n_frames)]
    result = dict(streams=S, steps=args.steps, warmup=args.warmup, size=[W, H])
    for rnd in range(3):                                   # every case three times, alternating: the spread is part of the record
        for name in ('off', 'on', 'on_exposure_reference', 'on_exposure_varying'):
            cfg = ConfigEuRoC()
            if name != 'off':
                cfg.cam0_response = cfg.cam1_response = u
                cfg.cam0_vignette = cfg.cam1_vignette = v
            if name.startswith('on_exposure'):
                cfg.exposure_reference = 8.0
            eng = FrontendEngine(cfg, n_streams=S)
            its = [iter(st.imu) for st in streams]
            pend = [next(it, None) for it in its]
            wall = 0.0
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
                kw, fr = {}, frames[k]
                if name == 'on_exposure_reference':
                    kw = dict(exposure=(np.full(S, 8.0), np.full(S, 8.0)))
                elif name == 'on_exposure_varying':
                    kw, fr = dict(exposure=(8.0 * ratio[k, 0], 8.0 * ratio[k, 1])), recorded[k]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.step(fr[0], fr[1], [t] * S, **kw)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    wall += time.perf_counter() - t1
            tm = eng.read_timing()
            eng.close()
            result.setdefault(name, []).append(dict(wall_ms_per_step=1e3 * wall / args.steps, frames_per_s=S * args.steps / wall,
                                                    ms_per_step={c: v2[0] / args.steps for c, v2 in tm.items()}, spans_per_step={c: v2[1] / args.steps for c, v2 in tm.items()}))
    return result


def table():
    import exposure_ref as er
    import photometric_ref as pr
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.synth import SyntheticStream
    NF, T_REF = 4, 8.0
    v = (pr.radial_vignette(W, H, 0.35), pr.radial_vignette(W, H, 0.45))
    u = (pr.gamma_inverse_response(2.2), pr.gamma_inverse_response(1.8))
    fwd = (pr.gamma_forward(2.2), pr.gamma_forward(1.8))

    def run(st, frames, tables, exposure):
        cfg = ConfigEuRoC()
        if tables:
            cfg.cam0_response, cfg.cam1_response, cfg.cam0_vignette, cfg.cam1_vignette = u[0], u[1], v[0], v[1]
        if exposure:
            cfg.exposure_reference = T_REF
        eng = FrontendEngine(cfg, n_streams=1)
        it = iter(st.imu)
        pend = next(it, None)
        match, pub = [], []
        for k in range(NF):
            ts = st.frame(k).timestamp
            while pend is not None and pend.timestamp <= ts:
                eng.push_imu(0, pend.timestamp, pend.angular_velocity)
                pend = next(it, None)
            kw = dict(exposure=([er.RATIOS[0][k] * T_REF], [er.RATIOS[1][k] * T_REF])) if exposure else {}
            eng.step_host(frames[k][0], frames[k][1], [ts], **kw)
            eng.read_features()
            c = eng.read_counters(0)
            match.append(c['after_matching']); pub.append(c['n_published'])
        eng.close()
        return dict(after_matching=match, published=pub)
    result = dict(frames=NF, size=[W, H], ratios=dict(cam0=list(er.RATIOS[0]), cam1=list(er.RATIOS[1])), streams={})
    for seed, motion in er.SEEDS:
        st = SyntheticStream(ConfigEuRoC(), seed=seed, n_frames=NF, motion_scale=motion)
        clean = [(st.frame(k).cam0_image, st.frame(k).cam1_image) for k in range(NF)]
        only = [tuple(er.degrade(clean[k][c], er.RATIOS[c][k]) for c in (0, 1)) for k in range(NF)]
        behind = [tuple(er.degrade(clean[k][c], er.RATIOS[c][k], v[c], fwd[c]) for c in (0, 1)) for k in range(NF)]
        flat = [tuple(er.degrade(clean[k][c], 1.0, v[c], fwd[c]) for c in (0, 1)) for k in range(NF)]
        result['streams']['seed %d' % seed] = dict(
            clean=run(st, clean, False, False),
            gamma_vignette_at_the_reference_exposure_photometric_on=run(st, flat, True, False),
            exposure_behind_gamma_vignette_photometric_on_exposure_off=run(st, behind, True, False),
            exposure_behind_gamma_vignette_photometric_on_exposure_on=run(st, behind, True, True),
            exposure_only_off=run(st, only, False, False),
            exposure_only_on=run(st, only, False, True))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--frontend', action='store_true')
    ap.add_argument('--table', action='store_true')
    ap.add_argument('--streams', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if args.kernels:
        print(json.dumps(kernels()))
    elif args.frontend:
        print(json.dumps(frontend(args)))
    elif args.table:
        print(json.dumps(table()))
    else:
        ap.error('one of --kernels, --frontend, --table')


if __name__ == '__main__':
    main()
