"""Cost and effect of the photometric calibration stage (config.cam*_response / cam*_vignette; csrc/photometric.hip).

    python profiles/photometric/photometric_cost.py --kernels                                  -> one JSON line
    python profiles/photometric/photometric_cost.py --frontend [--streams 64] [--steps 20] [--warmup 5]      -> one JSON line
    python profiles/photometric/photometric_cost.py --benefit [--frames 60]                    -> one JSON line

--kernels: ops.photometric out of place on 2048 images of 752 x 480 and on 64 of 1920 x 1200, for the three table combinations,
HIP-event-timed over ten launches after one, next to a device-to-device hipMemcpyAsync of the same bytes in + out (it copies the
images once).  With a response table av_photometric reads the 512-byte table back and waits for the stream before it launches, so a
call costs a fixed amount on top of its kernel: the same call on ONE 64 x 4 image is timed the same way and subtracted (`fixed_ms`;
the gain-only combination has no such read-back and is reported both ways as a check of the subtraction).
--frontend: 64 streams of 752 x 480 (16 distinct synthetic scenes, repeated), `step` on resident frames, with the stage off and on
(both tables, both cameras), every case twice, alternating: wall ms per step and the HIP-event time per kernel class.
--benefit: one synthetic stream as rendered, as a vignetting lens (cos^4-style, 0.35 at the corners) and a gamma 2.2 sensor would have
recorded it, and that corrected by the engine: features published per frame, mean lifetime of the published grid's features,
after_tracking / before_tracking, and the batched filter's position difference to the run on the rendered frames."""
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


def tables(w, h):
    import numpy as np
    import torch
    import photometric_ref as pr                          # the tests' own vignette and response
    resp = pr.quantise_response(pr.gamma_inverse_response(2.2))
    gain = pr.quantise_vignette(pr.radial_vignette(w, h, 0.35))
    return torch.from_numpy(resp.view(np.int16)).cuda(), torch.from_numpy(gain.view(np.int16)).cuda()


def kernels():
    import torch
    from uav_airvision_amd import _native as N, ops
    dev = torch.device('cuda', 0)
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    result = dict(launches_timed=10, cases=[])
    tiny = torch.zeros((1, 4, 64), dtype=torch.uint8, device=dev)
    tiny_out = torch.empty_like(tiny)
    for w, h, n in ((752, 480, 2048), (1920, 1200, 64)):
        img = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)
        out = torch.empty_like(img)
        resp, gain = tables(w, h)
        tiny_gain = gain.view(-1)[:256].view(4, 64).contiguous()
        ms_c = timed(lambda: hip.hipMemcpyAsync(out.data_ptr(), img.data_ptr(), img.numel(), 3, N.current_stream()))
        total = 2 * img.numel()
        for name, r, g, tg in (('both', resp, gain, tiny_gain), ('response', resp, None, None), ('gain', None, gain, tiny_gain)):
            ms_call = timed(lambda: ops.photometric(img, r, g, out=out))
            fixed = timed(lambda: ops.photometric(tiny, r, tg, out=tiny_out))
            ms_k = ms_call - fixed if r is not None else ms_call
            result['cases'].append(dict(size=[w, h], images=n, tables=name, bytes_in_plus_out=total, gain_map_bytes=0 if g is None else 2 * w * h,
                                        call_ms=ms_call, fixed_ms=fixed, kernel_ms=ms_k, call_minus_fixed_ms=ms_call - fixed,
                                        TB_per_s=total / (ms_k * 1e-3) / 1e12, memcpy_ms=ms_c, memcpy_TB_per_s=total / (ms_c * 1e-3) / 1e12, kernel_over_memcpy_rate=ms_c / ms_k))
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
        frames.append((torch.stack([p[0] for p in pairs]).repeat(S // D, 1, 1).contiguous(), torch.stack([p[1] for p in pairs]).repeat(S // D, 1, 1).contiguous()))
    u, v = pr.gamma_inverse_response(2.2), pr.radial_vignette(W, H, 0.35)
    result = dict(streams=S, steps=args.steps, warmup=args.warmup, size=[W, H])
    for rnd in range(2):                                   # every case twice, alternating: the spread is part of the record
        for name in ('off', 'on'):
            cfg = ConfigEuRoC()
            if name == 'on':
                cfg.cam0_response = cfg.cam1_response = u
                cfg.cam0_vignette = cfg.cam1_vignette = v
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
                if k == args.warmup:
                    torch.cuda.synchronize()
                    eng.enable_timing(64 * args.steps)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.step(frames[k][0], frames[k][1], [t] * S)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    wall += time.perf_counter() - t1
                    published.append(eng.read_counters(1)['n_published'])
            tm = eng.read_timing()
            eng.close()
            result.setdefault(name, []).append(dict(wall_ms_per_step=1e3 * wall / args.steps, frames_per_s=S * args.steps / wall,
                                                    ms_per_step={k: v2[0] / args.steps for k, v2 in tm.items()}, stream1_published_mean=float(np.mean(published))))
    return result


def benefit(args):
    import numpy as np
    import photometric_ref as pr
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine, apply_vignette
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    n = args.frames
    st = SyntheticStream(ConfigEuRoC(), seed=3, n_frames=n, motion_scale=2.0)
    u, v, fwd = pr.gamma_inverse_response(2.2), pr.radial_vignette(W, H, 0.35), pr.gamma_forward(2.2)
    rendered = [st.frame(k) for k in range(n)]
    degraded = [(apply_vignette(m.cam0_image, v, fwd), apply_vignette(m.cam1_image, v, fwd)) for m in rendered]

    def run(images, corrected):
        cfg = ConfigEuRoC()
        if corrected:
            cfg.cam0_response = cfg.cam1_response = u
            cfg.cam0_vignette = cfg.cam1_vignette = v
        eng = FrontendEngine(cfg, n_streams=1)
        flt = BatchedMSCKF(cfg, 1, device=0, max_features=eng.max_features)
        it = iter(st.imu)
        pend = next(it, None)
        rows, pos = [], []
        for k, m in enumerate(rendered):
            while pend is not None and pend.timestamp <= m.timestamp:
                eng.push_imu(0, pend.timestamp, pend.angular_velocity)
                flt.push_imu([0], [pend.timestamp], [pend.angular_velocity], [pend.linear_acceleration])
                pend = next(it, None)
            eng.step_host(images[k][0], images[k][1], [m.timestamp])
            ids_a, uv_a, n_a = eng.read_features_raw()
            c = eng.read_counters(0)
            life = eng.read_grid(0)['lifetime']
            rows.append((c['n_published'], c['before_tracking'], c['after_tracking'], c['n_fast'], float(life.mean()) if len(life) else 0.0))
            out = flt.step(ids_a, uv_a, n_a, [m.timestamp])
            pos.append(out[0, 2:5].copy() if out[0, 0] > 0.5 else None)
        eng.close(); flt.close()
        r = np.array(rows, np.float64)
        return dict(published_mean=float(r[1:, 0].mean()), published_min=int(r[1:, 0].min()), n_fast_mean=float(r[1:, 3].mean()),
                    tracked_ratio=float(r[1:, 2].sum() / max(1.0, r[1:, 1].sum())), mean_lifetime=float(r[1:, 4].mean()), last_frame_mean_lifetime=float(r[-1, 4])), pos
    result = dict(frames=n, size=[W, H], corner_v=float(v[0, 0]), gamma=2.2)
    ref, ref_pos = run([(m.cam0_image, m.cam1_image) for m in rendered], False)
    result['rendered'] = ref
    for name, corrected in (('degraded', False), ('degraded_corrected', True)):
        d, pos = run(degraded, corrected)
        diffs = [float(np.linalg.norm(a - b)) for a, b in zip(pos, ref_pos) if a is not None and b is not None]
        d.update(filter_frames_compared=len(diffs), position_diff_to_rendered_m_mean=float(np.mean(diffs)) if diffs else None,
                 position_diff_to_rendered_m_max=float(np.max(diffs)) if diffs else None, position_diff_to_rendered_m_last=diffs[-1] if diffs else None)
        result[name] = d
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--frontend', action='store_true')
    ap.add_argument('--benefit', action='store_true')
    ap.add_argument('--streams', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=60)
    args = ap.parse_args()
    if args.kernels:
        print(json.dumps(kernels()))
    elif args.frontend:
        print(json.dumps(frontend(args)))
    elif args.benefit:
        print(json.dumps(benefit(args)))
    else:
        ap.error('one of --kernels, --frontend, --benefit')


if __name__ == '__main__':
    main()
