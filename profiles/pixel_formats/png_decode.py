"""Per-file decode time of the library's PNG decoder on ONE core: 752 x 480 frames of a synthetic stream written by Pillow as 8-bit
grey, 16-bit grey (g << 8 | noise8 and g << 8) and RGB (smooth per-channel offsets), decoded with threads=1.  Host code: no GPU.

    python profiles/pixel_formats/png_decode.py [--frames 12] [--repeats 5]   -> one JSON line"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    from PIL import Image
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import decode_batch, frame_array
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(ConfigEuRoC(), seed=5, n_frames=args.frames)
    rng = np.random.default_rng(1)
    grey = [st.frame(k).cam0_image for k in range(args.frames)]
    y, x = np.mgrid[0:480, 0:752]
    off = np.stack([np.rint(30 * np.sin(x / (23.0 + 9 * i)) + 20 * np.cos(y / (31.0 - 6 * i))) for i in range(3)], -1).astype(np.int64)
    sets = {
        'gray8': ('gray8', grey),
        'gray16_high_byte_only': ('gray16', [g.astype(np.uint16) << 8 for g in grey]),
        'gray16_noisy_low_byte': ('gray16', [(g.astype(np.uint16) << 8) | rng.integers(0, 256, g.shape, dtype=np.uint16) for g in grey]),
        'rgb8': ('rgb8', [np.clip(g[..., None] + off, 0, 255).astype(np.uint8) for g in grey]),
    }
    result = dict(frames=args.frames, repeats=args.repeats, threads=1)
    with tempfile.TemporaryDirectory() as d:
        for name, (fmt, imgs) in sets.items():
            paths = []
            for i, a in enumerate(imgs):
                p = os.path.join(d, '%s_%d.png' % (name, i))
                Image.fromarray(a).save(p)
                paths.append(p)
            out = frame_array(fmt, len(paths), 480, 752)
            decode_batch(paths, out, threads=1)
            assert all(np.array_equal(o, a) for o, a in zip(out, imgs))
            best = 1e9
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                decode_batch(paths, out, threads=1)
                best = min(best, time.perf_counter() - t0)
            result[name] = dict(ms_per_file=1e3 * best / len(paths), file_kb=sum(os.path.getsize(p) for p in paths) / len(paths) / 1024.0)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
