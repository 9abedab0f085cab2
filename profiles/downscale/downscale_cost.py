"""Cost of the binning kernels (csrc/downscale.hip).

    python profiles/downscale/downscale_cost.py [--images 64]      -> one JSON line

ops.downscale on `images` frames of 1920 x 1200 and of 4096 x 4096, both factors, HIP-event-timed over ten launches: on the vector path
(aligned tensors) and on the generic path (the same frames one byte into a larger buffer), and next to each a device-to-device
copy (torch's Tensor.copy_ of a contiguous tensor) of the same input bytes in the same run.  rate_over_copy = (input + output bytes) / time of the kernel over
(2 x input bytes) / time of the copy: the kernel's share of the rate at which the copy moves bytes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    args = ap.parse_args()
    import torch
    from uav_airvision_amd import ops
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    result = dict(images=args.images)
    for W, H in ((1920, 1200), (4096, 4096)):
        n = args.images
        img = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=dev, generator=gen)
        dst = torch.empty_like(img)
        flat = torch.empty(img.numel() + 1, dtype=torch.uint8, device=dev)
        un = flat[1:].view(img.shape)
        un.copy_(img)
        ms_c = timed(lambda: dst.copy_(img))      # a contiguous device-to-device copy through torch's own HIP runtime
        entry = dict(input_bytes=img.numel(), memcpy_ms=ms_c, memcpy_TB_per_s=2 * img.numel() / (ms_c * 1e-3) / 1e12)
        for f in (2, 4):
            out = torch.empty((n, H // f, W // f), dtype=torch.uint8, device=dev)
            total = img.numel() + out.numel()
            ms_v = timed(lambda: ops.downscale(img, f, out=out))
            ms_g = timed(lambda: ops.downscale(un, f, out=out))
            copy_rate = 2 * img.numel() / ms_c
            entry['f%d' % f] = dict(bytes_in_plus_out=total, vector_ms=ms_v, vector_TB_per_s=total / (ms_v * 1e-3) / 1e12, vector_rate_over_copy=(total / ms_v) / copy_rate,
                                    vector_time_over_copy=ms_v / ms_c, generic_ms=ms_g, generic_TB_per_s=total / (ms_g * 1e-3) / 1e12,
                                    generic_rate_over_copy=(total / ms_g) / copy_rate, generic_time_over_copy=ms_g / ms_c)
            del out
        result['%dx%d' % (W, H)] = entry
        del img, dst, flat, un
    print(json.dumps(result))


if __name__ == '__main__':
    main()
