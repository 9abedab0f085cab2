"""tests/pixfmt_helpers.py -- TEST INFRASTRUCTURE ONLY: what the pixel-format GPU tests share: synthetic streams re-encoded as 16-bit
or colour frames, their reference-converted twins for the unmodified oracle, and an engine runner for every entry path."""
import numpy as np

import pixfmt_ref as pr
from clahe_helpers import make_cfg, run_oracle, same  # noqa: F401  (re-exported)

MODES = ('step', 'persist', 'prestage', 'host', 'frames')


def encode(gray, fmt, rng):
    """An 8-bit frame as a frame of `fmt` that does NOT convert back to it trivially: gray16 = g << 8 | noise8; colour = grey plus an
    independent smooth offset pattern per channel, clipped (alpha random)."""
    g = np.asarray(gray, np.uint8)
    if fmt == 'gray16':
        return (g.astype(np.uint16) << 8) | rng.integers(0, 256, g.shape, dtype=np.uint16)
    c = pr.BYTES[fmt]
    h, w = g.shape
    y, x = np.mgrid[0:h, 0:w]
    # a smooth pattern of its own per channel (own frequencies and phase, the same on every frame and camera, as a colour cast is), up to +- 50 grey levels: the channels differ by tens of
    # levels everywhere, and the scene keeps its corners (independent noise per pixel would make every pixel one, past max_corners)
    off = np.stack([np.rint(30 * np.sin(x / (23.0 + 9 * i) + 1.7 * i) + 20 * np.cos(y / (31.0 - 6 * i) + 0.9 * i)) for i in range(c)], -1).astype(np.int64)
    out = np.clip(g[..., None].astype(np.int64) + off, 0, 255).astype(np.uint8)
    if c == 4:
        out[..., 3] = rng.integers(0, 256, g.shape, dtype=np.uint8)
    return out


def encode_exact(gray, fmt):
    """The frame of `fmt` that converts back to `gray` exactly: g << 8, or equal colour channels."""
    g = np.asarray(gray, np.uint8)
    if fmt == 'gray16':
        return g.astype(np.uint16) << 8
    return np.repeat(g[..., None], pr.BYTES[fmt], -1)


class Encoded(object):
    """A synthetic stream with its first n frames rendered once, their raw twins in `fmt` and the reference conversion of those."""

    def __init__(self, base, fmt, n_frames, seed=0, shift=8, exact=False, post=None):
        self.imu, self.n_frames, self.fmt = base.imu, n_frames, fmt
        rng = np.random.default_rng(seed)
        self.raw, self._conv = [], []
        for k in range(n_frames):
            m = base.frame(k)
            r0, r1 = (encode_exact(m.cam0_image, fmt), encode_exact(m.cam1_image, fmt)) if exact else (encode(m.cam0_image, fmt, rng), encode(m.cam1_image, fmt, rng))
            a, b = pr.to_gray8(r0, fmt, shift), pr.to_gray8(r1, fmt, shift)
            if post is not None:
                a, b = post(a), post(b)
            self.raw.append((m.timestamp, r0, r1))
            self._conv.append(type(m)(m.timestamp, a, b, type(m.cam0_msg)(m.timestamp, a), type(m.cam1_msg)(m.timestamp, b)))

    def frame(self, k):
        """The reference-converted frame: what the oracle (or a gray8 engine) is fed."""
        return self._conv[k]


def run_engine(cfg, streams, mode='step', images_of=None, timing=False):
    """Feeds the RAW frames of `streams` (Encoded, all of cfg.image_format) through one entry path.  Returns per stream a list of (ids,
    uv, counters) per frame; with images_of also read_image of both cameras per frame; with timing the span counts of every step.
    The caller's arrays and tensors are compared with copies taken before the step."""
    import torch
    from uav_airvision_amd.frontend import FrontendEngine
    S, n_frames = len(streams), streams[0].n_frames
    eng = FrontendEngine(cfg, n_streams=S, inputs_persist=mode in ('persist', 'prestage'))
    if mode == 'frames':
        eng.frames_reserve(2 * S + 1)
    if timing:
        eng.enable_timing(64)
    out, images, spans = [[] for _ in streams], [], []
    its = [iter(s.imu) for s in streams]
    pend = [next(it, None) for it in its]

    def arrays(k):
        return np.stack([s.raw[k][1] for s in streams]), np.stack([s.raw[k][2] for s in streams]), [s.raw[k][0] for s in streams]
    dev = {}
    for k in range(n_frames):
        a0, a1, ts = arrays(k)
        for i in range(S):
            while pend[i] is not None and pend[i].timestamp <= ts[i]:
                eng.push_imu(i, pend[i].timestamp, pend[i].angular_velocity)
                pend[i] = next(its[i], None)
        if mode in ('step', 'persist', 'prestage'):
            if k not in dev:
                dev[k] = (torch.from_numpy(a0).cuda(), torch.from_numpy(a1).cuda())
            eng.step(dev[k][0], dev[k][1], ts)
        elif mode == 'host':
            h0, h1 = a0.copy(), a1.copy()
            eng.step_host(h0, h1, ts)
            assert np.array_equal(h0, a0) and np.array_equal(h1, a1)
        else:
            # entries out of order and away from the upload's own positions, so that the indexed conversion has to follow the list
            slots = (np.arange(S, dtype=np.int32)[::-1] + 1 + (k & 1) * S).astype(np.int32)
            h0, h1 = a0.copy(), a1.copy()
            eng.frames_upload(slots, h0, h1)
            assert np.array_equal(h0, a0) and np.array_equal(h1, a1)
            eng.step_frames(slots, ts)
        feats = eng.read_features()
        for i in range(S):
            out[i].append((feats[i][0], feats[i][1], eng.read_counters(i)))
        if images_of is not None:
            images.append((eng.read_image(images_of, 0), eng.read_image(images_of, 1)))
        if timing:
            spans.append({c: v[1] for c, v in eng.read_timing().items()})
        if k in dev:                                  # the caller's tensors are what they were
            assert np.array_equal(dev[k][0].cpu().numpy(), a0) and np.array_equal(dev[k][1].cpu().numpy(), a1), (mode, k)
            if mode == 'prestage' and k + 1 < n_frames:
                b0, b1, _ts = arrays(k + 1)
                dev[k + 1] = (torch.from_numpy(b0).cuda(), torch.from_numpy(b1).cuda())
                eng.prestage(*dev[k + 1])
            dev.pop(k - 1, None)
    eng.close()
    res = [out]
    if images_of is not None:
        res.append(images)
    if timing:
        res.append(spans)
    return res[0] if len(res) == 1 else tuple(res)
