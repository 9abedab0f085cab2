"""tests/pixfmt_helpers.py -- TEST INFRASTRUCTURE ONLY: what the pixel-format GPU tests share: synthetic streams re-encoded as 16-bit
or colour frames with their reference-converted twins for the unmodified oracle (streams, runners and comparisons are those of
tests/fe_harness.py)."""
import numpy as np

import pixfmt_ref as pr
from fe_harness import Frames


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


def encoded_stream(base, fmt, n_frames, seed=0, shift=8, exact=False, post=None):
    """The first n frames of `base` as raw frames of `fmt` (`.raw`; exact: the ones that convert back trivially) and the reference
    conversion of those (`.frame`: what the oracle, or a gray8 engine, is fed)."""
    rng = np.random.default_rng(seed)
    return Frames.raw_twin(base, (lambda g: encode_exact(g, fmt)) if exact else (lambda g: encode(g, fmt, rng)),
                           lambda r: pr.to_gray8(r, fmt, shift), n_frames, post)
