"""tests/range16_helpers.py -- TEST INFRASTRUCTURE ONLY: what the range-scaling GPU tests share: a stream of 16-bit "thermal" frames whose
reference conversion pools the two images of every stereo pair (Frames.raw_twin converts them independently, so it does not serve)."""
import numpy as np

import range16_ref as rr
from fe_harness import Frames, with_images


def squeeze(g, offset, band=300):
    """An 8-bit grey image squeezed into `band` counts above `offset`: what a thermal core makes of a scene."""
    return (offset + (g.astype(np.uint32) * band) // 255).astype(np.uint16)


def range_stream(base, n_frames, offset=7800, drift=37, band=300, post=None, **range_kw):
    """The first n frames of `base` as 16-bit frames (`.raw`): frame k squeezed into `band` counts above offset + k * drift, cam1 a
    further 23 counts up -- and their reference conversion (`.frame`), every pair POOLED into one range (`.ranges[k]` = (lo, hi));
    range_kw: scale / window / clip / min_span of range16_ref.to_gray8; post (optional) is applied to every converted image."""
    raw, conv, ranges = [], [], []
    for k in range(n_frames):
        m = base.frame(k)
        r0, r1 = squeeze(m.cam0_image, offset + k * drift, band), squeeze(m.cam1_image, offset + k * drift + 23, band)
        a, b, r = rr.pair_to_gray8(r0, r1, **range_kw)
        if post is not None:
            a, b = post(a), post(b)
        raw.append((m.timestamp, r0, r1))
        conv.append(with_images(m, a, b))
        ranges.append(r)
    st = Frames(base, conv, raw)
    st.ranges = ranges
    return st
