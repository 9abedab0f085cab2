"""tests/bayer_helpers.py -- TEST INFRASTRUCTURE ONLY: what the Bayer GPU tests share: synthetic streams mosaicked with per-channel gains,
their reference-converted twins for the unmodified oracle (tests/bayer_ref.py), and the runners of the other pixel formats' tests."""
import bayer_ref as br
from pixfmt_helpers import MODES, make_cfg, run_engine, run_oracle, same  # noqa: F401  (re-exported)


class Mosaicked(object):
    """A synthetic stream with its first n frames rendered once, their raw mosaics in `fmt` (gains 0.8, 1.0, 0.6; 16-bit samples
    << shift) and the reference conversion of those: `.raw`, `.frame`, `.imu`, `.n_frames` as run_engine / run_oracle read them."""

    def __init__(self, base, fmt, n_frames, shift=8, gains=br.GAINS, post=None):
        self.imu, self.n_frames, self.fmt = base.imu, n_frames, fmt
        self.raw, self._conv = [], []
        for k in range(n_frames):
            m = base.frame(k)
            r0, r1 = br.mosaic(m.cam0_image, fmt, gains, shift), br.mosaic(m.cam1_image, fmt, gains, shift)
            a, b = br.to_gray8(r0, fmt, shift), br.to_gray8(r1, fmt, shift)
            if post is not None:
                a, b = post(a), post(b)
            self.raw.append((m.timestamp, r0, r1))
            self._conv.append(type(m)(m.timestamp, a, b, type(m.cam0_msg)(m.timestamp, a), type(m.cam1_msg)(m.timestamp, b)))

    def frame(self, k):
        """The reference-converted frame: what the oracle (or a gray8 engine) is fed."""
        return self._conv[k]
