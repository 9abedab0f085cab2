"""tests/bayer_helpers.py -- TEST INFRASTRUCTURE ONLY: what the Bayer GPU tests share: synthetic streams mosaicked with per-channel gains
and their reference-converted twins for the unmodified oracle (tests/bayer_ref.py; streams, runners and comparisons are those of
tests/fe_harness.py)."""
import bayer_ref as br
from fe_harness import Frames


def mosaicked_stream(base, fmt, n_frames, shift=8, gains=br.GAINS, post=None):
    """The first n frames of `base` as raw mosaics in `fmt` (`.raw`: gains 0.8, 1.0, 0.6; 16-bit samples << shift) and the reference
    conversion of those (`.frame`: what the oracle, or a gray8 engine, is fed)."""
    return Frames.raw_twin(base, lambda g: br.mosaic(g, fmt, gains, shift), lambda r: br.to_gray8(r, fmt, shift), n_frames, post)
