"""tests/downscale_helpers.py -- TEST INFRASTRUCTURE ONLY: what the binning GPU tests share: the host-binned twin of a stream (what the
unmodified oracle is fed, with frontend.downscaled_config) and the condition of every compared run."""
import downscale_ref as dr

MIN_FEATURES = 20          # the oracle publishes at least this many features in every frame after the first, in every compared run
FLOOR = dict(min_features=MIN_FEATURES, floor_from=1)         # the same as arguments of fe_harness.against_oracle


def binned_stream(stream, f, n_frames=None, post=None):
    """The frames of `stream` (a fe_harness.Frames) binned f x f by tests/downscale_ref.py; `post` (optional) is applied to every
    binned image (the reference CLAHE)."""
    return stream.map((lambda a: dr.downscale(a, f)) if post is None else (lambda a: post(dr.downscale(a, f))), n_frames)


def check_reference(ref, n_frames):
    """The condition of every compared run, on the oracle alone."""
    assert len(ref) == n_frames
    assert all(len(r['ids']) >= MIN_FEATURES for r in ref[1:]), [len(r['ids']) for r in ref]
