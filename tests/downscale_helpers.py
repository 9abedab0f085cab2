"""tests/downscale_helpers.py -- TEST INFRASTRUCTURE ONLY: what the binning GPU tests share: the host-binned twin of a stream (what the
unmodified oracle is fed, with frontend.downscaled_config) and the comparison of an engine run with the oracle's."""
import numpy as np

import downscale_ref as dr

MIN_FEATURES = 20          # the oracle publishes at least this many features in every frame after the first, in every compared run


class Binned(object):
    """The frames of `stream` (anything with .imu, .n_frames, .frame(k)) binned f x f by tests/downscale_ref.py, once; `post` (optional)
    is applied to every binned image (the reference CLAHE)."""

    def __init__(self, stream, f, n_frames=None, post=None):
        self.imu, self.n_frames = stream.imu, stream.n_frames if n_frames is None else n_frames
        self._frames = []
        for k in range(self.n_frames):
            m = stream.frame(k)
            a, b = dr.downscale(m.cam0_image, f), dr.downscale(m.cam1_image, f)
            if post is not None:
                a, b = post(a), post(b)
            self._frames.append(type(m)(m.timestamp, a, b, type(m.cam0_msg)(m.timestamp, a), type(m.cam1_msg)(m.timestamp, b)))

    def frame(self, k):
        return self._frames[k]


def check_reference(ref, n_frames):
    """The condition of every compared run, on the oracle alone."""
    assert len(ref) == n_frames
    assert all(len(r['ids']) >= MIN_FEATURES for r in ref[1:]), [len(r['ids']) for r in ref]


def against_oracle(ref, got, tag, images=None, binned=None):
    """ids and uv bit-identical on every frame, the tracker's counters equal, no overflow; read_image = the binned frames."""
    check_reference(ref, len(got))
    for k, (r, g) in enumerate(zip(ref, got)):
        ids, uv, cnt = g[0], g[1], g[2]
        where = '%s frame %d' % (tag, k)
        if k > 0:
            assert [cnt['before_tracking'], cnt['after_tracking'], cnt['after_matching']] == \
                   [r['nf'].get('before_tracking', 0), r['nf'].get('after_tracking', 0), r['nf'].get('after_matching', 0)], where
        assert cnt['overflow'] == 0 and cnt['n_published'] == len(r['ids']) and np.array_equal(ids, r['ids']), where
        assert np.array_equal(uv.view(np.uint64), r['uv'].view(np.uint64)), where
        if images is not None:
            m = binned.frame(k)
            assert images[k][0].shape == m.cam0_image.shape, where
            assert np.array_equal(images[k][0], m.cam0_image) and np.array_equal(images[k][1], m.cam1_image), where
