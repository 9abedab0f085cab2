"""The engine's input chain [convert] -> [bin] -> [equalise] (grey_chain of csrc/frontend.hip) with every stage on at once, in every
entry path, against the unmodified CPU oracle front-end fed clahe_ref(downscale_ref(bayer_ref(mosaic))); and the list of the launch
that first writes the frame store when that launch is the binning."""
import numpy as np
import pytest

import clahe_ref as cr
import downscale_ref as dr
from bayer_helpers import mosaicked_stream
from downscale_helpers import FLOOR, binned_stream, check_reference
from fe_harness import MODES, Frames, against_oracle, make_cfg as _cfg, run_engine, run_oracle, same as _same

pytestmark = pytest.mark.gpu

NF = 3                       # 752 x 480 -> 376 x 240
FMT = 'bayer_rggb16'


def _all_on():
    return _cfg(image_format=FMT, image_downscale=2, use_clahe=True)


@pytest.fixture(scope='module')
def bases():
    from uav_airvision_amd.synth import SyntheticStream
    return [Frames.cached(SyntheticStream(_cfg(), seed=17 + i, n_frames=NF, motion_scale=2.0 - 0.5 * i)) for i in range(2)]


@pytest.fixture(scope='module')
def chain(bases):
    """Two streams as 16-bit mosaics, their reference grey frames (converted, binned by two, equalised: what read_image has to give)
    and the oracle on those, computed once and never changed."""
    from uav_airvision_amd.frontend import downscaled_config
    streams = [mosaicked_stream(b, FMT, NF, post=lambda a: cr.clahe(dr.downscale(a, 2), 2.0, (8, 8))) for b in bases]
    assert streams[0].frame(0).cam0_image.shape == (240, 376)
    refs = [run_oracle(downscaled_config(_cfg(image_downscale=2)), s) for s in streams]
    for r in refs:
        check_reference(r, NF)
    return streams, refs


@pytest.fixture(scope='module')
def runs(chain):
    """Every entry path once: per mode the features of both streams and the images of stream 1."""
    streams, _refs = chain
    return {mode: run_engine(_all_on(), streams, mode=mode, raw=True, images_of=1) for mode in MODES}


@pytest.mark.parametrize('mode', MODES)
def test_all_three_stages_in_every_entry_path(chain, runs, mode):
    """Conversion into the full-size scratch, binning into level 0, equalisation in place there: read_image of both cameras is the
    reference chain byte for byte, ids, points and counts are the oracle's on those grey frames, for both streams of the batch."""
    streams, refs = chain
    got, images = runs[mode]
    against_oracle(refs[1], got[1], 'all stages %s stream 1' % mode, images, streams[1], **FLOOR)
    against_oracle(refs[0], got[0], 'all stages %s stream 0' % mode, **FLOOR)


def test_all_three_stages_agree_across_the_entry_paths(runs):
    first, first_images = runs[MODES[0]]
    for mode in MODES[1:]:
        got, images = runs[mode]
        for s in range(2):
            assert all(_same(a, b) for a, b in zip(first[s], got[s])), (mode, s)
        assert all(np.array_equal(a[c], b[c]) for a, b in zip(first_images, images) for c in (0, 1)), mode


def test_an_entry_named_twice_takes_the_later_frame_with_binning_alone(bases):
    """8-bit grey frames and image_downscale = 2: the binning is then the launch that first writes the store, and it follows the same
    write list as the conversion does (tests/test_gpu_pixfmt_engine.py): of an entry named twice the later frame wins, as with plain
    grey frames, and the entry named once between the two is its own frame."""
    from uav_airvision_amd.frontend import FrontendEngine
    binned = [binned_stream(b, 2, n_frames=2) for b in bases]
    eng = FrontendEngine(_cfg(image_downscale=2), n_streams=2)
    eng.frames_reserve(4)
    a, b, x = bases[0].frame(0), bases[0].frame(1), bases[1].frame(0)
    eng.frames_upload(np.array([2, 1, 2], np.int32), np.stack([b.cam0_image, x.cam0_image, a.cam0_image]), np.stack([b.cam1_image, x.cam1_image, a.cam1_image]))
    eng.step_frames([2, 1], [a.timestamp, x.timestamp])
    eng.read_features()
    for s, want in ((0, binned[0].frame(0)), (1, binned[1].frame(0))):
        assert np.array_equal(eng.read_image(s, 0), want.cam0_image) and np.array_equal(eng.read_image(s, 1), want.cam1_image), s
    assert not np.array_equal(binned[0].frame(0).cam0_image, binned[0].frame(1).cam0_image)
    eng.close()
