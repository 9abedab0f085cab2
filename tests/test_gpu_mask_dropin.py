"""config.cam0_mask / cam1_mask through the drop-in ImageProcessor: a PNG path and an array on the config object are all it takes."""
import os
import sys

import numpy as np
import pytest

import mask_ref as mr
from conftest import ROOT
from fe_harness import Frames, make_cfg as _cfg

pytestmark = pytest.mark.gpu

W, H = 752, 480


def test_drop_in_pipeline_reads_the_masks_from_its_config(tmp_path):
    from PIL import Image
    from uav_airvision_amd.synth import SyntheticStream, replay
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    m0, m1 = mr.comb_mask(W, H, 96, 24, 0), mr.comb_mask(W, H, 96, 24, 48)
    Image.fromarray(m0 * 255).save(str(tmp_path / 'cam0_mask.png'))
    st = Frames.cached(SyntheticStream(_cfg(), seed=13, n_frames=6, motion_scale=3.0))
    ref, fe = mr.run_masked_oracle(_cfg(), st, m0, m1)
    assert fe.drops['track'] + fe.drops['stereo'] >= 100, fe.drops
    proc = ip.ImageProcessor(_cfg(cam0_mask=str(tmp_path / 'cam0_mask.png'), cam1_mask=m1))
    seen, counts = [], []
    replay(st, [proc.imu_callback], lambda m: (seen.append(proc.stereo_callback(m)), counts.append(dict(proc.num_features))))
    for k, (msg, r) in enumerate(zip(seen, ref)):
        assert np.array_equal(np.array([f.id for f in msg.features], np.int64), r['ids']), k
        assert np.array_equal(np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features]).reshape(-1, 4).view(np.uint64), r['uv'].view(np.uint64)), k
        if k > 0:
            assert [counts[k][c] for c in ('after_tracking', 'after_matching')] == [r['nf'][c] for c in ('after_tracking', 'after_matching')], k
    grid = proc.prev_features                                 # the reference's grid of FeatureMetaData: all on valid pixels
    pts = [(f.cam0_point, f.cam1_point) for cell in grid for f in cell]
    assert len(pts) >= 50 and all(m0[int(p[1]), int(p[0])] == 1 and m1[int(q[1]), int(q[0])] == 1 for p, q in pts)
    proc.close()
    with pytest.raises(ValueError, match='cam1 mask'):
        ip.ImageProcessor(_cfg(cam1_mask=m1[:100]))
