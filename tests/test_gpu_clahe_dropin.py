"""config.use_clahe through the drop-in pipeline, through the sweep command line and through the filter."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import clahe_ref as cr
from clahe_helpers import STREAM
from conftest import ROOT
from fe_harness import Frames, make_cfg as _cfg, run_engine

pytestmark = pytest.mark.gpu


def test_drop_in_pipeline_honours_the_switch_and_shows_the_viewer_the_equalised_frame():
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.synth import SyntheticStream, replay
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip
    from viewer import HeadlessViewer
    cfg = _cfg(use_clahe=True)
    st = Frames.cached(SyntheticStream(cfg, **dict(STREAM, n_frames=6)))
    eq = st.map(cr.clahe)
    eng = run_engine(cfg, [st], mode='host')[0]
    proc = ip.ImageProcessor(cfg)
    assert proc.use_clahe is True
    viewer = HeadlessViewer(keep_images=True)
    proc.viewer = viewer
    seen, shown = [], []
    replay(st, [proc.imu_callback], lambda m: (seen.append(proc.stereo_callback(m)), shown.append(np.array(viewer.last_image))))
    for k, (msg, (ids, uv, _cnt)) in enumerate(zip(seen, eng)):
        assert np.array_equal(np.array([f.id for f in msg.features], np.int64), ids), k
        assert np.array_equal(np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features]).reshape(-1, 4).view(np.uint64), uv.view(np.uint64)), k
        assert np.array_equal(shown[k], eq.frame(k).cam0_image), k
    assert np.array_equal(proc.equalized_image(1), eq.frame(5).cam1_image)
    proc.close()
    off = ip.ImageProcessor(_cfg())
    assert off.use_clahe is False
    off.viewer = HeadlessViewer()
    off.stereo_callback(st.frame(0))
    assert off.viewer.n_images == 0                         # nothing is handed over without the switch
    with pytest.raises(N.AirvisionError):
        off.equalized_image(0)
    off.close()


def test_stage_classes_say_that_they_do_not_equalise():
    """FeatureInitializer and FeatureAdder are handed the config: with use_clahe set they warn that they work on the images as given;
    without it they stay silent."""
    import warnings
    d = os.path.join(ROOT, 'uav_airvision_amd', 'dropin')
    if d not in sys.path:
        sys.path.insert(0, d)
    import image_processing as ip

    class Matcher(object):
        stereo_match = None
    kw = dict(detector=None, stereo_matcher=Matcher(), cam0_curr_img_msg=None, curr_features=[], next_feature_id=0, grid_row=4, grid_col=5,
              grid_min_feature_num=3)
    with pytest.warns(RuntimeWarning, match='use_clahe'):
        ip.FeatureInitializer(config=_cfg(use_clahe=True), **kw)
    with pytest.warns(RuntimeWarning, match='use_clahe'):
        ip.FeatureAdder(config=_cfg(use_clahe=True), grid_max_feature_num=5, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ip.FeatureInitializer(config=_cfg(), **kw)
        ip.FeatureAdder(config=_cfg(), grid_max_feature_num=5, **kw)


def test_frame_torch_applies_contrast_and_offset():
    """The torch renderer maps grey values as `frame` does: same scene, a quarter of the spread, 40 grey levels darker."""
    import torch
    from uav_airvision_amd.synth import SyntheticStream
    cfg = _cfg()
    flat = SyntheticStream(cfg, seed=0, n_frames=3, contrast=0.25, brightness_offset=-40.0, pixel_noise=0.0)
    dev = torch.device('cuda', 0)
    a = flat.frame_torch(2, flat.torch_state(dev))[0].cpu().numpy().astype(np.int32)
    b = flat.frame(2).cam0_image.astype(np.int32)
    assert np.abs(a - b).max() <= 1 and b.std() < 20          # fp32 bilinear look-up on two devices: a rounding boundary may fall either way


def test_sweep_cli_with_clahe(tmp_path):
    """One short `sweep --clahe` run through the frame store: it finishes, reports the switch, and its trajectories differ from the
    run without it (the same sequences, equalised or not)."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    reps = {}
    for tag, extra in (('on', ['--clahe', '--clahe-clip', '3', '--clahe-tiles', '8', '6']), ('off', [])):
        p = subprocess.run([sys.executable, '-m', 'uav_airvision_amd.sweep', '--make-synthetic', str(tmp_path / 'syn'), '--frames', '40',
                            '--sequences', 'SYN_A', '--offsets', '0', '0.5', '--out', str(tmp_path / tag)] + extra,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        reps[tag] = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert reps['on']['clahe'] == dict(clip_limit=3.0, tiles=[8, 6]) and 'clahe' not in reps['off']
    assert reps['on']['stream_frames'] == reps['off']['stream_frames'] > 0
    a = (tmp_path / 'on' / 'output_SYN_A_offset0.txt').read_text()
    b = (tmp_path / 'off' / 'output_SYN_A_offset0.txt').read_text()
    assert a and b and a != b


def test_front_end_with_clahe_feeds_the_filter():
    """Front-end + BatchedMSCKF on the low-contrast stream, CLAHE on: the stream is never stopped and its poses stay finite.  The ATE
    against the synthetic truth, switch on and off, is printed (recorded in DESIGN.md), not asserted."""
    from uav_airvision_amd.evaluate import ate
    from uav_airvision_amd.frontend import FrontendEngine
    from uav_airvision_amd.msckf_ops import BatchedMSCKF
    from uav_airvision_amd.synth import SyntheticStream
    st = Frames.cached(SyntheticStream(_cfg(), **dict(STREAM, n_frames=60)))
    res = {}
    for on in (True, False):
        cfg = _cfg(use_clahe=on)
        eng = FrontendEngine(cfg, n_streams=1)
        flt = BatchedMSCKF(cfg, 1, max_features=eng.max_features)
        it = iter(st.imu)
        pend = next(it, None)
        traj, nfeat = [], []
        for k in range(st.n_frames):
            m = st.frame(k)
            while pend is not None and pend.timestamp <= m.timestamp:
                eng.push_imu(0, pend.timestamp, pend.angular_velocity)
                flt.push_imu([0], [pend.timestamp], [pend.angular_velocity], [pend.linear_acceleration])
                pend = next(it, None)
            eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
            ids, uv, n = eng.read_features_raw()
            nfeat.append(int(n[0]))
            out = flt.step(ids, uv, n, [m.timestamp])
            if on:
                assert out[0, 0] >= 0, 'the filter stopped the stream at frame %d' % k
                assert np.isfinite(out[0]).all(), k
            if out[0, 0] > 0.5 and np.isfinite(out[0]).all():
                traj.append(out[0, 1:5].copy())
        eng.close(); flt.close()
        res[on] = (float('nan'), len(traj), float(np.mean(nfeat)))
        if len(traj) > 20:
            traj = np.array(traj)
            gt = np.array([[t] + list(st.position(t)) for t in traj[:, 0]])
            res[on] = (ate(traj, gt)['rmse'], len(traj), float(np.mean(nfeat)))
    assert res[True][1] >= 40 and res[True][2] >= 2 * res[False][2]
    print('ATE rmse over %d frames: CLAHE on %.4f m (%d poses, %.1f features / frame), off %.4f m (%d poses, %.1f features / frame)'
          % ((st.n_frames,) + res[True] + res[False]))
