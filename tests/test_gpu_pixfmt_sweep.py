"""The sweep on 16-bit and RGB sequences: one short EuRoC-layout sequence written as 8-bit, as 16-bit (g << 8) and as RGB with equal
channels gives, swept from two offsets with --pixel-format auto, identical published features on every frame and identical
trajectories; a batch that mixes two formats is refused."""
import os

import numpy as np
import pytest

from fe_harness import Frames

pytestmark = pytest.mark.gpu

N_FRAMES = 40                     # 2 s at 20 Hz: the first second initialises the filter, the second publishes poses
OFFSETS = [0.0, 0.27]             # the second stream starts six frames in


@pytest.fixture(scope='module')
def sequences(tmp_path_factory):
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    root = tmp_path_factory.mktemp('pixfmt_sweep')
    st = SyntheticStream(ConfigEuRoC(), seed=77, n_frames=N_FRAMES, motion_scale=1.5, t0=1403636580.0, rest=1.0)
    st.frame = Frames.cached(st).frame                    # rendered once, written three times
    return {fmt: write_euroc_layout(str(root / ('SEQ_' + fmt)), st, compress_level=1, pixel_format=fmt) for fmt in ('gray8', 'gray16', 'rgb8')}


def _sweep(path):
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.sweep import batch_pixel_format, run_batched
    paths = [path] * len(OFFSETS)
    cfg = ConfigEuRoC()
    cfg.image_format = batch_pixel_format(paths, 'auto')
    got = [[] for _ in OFFSETS]

    def on_step(step, ts, ids, uv, n, out):
        for s in range(len(OFFSETS)):
            if ts[s] >= 0:
                got[s].append((ts[s], ids[s, :n[s]].copy(), uv[s, :n[s]].copy()))
    trajs, _dss = run_batched(cfg, paths, OFFSETS, on_step=on_step)
    return cfg.image_format, got, trajs


def test_three_flavours_of_one_sequence_sweep_identically(sequences, tmp_path):
    runs = {fmt: _sweep(path) for fmt, path in sequences.items()}
    assert [runs[f][0] for f in ('gray8', 'gray16', 'rgb8')] == ['gray8', 'gray16', 'rgb8']            # what auto found
    _f, want, want_traj = runs['gray8']
    assert [len(w) for w in want] == [N_FRAMES, N_FRAMES - 6] and all(len(f[1]) > 30 for w in want for f in w)
    assert all(len(t) >= 10 for t in want_traj)
    for fmt in ('gray16', 'rgb8'):
        _f, got, traj = runs[fmt]
        for s in range(len(OFFSETS)):
            assert len(got[s]) == len(want[s])
            for k, (a, b) in enumerate(zip(want[s], got[s])):
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), (fmt, s, k)
            assert traj[s].shape == want_traj[s].shape and np.array_equal(traj[s].view(np.uint64), want_traj[s].view(np.uint64)), (fmt, s)
    # the command line: --pixel-format auto on the 16-bit directory writes the trajectories of the 8-bit run
    from uav_airvision_amd import evaluate
    from uav_airvision_amd.sweep import main
    out = tmp_path / 'txts'
    root = os.path.dirname(sequences['gray16'])
    main(['--root', root, '--sequences', 'SEQ_gray16', '--offsets'] + [str(o) for o in OFFSETS] + ['--pixel-format', 'auto', '--out', str(out)])
    # (a file name carries the whole seconds of its offset, 0 for both streams: the later stream's trajectory is what stays)
    tr = evaluate.load_trajectory_txt(str(out / 'output_SEQ_gray16_offset0.txt'))
    assert tr.shape == want_traj[-1].shape and np.abs(tr[:, 1:] - want_traj[-1][:, 1:]).max() < 5e-9


def test_a_batch_mixing_two_formats_is_refused(sequences, tmp_path):
    from uav_airvision_amd.sweep import batch_pixel_format, main
    root = os.path.dirname(sequences['gray8'])
    with pytest.raises(ValueError, match='share one pixel format.*SEQ_gray8: gray8.*SEQ_rgb8: rgb8'):
        main(['--root', root, '--sequences', 'SEQ_gray8', 'SEQ_rgb8', '--pixel-format', 'auto', '--out', str(tmp_path / 'txts')])
    assert batch_pixel_format([sequences['gray8'], sequences['rgb8']], 'gray8') == 'gray8'      # a named format is taken as given
    # a named format that is not the files' is refused by the decoder, by file name
    with pytest.raises(ValueError, match='not a 752 x 480 gray16 PNG'):
        main(['--root', root, '--sequences', 'SEQ_rgb8', '--pixel-format', 'gray16', '--max-frames', '2', '--out', str(tmp_path / 'txts')])
