"""The sweep on a Bayer sequence: one short EuRoC-layout sequence written as raw rggb mosaics (grey PNGs) goes through
`python -m uav_airvision_amd.sweep --pixel-format bayer_rggb8` and through the frame-store path of run_batched; the published
features and trajectories equal those of the 8-bit engine fed the reference-converted frames of the same mosaics, and --pixel-format
auto reads the files as plain grey."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bayer_ref as br
from fe_harness import Frames

pytestmark = pytest.mark.gpu

N_FRAMES = 30
FMT = 'bayer_rggb8'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    """One synthetic sequence written twice: as raw rggb mosaics, and as the 8-bit grey frames the NumPy reference makes of those
    mosaics (same IMU and ground-truth files)."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    root = tmp_path_factory.mktemp('bayer_sweep')
    st = SyntheticStream(ConfigEuRoC(), seed=77, n_frames=N_FRAMES, motion_scale=1.5, t0=1403636580.0, rest=1.0)
    frames = Frames.cached(st)
    st.frame = frames.frame                               # rendered once, written twice
    bayer = write_euroc_layout(str(root / 'SEQ_bayer'), st, compress_level=1, pixel_format=FMT)
    conv = frames.map(lambda im: br.to_gray8(br.mosaic(im, FMT), FMT))
    st.frame = conv.frame
    grey = write_euroc_layout(str(root / 'SEQ_conv'), st, compress_level=1, pixel_format='gray8')
    return bayer, grey, conv


def _sweep(path, fmt, share):
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.sweep import run_batched
    cfg = ConfigEuRoC()
    cfg.image_format = fmt
    got = []

    def on_step(step, ts, ids, uv, n, out):
        if ts[0] >= 0:
            got.append((ts[0], ids[0, :n[0]].copy(), uv[0, :n[0]].copy()))
    trajs, _dss = run_batched(cfg, [path], [0.0], on_step=on_step, share_frames=share)
    return got, trajs[0]


def test_the_sweep_equals_the_engine_fed_the_converted_frames(sequence):
    """The mosaics through the frame store and through the per-stream staging slots publish, on every frame, what a gray8 engine
    publishes on the reference-converted frames; the decoded arrays are the mosaics."""
    from uav_airvision_amd.euroc import EuRoCDataset, decode_batch, frame_array
    from uav_airvision_amd.sweep import batch_pixel_format
    bayer, grey, conv = sequence
    assert batch_pixel_format([bayer], 'auto') == 'gray8' and batch_pixel_format([bayer], FMT) == FMT      # auto never finds a mosaic
    files = EuRoCDataset._list_images(os.path.join(bayer, 'mav0', 'cam0', 'data'))[0]
    arr = frame_array(FMT, 2, 480, 752)
    decode_batch(files[:2], arr)
    assert np.array_equal(br.to_gray8(arr, FMT), np.stack([conv.frame(0).cam0_image, conv.frame(1).cam0_image]))
    want, want_traj = _sweep(grey, 'gray8', True)
    assert len(want) == N_FRAMES and all(len(w[1]) > 30 for w in want)
    for share in (True, False):
        got, traj = _sweep(bayer, FMT, share)
        assert len(got) == N_FRAMES, share
        for k, (w, g) in enumerate(zip(want, got)):
            assert w[0] == g[0] and np.array_equal(w[1], g[1]) and np.array_equal(w[2].view(np.uint64), g[2].view(np.uint64)), (share, k)
        assert traj.shape == want_traj.shape and np.array_equal(traj.view(np.uint64), want_traj.view(np.uint64)), share
    assert not np.array_equal(arr[0], conv.frame(0).cam0_image)       # (the files do hold a mosaic, not the grey frames)


def test_the_command_line(sequence, tmp_path):
    """python -m uav_airvision_amd.sweep --pixel-format bayer_rggb8 in a process of its own: it runs, reports the format, and writes the
    trajectory run_batched gives in this process."""
    from uav_airvision_amd import evaluate
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.sweep import run_batched
    path, _grey, _conv = sequence
    out = tmp_path / 'txts'
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'uav_airvision_amd.sweep', '--root', os.path.dirname(path), '--sequences', 'SEQ_bayer', '--offsets', '0',
                        '--pixel-format', FMT, '--out', str(out)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    rep = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    assert rep['pixel_format']['asked'] == FMT and rep['pixel_format']['last_batch'] == FMT
    cfg = ConfigEuRoC()
    cfg.image_format = FMT
    trajs, _dss = run_batched(cfg, [path], [0.0])
    tr = evaluate.load_trajectory_txt(str(out / 'output_SEQ_bayer_offset0.txt'))
    assert tr.shape == trajs[0].shape and len(tr) >= 1 and np.abs(tr[:, 1:] - trajs[0][:, 1:]).max() < 5e-9
