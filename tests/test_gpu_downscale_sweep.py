"""The sweep with --downscale 2: one short EuRoC-layout sequence of 752 x 480 frames; the published features of every frame equal the
CPU oracle's on the host-binned frames with the scaled calibration; the report says so."""
import json
import os

import numpy as np
import pytest

import downscale_ref as dr
from downscale_helpers import check_reference
from fe_harness import make_cfg, with_images

pytestmark = pytest.mark.gpu

N_FRAMES = 8


def _oracle_on_binned_files(cfg, path, f):
    """The CPU oracle on the sequence read through the same EuRoC reader and replay, every frame binned on the host."""
    from oracle.frontend import OracleFrontend
    from uav_airvision_amd.euroc import EuRoCDataset, replay
    from uav_airvision_amd.frontend import downscaled_config
    ds = EuRoCDataset(path)
    ds.set_starttime(0.0)
    fe = OracleFrontend(downscaled_config(cfg))
    out = []

    def on_stereo(m):
        assert m.cam0_image.shape == (480, 752)
        msg = fe.stereo_callback(with_images(m, dr.downscale(m.cam0_image, f), dr.downscale(m.cam1_image, f)))
        out.append(dict(ts=m.timestamp, ids=np.array([x.id for x in msg.features], np.int64),
                        uv=np.array([[x.u0, x.v0, x.u1, x.v1] for x in msg.features], np.float64).reshape(-1, 4)))
    replay(ds, [fe.imu_callback], on_stereo)
    return out


def test_the_sweep_bins_full_size_files(tmp_path, capsys):
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.sweep import apply_args, main, make_parser, run_batched
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(make_cfg(), seed=77, n_frames=N_FRAMES, motion_scale=1.5, t0=1403636580.0)
    path = write_euroc_layout(str(tmp_path / 'SEQ'), st, compress_level=1)
    args = make_parser().parse_args(['--root', str(tmp_path), '--sequences', 'SEQ', '--downscale', '2'])
    cfg = apply_args(make_cfg(), args)
    assert cfg.image_downscale == 2
    ref = _oracle_on_binned_files(cfg, path, 2)
    check_reference(ref, N_FRAMES)
    got = []

    def on_step(step, ts, ids, uv, n, out):
        got.append((ts[0], ids[0, :n[0]].copy(), uv[0, :n[0]].copy()))
    for share in (True, False):                              # the frame store and the per-stream staging
        del got[:]
        run_batched(cfg, [path], [0.0], on_step=on_step, share_frames=share)
        assert len(got) == N_FRAMES
        for k, (g, r) in enumerate(zip(got, ref)):
            assert g[0] == r['ts'], (share, k)
            assert np.array_equal(g[1], r['ids']) and np.array_equal(g[2].view(np.uint64), r['uv'].view(np.uint64)), (share, k)
    # the command line itself: the report carries the factor (and does not without the switch)
    capsys.readouterr()
    main(['--root', str(tmp_path), '--sequences', 'SEQ', '--downscale', '2', '--out', str(tmp_path / 'txts')])
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep['downscale'] == 2 and rep['stream_frames'] == N_FRAMES
    assert os.path.exists(str(tmp_path / 'txts' / 'output_SEQ_offset0.txt'))
    main(['--root', str(tmp_path), '--sequences', 'SEQ', '--max-frames', '2', '--out', str(tmp_path / 'txts1')])
    assert 'downscale' not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
