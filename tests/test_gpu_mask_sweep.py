"""The sweep command line with --mask0 / --mask1: one short EuRoC-layout sequence swept from two offsets, every frame of both streams
pinned to the CPU oracle front-end with the masks of tests/mask_ref.py read through the same EuRoC reader."""
import json

import numpy as np
import pytest

import mask_ref as mr

pytestmark = pytest.mark.gpu

W, H = 752, 480
N_FRAMES = 12
OFFSETS = [0.0, 0.27]             # the second stream starts six frames in


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    from PIL import Image
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    root = tmp_path_factory.mktemp('mask_sweep')
    st = SyntheticStream(ConfigEuRoC(), seed=13, n_frames=N_FRAMES, motion_scale=3.0, t0=1403636580.0, rest=1.0)
    write_euroc_layout(str(root / 'SEQ'), st, compress_level=1)
    m0, m1 = mr.comb_mask(W, H, 96, 24, 0), mr.comb_mask(W, H, 96, 24, 48)
    Image.fromarray(m0 * 255).save(str(root / 'mask0.png'))
    Image.fromarray(m1 * 255).save(str(root / 'mask1.png'))
    return root, m0, m1


def _oracle(path, offset, m0, m1):
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import EuRoCDataset, replay
    ds = EuRoCDataset(path)
    ds.set_starttime(offset)
    fe = mr.MaskedOracle(ConfigEuRoC(), m0, m1)
    out = []

    def on_stereo(m):
        msg = fe.stereo_callback(m)
        out.append((m.timestamp, np.array([f.id for f in msg.features], np.int64),
                    np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features], np.float64).reshape(-1, 4)))
    replay(ds, [fe.imu_callback], on_stereo)
    return out, fe.drops


def test_sweep_cli_with_masks_is_pinned_to_the_masked_oracle(sequence, tmp_path, monkeypatch, capsys):
    from uav_airvision_amd import sweep
    root, m0, m1 = sequence
    got = [[] for _ in OFFSETS]

    def on_step(step, ts, ids, uv, n, out):
        for s in range(len(OFFSETS)):
            if ts[s] >= 0:
                got[s].append((ts[s], ids[s, :n[s]].copy(), uv[s, :n[s]].copy()))
    seen = []
    inner = sweep.run_batched

    def run_batched(cfg, *a, **kw):                    # the command line's own batch, with the per-step hook of the parity tests
        seen.append((cfg.cam0_mask, cfg.cam1_mask))
        return inner(cfg, *a, on_step=on_step, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    sweep.main(['--root', str(root), '--sequences', 'SEQ', '--offsets'] + [str(o) for o in OFFSETS] +
               ['--mask0', str(root / 'mask0.png'), '--mask1', str(root / 'mask1.png'), '--out', str(tmp_path / 'txts')])
    assert seen == [(str(root / 'mask0.png'), str(root / 'mask1.png'))]
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert rep['masks'] == dict(mask0=str(root / 'mask0.png'), mask1=str(root / 'mask1.png')) and rep['stream_frames'] == 2 * N_FRAMES - 6
    dropped = 0
    for s, off in enumerate(OFFSETS):
        want, drops = _oracle(str(root / 'SEQ'), off, m0, m1)
        dropped += drops['stereo']
        assert len(want) == len(got[s]) == N_FRAMES - 6 * s
        for k, (a, b) in enumerate(zip(want, got[s])):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), (s, k)
            assert len(a[1]) >= 50, (s, k)
    assert dropped >= 100
    # without the switches the same sweep publishes something else
    plain, _d = _oracle(str(root / 'SEQ'), 0.0, None, None)
    assert not all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(plain, got[0]))
