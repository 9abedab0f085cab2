"""The sweep command line with --response0/1 and --vignette0/1: one short EuRoC-layout sequence written with a vignetting lens and a
gamma-like sensor (write_euroc_layout(..., vignette=...)), the calibration as a pcalib-style text file and a 16-bit PNG per camera,
swept from two offsets; every frame of both streams against an engine that was handed the same tables as arrays."""
import json

import numpy as np
import pytest

import photometric_ref as pr

pytestmark = pytest.mark.gpu

W, H = 752, 480
N_FRAMES = 8
OFFSETS = [0.0, 0.12]             # the second stream starts three frames in
SWITCHES = ('response0', 'response1', 'vignette0', 'vignette1')


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    from PIL import Image
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    root = tmp_path_factory.mktemp('photometric_sweep')
    st = SyntheticStream(ConfigEuRoC(), seed=13, n_frames=N_FRAMES, motion_scale=3.0, t0=1403636580.0, rest=1.0)
    png = [np.floor(pr.radial_vignette(W, H, c) * 65535.0 + 0.5).astype(np.uint16) for c in (0.35, 0.45)]
    v = [p.astype(np.float64) / float(p.max()) for p in png]                 # what the reader makes of the files
    u = [pr.gamma_inverse_response(2.2), pr.gamma_inverse_response(2.2)]     # one sensor type: write_euroc_layout takes one forward response
    write_euroc_layout(str(root / 'SEQ'), st, compress_level=1, vignette=(v[0], v[1], pr.gamma_forward(2.2)))
    files = {}
    for cam in (0, 1):
        Image.fromarray(png[cam]).save(str(root / ('vignette%d.png' % cam)))
        (root / ('pcalib%d.txt' % cam)).write_text(' '.join(repr(float(x)) for x in u[cam]) + '\n')
        files['response%d' % cam], files['vignette%d' % cam] = str(root / ('pcalib%d.txt' % cam)), str(root / ('vignette%d.png' % cam))
    return root, files, u, v


def _engine_on_arrays(path, offset, cfg):
    """The sequence through the same EuRoC reader into a one-stream engine of `cfg`: per frame (timestamp, ids, uv)."""
    from uav_airvision_amd.euroc import EuRoCDataset, replay
    from uav_airvision_amd.frontend import FrontendEngine
    ds = EuRoCDataset(path)
    ds.set_starttime(offset)
    eng = FrontendEngine(cfg, n_streams=1)
    out = []

    def on_stereo(m):
        eng.step_host(m.cam0_image, m.cam1_image, [m.timestamp])
        (ids, uv), = eng.read_features()
        out.append((m.timestamp, ids, uv))
    replay(ds, [lambda m: eng.push_imu(0, m.timestamp, m.angular_velocity)], on_stereo)
    eng.close()
    return out


def test_sweep_cli_with_the_calibration_files_is_the_engine_fed_arrays(sequence, tmp_path, monkeypatch, capsys):
    from uav_airvision_amd import sweep
    from uav_airvision_amd.config import ConfigEuRoC
    root, files, u, v = sequence
    got = [[] for _ in OFFSETS]

    def on_step(step, ts, ids, uv, n, out):
        for s in range(len(OFFSETS)):
            if ts[s] >= 0:
                got[s].append((ts[s], ids[s, :n[s]].copy(), uv[s, :n[s]].copy()))
    seen = []
    inner = sweep.run_batched

    def run_batched(cfg, *a, **kw):                    # the command line's own batch, with the per-step hook of the parity tests
        seen.append(tuple(getattr(cfg, 'cam%s_%s' % (k[-1], k[:-1])) for k in SWITCHES))
        return inner(cfg, *a, on_step=on_step, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    sweep.main(['--root', str(root), '--sequences', 'SEQ', '--offsets'] + [str(o) for o in OFFSETS] +
               [x for k in SWITCHES for x in ('--' + k, files[k])] + ['--out', str(tmp_path / 'txts')])
    assert seen == [tuple(files[k] for k in SWITCHES)]
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert rep['photometric'] == files and rep['stream_frames'] == 2 * N_FRAMES - 3
    cfg = ConfigEuRoC()
    cfg.cam0_response, cfg.cam1_response, cfg.cam0_vignette, cfg.cam1_vignette = u[0], u[1], v[0], v[1]
    for s, off in enumerate(OFFSETS):
        want = _engine_on_arrays(str(root / 'SEQ'), off, cfg)
        assert len(want) == len(got[s]) == N_FRAMES - 3 * s
        for k, (a, b) in enumerate(zip(want, got[s])):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), (s, k)
            assert len(a[1]) >= 50, (s, k)
    # without the switches the same sweep publishes something else
    plain = _engine_on_arrays(str(root / 'SEQ'), 0.0, ConfigEuRoC())
    assert not all(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(plain, got[0]))


def test_a_value_on_the_config_object_stays_unless_the_switch_is_given():
    from uav_airvision_amd import sweep
    from uav_airvision_amd.config import ConfigEuRoC
    cfg = ConfigEuRoC()
    cfg.cam0_vignette, cfg.cam1_response = 'kept.png', 'kept.txt'
    sweep.apply_args(cfg, sweep.make_parser().parse_args(['--sequences', 'SEQ', '--vignette1', 'new.png', '--response1', 'new.txt']))
    assert (cfg.cam0_response, cfg.cam1_response, cfg.cam0_vignette, cfg.cam1_vignette) == (None, 'new.txt', 'kept.png', 'new.png')
