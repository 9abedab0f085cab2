"""The sweep command line with --exposure-reference: one short EuRoC-layout sequence written by an auto-exposing rig
(write_euroc_layout(..., exposure=...), which also writes both times.txt), swept from two offsets through the shared frame store and
with --no-share-frames; every frame of both streams against the unmodified CPU oracle on the frames the NumPy definition of
tests/exposure_ref.py corrected."""
import json
import os

import numpy as np
import pytest

import exposure_ref as er
from fe_harness import Frames, make_cfg, run_oracle, with_images

pytestmark = pytest.mark.gpu

N_FRAMES = 6
OFFSETS = [0.0, 0.12]             # the second stream starts three frames in
T_REF = 8.0
T0 = [8.0, 4.4, 12.8, 6.4, 8.0, 5.2]          # ms, cam0 by frame
T1 = [8.0, 4.8, 12.0, 5.6, 9.6, 6.0]          # cam1


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    from uav_airvision_amd.euroc import EuRoCDataset, write_euroc_layout
    from uav_airvision_amd.synth import SyntheticStream
    root = tmp_path_factory.mktemp('exposure_sweep')
    st = SyntheticStream(make_cfg(), seed=13, n_frames=N_FRAMES, motion_scale=3.0, t0=1403636580.0, rest=1.0)
    write_euroc_layout(str(root / 'SEQ'), st, compress_level=1, exposure=(T0, T1, T_REF))
    lines = [(root / 'SEQ' / 'mav0' / ('cam%d' % c) / 'times.txt').read_text().split('\n') for c in (0, 1)]
    assert [len(l) for l in lines] == [N_FRAMES + 1] * 2 and [float(l.split()[2]) for l in lines[1][:N_FRAMES]] == T1
    # the oracle on the frames as the reader returns them, corrected by the definition, from either offset
    refs = []
    for off in OFFSETS:
        ds = EuRoCDataset(str(root / 'SEQ'))
        ds.set_starttime(off)
        first = N_FRAMES - len(list(ds.stereo_files))
        frames = [with_images(m, er.correct(m.cam0_image, None, None, int(er.quantise(T0[first + k], T_REF))),
                              er.correct(m.cam1_image, None, None, int(er.quantise(T1[first + k], T_REF)))) for k, m in enumerate(ds.stereo)]

        class Base(object):
            imu = list(ds.imu)
        refs.append(run_oracle(make_cfg(), Frames(Base, frames)))
    assert [len(r) for r in refs] == [N_FRAMES, N_FRAMES - 3] and all(len(f['ids']) >= 20 for r in refs for f in r)
    return root, refs


@pytest.mark.parametrize('share', [True, False])
def test_sweep_cli_pins_every_frame_to_the_oracle_on_corrected_frames(sequence, share, tmp_path, monkeypatch, capsys):
    from uav_airvision_amd import sweep
    root, refs = sequence
    got = [[] for _ in OFFSETS]

    def on_step(step, ts, ids, uv, n, out):
        for s in range(len(OFFSETS)):
            if ts[s] >= 0:
                got[s].append((ids[s, :n[s]].copy(), uv[s, :n[s]].copy()))
    seen = []
    inner = sweep.run_batched

    def run_batched(cfg, *a, **kw):                    # the command line's own batch, with the per-step hook of the parity tests
        seen.append((cfg.exposure_reference, kw.get('share_frames')))
        return inner(cfg, *a, on_step=on_step, **kw)
    monkeypatch.setattr(sweep, 'run_batched', run_batched)
    sweep.main(['--root', str(root), '--sequences', 'SEQ', '--offsets'] + [str(o) for o in OFFSETS] + ['--exposure-reference', str(T_REF)] +
               ([] if share else ['--no-share-frames']) + ['--out', str(tmp_path / 'txts')])
    assert seen == [(T_REF, share)]
    rep = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert rep['exposure_reference'] == T_REF and rep['stream_frames'] == 2 * N_FRAMES - 3
    for s, ref in enumerate(refs):
        assert len(got[s]) == len(ref)
        for k, (r, (ids, uv)) in enumerate(zip(ref, got[s])):
            assert np.array_equal(ids, r['ids']) and np.array_equal(uv.view(np.uint64), r['uv'].view(np.uint64)), (share, s, k)


def test_a_missing_times_file_or_line_is_an_error_that_names_the_file(sequence, tmp_path):
    import shutil
    from uav_airvision_amd import sweep
    root, _refs = sequence
    for cam, how in ((1, 'missing'), (0, 'short')):
        broken = tmp_path / how
        shutil.copytree(str(root / 'SEQ'), str(broken / 'SEQ'))
        path = broken / 'SEQ' / 'mav0' / ('cam%d' % cam) / 'times.txt'
        if how == 'missing':
            os.remove(str(path))
        else:
            path.write_text(''.join(path.read_text().splitlines(True)[:-2]))
        with pytest.raises(ValueError, match=r'cam%d.times\.txt' % cam) as e:
            sweep.main(['--root', str(broken), '--sequences', 'SEQ', '--exposure-reference', str(T_REF), '--out', str(tmp_path / 'txts')])
        assert ('is missing' if how == 'missing' else 'has no line for frame') in str(e.value)
    # without the switch the files are never opened: the sequence without them sweeps as ever
    sweep.main(['--root', str(tmp_path / 'missing'), '--sequences', 'SEQ', '--max-frames', '2', '--out', str(tmp_path / 'txts')])
