"""The NumPy statement of the static masks (tests/mask_ref.py) on its own, the host-only validation of frontend.check_mask, and the
preconditions of the GPU comparisons (tests/test_gpu_mask_engine.py) on the oracle's own run.  No GPU."""
import ctypes

import numpy as np
import pytest

import mask_ref as mr
from fe_harness import Frames, run_oracle

W, H = 752, 480
STREAM = dict(seed=13, n_frames=10, motion_scale=3.0)


def test_bin_mask_hand_cases():
    m = np.ones((4, 8), np.uint8)
    assert np.array_equal(mr.bin_mask(m, 2), np.ones((2, 4), np.uint8))
    m[1, 3] = 0                                              # one zero pixel kills its whole 2 x 2 block, and only that one
    want = np.ones((2, 4), np.uint8); want[0, 1] = 0
    assert np.array_equal(mr.bin_mask(m, 2), want)
    want4 = np.ones((1, 2), np.uint8); want4[0, 0] = 0      # ... and its whole 4 x 4 block
    assert np.array_equal(mr.bin_mask(m, 4), want4)
    # a band edge at odd x matters: columns 3 .. 4 masked take binned columns 1 AND 2; columns 4 .. 5 (even edge) take only column 2
    odd = np.ones((2, 8), np.uint8); odd[:, 3:5] = 0
    even = np.ones((2, 8), np.uint8); even[:, 4:6] = 0
    assert mr.bin_mask(odd, 2).tolist() == [[1, 0, 0, 1]] and mr.bin_mask(even, 2).tolist() == [[1, 1, 0, 1]]
    # any non-zero value is valid; the result is 0 / 1
    grey = np.full((2, 2), 200, np.uint8)
    assert mr.bin_mask(grey, 2).tolist() == [[1]] and mr.bin_mask(grey, 1).tolist() == [[1, 1], [1, 1]]
    assert mr.bin_mask(np.array([[True, False], [True, True]]), 1).tolist() == [[1, 0], [1, 1]]


def test_comb_mask_hand_cases():
    assert mr.comb_mask(8, 2, 4, 1, 0).tolist() == [[0, 1, 1, 1, 0, 1, 1, 1]] * 2
    assert mr.comb_mask(8, 1, 4, 2, 3).tolist() == [[1, 0, 0, 1, 1, 0, 0, 1]]            # (x + 3) % 4 < 2: x = 1, 2, 5, 6
    m = mr.comb_mask(W, H, 96, 24, 0)
    assert m.shape == (H, W) and m.dtype == np.uint8 and m.flags['C_CONTIGUOUS'] and m[:, :24].max() == 0 and m[:, 24:96].min() == 1 and m[0, 96] == 0


def test_circle_mask_hand_cases():
    from uav_airvision_amd.frontend import circle_mask
    want = [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]       # radius 2: the boundary belongs to the circle
    assert mr.circle_mask(5, 5, 2, 2, 2).tolist() == want and circle_mask(5, 5, 2, 2, 2).tolist() == want
    assert mr.circle_mask(4, 2, 0, 0, 1).tolist() == [[1, 1, 0, 0], [1, 0, 0, 0]]
    assert mr.circle_mask(3, 2, 1, 0, 0).tolist() == [[0, 1, 0], [0, 0, 0]]
    assert circle_mask(6, 3, 2.5, 1.0, 1.6).tolist() == mr.circle_mask(6, 3, 2.5, 1.0, 1.6).tolist()
    big = circle_mask(W, H, 376, 240, 300)
    assert big.dtype == np.uint8 and big.shape == (H, W) and np.array_equal(big, mr.circle_mask(W, H, 376, 240, 300))
    assert big[0, 0] == 0 and big[240, 376] == 1 and big[240, 76] == 1 and big[240, 75] == 0 and big[0, 376] == 1


@pytest.fixture(scope='module')
def stream():
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.synth import SyntheticStream
    cfg = ConfigEuRoC()
    st = Frames.cached(SyntheticStream(cfg, **STREAM))
    return cfg, st, run_oracle(cfg, st)


def _same(a, b):
    return np.array_equal(a['ids'], b['ids']) and np.array_equal(a['uv'].view(np.uint64), b['uv'].view(np.uint64))


def test_all_ones_masks_are_the_plain_oracle(stream):
    cfg, st, plain = stream
    ones = np.ones((H, W), np.uint8)
    got, fe = mr.run_masked_oracle(cfg, st, ones, ones, n_frames=6)
    assert len(got) == 6 and all(len(g['ids']) > 50 for g in got)
    assert all(_same(a, b) for a, b in zip(got, plain))
    assert fe.drops == dict(track=0, stereo=0)
    none, _fe = mr.run_masked_oracle(cfg, st, None, None, n_frames=6)
    assert all(_same(a, b) and a['nf'] == b['nf'] for a, b in zip(none, plain))


def test_the_comb_and_circle_runs_exercise_every_gate(stream):
    """The preconditions of the GPU comparisons, on the oracle alone: the masks drop tracked points, stereo matches and corners, the
    run still publishes, every published point lies on a valid pixel of its camera's mask, and the result differs from the plain run."""
    cfg, st, plain = stream
    for tag, m0, m1, min_track, min_stereo in (('comb', mr.comb_mask(W, H, 96, 24, 0), mr.comb_mask(W, H, 96, 24, 48), 5, 100),
                                               ('circle', mr.circle_mask(W, H, 376, 240, 300), mr.circle_mask(W, H, 376, 240, 300), 1, 50)):
        got, fe = mr.run_masked_oracle(cfg, st, m0, m1)
        print(tag, fe.drops, 'n_fast', [g['add']['n_fast'] for g in got], 'published', [len(g['ids']) for g in got])
        assert fe.drops['track'] >= min_track and fe.drops['stereo'] >= min_stereo, (tag, fe.drops)
        assert all(g['add']['n_fast'] < p['add']['n_fast'] for g, p in zip(got[1:], plain[1:])), tag
        assert all(len(g['ids']) >= 50 for g in got), tag
        for g in got:
            assert m0[g['p0'][:, 1].astype(int), g['p0'][:, 0].astype(int)].min() == 1, tag
            assert m1[g['p1'][:, 1].astype(int), g['p1'][:, 0].astype(int)].min() == 1, tag
        assert not all(_same(a, b) for a, b in zip(got, plain)), tag


def test_validation_errors(tmp_path):
    from PIL import Image
    from uav_airvision_amd.frontend import check_mask
    assert check_mask(0, None, H, W) is None
    ok = check_mask(1, np.ones((H, W), bool), H, W)
    assert ok.dtype == np.uint8 and ok.shape == (H, W) and ok.flags['C_CONTIGUOUS'] and ok.min() == 1
    strided = np.ones((H, 2 * W), np.uint8)[:, ::2]
    assert check_mask(0, strided, H, W).flags['C_CONTIGUOUS']
    with pytest.raises(ValueError, match=r'cam1 mask.*\(480, 752\).*\(752, 480\)'):
        check_mask(1, np.ones((W, H), np.uint8), H, W)
    with pytest.raises(ValueError, match=r'cam0 mask.*\(480, 752\).*\(240, 376\)'):
        check_mask(0, np.ones((H // 2, W // 2), np.uint8), H, W)
    with pytest.raises(ValueError, match=r'cam0 mask.*uint8 or bool.*\(480, 752\).*float32 \(480, 752\)'):
        check_mask(0, np.ones((H, W), np.float32), H, W)
    with pytest.raises(ValueError, match=r'cam1 mask.*int32'):
        check_mask(1, np.ones((H, W), np.int32), H, W)
    # PNG files: an 8-bit grey file of the right size is decoded as it is; another size or flavour is refused by name
    comb = mr.comb_mask(W, H, 96, 24, 0) * 255
    Image.fromarray(comb).save(str(tmp_path / 'comb.png'))
    assert np.array_equal(check_mask(0, str(tmp_path / 'comb.png'), H, W), comb)
    assert np.array_equal(check_mask(0, tmp_path / 'comb.png', H, W), comb)
    Image.fromarray(comb[:240, :376]).save(str(tmp_path / 'small.png'))
    with pytest.raises(ValueError, match=r'cam1 mask.*small\.png.*\(480, 752\).*\(240, 376\)'):
        check_mask(1, str(tmp_path / 'small.png'), H, W)
    Image.fromarray(np.repeat(comb[..., None], 3, axis=2)).save(str(tmp_path / 'rgb.png'))
    with pytest.raises(ValueError, match=r'cam0 mask.*rgb\.png.*8-bit grey.*rgb8'):
        check_mask(0, str(tmp_path / 'rgb.png'), H, W)
    with pytest.raises(ValueError, match=r'cam0 mask.*missing\.png'):
        check_mask(0, str(tmp_path / 'missing.png'), H, W)


def test_an_engine_refuses_a_wrong_mask_before_any_device_call():
    """The constructor validates config.cam0_mask / cam1_mask first: the ValueError comes with or without a GPU."""
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.frontend import FrontendEngine
    cfg = ConfigEuRoC()
    cfg.cam1_mask = np.ones((H, W + 1), np.uint8)
    with pytest.raises(ValueError, match=r'cam1 mask.*\(480, 752\).*\(480, 753\)'):
        FrontendEngine(cfg, n_streams=1)
    cfg = ConfigEuRoC()
    cfg.image_downscale = 2
    cfg.cam0_mask = np.ones((H // 2, W // 2), np.uint8)      # masks are given at the input size, not the processed one
    with pytest.raises(ValueError, match=r'cam0 mask.*\(480, 752\).*\(240, 376\)'):
        FrontendEngine(cfg, n_streams=1)


def test_set_masks_without_an_engine_is_refused_without_a_gpu():
    from uav_airvision_amd import _native as N
    m = np.ones((H, W), np.uint8)
    assert N.lib().av_frontend_set_masks(None, m.ctypes.data_as(ctypes.c_void_p), None) == N.AV_E_INVALID
    assert b'av_frontend_set_masks' in N.lib().av_last_error()
    assert N.lib().av_frontend_read_mask(None, 0, m.ctypes.data_as(ctypes.c_void_p)) == N.AV_E_INVALID
    assert b'av_frontend_read_mask' in N.lib().av_last_error()


def test_config_and_sweep_switches_carry_the_masks():
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.sweep import apply_args, make_parser
    cfg = ConfigEuRoC()
    assert cfg.cam0_mask is None and cfg.cam1_mask is None
    args = make_parser().parse_args(['--sequences', 'A', '--mask0', 'm0.png'])
    apply_args(cfg, args)
    assert cfg.cam0_mask == 'm0.png' and cfg.cam1_mask is None
    cfg.cam1_mask = 'kept.png'
    apply_args(cfg, make_parser().parse_args(['--sequences', 'A']))
    assert cfg.cam1_mask == 'kept.png'                       # a mask on the config object stays unless the switch is given
