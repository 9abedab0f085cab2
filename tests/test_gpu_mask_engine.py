"""The front-end engine with static per-camera masks (FrontendEngine.set_masks / config.cam0_mask, cam1_mask) against the CPU oracle
front-end with the three gates of tests/mask_ref.py: published ids and uv bit for bit and the counters equal on every frame, in every
entry path; circles; off is off; binning; CLAHE; RANSAC; placement in a batch; a width FAST reads the mask of byte by byte; refusals."""
import numpy as np
import pytest

import clahe_ref as cr
import mask_ref as mr
from downscale_helpers import binned_stream
from fe_harness import MODES, Frames, against_oracle as against, bare_cfg, make_cfg as _cfg, read_grid, read_ransac_counts, run_engine, run_oracle, \
    same as _same, scaled_cfg

pytestmark = pytest.mark.gpu

W, H = 752, 480
STREAM = dict(seed=13, n_frames=10, motion_scale=3.0)


@pytest.fixture(scope='module')
def base():
    """The stream of every test at 752 x 480, rendered once."""
    from uav_airvision_amd.synth import SyntheticStream
    return Frames.cached(SyntheticStream(_cfg(), **STREAM))


@pytest.fixture(scope='module')
def plain(base):
    """The plain oracle's run (computed once, shared, never changed)."""
    return run_oracle(_cfg(), base)


@pytest.fixture(scope='module')
def combs(base, plain):
    """cam0 comb(96, 24, 0), cam1 comb(96, 24, 48) and the masked oracle's run, with the preconditions of the comparison."""
    m0, m1 = mr.comb_mask(W, H, 96, 24, 0), mr.comb_mask(W, H, 96, 24, 48)
    ref, fe = mr.run_masked_oracle(_cfg(), base, m0, m1)
    print('comb masks: drops', fe.drops, 'n_fast masked', [r['add']['n_fast'] for r in ref], 'plain', [r['add'].get('n_fast') for r in plain])
    assert fe.drops['track'] >= 5 and fe.drops['stereo'] >= 100, fe.drops
    assert all(r['add']['n_fast'] < p['add']['n_fast'] for r, p in zip(ref[1:], plain[1:]))
    assert all(len(r['ids']) >= 50 for r in ref)
    return m0, m1, ref


@pytest.mark.parametrize('mode', MODES)
def test_comb_masks_in_every_entry_path(base, combs, mode):
    """step in both level-0 modes, prestage + step, step_host and the frame store (where FAST runs at upload time)."""
    m0, m1, ref = combs
    got = run_engine(_cfg(cam0_mask=m0, cam1_mask=m1), [base], mode=mode)
    against(ref, got[0], 'comb ' + mode)


def test_circle_masks(base):
    """Both cameras behind a fisheye's image circle of radius 300 around the image centre."""
    from uav_airvision_amd.frontend import circle_mask
    c = circle_mask(W, H, 376, 240, 300)
    assert np.array_equal(c, mr.circle_mask(W, H, 376, 240, 300))
    ref, fe = mr.run_masked_oracle(_cfg(), base, c, c)
    print('circle masks: drops', fe.drops)
    assert fe.drops['track'] >= 1 and fe.drops['stereo'] >= 50, fe.drops
    got = run_engine(_cfg(cam0_mask=c, cam1_mask=c), [base], mode='step')
    against(ref, got[0], 'circle')


def test_off_is_off(base, plain, combs):
    """No masks = all-ones masks = a config object without the attributes: the same outputs and the same timing spans per step (a mask
    adds no launch).  One mask alone = the masked oracle with the other camera all valid."""
    m0, m1, _ref = combs
    ones = np.ones((H, W), np.uint8)

    bare = bare_cfg(lambda k: k in ('cam0_mask', 'cam1_mask'))
    assert not hasattr(bare, 'cam0_mask') and not hasattr(bare, 'cam1_mask')
    n = 6
    for mode in ('step', 'frames'):
        off, sp_off = run_engine(_cfg(), [base], mode=mode, n_frames=n, timing=True)
        none, sp_none = run_engine(bare, [base], mode=mode, n_frames=n, timing=True)
        full, sp_full = run_engine(_cfg(cam0_mask=ones, cam1_mask=ones), [base], mode=mode, n_frames=n, timing=True)
        _on, sp_on = run_engine(_cfg(cam0_mask=m0, cam1_mask=m1), [base], mode=mode, n_frames=n, timing=True)
        assert all(_same(a, b) for a, b in zip(off[0], none[0])) and all(_same(a, b) for a, b in zip(off[0], full[0])), mode
        assert sp_off == sp_none == sp_full == sp_on and sum(sp_off[-1].values()) > 10, (mode, sp_off[-1], sp_on[-1])
        for r, g in zip(plain, off[0]):
            assert np.array_equal(g[0], r['ids']) and np.array_equal(g[1].view(np.uint64), r['uv'].view(np.uint64)), mode
    for tag, a, b in (('mask0 only', m0, None), ('mask1 only', None, m1)):
        ref, fe = mr.run_masked_oracle(_cfg(), base, ones if a is None else a, ones if b is None else b, n_frames=n)
        assert fe.drops['track'] + fe.drops['stereo'] > 0, tag
        got = run_engine(_cfg(cam0_mask=a, cam1_mask=b), [base], mode='step', n_frames=n)
        against(ref, got[0], tag)


def test_binning(base):
    """image_downscale = 2 with full-size combs whose band edges fall on odd x (23 | 24 and 95 | 96 for cam0): a binned pixel that
    straddles an edge is masked.  Against the masked oracle fed host-binned frames, downscaled_config and bin_mask; read_mask = bin_mask."""
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine, downscaled_config
    m0, m1 = mr.comb_mask(W, H, 96, 24, 1), mr.comb_mask(W, H, 96, 24, 49)
    assert m0[0, 22] == 0 and m0[0, 23] == 1 and m0[0, 94] == 1 and m0[0, 95] == 0
    b0, b1 = mr.bin_mask(m0, 2), mr.bin_mask(m1, 2)
    assert b0[0, 11] == 0 and b0[0, 12] == 1 and b0[0, 46] == 1 and b0[0, 47] == 0 and b0.sum() < m0.sum() // 4
    cfg = _cfg(image_downscale=2, cam0_mask=m0 * 255, cam1_mask=m1.astype(bool))          # any non-zero value, or bool, is valid
    ref, fe = mr.run_masked_oracle(downscaled_config(_cfg(image_downscale=2)), binned_stream(base, 2), b0, b1)
    assert fe.drops['track'] >= 1 and fe.drops['stereo'] >= 50, fe.drops
    for mode in ('step', 'frames'):
        got = run_engine(cfg, [base], mode=mode)
        against(ref, got[0], 'binned ' + mode)
    eng = FrontendEngine(cfg, n_streams=1)
    r0, r1 = eng.read_mask(0), eng.read_mask(1)
    assert r0.shape == (H // 2, W // 2) and r0.dtype == np.uint8 and np.array_equal(r0, b0) and np.array_equal(r1, b1)
    eng.set_masks(None, m1)
    with pytest.raises(N.AirvisionError, match='no mask is set for camera 0'):
        eng.read_mask(0)
    assert np.array_equal(eng.read_mask(1), b1)
    eng.close()
    full = FrontendEngine(_cfg(cam0_mask=m0 * 7), n_streams=2)                             # full size: stored as 0 / 1
    assert np.array_equal(full.read_mask(0), m0)
    full.close()


def test_with_clahe(base, combs):
    """The masks do not change what CLAHE sees: against the masked oracle fed reference-equalised frames."""
    m0, m1, _ref = combs
    ref, fe = mr.run_masked_oracle(_cfg(), base.map(cr.clahe), m0, m1)
    assert fe.drops['track'] >= 1 and fe.drops['stereo'] >= 100, fe.drops
    for mode in ('step', 'frames'):
        got = run_engine(_cfg(use_clahe=True, cam0_mask=m0, cam1_mask=m1), [base], mode=mode)
        against(ref, got[0], 'clahe ' + mode)


def test_with_ransac_every_published_point_lies_on_valid_pixels(base, combs):
    """No oracle combines the masks with the outlier rejection, so the property: on every frame every point of read_grid lies on a valid
    pixel of its camera's mask, and at least one frame publishes fewer features than the run without masks."""
    m0, m1, _ref = combs

    def run(cfg):
        got = run_engine(cfg, [base], mode='host', read=lambda eng, i: read_grid(eng, i) + read_ransac_counts(eng, i))[0]
        assert all(len(g['ids']) == len(ids) and cnt['overflow'] == 0 for ids, _uv, cnt, g, _rc in got)
        return [(len(ids), g['cam0'], g['cam1'], rc) for ids, _uv, _cnt, g, rc in got]
    masked, free = run(_cfg(use_ransac=True, cam0_mask=m0, cam1_mask=m1)), run(_cfg(use_ransac=True))
    assert any(r[3]['after_ransac'] > 0 for r in masked[1:])                   # the stage ran
    for k, (n, p0, p1, _rc) in enumerate(masked):
        assert n >= 40, (k, n)
        assert m0[p0[:, 1].astype(int), p0[:, 0].astype(int)].min() == 1, k
        assert m1[p1[:, 1].astype(int), p1[:, 0].astype(int)].min() == 1, k
    assert any(m0[p0[:, 1].astype(int), p0[:, 0].astype(int)].min() == 0 or m1[p1[:, 1].astype(int), p1[:, 0].astype(int)].min() == 0
               for _n, p0, p1, _rc in free)                                    # (without masks the run does publish points there)
    assert any(a[0] < b[0] for a, b in zip(masked, free)), [(a[0], b[0]) for a, b in zip(masked, free)]


def test_a_stream_gives_the_same_result_anywhere_in_a_batch(base, combs):
    """One stream alone = the same stream as entry 0, 17 and 63 of a 64-stream batch, masks set: one mask, read at stride 0 by every
    stream's detector tiles, and through the frame store's index maps."""
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    m0, m1, ref = combs
    nf = 5
    cfg = _cfg(cam0_mask=m0, cam1_mask=m1)
    tex = make_texture(0xA1B0 + 3)
    # the other 61 entries replay three other streams (rendering 61 would take minutes): what matters is that they are not the probe
    pool = [Frames.cached(SyntheticStream(cfg, seed=100 + i, n_frames=nf, motion_scale=1.0 + 0.4 * i, texture=tex, tex_offset=(37.0 * i, 11.0 * i)))
            for i in range(3)]
    batch = [pool[i % 3] for i in range(61)]
    for pos in (0, 17, 63):
        batch.insert(pos, base)
    assert len(batch) == 64 and all(batch[p] is base for p in (0, 17, 63))
    for mode in ('step', 'frames'):
        got = run_engine(cfg, batch, mode=mode, n_frames=nf)
        for pos in (0, 17, 63):
            against(ref[:nf], got[pos], 'batch %s entry %d' % (mode, pos))
        assert not all(_same(a, b) for a, b in zip(got[0], got[1])), mode


def test_a_width_that_is_no_multiple_of_four():
    """374 x 240: the detector reads the mask byte by byte instead of a dword per four pixels."""
    from uav_airvision_amd.synth import SyntheticStream
    w, h = 374, 240

    def cfg(**kw):
        return scaled_cfg(w, h, **kw)
    st = Frames.cached(SyntheticStream(cfg(), seed=13, n_frames=5, motion_scale=3.0))
    m0, m1 = mr.comb_mask(w, h, 48, 12, 0), mr.comb_mask(w, h, 48, 12, 24)
    ref, fe = mr.run_masked_oracle(cfg(), st, m0, m1)
    assert fe.drops['stereo'] >= 50 and all(len(r['ids']) >= 50 for r in ref), fe.drops
    for mode in ('step', 'frames'):
        got = run_engine(cfg(cam0_mask=m0, cam1_mask=m1), [st], mode=mode)
        against(ref, got[0], '374x240 ' + mode)


def test_refusals(base, combs):
    """set_masks is refused once the engine has been handed a frame -- by a step, a prestage or a frames_upload -- with a text that says
    so; before that it may be called again, and cleared.  A wrong shape is a ValueError before anything reaches the library."""
    import torch
    from uav_airvision_amd import _native as N
    from uav_airvision_amd.frontend import FrontendEngine
    m0, m1, _ref = combs
    f = base.frame(0)
    a0, a1 = f.cam0_image[None], f.cam1_image[None]

    def feed_step(eng):
        eng.step_host(a0, a1, [f.timestamp])

    def feed_prestage(eng):
        eng.prestage(torch.from_numpy(a0).cuda(), torch.from_numpy(a1).cuda())

    def feed_upload(eng):
        eng.frames_reserve(2)
        eng.frames_upload(np.array([0], np.int32), a0, a1)
    for feed in (feed_step, feed_prestage, feed_upload):
        eng = FrontendEngine(_cfg(), n_streams=1, inputs_persist=feed is feed_prestage)
        eng.set_masks(m0, m1)
        eng.set_masks(m1, None)                       # again, before the first frame
        assert np.array_equal(eng.read_mask(0), m1)
        eng.set_masks(None, None)                     # cleared
        with pytest.raises(N.AirvisionError, match='no mask is set'):
            eng.read_mask(0)
        eng.set_masks(m0, m1)
        feed(eng)
        for args in ((m0, m1), (None, None)):
            with pytest.raises(N.AirvisionError, match='already been handed a frame') as e:
                eng.set_masks(*args)
            assert e.value.code == N.AV_E_INVALID
        assert np.array_equal(eng.read_mask(0), m0) and np.array_equal(eng.read_mask(1), m1)      # the masks it had stay
        eng.close()
    with pytest.raises(ValueError, match=r'cam0 mask.*\(480, 752\).*\(240, 376\)'):
        FrontendEngine(_cfg(cam0_mask=m0[::2, ::2]), n_streams=1)
    eng = FrontendEngine(_cfg(), n_streams=1)
    with pytest.raises(ValueError, match=r'cam1 mask.*\(480, 752\).*\(752, 480\)'):
        eng.set_masks(m0, np.ascontiguousarray(m1.T))
    with pytest.raises(ValueError, match=r'cam0 mask.*float64'):
        eng.set_masks(m0.astype(np.float64), m1)
    with pytest.raises(N.AirvisionError):
        eng.read_mask(0)                              # nothing was set by the refused calls
    eng.close()
