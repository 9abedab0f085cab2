"""Images above 2^19 pixels on the GPU: the detector's wide keypoint word against the CPU oracle, CLAHE against its NumPy definition,
the engine in every entry path against OracleFrontend at 832 x 640 and 1280 x 720, and a 1280 x 720 EuRoC-layout sweep."""
import numpy as np
import pytest

import clahe_ref as cr
from fe_harness import MODES, Frames, against_oracle, read_ransac_counts, run_engine, run_oracle, scaled_cfg as _scaled_cfg
from ransac_helpers import check_ransac_counts, run_ransac_oracle

pytestmark = pytest.mark.gpu

GRID_FLOOR = 4 * 5 * 3          # grid_num * grid_min_feature_num of ConfigEuRoC: what a healthy frame publishes at the least


# ---- detector ------------------------------------------------------------------------------------------------------------------
def _raw_words(entry, img, threshold, cap=1 << 17):
    """The unordered packed words of one image from av_fast_detect / av_fast_detect_wide, sorted."""
    import torch
    from uav_airvision_amd import _native as N
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    h, w = img.shape
    kp = torch.empty(cap, dtype=torch.int32, device='cuda')
    cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
    rc = getattr(N.lib(), entry)(N.dptr(t), w * h, None, 0, 1, w, h, int(threshold), N.dptr(kp), N.dptr(cnt), cap, N.current_stream())
    if rc:
        return rc, N.lib().av_last_error().decode()
    torch.cuda.synchronize()
    n = int(cnt.item())
    assert n <= cap
    return 0, np.sort(kp[:n].cpu().numpy().view(np.uint32))


def _textured(seed, w, h):
    from uav_airvision_amd.synth import make_texture
    return np.ascontiguousarray(np.rint(make_texture(seed, size=(h, w))).astype(np.uint8))


def test_fast_at_832x640_matches_the_oracle_with_rasters_above_2_19():
    """532,480 pixels: the smallest kind of image past the old limit, with a partial bottom tile row (640 = 13 x 48 + 16).  Keypoints,
    scores and order equal the oracle's, with and without a mask; corners lie in the rows whose rasters need bit 19; the narrow
    entry still refuses the size and the wide entry's words are the documented ones."""
    from oracle import cvops
    from uav_airvision_amd import _native as N, ops
    w, h = 832, 640
    img = _textured(51, w, h)
    rx, ry, rs = cvops.fast_detect(img, 15)
    assert len(rx) > 2000 and int((ry.astype(np.int64) * w + rx >= 1 << 19).sum()) >= 1
    gx, gy, gs = ops.fast_detect(img, 15, cap=1 << 17)
    assert np.array_equal(gx, rx) and np.array_equal(gy, ry) and np.array_equal(gs, rs)
    rc, words = _raw_words('av_fast_detect_wide', img, 15)
    assert rc == 0 and np.array_equal(words, np.sort(ops.pack_keypoints(rx, ry, rs, w, 24)))
    rc, text = _raw_words('av_fast_detect', img, 15)
    assert rc == N.AV_E_INVALID and '2^19' in text
    mask = np.ones((h, w), np.uint8)
    mask[600:, 100:700] = 0
    mask[::7, ::5] = 0
    mx, my, ms = cvops.fast_detect(img, 15, mask)
    assert 0 < len(mx) < len(rx) and int((my.astype(np.int64) * w + mx >= 1 << 19).sum()) >= 1
    ax, ay, a_s = ops.fast_detect(img, 15, mask, cap=1 << 17)
    assert np.array_equal(ax, mx) and np.array_equal(ay, my) and np.array_equal(a_s, ms)


def test_fast_at_4096x4096_reaches_both_ends_of_the_24_bit_raster():
    """2^24 pixels, near-uniform, with corners planted in the first and last 64 rows and at x = 3 and x = w - 4: rasters from
    3 * w + 3 to the last one a corner can have, (h - 4) * w + w - 4, every raster bit 19 .. 23 in use."""
    from oracle import cvops
    from uav_airvision_amd import ops
    w = h = 4096
    rng = np.random.default_rng(52)
    img = np.full((h, w), 100, np.uint8)
    img[:64] += rng.integers(0, 4, (64, w), dtype=np.uint8)
    img[-64:] += rng.integers(0, 4, (64, w), dtype=np.uint8)
    rows = list(range(3, 64, 6)) + list(range(h - 64, h - 3, 6))
    for j, y in enumerate(rows):
        for x in [3, w - 4] + rng.integers(8, w - 8, 12).tolist():
            img[y, x] = 160 + (7 * j + x) % 90
    rx, ry, rs = cvops.fast_detect(img, 15)
    raster = ry.astype(np.int64) * w + rx
    assert len(rx) >= 2 * len(rows) and raster.min() == 3 * w + 3 and raster.max() == (h - 4) * w + w - 4
    assert all(((raster >> b) & 1).any() for b in range(19, 24))
    gx, gy, gs = ops.fast_detect(img, 15)
    assert np.array_equal(gx, rx) and np.array_equal(gy, ry) and np.array_equal(gs, rs)


def test_fast_at_the_old_limit_is_the_same_through_both_entries():
    """1024 x 512 = 2^19 pixels: av_fast_detect writes the words it always wrote -- score << 19 | (2^19 - 1 - raster) of the oracle's
    keypoints, bit for bit -- and av_fast_detect_wide the same keypoints in its own format."""
    from oracle import cvops
    from uav_airvision_amd import ops
    w, h = 1024, 512
    img = _textured(53, w, h)
    rx, ry, rs = cvops.fast_detect(img, 15)
    assert len(rx) > 2000
    rc, narrow = _raw_words('av_fast_detect', img, 15)
    assert rc == 0 and np.array_equal(narrow, np.sort(ops.pack_keypoints(rx, ry, rs, w, 19)))
    rc, wide = _raw_words('av_fast_detect_wide', img, 15)
    assert rc == 0 and np.array_equal(wide, np.sort(ops.pack_keypoints(rx, ry, rs, w, 24)))
    for words, bits in ((narrow, 19), (wide, 24)):
        x, y, s = ops.unpack_keypoints(words, w, bits)
        assert np.array_equal(x, rx) and np.array_equal(y, ry) and np.array_equal(s, rs)
    assert ops.kp_raster_bits(w, h) == 19                # the Python wrapper keeps the narrow entry here


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w,h,tiles', [(832, 640, (8, 8)), (1280, 720, (1, 1))])
def test_clahe_above_the_old_limit_is_bit_identical_to_the_numpy_definition(w, h, tiles):
    """Image and look-up tables equal tests/clahe_ref.py bit for bit.  1280 x 720 with one tile is the largest tile area tested:
    921,600 pixels.  The arithmetic is proven exact for every area up to 2^24 = AV_MAX_IMAGE_PIXELS, the largest a tile can have:
    every histogram bin, the clipped total and every prefix sum is an integer of at most 2^24, which int32 and float32 both hold
    exactly, so (float)sum * (255.0f / (float)area) sees the same two operands as the NumPy definition; no product of 255 and a count
    is formed in integers anywhere.  (tests/clahe_ref.py itself handles these sizes; its padding helper walks the rows and columns
    in Python, which a 2^24-pixel image would make slow, not wrong.)"""
    from uav_airvision_amd import ops
    img = cr.seeded_image(60 + w, w, h)
    ref, ref_lut = cr.clahe(img, 2.0, tiles, return_lut=True)
    out, lut = ops.clahe(img, 2.0, tiles, return_lut=True)
    assert np.array_equal(lut[0].cpu().numpy(), ref_lut)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert not np.array_equal(ref, img)


# ---- engine --------------------------------------------------------------------------------------------------------------------
def _streams(cfg, seeds, n_frames, **kw):
    from uav_airvision_amd.synth import SyntheticStream, make_texture
    tex = make_texture(0xA1B0 + 3)               # one texture, another part of it and another trajectory noise per seed
    return [Frames.cached(SyntheticStream(cfg, seed=s, n_frames=n_frames, motion_scale=1.5, texture=tex, tex_offset=(37.0 * i, 11.0 * i), **kw))
            for i, s in enumerate(seeds)]


def _check(ref, got, tag):
    """The harness's comparison, and a full grid from the third frame on."""
    against_oracle(ref, got, tag, min_features=GRID_FLOOR, floor_from=2)


@pytest.fixture(scope='module')
def at_832x640():
    """Three streams of different seeds, eight frames, and the oracle's run on each (seeds checked on the CPU oracle alone: 60
    features on the first frame, 98 .. 100 on every later one)."""
    cfg = _scaled_cfg(832, 640)
    streams = _streams(cfg, (41, 42, 43), 8)
    refs = [run_oracle(cfg, st) for st in streams]
    for ref in refs:
        assert all(len(r['ids']) >= GRID_FLOOR for r in ref[2:])
    return cfg, streams, refs


@pytest.mark.parametrize('mode', MODES)
def test_engine_at_832x640_matches_the_oracle_in_every_entry_path(at_832x640, mode):
    cfg, streams, refs = at_832x640
    got = run_engine(cfg, streams, mode=mode)
    for i, ref in enumerate(refs):
        _check(ref, got[i], '%s stream %d' % (mode, i))
    assert not np.array_equal(got[0][-1][1], got[1][-1][1])


@pytest.fixture(scope='module')
def at_1280x720():
    cfg = _scaled_cfg(1280, 720)
    st, = _streams(cfg, (44,), 6)
    ref = run_oracle(cfg, st)
    assert all(len(r['ids']) >= GRID_FLOOR for r in ref[2:])
    return cfg, st, ref


@pytest.mark.parametrize('mode', ('step', 'frames'))
def test_engine_at_1280x720_matches_the_oracle(at_1280x720, mode):
    """921,600 pixels: most rasters need the wide word; 720 rows are no whole number of the fused pyramid kernel's tiles and levels
    2 and 3 no longer fit one workgroup's LDS, so the per-level pyramid kernels run."""
    cfg, st, ref = at_1280x720
    got = run_engine(cfg, [st], mode=mode)
    _check(ref, got[0], mode)
    assert int(np.max([c['n_fast'] for _i, _u, c in got[0]])) > 4000


def test_engine_at_832x640_with_clahe_and_ransac_matches_the_oracle_with_both_references_inserted():
    """use_clahe and use_ransac together: the oracle runs on frames the NumPy CLAHE definition equalised, with the reference RANSAC
    inserted where the engine runs its stage (the patterns of test_gpu_clahe_engine.py and test_gpu_ransac_engine.py)."""
    from uav_airvision_amd.synth import SyntheticStream
    cfg = _scaled_cfg(832, 640, use_clahe=True, use_ransac=True)
    st = Frames.cached(SyntheticStream(cfg, seed=13, n_frames=6, motion_scale=3.0, moving_region=(280, 200, 550, 440), moving_amplitude=0.3))
    ref = run_ransac_oracle(cfg, st.map(cr.clahe))
    assert all(r['margin'] >= 1e-9 for r in ref), [r['margin'] for r in ref]
    got = run_engine(cfg, [st], mode='step', read=read_ransac_counts)[0]
    _check(ref, got, 'clahe + ransac')
    check_ransac_counts(ref, got, 'clahe + ransac')


# ---- EuRoC-layout sweep --------------------------------------------------------------------------------------------------------
def test_sweep_runner_on_1280x720_pngs_is_pinned_to_the_oracle(at_1280x720, tmp_path):
    """Six 1280 x 720 frames written as PNGs in the dataset's layout go reader -> PNG decoder -> frame store -> engine -> filter
    through the sweep runner with the scaled config; every frame's ids, coordinates, filter activation and state are pinned to the
    CPU oracle pipeline on the same files, as tests/test_gpu_sweep.py does at the default size."""
    from oracle.frontend import OracleFrontend
    from oracle.msckf_np import OracleMSCKF
    from uav_airvision_amd.euroc import EuRoCDataset, replay, write_euroc_layout
    from uav_airvision_amd.sweep import BatchedRunner
    cfg, st, _ref = at_1280x720
    root = str(tmp_path / 'SYN_720P')
    write_euroc_layout(root, st, compress_level=1)
    ds = EuRoCDataset(root)
    fe, flt = OracleFrontend(cfg), OracleMSCKF(cfg)
    want = []

    def on_stereo(m):
        assert m.cam0_image.shape == (720, 1280)
        msg = fe.stereo_callback(m)
        r = flt.feature_callback(msg)
        s = flt.imu_state
        want.append((m.timestamp, np.array([f.id for f in msg.features], np.int64),
                     np.array([[f.u0, f.v0, f.u1, f.v1] for f in msg.features], np.float64).reshape(-1, 4), r is not None,
                     np.concatenate([[s.timestamp if s.timestamp is not None else -1.0], s.position, s.orientation, s.velocity])))
    replay(ds, [fe.imu_callback, flt.imu_callback], on_stereo)
    got = []

    def on_step(step, ts, ids, uv, n, out):
        got.append((ts[0], ids[0, :n[0]].copy(), uv[0, :n[0]].copy(), bool(out[0, 0] > 0.5), out[0, 1:12].copy()))
    ds2 = EuRoCDataset(root)
    runner = BatchedRunner(cfg, 1)
    assert (runner.eng.width, runner.eng.height) == (1280, 720)
    runner.run([ds2], on_step=on_step)
    assert runner.plan is not None and runner.eng.read_counters(0)['overflow'] == 0          # the shared frame store carried the frames
    runner.close()
    assert len(got) == len(want) == 6
    for k, (g, r) in enumerate(zip(got, want)):
        assert g[0] == r[0], k
        assert np.array_equal(g[1], r[1]), 'frame %d: feature ids differ from the CPU oracle' % k
        assert np.array_equal(g[2].view(np.uint64), r[2].view(np.uint64)), 'frame %d: published coordinates differ' % k
        assert g[3] == r[3], k
        if r[3]:
            assert float(np.abs(g[4] - r[4]).max()) < 1e-6, k
        if k >= 2:
            assert len(g[1]) >= GRID_FLOOR, k
