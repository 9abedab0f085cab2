"""The detector's keep-out rule -- no new corner within 3 pixels of a tracked feature (feature_adder.py:59-62) -- as the engine
decides it: select_kernel tests every FAST survivor against the 7x7 boxes of the stream's tracked features, which it buckets per
detector tile in LDS; there is no per-stream byte image of the boxes.  The engine against the CPU oracle, which paints the image,
on inputs where every border case of the rule occurs; the oracle's side counts them, so that the inputs cannot quietly stop binding."""
import numpy as np
import pytest

from fe_harness import Frames, against_oracle, make_cfg, read_ransac_counts, run_engine, run_oracle, scaled_cfg
from oracle.frontend import OracleFrontend, cell_of, cvops, grid_size

pytestmark = pytest.mark.gpu

W, H = 376, 240                       # 6 x 5 detector tiles of 64 x 48, the last column 56 wide
SEEDS = (3, 0)
STREAM = dict(n_frames=16, motion_scale=1.6)
CLASSES = ('no_box', 'box_crosses_cell', 'box_clipped', 'dropped', 'dropped_by_other_cell')


def grid_cfg(rows=4, cols=5, **kw):
    return scaled_cfg(W, H, grid_row=rows, grid_col=cols, grid_num=rows * cols, grid_min_feature_num=3, grid_max_feature_num=15, **kw)


class TapOracle(OracleFrontend):
    """OracleFrontend that counts, in every frame that adds features, how often each case of the rule occurred: from curr_features
    as _add_new finds them, and from the detector run once with and once without the image of the boxes."""

    def _add_new(self, img0, img1):
        cfg = self.config
        h, w = img0.shape[:2]
        gh, gw = grid_size(img0, cfg)
        tap = dict.fromkeys(CLASSES, 0)
        boxes = []                                               # (x0, y0, x1, y1, cell of the feature), clipped, ends inclusive
        for cell in self.curr_features:
            for f in cell:
                x, y = int(f.cam0_point[0]), int(f.cam0_point[1])
                if x < 3 or y < 3:                               # negative slice start: an empty slice
                    tap['no_box'] += 1
                    continue
                x1, y1 = min(x + 3, w - 1), min(y + 3, h - 1)
                tap['box_clipped'] += x + 3 > w - 1 or y + 3 > h - 1
                tap['box_crosses_cell'] += (x - 3) // gw != x1 // gw or (y - 3) // gh != y1 // gh
                boxes.append((x - 3, y - 3, x1, y1, cell_of(f.cam0_point, gh, gw, cfg)))
        xs, ys, _sc = cvops.fast_detect(img0, cfg.fast_threshold, None)
        OracleFrontend._add_new(self, img0, img1)
        tap['n_unmasked'] = len(xs)
        tap['dropped'] = len(xs) - self.debug['add']['n_fast']
        b = np.array(boxes, np.int64).reshape(-1, 5)
        x, y = np.asarray(xs, np.int64)[:, None], np.asarray(ys, np.int64)[:, None]
        inside = (b[:, 0] <= x) & (x <= b[:, 2]) & (b[:, 1] <= y) & (y <= b[:, 3])                # [survivor][box]
        own = b[:, 4] == np.array([cell_of((float(u), float(v)), gh, gw, cfg) for u, v in zip(xs, ys)], np.int64).reshape(-1, 1)
        assert int(inside.any(1).sum()) == tap['dropped'], tap   # the boxes recomputed here are the ones the oracle painted
        tap['dropped_by_other_cell'] = int((inside.any(1) & ~(inside & own).any(1)).sum())
        self.tap = tap

    def stereo_callback(self, stereo_msg):
        self.tap = {}
        return OracleFrontend.stereo_callback(self, stereo_msg)


def tapped_case(cfg, seeds, **stream):
    from uav_airvision_amd.synth import SyntheticStream
    streams = [Frames.cached(SyntheticStream(cfg, seed=s, **dict(STREAM, **stream))) for s in seeds]
    refs = [run_oracle(cfg, st, oracle=TapOracle(cfg), extra=lambda fe, _msg: dict(tap=dict(fe.tap))) for st in streams]
    return cfg, streams, refs


def class_totals(ref):
    return {c: sum(r['tap'].get(c, 0) for r in ref) for c in CLASSES + ('n_unmasked',)}


@pytest.fixture(scope='module')
def case():
    return tapped_case(grid_cfg(), SEEDS)


def test_the_inputs_make_every_case_of_the_rule_bind(case):
    """Summed over frames 1-15 of either seed, recounted here on the oracle's side: features too close to the left / top border to
    have a box, boxes that cross a grid-cell border, boxes cut at the right / bottom border, survivors the boxes drop, and among those
    the ones only a feature of ANOTHER cell drops (which a per-cell test would miss).  No class may be empty over the two seeds."""
    _cfg, _streams, refs = case
    totals = [class_totals(ref) for ref in refs]
    for seed, t in zip(SEEDS, totals):
        print('seed %d: %s' % (seed, t))
    for c in CLASSES:
        assert sum(t[c] for t in totals) > 0, (c, totals)
    assert all(0 < t['dropped'] < t['n_unmasked'] for t in totals), totals


@pytest.mark.parametrize('mode', ['step', 'frames'])
def test_engine_matches_the_oracle_where_the_rule_binds(case, mode):
    """Both seeds and a third stream (seed 3 again, so that a batch is not a multiple of anything) in one batch of 3: ids, uv bits and
    the counters n_fast / n_candidates / n_new / tracked equal to the oracle's on every frame."""
    cfg, streams, refs = case
    got = run_engine(cfg, streams + [streams[0]], mode=mode)
    for i, ref in enumerate(refs + [refs[0]]):
        against_oracle(ref, got[i], '%s stream %d' % (mode, i), min_features=20)


def test_engine_matches_the_oracle_on_a_fine_grid():
    """Grid 10 x 15 = 150 cells of 26 x 24 pixels, smaller than a detector tile and not aligned with it: most boxes lie over several
    cells, many over two or four tiles, and the lists are sized for 2,250 features (some 1,500 are tracked from frame 4 on).  8 frames."""
    cfg, streams, refs = tapped_case(grid_cfg(10, 15), SEEDS[:1], n_frames=8)
    t = class_totals(refs[0])
    print(t)
    assert t['box_crosses_cell'] > 0 and t['dropped'] > 0 and t['dropped_by_other_cell'] > 0, t
    got = run_engine(cfg, streams)
    against_oracle(refs[0], got[0], 'grid 10 x 15', min_features=20)


def test_engine_with_ransac_matches_the_oracle():
    """With use_ransac the boxes are those of the features that survive the rejection: the moving-region stream of the RANSAC tests,
    a batch of 2, 12 frames; features are rejected, and the adder's counters follow the oracle's."""
    from ransac_helpers import STREAM as MOVING, check_ransac_counts, run_ransac_oracle
    from uav_airvision_amd.synth import SyntheticStream
    cfg = make_cfg(use_ransac=True)
    st = Frames.cached(SyntheticStream(cfg, **dict(MOVING, n_frames=12)))
    ref = run_ransac_oracle(cfg, st)
    assert any(r['nf']['after_ransac'] < r['nf']['after_matching'] for r in ref[1:])
    got = run_engine(cfg, [st, st], read=read_ransac_counts)
    for i in range(2):
        against_oracle(ref, got[i], 'ransac stream %d' % i, min_features=20)
        check_ransac_counts(ref, got[i], 'ransac stream %d' % i)
