"""The exposure-time normalisation on the CPU: the quantiser of uav_airvision_amd/frontend.py against its restatement, the NumPy
definition of tests/exposure_ref.py against tests/photometric_ref.py, and the fact that motivates the stage -- the unmodified oracle
front-end loses its tracks on an auto-exposing camera and keeps all of them on normalised frames.  No GPU."""
import numpy as np
import pytest

import exposure_ref as er
import photometric_ref as pr
from fe_harness import Frames, make_cfg, run_oracle

NF = 4
MIN_FEATURES = 20


def test_the_quantiser():
    from uav_airvision_amd.frontend import quantise_exposure
    ratios = [1.0, 0.55, 1.6, 1.0 / 16, 1e-9]
    want = [4096, 7447, 2560, 65535, 65535]                # floor(4096 / r + 0.5): 7447.27 -> 7447; 4096 * 16 = 65536 clamps
    k = quantise_exposure(np.array(ratios) * 8.0, 8.0)
    assert k.dtype == np.uint16 and k.tolist() == want == er.quantise(np.array(ratios) * 8.0, 8.0).tolist()
    assert int(quantise_exposure(3.0, 3.0)) == 4096 and quantise_exposure(3.0, 3.0).shape == ()
    assert int(quantise_exposure(1e12, 1.0)) == 1                                  # the lower clamp
    rng = np.random.default_rng(3)
    t = rng.uniform(0.05, 40.0, 500)
    assert np.array_equal(quantise_exposure(t, 7.5), er.quantise(t, 7.5))
    for bad_t, bad_ref in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (np.inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, np.nan), ([1.0, 0.0], 1.0)):
        with pytest.raises(ValueError):
            quantise_exposure(bad_t, bad_ref)


def test_the_reference_at_the_reference_exposure_is_the_photometric_definition():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (3, 31, 45), dtype=np.uint8)
    resp = np.sort(rng.integers(0, pr.RESPONSE_MAX + 1, 256)).astype(np.uint16)
    gain = rng.integers(1, 65536, (31, 45)).astype(np.uint16)
    assert np.array_equal(er.effective_table(resp, 4096), resp)
    for r, g in ((resp, gain), (resp, None), (None, gain)):
        assert np.array_equal(er.correct(img, r, g, [4096] * 3), pr.correct(img, r, g))
    assert np.array_equal(er.correct(img, None, None, 4096), img)


def test_the_factor_commutes_with_an_absent_response():
    """An absent response is the table p << 8: the same result whether it is left out or written out, for any factor."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (20, 33), dtype=np.uint8)
    gain = rng.integers(1, 65536, (20, 33)).astype(np.uint16)
    ident = (np.arange(256) << 8).astype(np.uint16)
    for k in (1, 2047, 4095, 4096, 4097, 7447, 65535):
        assert np.array_equal(er.correct(img, None, gain, k), er.correct(img, ident, gain, k)), k
        assert np.array_equal(er.effective_table(None, k), np.minimum(65280, (np.arange(256) * 256 * k + 2048) >> 12)), k
    assert int(er.effective_table(None, 65535).max()) == 65280 and 65280 * 65535 + 2048 < 2 ** 32


def test_the_forward_model():
    from uav_airvision_amd.frontend import apply_exposure, apply_vignette
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (24, 40), dtype=np.uint8)
    v = pr.radial_vignette(40, 24, 0.4)
    fwd = pr.gamma_forward(2.2)
    assert np.array_equal(apply_exposure(img, 1.0, v, fwd), apply_vignette(img, v, fwd))
    assert np.array_equal(apply_exposure(img, 0.55, v, fwd), er.degrade(img, 0.55, v, fwd))
    assert np.array_equal(apply_exposure(img, 1.6), np.clip(np.floor(img * 1.6 + 0.5), 0, 255).astype(np.uint8))


@pytest.mark.parametrize('which', [0, 1])
def test_the_oracle_loses_its_tracks_on_an_exposure_step_and_keeps_them_on_normalised_frames(which):
    """The motivating fact, on the project's own synthetic streams, 752 x 480, 4 frames, exposure ratios 1 / 0.55 / 1.6 / 0.8 (cam0) and
    1 / 0.6 / 1.5 / 0.7 (cam1): the unmodified oracle on frames normalised by the integer rule tracks what it tracks on the clean
    frames, and less than half of that on the frames as recorded."""
    from uav_airvision_amd.synth import SyntheticStream
    cfg = make_cfg()
    seed, motion = er.SEEDS[which]
    clean = Frames.cached(SyntheticStream(cfg, seed=seed, n_frames=NF, motion_scale=motion))
    r0, r1 = er.RATIOS
    deg, cor = [], []
    for k in range(NF):
        m = clean.frame(k)
        d = (er.degrade(m.cam0_image, r0[k]), er.degrade(m.cam1_image, r1[k]))
        c = (er.correct(d[0], None, None, int(er.quantise(r0[k], 1.0))), er.correct(d[1], None, None, int(er.quantise(r1[k], 1.0))))
        deg.append(type(m)(m.timestamp, d[0], d[1], type(m.cam0_msg)(m.timestamp, d[0]), type(m.cam1_msg)(m.timestamp, d[1])))
        cor.append(type(m)(m.timestamp, c[0], c[1], type(m.cam0_msg)(m.timestamp, c[0]), type(m.cam1_msg)(m.timestamp, c[1])))
    runs = {name: run_oracle(cfg, Frames(clean, fr)) for name, fr in (('clean', [clean.frame(k) for k in range(NF)]), ('degraded', deg), ('corrected', cor))}
    match = {name: [f['nf'].get('after_matching', 0) for f in r] for name, r in runs.items()}
    published = [len(f['ids']) for f in runs['corrected']]
    print(match, published)
    assert all(n >= MIN_FEATURES for n in published) and all(n >= 60 for n in published), published
    assert match['corrected'][1:] == match['clean'][1:] and min(match['clean'][1:]) >= 60, match
    for k in (2, 3):
        assert 2 * match['degraded'][k] < match['corrected'][k], (k, match)
