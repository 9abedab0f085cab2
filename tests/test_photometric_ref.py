"""The NumPy definition of the photometric calibration (tests/photometric_ref.py) against exact arithmetic, against the float model
it quantises, and against the host helpers of uav_airvision_amd/frontend.py.  CPU only."""
import numpy as np
import pytest

import photometric_ref as pr

GAINS = [0, 1, 2, 2047, 2048, 4095, 4096, 4097, 8191, 8192, 40000, 65534, 65535]


def _tables():
    rng = np.random.default_rng(3)
    rand = rng.integers(0, pr.RESPONSE_MAX + 1, 256).astype(np.uint16)
    rand[0], rand[255], rand[7] = 0, pr.RESPONSE_MAX, pr.RESPONSE_MAX
    return {'identity': (np.arange(256) * 256).astype(np.uint16), 'random': rand, 'gamma': pr.quantise_response(pr.gamma_inverse_response(2.2))}


def _sweep():
    """All 256 grey levels against every gain of GAINS: img [len(GAINS), 256], gain of the same shape."""
    img = np.tile(np.arange(256, dtype=np.uint8), (len(GAINS), 1))
    gain = np.repeat(np.array(GAINS, np.uint16)[:, None], 256, axis=1)
    return img, gain


@pytest.mark.parametrize('name', ['identity', 'random', 'gamma'])
def test_the_ref_is_exact_rational_rounding(name):
    """floor(r g / 2^20 + 1/2), in Python's unbounded integers: (2 r g + 2^20) // 2^21, then the clip at 255."""
    tab = _tables()[name]
    img, gain = _sweep()
    got = pr.correct(img, tab, gain)
    for i, g in enumerate(GAINS):
        for p in range(256):
            want = min(255, (2 * int(tab[p]) * g + (1 << 20)) // (1 << 21))
            assert int(got[i, p]) == want, (name, g, p)
    assert int(pr.RESPONSE_MAX) * 65535 + (1 << 19) < 1 << 32          # the bound that lets a kernel work in 32 bits


def test_the_ref_is_within_one_level_of_the_float_model():
    """Against round(clip(U[p] / V)) in float64 with the unquantised tables.  With r = 256 U + e_r and g = 4096 / V + e_g, both errors at
    most 1/2 in magnitude, r g / 2^20 = U / V + e_r / (256 V) + U e_g / 4096 + e_r e_g / 2^20: for V >= 1/16 (the gain does not
    saturate) the three error terms are at most 0.5 / 16 + 255 * 0.5 / 4096 + 2^-22 = 0.03125 + 0.03113 + 0.0000003 < 0.07 grey levels
    ahead of the final rounding, so the two roundings differ by at most one level; and they agree wherever U / V is further than 0.07
    from a half."""
    rng = np.random.default_rng(11)
    u = np.sort(rng.uniform(0.0, 255.0, 256))
    h, w = 64, 256
    v = rng.uniform(1.0 / 16.0 + 1e-6, 1.0, (h, w))
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    got = pr.correct(img, pr.quantise_response(u), pr.quantise_vignette(v)).astype(np.int64)
    exact = u[img] / v
    want = np.clip(np.floor(exact + 0.5), 0, 255).astype(np.int64)
    diff = np.abs(got - want)
    assert diff.max() <= 1
    frac = np.abs(exact - np.floor(exact) - 0.5)
    assert (diff[(frac > 0.07) | (exact > 256)] == 0).all()
    assert (diff == 0).mean() > 0.9 and len(np.unique(got)) > 200          # (the comparison is not vacuous)


def test_identity_tables_give_the_identity():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    ident_r = (np.arange(256) * 256).astype(np.uint16)
    ident_g = np.full((16, 16), pr.GAIN_ONE, np.uint16)
    for r, g in ((ident_r, ident_g), (ident_r, None), (None, ident_g), (None, None)):
        assert np.array_equal(pr.correct(img, r, g), img)
    assert np.array_equal(pr.quantise_response(np.arange(256.0)), ident_r) and np.array_equal(pr.quantise_vignette(np.ones((16, 16))), ident_g)


def test_saturation_at_both_ends():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    top = np.full(256, pr.RESPONSE_MAX, np.uint16)
    assert (pr.correct(img, top, np.full((16, 16), 65535, np.uint16)) == 255).all()          # the largest product: no wrap
    assert (pr.correct(img, None, np.full((16, 16), 65535, np.uint16))[1:] == 255).all()     # 16 p >= 255 from p = 16 on, and p = 1 .. 15 give 16 p
    assert list(pr.correct(img, None, np.full((16, 16), 65535, np.uint16))[0, :4]) == [0, 16, 32, 48]
    assert (pr.correct(img, top, np.zeros((16, 16), np.uint16)) == 0).all()
    assert (pr.correct(img, np.zeros(256, np.uint16), np.full((16, 16), 65535, np.uint16)) == 0).all()
    assert pr.quantise_vignette(np.array([[0.0, -1.0, 1e-9, 1.0 / 16.0, 1.0]])).tolist() == [[65535, 65535, 65535, 65535, 4096]]
    assert pr.quantise_response(np.r_[-5.0, 300.0, np.zeros(254)])[:2].tolist() == [0, pr.RESPONSE_MAX]


def test_the_two_reduced_forms():
    """Only a response: (response[p] + 128) >> 8.  Only a gain: min(255, (p * gain + 2048) >> 12)."""
    tabs = _tables()
    img, gain = _sweep()
    for name in ('random', 'gamma'):
        assert np.array_equal(pr.correct(img, tabs[name], None), ((tabs[name][img].astype(np.int64) + 128) >> 8).astype(np.uint8)), name
    assert np.array_equal(pr.correct(img, None, gain), np.minimum(255, (img.astype(np.int64) * gain.astype(np.int64) + 2048) >> 12).astype(np.uint8))


def test_apply_vignette_then_correct_recovers_a_mid_grey_image_where_v_is_at_least_a_half():
    """The forward model rounds img * V to a grey level (error at most 1/2), the gain 1 / V <= 2 doubles that at most, and the tables add
    less than 0.07: |result - img| < 1.07 ahead of the final rounding, so at most one level.  The run shows exactly that: the largest
    difference is 1 (it is not 0: half of the information below V = 1 is lost in the 8-bit degraded frame)."""
    from uav_airvision_amd.frontend import apply_vignette, photometric_tables
    h, w = 120, 188
    v = pr.radial_vignette(w, h, 0.35)
    rng = np.random.default_rng(5)
    img = rng.integers(64, 193, (h, w), dtype=np.uint8)
    deg = apply_vignette(img, v)
    assert deg.dtype == np.uint8 and np.array_equal(deg, np.floor(img * v + 0.5).astype(np.uint8))
    _r, gain = photometric_tables(None, v)
    back = pr.correct(deg, None, gain).astype(np.int64)
    good = v >= 0.5
    assert 0.3 < good.mean() < 0.95
    diff = np.abs(back - img.astype(np.int64))
    assert diff[good].max() == 1
    assert np.abs(deg.astype(np.int64) - img)[good].max() > 40          # (the degradation was worth correcting)
    # the forward response as a callable and as a table
    fwd = apply_vignette(img, np.ones((h, w)), pr.gamma_forward(2.2))
    tab = apply_vignette(img, np.ones((h, w)), pr.gamma_forward(2.2)(np.arange(256.0)))
    assert np.array_equal(fwd, tab) and np.array_equal(fwd, np.floor(255.0 * (img / 255.0) ** (1 / 2.2) + 0.5).astype(np.uint8))


def test_the_package_quantisers_equal_the_refs():
    from uav_airvision_amd import frontend as F
    rng = np.random.default_rng(9)
    u = np.r_[rng.uniform(-3.0, 260.0, 250), 0.0, 255.0, 127.998046875, 127.998046874, 1.0 / 512.0, 254.9990234375]
    assert np.array_equal(F.quantise_response(u), pr.quantise_response(u))
    v = np.r_[rng.uniform(0.01, 1.0, 500), 0.0, -0.5, 1.0, 1.0 / 16.0, 0.0625001, 4096.0 / 4096.5, 4096.0 / 8190.5].reshape(39, 13)
    assert np.array_equal(F.quantise_vignette(v), pr.quantise_vignette(v))
    r, g = F.photometric_tables(u, v)
    assert r.dtype == np.uint16 and g.dtype == np.uint16 and np.array_equal(r, pr.quantise_response(u)) and np.array_equal(g, pr.quantise_vignette(v))
    assert F.photometric_tables() == (None, None) and F.photometric_tables(u)[1] is None and F.photometric_tables(None, v)[0] is None
    with pytest.raises(ValueError, match='256'):
        F.photometric_tables(np.zeros(255))
    with pytest.raises(ValueError, match='height, width'):
        F.photometric_tables(None, np.ones(7))


def test_the_file_readers(tmp_path):
    """A pcalib-style text file (256 numbers on one line) and a 16-bit grey PNG normalised by its maximum."""
    from PIL import Image
    from uav_airvision_amd import frontend as F
    u = pr.gamma_inverse_response(2.2)
    txt = tmp_path / 'pcalib.txt'
    txt.write_text(' '.join(repr(float(x)) for x in u) + '\n')
    v = pr.radial_vignette(94, 60, 0.35)
    png16 = np.floor(v * 60000.0 + 0.5).astype(np.uint16)
    Image.fromarray(png16).save(str(tmp_path / 'vignette.png'))
    r, g = F.photometric_tables(str(txt), str(tmp_path / 'vignette.png'))
    assert np.array_equal(r, pr.quantise_response(u))
    assert np.array_equal(g, pr.quantise_vignette(png16.astype(np.float64) / float(png16.max())))
    assert g.shape == (60, 94) and g.min() == 4096 and g.max() > 11000
    (tmp_path / 'short.txt').write_text('1 2 3\n')
    with pytest.raises(ValueError, match='256'):
        F.photometric_tables(str(tmp_path / 'short.txt'))
    Image.fromarray((v * 255).astype(np.uint8)).save(str(tmp_path / 'eight.png'))
    with pytest.raises(ValueError, match='16-bit grey'):
        F.photometric_tables(None, str(tmp_path / 'eight.png'))
    with pytest.raises(ValueError, match='vignette'):
        F.photometric_tables(None, str(tmp_path / 'missing.png'))


def test_write_euroc_layout_without_a_vignette_writes_what_it_wrote(tmp_path):
    """The optional argument changes nothing when it is absent, and degrades both cameras' files when it is given."""
    from PIL import Image
    from uav_airvision_amd.config import ConfigEuRoC
    from uav_airvision_amd.euroc import write_euroc_layout
    from uav_airvision_amd.frontend import apply_vignette
    from uav_airvision_amd.synth import SyntheticStream
    st = SyntheticStream(ConfigEuRoC(), seed=4, n_frames=1)
    m = st.frame(0)
    v0, v1 = pr.radial_vignette(752, 480, 0.35), pr.radial_vignette(752, 480, 0.5)
    write_euroc_layout(str(tmp_path / 'A'), st, compress_level=1)
    write_euroc_layout(str(tmp_path / 'B'), st, compress_level=1, vignette=(v0, v1, pr.gamma_forward(2.2)))
    name = '%d.png' % int(round(m.timestamp * 1e9))
    rd = lambda seq, cam: np.array(Image.open(str(tmp_path / seq / 'mav0' / cam / 'data' / name)))      # noqa: E731
    assert np.array_equal(rd('A', 'cam0'), m.cam0_image) and np.array_equal(rd('A', 'cam1'), m.cam1_image)
    assert np.array_equal(rd('B', 'cam0'), apply_vignette(m.cam0_image, v0, pr.gamma_forward(2.2)))
    assert np.array_equal(rd('B', 'cam1'), apply_vignette(m.cam1_image, v1, pr.gamma_forward(2.2)))
