"""tests/photometric_ref.py -- the photometric calibration of include/airvision.h ("Photometric calibration") in NumPy: the definition
the kernels of csrc/photometric.hip are held to bit for bit, and the two quantisers restated independently of
uav_airvision_amd/frontend.py.  Integers only past the quantisers."""
import numpy as np

RESPONSE_MAX = 65280          # 255 in Q8: the largest response entry (65280 * 65535 + 2^19 < 2^32)
GAIN_ONE = 4096               # 1.0 in Q12


def correct(img_u8, response_u16=None, gain_u16=None):
    """out = min(255, (response[p] * gain[x] + (1 << 19)) >> 20); response absent: p * 256, gain absent: 4096.  img uint8 [..., h, w],
    response uint16[256], gain uint16 [h, w] (broadcast over the leading dimensions)."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8
    if response_u16 is None:
        r = img.astype(np.uint64) * np.uint64(256)
    else:
        tab = np.asarray(response_u16)
        assert tab.dtype == np.uint16 and tab.shape == (256,) and int(tab.max()) <= RESPONSE_MAX
        r = tab[img].astype(np.uint64)
    if gain_u16 is None:
        g = np.uint64(GAIN_ONE)
    else:
        g = np.asarray(gain_u16)
        assert g.dtype == np.uint16 and g.shape == img.shape[-2:]
        g = g.astype(np.uint64)
    return np.minimum(np.uint64(255), (r * g + np.uint64(1 << 19)) >> np.uint64(20)).astype(np.uint8)


def quantise_response(u):
    """256 floats in [0, 255] -> Q8: floor(clip(U, 0, 255) * 256 + 0.5), float64."""
    out = []
    for v in np.asarray(u, np.float64).reshape(256):
        v = min(255.0, max(0.0, float(v)))
        out.append(int(np.floor(v * 256.0 + 0.5)))
    return np.array(out, np.uint16)


def quantise_vignette(v):
    """V in (0, 1] -> Q12 gain: min(65535, floor(4096 / V + 0.5)), float64; V <= 0 gives 65535."""
    v = np.asarray(v, np.float64)
    pos = v > 0
    g = np.floor(4096.0 / np.where(pos, v, 1.0) + 0.5)
    return np.where(pos & (g < 65535.0), g, 65535.0).astype(np.uint16)


def radial_vignette(w, h, corner=0.35):
    """A cos^4-style radial fall-off: V = cos(theta)^4 with theta growing linearly with the distance from the image centre, 1 at the
    centre and `corner` at the corners.  float64 [h, w]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    r = np.hypot(x - cx, y - cy) / np.hypot(cx, cy)
    return np.cos(r * np.arccos(corner ** 0.25)) ** 4


def gamma_inverse_response(gamma):
    """G^-1 of a sensor with the forward response G(e) = 255 (e / 255)^(1 / gamma): U[p] = 255 (p / 255)^gamma, 256 floats."""
    return 255.0 * (np.arange(256.0) / 255.0) ** float(gamma)


def gamma_forward(gamma):
    """The forward response that goes with gamma_inverse_response, as a callable on irradiance in [0, 255]."""
    return lambda e: 255.0 * (np.clip(e, 0.0, 255.0) / 255.0) ** (1.0 / float(gamma))
