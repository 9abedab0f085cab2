"""The packed 10 / 12-bit transports without a GPU: the NumPy reference (tests/packed_ref.py) against the contract's byte examples and
against the 16-bit and Bayer references, names and codes through every host layer, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import bayer_ref as br
import packed_ref as kr
import pixfmt_ref as pr
from uav_airvision_amd import _native as N
from uav_airvision_amd.config import ConfigEuRoC
from uav_airvision_amd.frontend import check_device_frames, check_host_frames, pack_frames, pack_frontend_config, unpack_frames

PAIR12 = np.array([[0xABC, 0x123]], np.uint16)
QUAD10 = np.array([[0x2A5, 0x13C, 0x3FF, 0x001]], np.uint16)
EXAMPLES = (('gray12p', PAIR12, 'bc3a12', [171, 18]), ('gray12_csi2', PAIR12, 'ab123c', [171, 18]),
            ('gray10p', QUAD10, 'a5f2f47f00', [169, 79, 255, 0]), ('gray10_csi2', QUAD10, 'a94fff0071', [169, 79, 255, 0]))


# ---- the reference ----

@pytest.mark.parametrize('fmt, v, text, s8', EXAMPLES)
def test_the_contracts_byte_examples(fmt, v, text, s8):
    raw = kr.pack(v, fmt)
    assert raw.tobytes().hex() == text and raw.shape == (1, len(text) // 2)
    assert np.array_equal(kr.unpack(np.frombuffer(bytes.fromhex(text), np.uint8)[None], fmt), v)
    assert kr.to_gray8(raw, fmt, 8)[0].tolist() == s8
    assert np.array_equal(pack_frames(v, fmt), raw) and np.array_equal(unpack_frames(raw, fmt), v)      # the package's own helpers


def test_shift_6_on_the_12_bit_pair():
    for fmt in ('gray12p', 'gray12_csi2'):
        assert kr.to_gray8(kr.pack(PAIR12, fmt), fmt, 6)[0].tolist() == [255, 72]


@pytest.mark.parametrize('fmt', kr.GREY)
def test_unpack_inverts_pack_and_the_package_agrees(fmt):
    rng = np.random.default_rng(41)
    d = kr.depth(fmt)
    v = rng.integers(0, 1 << d, (3, 7, 24), dtype=np.uint16)
    v[0, 0, :4] = [0, 1, (1 << d) - 1, 1 << (d - 1)]
    raw = kr.pack(v, fmt)
    assert raw.dtype == np.uint8 and raw.shape == (3, 7, 24 * d // 8)
    assert np.array_equal(kr.unpack(raw, fmt), v)
    assert np.array_equal(pack_frames(v, fmt), raw) and np.array_equal(unpack_frames(raw, fmt), v)
    assert np.array_equal(pack_frames(v, N.PACKED_FORMATS[fmt]), raw)                                    # by code as well


@pytest.mark.parametrize('fmt', kr.GREY)
def test_the_value_rule_is_gray16_on_the_left_justified_sample(fmt):
    rng = np.random.default_rng(42)
    d = kr.depth(fmt)
    v = rng.integers(0, 1 << d, (2, 9, 36), dtype=np.uint16)
    raw = kr.pack(v, fmt)
    for shift in (0, 4, 6, 8):
        want = pr.to_gray8((v.astype(np.uint32) << (16 - d)).astype(np.uint16), 'gray16', shift)
        assert np.array_equal(kr.to_gray8(raw, fmt, shift), want), shift
    assert (kr.to_gray8(raw, fmt, 0) == 255).sum() > v.size // 2                                          # shift 0 saturates most of it
    assert np.array_equal(kr.to_gray8(raw, fmt), v >> (d - 8))                                            # the default: the top eight bits
    with pytest.raises(ValueError, match='shift'):
        kr.to_gray8(raw, fmt, 9)


@pytest.mark.parametrize('fmt', ['bayer_rggb10p', 'bayer_bggr12p', 'bayer_grbg10_csi2', 'bayer_gbrg12_csi2'])
def test_a_packed_mosaic_is_the_8_bit_mosaic_of_its_reduced_samples(fmt):
    rng = np.random.default_rng(43)
    raw = kr.random_frames(rng, fmt, (2, 6, 12))
    for shift in (4, 8):
        s = kr.reduce8(raw, fmt, shift)
        assert np.array_equal(kr.to_gray8(raw, fmt, shift), br.to_gray8(s, 'bayer_%s8' % fmt[6:10]))
    # the same as the 16-bit mosaic of the left-justified samples
    v16 = (kr.unpack(raw, fmt).astype(np.uint32) << (16 - kr.depth(fmt))).astype(np.uint16)
    assert np.array_equal(kr.to_gray8(raw, fmt, 6), br.to_gray8(v16, 'bayer_%s16' % fmt[6:10], 6))


# ---- names, codes, sizes ----

def test_every_name_maps_to_its_code_and_back():
    assert len(kr.FORMATS) == 20 and N.PACKED_FORMATS == kr.CODES
    assert [kr.CODES[f] for f in kr.GREY] == [32, 33, 34, 35]
    assert (N.AV_PIX_GRAY10P, N.AV_PIX_GRAY12P, N.AV_PIX_GRAY10_CSI2, N.AV_PIX_GRAY12_CSI2) == (32, 33, 34, 35)
    assert [kr.CODES['bayer_%s%s' % (p, k)] for k in kr.PACKINGS for p in br.PATTERNS] == list(range(40, 56))
    cfg = ConfigEuRoC()
    for f, c in kr.CODES.items():
        assert N.pixel_format_code(f) == c == N.pixel_format_code(c) and N.PIXEL_FORMAT_NAMES[c] == f
        assert N.is_packed(c) and N.packed_depth(c) == kr.depth(f) and not N.is_16bit(c)
        assert N.is_bayer(c) == f.startswith('bayer') and (not N.is_bayer(c) or N.BAYER_PATTERNS[c & 3] == f[6:10])
        cfg.image_format = f
        assert pack_frontend_config(cfg).pixel_format == c
    for c in list(range(6)) + list(range(16, 24)):
        assert not N.is_packed(c) and N.packed_depth(c) == 0
    assert N.is_bayer(16) and N.is_bayer(23) and not N.is_bayer(1) and N.is_16bit(1) and N.is_16bit(20)


@pytest.mark.parametrize('code', [6, 15, 24, 31, 36, 39, 56])
def test_the_codes_between_and_beyond_stay_unknown(code):
    with pytest.raises(ValueError, match='format'):
        N.pixel_format_code(code)
    assert not N.is_packed(code) and not N.is_bayer(code) and N.frame_bytes(code, 752, 480) == 0
    # av_to_gray8: refused for the format before any pointer is looked at
    assert N.lib().av_to_gray8(None, 0, 1, 8, 8, code, 8, None, 0, None) == N.AV_E_INVALID
    assert b'pixel format' in N.lib().av_last_error()
    c = pack_frontend_config(ConfigEuRoC())
    c.pixel_format = code
    h = C.c_void_p()
    assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID
    assert b'pixel format' in N.lib().av_last_error()


def test_frame_bytes():
    for f, c in kr.CODES.items():
        d = kr.depth(f)
        for (w, h) in ((4, 1), (36, 5), (752, 480), (4096, 4096)):
            assert N.frame_bytes(c, w, h) == w * h * d // 8 == N.lib().av_pixfmt_frame_bytes(c, w, h), (f, w, h)
        assert N.frame_bytes(c, 6, 4) == (0 if d == 10 else 36) and N.frame_bytes(c, 7, 4) == 0
        assert N.frame_bytes(c, 0, 4) == 0 and N.frame_bytes(c, 4, -1) == 0
    assert [N.frame_bytes(c, 10, 3) for c in (0, 1, 2, 3, 4, 5, 16, 20)] == [30, 60, 90, 90, 120, 120, 30, 60]      # the unpacked formats: w h bytes-per-pixel
    assert N.frame_bytes(-1, 8, 8) == 0


def test_engine_creation_refuses_a_ragged_width_by_name_before_a_device_is_touched():
    """750 is a multiple of 2 but not of 4: refused for gray10p (AV_E_INVALID, the text names the format), while gray12p passes the
    check -- a machine without a GPU then answers AV_E_NODEVICE, one with a GPU creates the engine."""
    cfg = ConfigEuRoC()
    cfg.cam0_resolution = cfg.cam1_resolution = np.array([750, 480])
    cfg.image_format = 'gray10p'
    c = pack_frontend_config(cfg)
    h = C.c_void_p()
    assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID
    err = N.lib().av_last_error()
    assert b'gray10p' in err and b'750' in err and not h.value
    c.pixel_format = N.AV_PIX_BAYER_RGGB10P + 2
    assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID and b'bayer_grbg10p' in N.lib().av_last_error()
    c.pixel_format = N.AV_PIX_GRAY12P
    rc = N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h))
    assert rc in (N.AV_OK, N.AV_E_NODEVICE)
    if rc == N.AV_OK:
        N.lib().av_frontend_destroy(h)
    c.gray16_shift = 9                                           # a packed code with a bad shift is refused for the shift: the format check knows the code
    assert N.lib().av_frontend_create(C.byref(c), 1, 0, C.byref(h)) == N.AV_E_INVALID
    assert b'shift' in N.lib().av_last_error() and b'pixel format' not in N.lib().av_last_error()


# ---- host layers ----

def test_pack_frames_refuses_over_range_values_and_ragged_widths():
    with pytest.raises(ValueError, match=r'gray10p.*1024'):
        pack_frames(np.array([[0, 1, 2, 1024]], np.uint16), 'gray10p')
    with pytest.raises(ValueError, match=r'gray12_csi2.*4096'):
        pack_frames(np.array([[4096, 1]], np.uint16), 'gray12_csi2')
    assert pack_frames(np.array([[0, 1, 2, 1023]], np.uint16), 'gray10p').shape == (1, 5)
    with pytest.raises(ValueError, match=r'gray10p.*width 6'):
        pack_frames(np.zeros((2, 6), np.uint16), 'gray10p')
    with pytest.raises(ValueError, match=r'gray12p.*width 3'):
        pack_frames(np.zeros((2, 3), np.uint16), 'gray12p')
    with pytest.raises(ValueError, match='uint16'):
        pack_frames(np.zeros((2, 4), np.uint8), 'gray12p')
    with pytest.raises(ValueError, match='no packed format'):
        pack_frames(np.zeros((2, 4), np.uint16), 'gray16')
    with pytest.raises(ValueError, match=r'gray10p.*5-byte'):
        unpack_frames(np.zeros((2, 6), np.uint8), 'gray10p')


def test_frame_checks_name_the_format_and_both_shapes():
    import torch
    h, w = 6, 8
    assert check_host_frames('x', np.zeros((2, h, 12), np.uint8), N.AV_PIX_GRAY12P, 2, h, w).shape == (2, h, 12)
    assert check_host_frames('x', np.zeros((h, 10), np.uint8), N.AV_PIX_GRAY10_CSI2, 1, h, w).shape == (1, h, 10)
    for arr, fmt in ((np.zeros((2, h, w), np.uint16), N.AV_PIX_GRAY12P), (np.zeros((2, h, w), np.uint8), N.AV_PIX_GRAY12P),
                     (np.zeros((2, h, 12), np.uint8), N.AV_PIX_GRAY10P), (np.zeros((2, h, 12), np.uint16), N.AV_PIX_BAYER_RGGB12P)):
        with pytest.raises(ValueError) as e:
            check_host_frames('step_host: img0', arr, fmt, 2, h, w)
        msg = str(e.value)
        want = (2, h, w * N.packed_depth(fmt) // 8)
        assert N.PIXEL_FORMAT_NAMES[fmt] in msg and 'uint8' in msg and str(want) in msg and str(arr.dtype) in msg and str(tuple(arr.shape)) in msg
    with pytest.raises(ValueError, match=r'gray12p.*uint8'):
        check_host_frames('step_host: img0', np.zeros((2, h, w), np.uint16), N.AV_PIX_GRAY12P, 2, h, w)
    with pytest.raises(ValueError) as e:
        check_device_frames('step: img1', torch.zeros((2, h, w), dtype=torch.int16), N.AV_PIX_GRAY12P, 2, h, w)
    assert 'gray12p' in str(e.value) and str((2, h, 12)) in str(e.value) and str((2, h, w)) in str(e.value)
    with pytest.raises(ValueError, match='cuda'):                                     # right dtype and shape, but host memory
        check_device_frames('step: img0', torch.zeros((2, h, 12), dtype=torch.uint8), N.AV_PIX_GRAY12P, 2, h, w)
    with pytest.raises(ValueError, match=r'gray10p.*width 6'):                        # a width the format cannot have
        check_host_frames('x', np.zeros((1, h, 7), np.uint8), N.AV_PIX_GRAY10P, 1, h, 6)


def test_the_png_decoder_refuses_a_packed_code_and_never_probes_one(tmp_path):
    out = np.zeros((1, 4, 6), np.uint8)
    paths = (C.c_char_p * 1)(b'nowhere.png')
    status = (C.c_int32 * 1)()
    for code in (33, 32, 44):
        assert N.lib().av_png_decode(paths, 1, 4, 4, code, out.ctypes.data_as(C.c_void_p), out.nbytes, 1, status) == N.AV_E_INVALID
        assert b'no PNG flavour' in N.lib().av_last_error()
    from PIL import Image
    from uav_airvision_amd.euroc import probe_png
    for k, arr in enumerate((np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint16), np.zeros((4, 6, 3), np.uint8))):
        p = str(tmp_path / ('%d.png' % k))
        Image.fromarray(arr).save(p)
        assert probe_png(p)[2] in ('gray8', 'gray16', 'rgb8')


def test_the_euroc_layers_refuse_packed_names_and_say_why(tmp_path):
    from uav_airvision_amd.euroc import FrameStager, SharedFrameStager, encode_frame, frame_array, png_pixel_format, write_euroc_layout
    for f in ('gray12p', 'bayer_rggb10_csi2', N.AV_PIX_GRAY10P):
        for call in (lambda: frame_array(f, 1, 4, 8), lambda: png_pixel_format(f), lambda: encode_frame(np.zeros((4, 8), np.uint8), f),
                     lambda: FrameStager([], 4, 8, pixel_format=f), lambda: SharedFrameStager(None, 4, 8, pixel_format=f)):
            with pytest.raises(ValueError, match='packed transport, which no PNG file holds'):
                call()
    with pytest.raises(ValueError, match=r'gray12p is a packed transport'):
        write_euroc_layout(str(tmp_path / 'SEQ'), None, pixel_format='gray12p')


def test_the_sweep_does_not_offer_packed_formats():
    from uav_airvision_amd.sweep import make_parser
    ap = make_parser()
    for f in ('gray12p', 'gray10_csi2', 'bayer_rggb12p'):
        with pytest.raises(SystemExit):
            ap.parse_args(['--sequences', 'X', '--pixel-format', f])
    assert ap.parse_args(['--sequences', 'X', '--pixel-format', 'gray16']).pixel_format == 'gray16'


def test_to_gray8_refuses_wrong_packed_arrays_before_a_device_is_needed():
    import torch
    from uav_airvision_amd import ops
    with pytest.raises(ValueError, match=r'gray12p.*uint8'):
        ops.to_gray8(torch.zeros((2, 4, 6), dtype=torch.int16), 'gray12p')
    with pytest.raises(ValueError, match=r'gray10p.*5-byte'):
        ops.to_gray8(torch.zeros((2, 4, 6), dtype=torch.uint8), 'gray10p')
    with pytest.raises(ValueError, match='2 x 2'):
        ops.to_gray8(torch.zeros((1, 6), dtype=torch.uint8), 'bayer_rggb12p')
