"""ctypes binding of libairvision_hip.so (the C ABI declared in include/airvision.h).

There is NO CPU fallback: if the shared library is missing this module raises, and every operator
raises when the HIP call fails.  torch is imported first so that the library binds to the HIP
runtime torch already loaded (same SONAME), i.e. one runtime / one context per process.
"""
import ctypes as C
import numbers
import os

import torch  # noqa: F401  (must be loaded before libairvision_hip.so, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libairvision_hip.so')

AV_MAX_LEVELS = 5
AV_PYR_BORDER = 16
AV_MAX_IMAGE_PIXELS = 1 << 24
AV_OK, AV_E_INVALID, AV_E_HIP, AV_E_CAPACITY, AV_E_NODEVICE, AV_E_NUMERIC = 0, -1, -2, -3, -4, -5
AV_FE_INPUTS_PERSIST = 1
AV_FE_RANSAC = 2
AV_FE_CLAHE = 4
AV_FE_PHOTOMETRIC = 8
AV_FE_EXPOSURE = 16
AV_PHOTOMETRIC_RESPONSE_MAX = 65280
AV_CLAHE_MAX_TILES = 16
AV_GRAY16_SHIFT, AV_GRAY16_WINDOW, AV_GRAY16_AUTO = 0, 1, 2
GRAY16_SCALES = {'shift': AV_GRAY16_SHIFT, 'window': AV_GRAY16_WINDOW, 'auto': AV_GRAY16_AUTO}      # config.gray16_scale
AV_GRAY16_MAX_CLIP_PPM = 500000
AV_GRAY16_WORK_WORDS = 4100
AV_PIX_GRAY8, AV_PIX_GRAY16, AV_PIX_RGB8, AV_PIX_BGR8, AV_PIX_RGBA8, AV_PIX_BGRA8 = 0, 1, 2, 3, 4, 5
AV_PIX_BAYER_RGGB8, AV_PIX_BAYER_BGGR8, AV_PIX_BAYER_GRBG8, AV_PIX_BAYER_GBRG8 = 16, 17, 18, 19
AV_PIX_BAYER_RGGB16, AV_PIX_BAYER_BGGR16, AV_PIX_BAYER_GRBG16, AV_PIX_BAYER_GBRG16 = 20, 21, 22, 23
AV_PIX_GRAY10P, AV_PIX_GRAY12P, AV_PIX_GRAY10_CSI2, AV_PIX_GRAY12_CSI2 = 32, 33, 34, 35
AV_PIX_BAYER_RGGB10P, AV_PIX_BAYER_RGGB12P, AV_PIX_BAYER_RGGB10_CSI2, AV_PIX_BAYER_RGGB12_CSI2 = 40, 44, 48, 52      # + pattern (rggb, bggr, grbg, gbrg)
AV_RANSAC_MAX_PAIRS = 1920
AV_RANSAC_MAX_HYPOTHESES = 64
AV_RANSAC_PATH_FEW, AV_RANSAC_PATH_STILL, AV_RANSAC_PATH_MODEL, AV_RANSAC_PATH_NONE = 1, 2, 4, 8


PIXEL_FORMATS = {'gray8': 0, 'gray16': 1, 'rgb8': 2, 'bgr8': 3, 'rgba8': 4, 'bgra8': 5,      # config.image_format -> AV_PIX_* (include/airvision.h)
                 # Bayer mosaics, named by the colours of the top-left 2 x 2 block in reading order (not OpenCV's BayerBG .. names)
                 'bayer_rggb8': 16, 'bayer_bggr8': 17, 'bayer_grbg8': 18, 'bayer_gbrg8': 19,
                 'bayer_rggb16': 20, 'bayer_bggr16': 21, 'bayer_grbg16': 22, 'bayer_gbrg16': 23}
BAYER_PATTERNS = ('rggb', 'bggr', 'grbg', 'gbrg')             # pattern of code c: BAYER_PATTERNS[(c - 16) & 3] = BAYER_PATTERNS[c & 3]
# Packed 10 / 12-bit transports (PFNC Mono10p / Mono12p, MIPI CSI-2 RAW10 / RAW12): a table of their own, because a frame of one is a
# byte array with no whole number of bytes per pixel -- PIXEL_FORMATS and PIXEL_BYTES stay the formats that have one array element per
# sample.  pixel_format_code and PIXEL_FORMAT_NAMES know both tables; frame_bytes sizes a frame of either.
PACKINGS = ('10p', '12p', '10_csi2', '12_csi2')               # grey: 32 + k; mosaics: 40 + 4 k + pattern
PACKED_FORMATS = dict([('gray' + k, 32 + i) for i, k in enumerate(PACKINGS)] +
                      [('bayer_%s%s' % (p, k), 40 + 4 * i + j) for i, k in enumerate(PACKINGS) for j, p in enumerate(BAYER_PATTERNS)])
PIXEL_FORMAT_NAMES = {v: k for k, v in list(PIXEL_FORMATS.items()) + list(PACKED_FORMATS.items())}
PIXEL_BYTES = {0: 1, 1: 2, 2: 3, 3: 3, 4: 4, 5: 4, 16: 1, 17: 1, 18: 1, 19: 1, 20: 2, 21: 2, 22: 2, 23: 2}


def is_packed(fmt):
    """An AV_PIX_* code names a packed 10 / 12-bit transport (grey or mosaic): its frames are uint8 [n, h, w * d / 8]."""
    return AV_PIX_GRAY10P <= fmt <= AV_PIX_GRAY12_CSI2 or AV_PIX_BAYER_RGGB10P <= fmt <= AV_PIX_BAYER_RGGB12_CSI2 + 3


def packed_depth(fmt):
    """Bits per sample of a packed format, 10 or 12; 0 for any other code."""
    if not is_packed(fmt):
        return 0
    return 12 if ((fmt - 32) if fmt < 40 else (fmt - 40) >> 2) & 1 else 10


def packing(fmt):
    """'10p' | '12p' | '10_csi2' | '12_csi2' of a packed format."""
    if not is_packed(fmt):
        raise ValueError('%r is no packed format' % (fmt,))
    return PACKINGS[(fmt - 32) if fmt < 40 else (fmt - 40) >> 2]


def packed_group(fmt):
    """(samples, bytes) of one group of a packed format: (4, 5) at 10 bits, (2, 3) at 12."""
    return (4, 5) if packed_depth(fmt) == 10 else (2, 3)


def frame_bytes(fmt, w, h):
    """Bytes of one tightly packed w x h frame of an AV_PIX_* code (av_pixfmt_frame_bytes): w * h * bytes per pixel, w * h * d / 8 for
    a packed format; 0 for an unknown code and for a packed width that is not whole groups (4 samples at 10 bits, 2 at 12)."""
    return int(lib().av_pixfmt_frame_bytes(int(fmt), int(w), int(h)))


def packed_row_bytes(fmt, width):
    """Bytes of one row of a packed format; ValueError, naming the format, for a width that is not whole groups."""
    gpx, gb = packed_group(fmt)
    if not is_packed(fmt) or width <= 0 or width % gpx:
        raise ValueError('%s: a row is whole groups of %d samples, width %d is not' % (PIXEL_FORMAT_NAMES.get(fmt, fmt), gpx, width))
    return width // gpx * gb


def is_bayer(fmt):
    """An AV_PIX_* code names a Bayer mosaic, packed or not."""
    return AV_PIX_BAYER_RGGB8 <= fmt <= AV_PIX_BAYER_GBRG16 or AV_PIX_BAYER_RGGB10P <= fmt <= AV_PIX_BAYER_RGGB12_CSI2 + 3


def is_16bit(fmt):
    """An AV_PIX_* code whose frames are uint16 arrays (gray16 and the 16-bit mosaics).  The packed formats read gray16_shift too, but
    their frames are uint8 arrays: is_packed."""
    return fmt == AV_PIX_GRAY16 or AV_PIX_BAYER_RGGB16 <= fmt <= AV_PIX_BAYER_GBRG16


def pixel_format_code(name):
    """config.image_format ('gray8', 'gray16', 'rgb8', 'bgr8', 'rgba8', 'bgra8', 'bayer_{rggb,bggr,grbg,gbrg}{8,16}', 'gray{10p,12p,10_csi2,
    12_csi2}', 'bayer_{rggb,bggr,grbg,gbrg}{10p,12p,10_csi2,12_csi2}') or an AV_PIX_* code -> AV_PIX_*; ValueError otherwise."""
    if isinstance(name, str) and name in PIXEL_FORMATS:
        return PIXEL_FORMATS[name]
    if isinstance(name, str) and name in PACKED_FORMATS:
        return PACKED_FORMATS[name]
    if isinstance(name, int) and not isinstance(name, bool) and name in PIXEL_FORMAT_NAMES:
        return name
    raise ValueError('unknown image format %r (one of %s)' % (name, ', '.join(PIXEL_FORMAT_NAMES[c] for c in sorted(PIXEL_FORMAT_NAMES))))


def gray16_shift_value(shift):
    """config.gray16_shift -> int in 0 .. 8; ValueError otherwise."""
    if isinstance(shift, bool) or int(shift) != shift or not 0 <= int(shift) <= 8:
        raise ValueError('gray16_shift %r outside 0 .. 8' % (shift,))
    return int(shift)


def _int_in(v, lo, hi):
    return not isinstance(v, bool) and isinstance(v, numbers.Real) and int(v) == v and lo <= int(v) <= hi


def gray16_range_settings(scale='shift', window=None, clip=(100, 100), min_span=256):
    """config.gray16_scale / gray16_window / gray16_auto_clip / gray16_auto_min_span -> (mode, lo, hi, ppm_lo, ppm_hi, min_span) as the
    C ABI takes them ("Range scaling of 16-bit grey" in include/airvision.h); ValueError, naming the setting, for a scale that is none of
    'shift', 'window', 'auto', and for what the chosen scale reads: a window that does not satisfy 0 <= lo < hi <= 65535, a clip that is
    not two integers >= 0 with a sum of at most 500000 ppm, a minimum span outside 16 .. 65535.  What a scale does not read is carried as
    its default and not checked."""
    if scale not in GRAY16_SCALES:
        raise ValueError("gray16_scale %r is none of 'shift', 'window', 'auto'" % (scale,))
    mode, lo, hi, ppm, span = GRAY16_SCALES[scale], 0, 65535, (100, 100), 256
    if mode == AV_GRAY16_WINDOW:
        try:
            lo, hi = window
        except (TypeError, ValueError):
            raise ValueError("gray16_scale 'window' needs gray16_window = (lo, hi), got %r" % (window,))
        if not (_int_in(lo, 0, 65535) and _int_in(hi, 0, 65535) and lo < hi):
            raise ValueError('gray16_window %r does not satisfy 0 <= lo < hi <= 65535' % (window,))
    if mode == AV_GRAY16_AUTO:
        try:
            ppm = tuple(clip)
        except TypeError:
            ppm = ()
        if len(ppm) != 2 or not all(_int_in(v, 0, AV_GRAY16_MAX_CLIP_PPM) for v in ppm) or sum(ppm) > AV_GRAY16_MAX_CLIP_PPM:
            raise ValueError('gray16_auto_clip %r: two integers >= 0 in parts per million whose sum is at most %d' % (clip, AV_GRAY16_MAX_CLIP_PPM))
        if not _int_in(min_span, 16, 65535):
            raise ValueError('gray16_auto_min_span %r outside 16 .. 65535' % (min_span,))
        span = min_span
    return mode, int(lo), int(hi), int(ppm[0]), int(ppm[1]), int(span)


def downscale_value(factor):
    """config.image_downscale -> 1, 2 or 4; ValueError otherwise (bool, 0, fractions, other factors)."""
    if isinstance(factor, bool) or not isinstance(factor, numbers.Real) or int(factor) != factor or int(factor) not in (1, 2, 4):
        raise ValueError('image_downscale %r is none of 1, 2, 4' % (factor,))
    return int(factor)


DISTORTION_MODELS = {'radtan': 0, 'equidistant': 1}          # AV_DISTORTION_* (include/airvision.h)


def distortion_model_code(name):
    """'radtan' / 'equidistant' (config.py:98,117; camera_model.py:41,69: anything but 'equidistant' is radtan there) -> AV_DISTORTION_*."""
    return 1 if name == 'equidistant' else 0


class AirvisionError(RuntimeError):
    def __init__(self, code, text):
        RuntimeError.__init__(self, 'libairvision_hip error %d: %s' % (code, text))
        self.code = code


class PyrLayout(C.Structure):
    _fields_ = [('levels', C.c_int32),
                ('w', C.c_int32 * AV_MAX_LEVELS), ('h', C.c_int32 * AV_MAX_LEVELS),
                ('pitch', C.c_int32 * AV_MAX_LEVELS),
                ('offset', C.c_int64 * AV_MAX_LEVELS),
                ('bytes', C.c_int64)]


class Landmark(C.Structure):                     # av_landmark (AV_LANDMARK_BYTES = 40)
    _fields_ = [('id', C.c_int64), ('p', C.c_double * 3), ('flags', C.c_int32), ('n_obs', C.c_int32)]


class ImuState(C.Structure):                     # av_imu_state (AV_IMU_STATE_BYTES = 112)
    _fields_ = [('t', C.c_double), ('p', C.c_double * 3), ('q', C.c_double * 4), ('v', C.c_double * 3), ('w', C.c_double * 3)]


class UpdateStats(C.Structure):                  # av_update_stats (64 bytes)
    _fields_ = [(n, C.c_int32) for n in ('n_cand', 'n_pos', 'n_eval', 'n_pass', 'dof_eval', 'dof_pass', 'rows', 'flags')] + \
               [(n, C.c_double) for n in ('gamma_eval', 'gamma_pass', 'dx_pos', 'dx_rot')]


class FilterStats(C.Structure):                  # av_filter_stats (AV_FILTER_STATS_BYTES = 128)
    _fields_ = [('upd', UpdateStats * 2)]


class Zupt(C.Structure):                         # av_zupt (AV_ZUPT_BYTES = 64)
    _fields_ = [(n, C.c_int32) for n in ('flags', 'n_imu', 'n_tracked', 'n_still', 'detected_total', 'applied_total')] + \
               [(n, C.c_double) for n in ('w_max', 'a_dev_max', 'v_norm', 'gamma', 'dx_pos')]


class ZuptParams(C.Structure):                   # av_zupt_params
    _fields_ = [(n, C.c_double) for n in ('gyro_max', 'acc_dev_max', 'disparity_max', 'velocity_sigma', 'gate')] + \
               [('min_tracks', C.c_int32), ('still_percent', C.c_int32)]


class FrontendConfig(C.Structure):
    _fields_ = [('width', C.c_int32), ('height', C.c_int32),
                ('grid_row', C.c_int32), ('grid_col', C.c_int32),
                ('grid_min_feature_num', C.c_int32), ('grid_max_feature_num', C.c_int32),
                ('fast_threshold', C.c_int32), ('lk_win', C.c_int32), ('lk_levels', C.c_int32),
                ('lk_max_iter', C.c_int32), ('max_corners', C.c_int32), ('flags', C.c_int32),
                ('lk_eps', C.c_double), ('lk_min_eig', C.c_double), ('stereo_threshold', C.c_double),
                ('cam0_intrinsics', C.c_double * 4), ('cam0_distortion', C.c_double * 4),
                ('cam1_intrinsics', C.c_double * 4), ('cam1_distortion', C.c_double * 4),
                ('R_cam0_imu', C.c_double * 9), ('R_cam1_imu', C.c_double * 9),
                ('R0to1', C.c_double * 9), ('E', C.c_double * 9), ('norm_unit', C.c_double),
                ('cam0_distortion_model', C.c_int32), ('cam1_distortion_model', C.c_int32),
                ('ransac_threshold', C.c_double), ('ransac_success_probability', C.c_double),
                ('ransac_seed', C.c_uint32), ('reserved0', C.c_int32),
                ('clahe_clip_limit', C.c_double), ('clahe_tiles_x', C.c_int32), ('clahe_tiles_y', C.c_int32),
                ('pixel_format', C.c_int32), ('gray16_shift', C.c_int32),
                ('image_downscale', C.c_int32), ('reserved1', C.c_int32)]


# name -> (restype, argtypes); the list doubles as the export check of tests/test_abi.py
_P = C.c_void_p
SIGNATURES = {
    'av_last_error': (C.c_char_p, []),
    'av_version': (C.c_char_p, []),
    'av_device_count': (C.c_int, []),
    'av_pyramid_layout': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(PyrLayout)]),
    'av_pyramid_build': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    'av_pyramid_build_levels': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    'av_lk_track': (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int,
                              C.c_int, C.c_int, C.c_double, C.c_double, _P]),
    'av_lk_track_images': (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int,
                                     C.c_int, C.c_int, C.c_double, C.c_double, _P]),
    'av_fast_detect': (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    'av_fast_detect_wide': (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P]),
    'av_undistort_points': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P]),
    'av_distort_points': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P]),
    'av_undistort_points_model': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, _P, _P]),
    'av_distort_points_model': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, _P, _P]),
    'av_frontend_create': (C.c_int, [C.POINTER(FrontendConfig), C.c_int, C.c_int, C.POINTER(_P)]),
    'av_frontend_destroy': (None, [_P]),
    'av_frontend_push_imu': (C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    'av_frontend_push_imu_batch': (C.c_int, [_P, _P, _P, _P, C.c_int]),
    'av_frontend_step': (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P]),
    'av_frontend_prestage': (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    'av_frontend_step_host': (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P]),
    'av_frontend_frames_reserve': (C.c_int, [_P, C.c_int]),
    'av_frontend_frames_upload': (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int64, _P]),
    'av_frontend_step_frames': (C.c_int, [_P, _P, C.POINTER(C.c_double), _P]),
    'av_frontend_max_features': (C.c_int, [_P]),
    'av_frontend_read_features': (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    'av_frontend_read_features_begin': (C.c_int, [_P, C.c_int, _P]),
    'av_frontend_features_dev': (C.c_int, [_P, _P, _P, _P, _P]),
    'av_frontend_read_features_end': (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    'av_frontend_read_grid': (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _P]),
    'av_frontend_read_counters': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32 * 8), _P]),
    'av_frontend_read_match_counts': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32 * 2), _P]),
    'av_msckf_create': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(_P)]),
    'av_msckf_destroy': (None, [_P]),
    'av_msckf_ld': (C.c_int, [_P]),
    'av_msckf_dim': (C.c_int, [_P]),
    'av_msckf_set_cov': (C.c_int, [_P, _P, C.c_int, _P]),
    'av_msckf_get_cov': (C.c_int, [_P, _P, C.c_int, _P]),
    'av_msckf_propagate': (C.c_int, [_P, C.c_double] + [C.POINTER(C.c_double)] * 11 + [_P]),
    'av_msckf_augment': (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    'av_msckf_remove_cam': (C.c_int, [_P, C.c_int, _P]),
    'av_msckf_triangulate': (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, _P, _P, _P]),
    'av_msckf_feature_blocks': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, _P, _P, _P]),
    'av_msckf_read_blocks': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    'av_msckf_update': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P]),
    'av_msckf_batch_create': (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 6 + [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(_P)]),
    'av_msckf_batch_destroy': (None, [_P]),
    'av_msckf_batch_push_imu': (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    'av_msckf_batch_step': (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P]),
    'av_msckf_batch_submit': (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P]),
    'av_msckf_batch_device_resident': (C.c_int, [_P]),
    'av_msckf_batch_submit_dev': (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    'av_msckf_batch_wait': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_get_cov': (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    'av_msckf_batch_set_odom_cov': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_next_odom_cov': (C.c_int, [_P, _P]),
    'av_msckf_batch_set_landmarks': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_next_landmarks': (C.c_int, [_P, _P, _P]),
    'av_msckf_batch_set_stats': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_next_stats': (C.c_int, [_P, _P]),
    'av_msckf_batch_set_imu_rate': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_next_imu_rate': (C.c_int, [_P, _P, _P]),
    'av_msckf_batch_set_forecast': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_next_forecast': (C.c_int, [_P, _P, _P, _P]),
    'av_msckf_batch_set_zupt': (C.c_int, [_P, C.POINTER(ZuptParams)]),
    'av_msckf_batch_read_zupt': (C.c_int, [_P, _P]),
    'av_msckf_zupt_ops_dev': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, _P, C.POINTER(ZuptParams), _P, _P]),
    'av_msckf_batch_sizes': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32 * 3)]),
    'av_msckf_batch_counters': (C.c_int, [_P, C.POINTER(C.c_int64 * 8)]),
    'av_msckf_batch_launch_shape': (C.c_int, [_P, C.POINTER(C.c_int32 * 17)]),
    'av_png_decode_gray8': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.c_int, _P]),
    'av_png_decode': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.c_int, _P]),
    'av_png_probe': (C.c_int, [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'av_to_gray8': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    'av_pixfmt_frame_bytes': (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    'av_to_gray8_range': (C.c_int, [_P, C.c_int64] + [C.c_int] * 10 + [_P, _P, C.c_int64, _P, _P, _P]),
    'av_frontend_set_gray16_scale': (C.c_int, [_P] + [C.c_int] * 6),
    'av_frontend_read_range': (C.c_int, [_P, _P, _P]),
    'av_downscale': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    'av_downscale_vector_path': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, C.c_int64]),
    'av_quat_to_rotation': (C.c_int, [_P, _P]),
    'av_rotation_to_quat': (C.c_int, [_P, _P]),
    'av_quat_multiply': (C.c_int, [_P, _P, _P]),
    'av_quat_small_angle': (C.c_int, [_P, _P]),
    'av_quat_from_two_vectors': (C.c_int, [_P, _P, _P]),
    'av_msckf_batch_debug_capture': (C.c_int, [_P, C.c_int]),
    'av_msckf_batch_debug_read': (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int32), _P, _P, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'av_msckf_feature_ops_dev': (C.c_int, [_P] + [C.c_int] * 7 + [_P] * 14 +[C.c_int, C.c_int64, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                           _P, _P, _P, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    'av_msckf_predict_ops_dev': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_double)] + [_P] * 6),
    'av_msckf_predict_ops_dev_rate': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_double)] + [_P] * 6 +
                                      [C.c_int, _P, _P]),
    'av_msckf_update_ops_dev': (C.c_int, [_P] + [C.c_int] * 6 + [_P] * 5 + [C.c_int, _P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int, _P, C.c_int, C.c_int64, C.c_double,
                                          _P, _P, _P, _P, _P]),
    'av_msckf_forecast_ops_dev': (C.c_int, [_P, C.c_int, C.c_int, C.c_int64, _P, _P, _P, C.c_int, _P, C.POINTER(C.c_double), _P, _P, C.c_int, _P, _P, _P]),
    'av_msckf_batch_work': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double * 8)]),
    'av_msckf_batch_work_executed': (C.c_int, [_P, C.POINTER(C.c_double * 2)]),
    'av_debug_live_resources': (C.c_int, [C.POINTER(C.c_int64 * 4)]),
    'av_msckf_batch_get_state': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double * 32), _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    'av_msckf_batch_stream_status': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.c_char_p, C.c_int]),
    'av_frontend_read_ransac_counts': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32 * 4), _P]),
    'av_ransac_hash': (C.c_uint32, [C.c_uint32] * 5),
    'av_ransac_num_hypotheses': (C.c_int, [C.c_double]),
    'av_two_point_ransac': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                      C.c_double, C.c_double, C.c_uint32, _P, _P, _P]),
    'av_frontend_read_image': (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    'av_clahe': (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _P, C.c_int64, _P, _P]),
    'av_frontend_set_masks': (C.c_int, [_P, _P, _P]),
    'av_frontend_read_mask': (C.c_int, [_P, C.c_int, _P]),
    'av_frontend_set_photometric': (C.c_int, [_P, _P, _P, _P, _P]),
    'av_frontend_read_photometric': (C.c_int, [_P, C.c_int, _P, _P]),
    'av_photometric': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, _P]),
    'av_photometric_exposure': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    'av_frontend_next_exposure': (C.c_int, [_P, _P, _P, C.c_int]),
    'av_frontend_read_exposure': (C.c_int, [_P, C.c_int, _P]),
    'av_photometric_vector_path': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P]),
    'av_msckf_batch_restart': (C.c_int, [_P, _P, C.c_int]),
    'av_frontend_restart': (C.c_int, [_P, _P, C.c_int, _P]),
    'av_frontend_enable_timing': (C.c_int, [_P, C.c_int]),
    'av_frontend_read_timing': (C.c_int, [_P, C.POINTER(C.c_double * 4), C.POINTER(C.c_int32 * 4)]),
}

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('libairvision_hip.so is not built (%s); run `python -m uav_airvision_amd.build` -- '
                               'there is no CPU fallback' % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise AirvisionError(rc, lib().av_last_error().decode('utf-8', 'replace'))


def current_stream():
    """hipStream_t of torch's current stream as a void pointer."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t):
    return C.c_void_p(t.data_ptr())


def darr(a):
    return (C.c_double * len(a))(*[float(v) for v in a])
