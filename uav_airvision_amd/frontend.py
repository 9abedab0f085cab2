"""FrontendEngine: Python handle of the device-resident image front-end (av_frontend_* C ABI).

One engine owns S independent stereo streams on one GPU.  This is the throughput path; the drop-in
`image_processing.ImageProcessor` (uav_airvision_amd/dropin) is the same engine with S = 1.
Reference surface mirrored: ImageProcessingPipeline.{__init__, imu_callback, stereo_callback}
(reference: src/image_processing/pipeline.py:14-150).
"""
import copy
import ctypes as C
import os

import numpy as np
import torch

from . import _native as N


def default_max_corners(width, height):
    """Capacity for the FAST corners of one image when the caller names none: 8192 at 752 x 480 and below, and as many more as the
    image has more pixels (a first frame keeps every corner, and at a given corner density their number grows with the area)."""
    return max(8192, -(-8192 * int(width) * int(height) // (752 * 480)))


def downscale_factor(config):
    """config.image_downscale (1 when the object has no such attribute) as 1, 2 or 4; ValueError for anything else and for an image
    size the factor does not divide."""
    f = N.downscale_value(getattr(config, 'image_downscale', 1))
    w, h = [int(v) for v in config.cam0_resolution]
    if w % f or h % f:
        raise ValueError('image_downscale %d does not divide the image size %d x %d' % (f, w, h))
    return f


def downscaled_config(config):
    """A copy of `config` for the image the engine works on when config.image_downscale = f is 2 or 4: cam0 / cam1_resolution divided
    by f, cam0 / cam1_intrinsics scaled by the pixel-centre map X = f x + (f - 1) / 2 -- fx / f, fy / f, (cx - (f - 1) / 2) / f,
    (cy - (f - 1) / 2) / f, in double precision and in this order, exactly what the engine does (include/airvision.h) -- and
    image_downscale = 1.  Distortion, extrinsics and thresholds are unchanged.  An engine of this configuration, handed frames binned
    with ops.downscale, publishes what the engine of `config` publishes from the full-size ones."""
    f = downscale_factor(config)
    out = copy.copy(config)
    half = (f - 1) / 2.0
    for cam in ('cam0', 'cam1'):
        w, h = [int(v) for v in getattr(config, cam + '_resolution')]
        if w % f or h % f:
            raise ValueError('image_downscale %d does not divide the %s size %d x %d' % (f, cam, w, h))
        fx, fy, cx, cy = [float(v) for v in getattr(config, cam + '_intrinsics')]
        setattr(out, cam + '_resolution', np.array([w // f, h // f]))
        setattr(out, cam + '_intrinsics', np.array([fx / f, fy / f, (cx - half) / f, (cy - half) / f]))
    out.image_downscale = 1
    return out


def pack_frontend_config(config, max_corners=None):
    """Build the packed av_frontend_config from a reference-style config object.  The
    extrinsics-derived matrices are computed with numpy exactly as the reference does
    (imu_processor.py:10-16, stereo_matcher.py:47,90-91,103-104).  max_corners None: default_max_corners of the processed image
    size (the image size divided by config.image_downscale).  width / height, the intrinsics and norm_unit are those of the full-size
    camera: the engine derives the binned size and calibration itself."""
    c = N.FrontendConfig()
    w, h = [int(v) for v in config.cam0_resolution]
    f = downscale_factor(config)
    if max_corners is None:
        max_corners = default_max_corners(w // f, h // f)
    c.width, c.height = w, h
    c.grid_row, c.grid_col = int(config.grid_row), int(config.grid_col)
    c.grid_min_feature_num = int(config.grid_min_feature_num)
    c.grid_max_feature_num = int(config.grid_max_feature_num)
    c.fast_threshold = int(config.fast_threshold)
    lk = config.lk_params
    if lk['winSize'][0] != lk['winSize'][1]:
        raise ValueError('square LK windows only')
    if not (lk['flags'] & 4):
        raise ValueError('the front-end requires OPTFLOW_USE_INITIAL_FLOW (config.py:44)')
    ctype, max_iter, eps = lk['criteria']
    c.lk_win = int(lk['winSize'][0])
    c.lk_levels = int(lk['maxLevel']) + 1
    c.lk_max_iter = int(max_iter) if (ctype & 1) else 30
    c.lk_eps = float(eps) if (ctype & 2) else 0.01
    c.lk_min_eig = 1e-4
    c.max_corners = int(max_corners)
    c.stereo_threshold = float(config.stereo_threshold)
    for name, src in (('cam0_intrinsics', config.cam0_intrinsics), ('cam0_distortion', config.cam0_distortion_coeffs),
                      ('cam1_intrinsics', config.cam1_intrinsics), ('cam1_distortion', config.cam1_distortion_coeffs)):
        getattr(c, name)[:] = [float(v) for v in src]
    c.cam0_distortion_model = N.distortion_model_code(config.cam0_distortion_model)      # 'equidistant' = cv2.fisheye.* (camera_model.py:41,69)
    c.cam1_distortion_model = N.distortion_model_code(config.cam1_distortion_model)
    T_cam0_imu = np.linalg.inv(config.T_imu_cam0)
    T_cam1_imu = np.linalg.inv(config.T_imu_cam1)
    R_cam0_imu, t_cam0_imu = T_cam0_imu[:3, :3], T_cam0_imu[:3, 3]
    R_cam1_imu, t_cam1_imu = T_cam1_imu[:3, :3], T_cam1_imu[:3, 3]
    R0to1 = R_cam1_imu.T @ R_cam0_imu
    t01 = R_cam1_imu.T @ (t_cam0_imu - t_cam1_imu)
    x, y, z = t01
    E = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]]) @ R0to1
    c.R_cam0_imu[:] = [float(v) for v in R_cam0_imu.reshape(-1)]
    c.R_cam1_imu[:] = [float(v) for v in R_cam1_imu.reshape(-1)]
    c.R0to1[:] = [float(v) for v in R0to1.reshape(-1)]
    c.E[:] = [float(v) for v in E.reshape(-1)]
    c.norm_unit = float(4.0 / (2 * config.cam0_intrinsics[0] + 2 * config.cam0_intrinsics[1]))
    # two-point RANSAC on the tracked features (AV_FE_RANSAC); getattr: the reference's own config object has no such switch
    c.ransac_threshold = float(getattr(config, 'ransac_threshold', 3))
    c.ransac_success_probability = float(getattr(config, 'ransac_success_probability', 0.99))
    c.ransac_seed = int(getattr(config, 'ransac_seed', 0)) & 0xFFFFFFFF
    c.flags = N.AV_FE_RANSAC if getattr(config, 'use_ransac', False) else 0
    # CLAHE ahead of everything that reads a frame (AV_FE_CLAHE); the fields are carried either way, read only with the flag
    c.clahe_clip_limit = float(getattr(config, 'clahe_clip_limit', 2.0))
    c.clahe_tiles_x, c.clahe_tiles_y = [int(v) for v in getattr(config, 'clahe_tiles', (8, 8))]
    if getattr(config, 'use_clahe', False):
        c.flags |= N.AV_FE_CLAHE
    # pixel format of the frames (AV_PIX_*); getattr: a config object without the two attributes is an 8-bit grey engine
    c.pixel_format = N.pixel_format_code(getattr(config, 'image_format', 'gray8'))
    c.gray16_shift = N.gray16_shift_value(getattr(config, 'gray16_shift', 8))
    # 2 x 2 / 4 x 4 binning ahead of CLAHE and the pyramids; getattr: a config object without the attribute is a full-size engine
    c.image_downscale = f
    c.reserved1 = 0
    # exposure-time normalisation (AV_FE_EXPOSURE); getattr: a config object without the attribute has none
    if exposure_reference(config) is not None:
        c.flags |= N.AV_FE_EXPOSURE
    return c


def exposure_reference(config):
    """config.exposure_reference as a float, or None (None, or a config object without the attribute): the reference exposure time
    t_ref of "Exposure-time normalisation" in include/airvision.h.  ValueError unless it is finite and > 0."""
    ref = getattr(config, 'exposure_reference', None)
    if ref is None:
        return None
    ref = float(ref)
    if not (np.isfinite(ref) and ref > 0):
        raise ValueError('exposure_reference: a finite time > 0 is wanted, got %r' % (ref,))
    return ref


def gray16_scale_settings(config):
    """config.gray16_scale / gray16_window / gray16_auto_clip / gray16_auto_min_span as av_frontend_set_gray16_scale takes them: (scale,
    lo, hi, clip_lo_ppm, clip_hi_ppm, min_span).  getattr: a config object without the attributes scales by the shift.  ValueError for a
    setting outside its limits (N.gray16_range_settings) and, naming both settings, for a scale other than 'shift' with an image_format
    other than 'gray16'."""
    scale = getattr(config, 'gray16_scale', 'shift')
    settings = N.gray16_range_settings(scale, getattr(config, 'gray16_window', None), getattr(config, 'gray16_auto_clip', (100, 100)),
                                       getattr(config, 'gray16_auto_min_span', 256))
    fmt = N.pixel_format_code(getattr(config, 'image_format', 'gray8'))
    if settings[0] != N.AV_GRAY16_SHIFT and fmt != N.AV_PIX_GRAY16:
        raise ValueError("gray16_scale %r applies to image_format 'gray16' only, not to image_format %r" % (scale, N.PIXEL_FORMAT_NAMES[fmt]))
    return settings


def gray16_range(frames, scale='auto', window=None, clip=(100, 100), min_span=256, pool=1):
    """What the engine and ops.to_gray8_range compute, in NumPy ("Range scaling of 16-bit grey" in include/airvision.h): frames uint16
    [n, h, w] in groups of `pool` (1 or 2) consecutive images -> (uint8 [n, h, w], int32 [n // pool, 2]), the grey frames and the (lo, hi)
    of every group.  scale 'window' applies `window` = (lo, hi) to every image; 'auto' takes each group's range from its 4,096-bin
    histogram of v >> 4 with `clip` = (ppm_lo, ppm_hi) and `min_span`.  The two images of a stereo pair are one group: pool = 2 on
    frames interleaved cam0, cam1."""
    mode, lo, hi, ppm_lo, ppm_hi, span_min = N.gray16_range_settings(scale, window, clip, min_span)
    if mode == N.AV_GRAY16_SHIFT:
        raise ValueError("gray16_range: scale is 'window' or 'auto'")
    a = np.asarray(frames)
    if a.dtype != np.uint16 or a.ndim != 3 or pool not in (1, 2) or a.shape[0] % pool:
        raise ValueError('gray16_range: frames are uint16 [n, h, w] with n a multiple of pool = 1 or 2, got %s %s, pool %r' % (a.dtype, a.shape, pool))
    n, h, w = a.shape
    out = np.empty((n, h, w), np.uint8)
    ranges = np.empty((n // pool, 2), np.int32)
    for g in range(n // pool):
        grp = a[g * pool:(g + 1) * pool]
        if mode == N.AV_GRAY16_AUTO:
            N_samples = grp.size
            k_lo, k_hi = N_samples * ppm_lo // 10 ** 6, N_samples * ppm_hi // 10 ** 6
            hist = np.bincount((grp >> 4).reshape(-1), minlength=4096).astype(np.int64)
            b_lo = int(np.argmax(np.cumsum(hist) > k_lo))
            b_hi = 4095 - int(np.argmax(np.cumsum(hist[::-1]) > k_hi))
            lo, hi = 16 * b_lo, 16 * b_hi + 15
            if hi - lo < span_min:
                need = span_min - (hi - lo)
                lo = max(0, min(lo - need // 2, 65535 - span_min))
                hi = lo + span_min
        span = hi - lo
        m = ((255 << 16) + span // 2) // span
        d = np.clip(grp.astype(np.int64), lo, hi) - lo
        out[g * pool:(g + 1) * pool] = np.minimum(255, (d * m + 32768) >> 16).astype(np.uint8)
        ranges[g] = (lo, hi)
    return out, ranges


def frame_shape(pixel_format, n, height, width):
    """Shape of n frames of an AV_PIX_* format: [n, h, w] for the grey formats and the mosaics, [n, h, w, 3 | 4] for the colour ones,
    [n, h, w * d / 8] (bytes) for the packed 10 / 12-bit transports."""
    if N.is_packed(pixel_format):
        return (n, height, N.packed_row_bytes(pixel_format, width))
    bpp = N.PIXEL_BYTES[pixel_format]
    return (n, height, width) if bpp <= 2 else (n, height, width, bpp)


def check_host_frames(what, a, pixel_format, n, height, width):
    """A NumPy batch of n frames of an AV_PIX_* format as a C-contiguous array of exactly the dtype and shape the engine reads: uint16
    [n, h, w] for gray16 and the 16-bit Bayer mosaics, uint8 [n, h, w, 3 | 4] for colour, uint8 [n, h, w] for gray8 and the 8-bit
    mosaics, uint8 [n, h, w * d / 8] for the packed transports ([h, w] / [h, w, c] is taken for n = 1).  Nothing is converted: a wrong dtype or shape is a ValueError naming both."""
    a = np.asarray(a)
    want_dtype = np.uint16 if N.is_16bit(pixel_format) else np.uint8
    want = frame_shape(pixel_format, n, height, width)
    shape = tuple(a.shape)
    if n == 1 and shape == want[1:]:
        shape = want
    if a.dtype != want_dtype or shape != want:
        raise ValueError('%s: %s frames are %s %s, got %s %s' % (what, N.PIXEL_FORMAT_NAMES[pixel_format], np.dtype(want_dtype).name, want, a.dtype, tuple(a.shape)))
    return np.ascontiguousarray(a).reshape(want)


def check_device_frames(what, t, pixel_format, n, height, width):
    """The same for a cuda tensor; 16-bit frames are torch.uint16, or torch.int16 holding the same bits (older torch has no
    unsigned 16-bit type).  The tensor must be contiguous: it is read where it lies."""
    want = frame_shape(pixel_format, n, height, width)
    dtypes = (torch.uint8,) if not N.is_16bit(pixel_format) else tuple(d for d in (getattr(torch, 'uint16', None), torch.int16) if d is not None)
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != want:
        raise ValueError('%s: %s frames are %s %s, got %s %s' % (what, N.PIXEL_FORMAT_NAMES[pixel_format], ' / '.join(str(d) for d in dtypes), want,
                                                               getattr(t, 'dtype', type(t).__name__), tuple(getattr(t, 'shape', ()))))
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError('%s: a contiguous cuda tensor is needed' % what)
    return t


def _packing_of(fmt):
    code = N.pixel_format_code(fmt)
    if not N.is_packed(code):
        raise ValueError('%r is no packed format (one of %s)' % (fmt, ', '.join(sorted(N.PACKED_FORMATS, key=N.PACKED_FORMATS.get))))
    return code, N.packed_depth(code), N.packing(code).endswith('csi2')


def pack_frames(samples_u16, fmt):
    """Right-aligned d-bit samples, uint16 [..., h, w], as the bytes of packed format `fmt` ('gray12p', 'bayer_rggb10_csi2', .. or the
    AV_PIX_* code), uint8 [..., h, w * d / 8]: the layouts of include/airvision.h ("Packed 10 / 12-bit transports"), in NumPy on the
    host.  ValueError for a value at or above 2^d and for a width that is not whole groups (4 samples at 10 bits, 2 at 12)."""
    code, d, csi2 = _packing_of(fmt)
    v = np.asarray(samples_u16)
    if v.dtype != np.uint16 or v.ndim < 2:
        raise ValueError('pack_frames: %s samples are uint16 [..., h, w], got %s %s' % (N.PIXEL_FORMAT_NAMES[code], v.dtype, tuple(v.shape)))
    wb = N.packed_row_bytes(code, v.shape[-1])
    if v.size and int(v.max()) >> d:
        raise ValueError('pack_frames: %s samples are below 2^%d = %d, got %d' % (N.PIXEL_FORMAT_NAMES[code], d, 1 << d, int(v.max())))
    gpx, gb = N.packed_group(code)
    p = v.astype(np.uint32).reshape(v.shape[:-1] + (v.shape[-1] // gpx, gpx))
    out = np.empty(p.shape[:-1] + (gb,), np.uint8)
    if csi2:
        out[..., :gpx] = p >> (d - 8)
        low = np.zeros(p.shape[:-1], np.uint32)
        for j in range(gpx):
            low |= (p[..., j] & ((1 << (d - 8)) - 1)) << ((d - 8) * j)
        out[..., gpx] = low
    else:
        word = np.zeros(p.shape[:-1], np.uint64)
        for j in range(gpx):
            word |= p[..., j].astype(np.uint64) << np.uint64(d * j)
        for i in range(gb):
            out[..., i] = (word >> np.uint64(8 * i)) & np.uint64(255)
    return out.reshape(v.shape[:-1] + (wb,))


def unpack_frames(raw_u8, fmt):
    """The inverse of pack_frames: uint8 [..., h, w * d / 8] -> right-aligned d-bit samples, uint16 [..., h, w].  ValueError for a row
    that is not whole groups of bytes."""
    code, d, csi2 = _packing_of(fmt)
    r = np.asarray(raw_u8)
    gpx, gb = N.packed_group(code)
    if r.dtype != np.uint8 or r.ndim < 2 or r.shape[-1] == 0 or r.shape[-1] % gb:
        raise ValueError('unpack_frames: %s frames are uint8 [..., h, w * %d / 8] with rows of whole %d-byte groups, got %s %s' % (
            N.PIXEL_FORMAT_NAMES[code], d, gb, r.dtype, tuple(r.shape)))
    b = r.astype(np.uint32).reshape(r.shape[:-1] + (r.shape[-1] // gb, gb))
    out = np.empty(b.shape[:-1] + (gpx,), np.uint16)
    if csi2:
        for j in range(gpx):
            out[..., j] = b[..., j] << (d - 8) | ((b[..., gpx] >> ((d - 8) * j)) & ((1 << (d - 8)) - 1))
    else:
        word = np.zeros(b.shape[:-1], np.uint64)
        for i in range(gb):
            word |= b[..., i].astype(np.uint64) << np.uint64(8 * i)
        for j in range(gpx):
            out[..., j] = (word >> np.uint64(d * j)) & np.uint64((1 << d) - 1)
    return out.reshape(r.shape[:-1] + (r.shape[-1] // gb * gpx,))


def circle_mask(width, height, cx, cy, radius):
    """A static mask (uint8 [height, width], 1 = scene) of a fisheye lens's image circle: pixel (x, y) is valid iff
    (x - cx)^2 + (y - cy)^2 <= radius^2."""
    y, x = np.mgrid[0:int(height), 0:int(width)]
    return ((x - float(cx)) ** 2 + (y - float(cy)) ** 2 <= float(radius) ** 2).astype(np.uint8)


def check_mask(cam, mask, height, width):
    """The static mask of camera `cam` (0 / 1) as a C-contiguous uint8 [height, width] array, or None for None.  `mask` is an ndarray,
    uint8 or bool, of exactly that shape (non-zero = scene, 0 = never scene), or the path of an 8-bit grey PNG of that size (decoded by
    the library's own av_png_decode).  Host only; nothing is cast or resized: a wrong dtype or shape is a ValueError naming the
    camera, the shape wanted and the shape it got."""
    if mask is None:
        return None
    want = (int(height), int(width))
    if isinstance(mask, (str, os.PathLike)):
        path = os.fspath(mask)
        w, h, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        if N.lib().av_png_probe(os.fsencode(path), C.byref(w), C.byref(h), C.byref(f)) != 0:
            raise ValueError('cam%d mask: %s: %s' % (cam, path, N.lib().av_last_error().decode('utf-8', 'replace')))
        if (int(h.value), int(w.value)) != want or int(f.value) != N.AV_PIX_GRAY8:
            raise ValueError('cam%d mask: %s: an 8-bit grey PNG of shape %s is wanted, got %s %s' % (cam, path, want, N.PIXEL_FORMAT_NAMES.get(int(f.value), 'an undecodable flavour'),
                                                                                                       (int(h.value), int(w.value))))
        out = np.empty(want, np.uint8)
        paths = (C.c_char_p * 1)(os.fsencode(path))
        status = (C.c_int32 * 1)()
        N.check(N.lib().av_png_decode(paths, 1, want[1], want[0], N.AV_PIX_GRAY8, out.ctypes.data_as(C.c_void_p), out.nbytes, 1, status))
        return out
    a = np.asarray(mask)
    if a.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)) or tuple(a.shape) != want:
        raise ValueError('cam%d mask: a uint8 or bool array of shape %s is wanted, got %s %s' % (cam, want, a.dtype, tuple(a.shape)))
    return np.ascontiguousarray(a).astype(np.uint8, copy=False)


def quantise_response(response):
    """The inverse response G^-1 (256 values in [0, 255]) as the engine's table: uint16[256] in Q8, floor(clip(U, 0, 255) * 256 + 0.5) in
    float64, so every entry is <= 65280."""
    u = np.asarray(response, dtype=np.float64).reshape(-1)
    if u.shape != (256,):
        raise ValueError('response: 256 numbers in [0, 255] are wanted, got %d' % u.size)
    if not np.isfinite(u).all():
        raise ValueError('response: entry %d is not finite (%r)' % (int(np.flatnonzero(~np.isfinite(u))[0]), float(u[~np.isfinite(u)][0])))
    return np.floor(np.clip(u, 0.0, 255.0) * 256.0 + 0.5).astype(np.uint16)


def quantise_vignette(vignette):
    """The vignette map V(x) in (0, 1] as the engine's gain map: uint16 [h, w] in Q12, min(65535, floor(4096 / V + 0.5)) in float64;
    V <= 0 (and a NaN) gives 65535.  Gains of 16 and above saturate at 15.9998."""
    v = np.asarray(vignette, dtype=np.float64)
    if v.ndim != 2 or v.size == 0:
        raise ValueError('vignette: a float array of shape (height, width) is wanted, got %s' % (tuple(v.shape),))
    ok = v > 0
    g = np.full(v.shape, 65535.0)
    g[ok] = np.minimum(65535.0, np.floor(4096.0 / v[ok] + 0.5))
    return g.astype(np.uint16)


def read_response_file(path):
    """A pcalib.txt-style text file: 256 numbers separated by white space (one line in the TUM mono-VO dataset), the inverse response
    G^-1 with values in [0, 255]."""
    with open(os.fspath(path)) as f:
        vals = f.read().split()
    try:
        u = np.array([float(v) for v in vals], np.float64)
    except ValueError:
        raise ValueError('response: %s holds something that is no number' % (path,))
    if u.shape != (256,):
        raise ValueError('response: %s holds %d numbers, 256 are wanted' % (path, u.size))
    return u


def read_vignette_png(path):
    """A vignette.png of the TUM mono-VO convention: a 16-bit grey PNG (decoded by the library's own av_png_decode), normalised by its
    maximum -> float64 [h, w] in [0, 1]."""
    path = os.fspath(path)
    w, h, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if N.lib().av_png_probe(os.fsencode(path), C.byref(w), C.byref(h), C.byref(f)) != 0:
        raise ValueError('vignette: %s: %s' % (path, N.lib().av_last_error().decode('utf-8', 'replace')))
    if int(f.value) != N.AV_PIX_GRAY16:
        raise ValueError('vignette: %s: a 16-bit grey PNG is wanted, got %s' % (path, N.PIXEL_FORMAT_NAMES.get(int(f.value), 'an undecodable flavour')))
    out = np.empty((int(h.value), int(w.value)), np.uint16)
    paths = (C.c_char_p * 1)(os.fsencode(path))
    status = (C.c_int32 * 1)()
    N.check(N.lib().av_png_decode(paths, 1, int(w.value), int(h.value), N.AV_PIX_GRAY16, out.ctypes.data_as(C.c_void_p), out.nbytes, 1, status))
    top = int(out.max())
    if top == 0:
        raise ValueError('vignette: %s is all zero' % path)
    return out.astype(np.float64) / float(top)


def photometric_tables(response=None, vignette=None):
    """The photometric calibration of one camera as the engine's integer tables ("Photometric calibration" in include/airvision.h):
    (response_u16 or None, gain_u16 or None).  response: the inverse response G^-1, 256 floats in [0, 255], or the path of a
    pcalib.txt-style text file of 256 numbers -> uint16[256] in Q8 (quantise_response).  vignette: V(x), an [h, w] float array with
    values in (0, 1], or the path of a 16-bit grey PNG, normalised by its maximum as TUM does -> uint16 [h, w] in Q12
    (quantise_vignette).  The quantisation happens here, once, on the host, in float64; everything after it is integer."""
    r = g = None
    if response is not None:
        r = quantise_response(read_response_file(response) if isinstance(response, (str, os.PathLike)) else response)
    if vignette is not None:
        g = quantise_vignette(read_vignette_png(vignette) if isinstance(vignette, (str, os.PathLike)) else vignette)
    return r, g


def apply_vignette(img_u8, vignette, response_forward=None):
    """The forward model of a vignetting lens and a non-linear sensor, for synthesising degraded frames: round(G(img * V)) clipped to
    0 .. 255, uint8 of img's shape.  vignette: V, float [h, w] in (0, 1] (broadcast against img [..., h, w]).  response_forward: G, the
    sensor's response -- None (the identity), a callable on float64 arrays of irradiance in [0, 255], or 256 values G(0) .. G(255)
    (interpolated linearly)."""
    x = np.asarray(img_u8).astype(np.float64) * np.asarray(vignette, dtype=np.float64)
    if callable(response_forward):
        x = np.asarray(response_forward(x), dtype=np.float64)
    elif response_forward is not None:
        tab = np.asarray(response_forward, dtype=np.float64).reshape(-1)
        if tab.shape != (256,):
            raise ValueError('apply_vignette: response_forward is a callable or 256 values, got %d' % tab.size)
        x = np.interp(x, np.arange(256.0), tab)
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)


def quantise_exposure(t, t_ref):
    """Exposure times t (a number or an array, in the unit of t_ref) as the engine's factors ("Exposure-time normalisation" in
    include/airvision.h): uint16 in Q12, k = min(65535, max(1, floor(4096 * t_ref / t + 0.5))) in float64, of t's shape.  t <= 0,
    t_ref <= 0 or a value that is not finite is a ValueError: nothing is cast silently."""
    a = np.asarray(t, dtype=np.float64)
    ref = float(t_ref)
    if not (np.isfinite(ref) and ref > 0):
        raise ValueError('quantise_exposure: the reference exposure is finite and > 0, got %r' % (ref,))
    if not (np.isfinite(a).all() and (a > 0).all()):
        bad = a.reshape(-1)[~(np.isfinite(a.reshape(-1)) & (a.reshape(-1) > 0))]
        raise ValueError('quantise_exposure: every exposure time is finite and > 0, got %r' % (float(bad[0]),))
    with np.errstate(over='ignore'):
        k = np.floor(4096.0 * ref / a + 0.5)
    return np.minimum(65535.0, np.maximum(1.0, k)).astype(np.uint16)


def apply_exposure(img_u8, ratio, vignette=None, response_forward=None):
    """The forward model of a frame taken at `ratio` = t / t_ref times the reference exposure, for synthesising degraded frames:
    round(G(ratio * V * img)) clipped to 0 .. 255 -- `apply_vignette` with the irradiance scaled first.  vignette None: V = 1."""
    x = np.asarray(img_u8).astype(np.float64) * float(ratio)
    v = 1.0 if vignette is None else np.asarray(vignette, dtype=np.float64)
    x = x * v
    if callable(response_forward):
        x = np.asarray(response_forward(x), dtype=np.float64)
    elif response_forward is not None:
        tab = np.asarray(response_forward, dtype=np.float64).reshape(-1)
        if tab.shape != (256,):
            raise ValueError('apply_exposure: response_forward is a callable or 256 values, got %d' % tab.size)
        x = np.interp(x, np.arange(256.0), tab)
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)


def check_photometric(cam, response, gain, height, width):
    """The integer tables of camera `cam` as C-contiguous uint16 arrays of the shapes the engine reads ([256], [height, width]), or None
    for None.  Nothing is cast: a wrong dtype or shape is a ValueError naming the camera; so is a response entry above 65280."""
    r = g = None
    if response is not None:
        r = np.asarray(response)
        if r.dtype != np.uint16 or r.shape != (256,):
            raise ValueError('cam%d response: a uint16 array of shape (256,) is wanted (photometric_tables makes one), got %s %s' % (cam, r.dtype, tuple(r.shape)))
        if int(r.max()) > N.AV_PHOTOMETRIC_RESPONSE_MAX:
            raise ValueError('cam%d response: entry %d is above %d (255 in Q8)' % (cam, int(r.max()), N.AV_PHOTOMETRIC_RESPONSE_MAX))
        r = np.ascontiguousarray(r)
    if gain is not None:
        g = np.asarray(gain)
        if g.dtype != np.uint16 or tuple(g.shape) != (int(height), int(width)):
            raise ValueError('cam%d gain: a uint16 array of shape %s is wanted (photometric_tables makes one), got %s %s' % (cam, (int(height), int(width)), g.dtype, tuple(g.shape)))
        g = np.ascontiguousarray(g)
    return r, g


COUNTER_NAMES = ('before_tracking', 'after_tracking', 'after_matching', 'n_fast', 'n_candidates', 'n_new',
                 'n_published', 'overflow')


RANSAC_COUNT_NAMES = ('after_ransac', 'cam0_set', 'cam1_set', 'path')


class FrontendEngine(object):
    exposure, _exposure_ref, _pre = False, None, None      # (off unless the constructor finds config.exposure_reference)

    def __init__(self, config, n_streams=1, device=0, max_corners=None, inputs_persist=False):
        """The image size is config.cam0_resolution: any width x height of up to AV_MAX_IMAGE_PIXELS = 2^24 pixels.  max_corners:
        capacity for the FAST corners of one image (None: 8192 at 752 x 480, scaled by the pixel count above that).
        inputs_persist: promise that the cuda tensors handed to `step` stay unmodified until the NEXT step has run
        (AV_FE_INPUTS_PERSIST, include/airvision.h): pyramid level 0 is then read in place instead of being copied.  The engine
        keeps a reference to the last cam0 tensor, so dropping yours is fine; overwriting it in place is not.  `step_host`
        always works in place on the library's own staging slots.  Same results either way.

        config.image_format other than 'gray8' (and config.gray16_shift): every entry below takes frames of that format instead --
        uint16 [S,h,w] for 'gray16' (cuda: torch.uint16, or torch.int16 holding the same bits), uint8 [S,h,w,3] for 'rgb8' / 'bgr8',
        uint8 [S,h,w,4] for 'rgba8' / 'bgra8', the raw mosaic as uint8 [S,h,w] for 'bayer_*8' and uint16 [S,h,w] for 'bayer_*16', the packed
        bytes as uint8 [S,h,w*d/8] for the 10 / 12-bit transports 'gray{10p,12p,10_csi2,12_csi2}' and 'bayer_*{10p,12p,10_csi2,12_csi2}' (PFNC
        Mono10p / Mono12p, MIPI CSI-2 RAW10 / RAW12: rows tightly packed, width a multiple of 4 / 2 samples; `pack_frames` / `unpack_frames`
        are their NumPy twins; a sample is left-justified to 16 bits before gray16_shift applies) -- and converts them to 8-bit grey on the GPU ahead of everything else (av_to_gray8 in
        include/airvision.h has the arithmetic).  Nothing is cast on the way: a wrong dtype or shape is a ValueError naming both.
        The caller's frames are never written; `read_image` returns the grey frame the step used.

        config.image_downscale = 2 or 4: every entry below still takes frames of config.cam0_resolution (`input_width` x
        `input_height`) with the calibration of the full-size camera; the engine bins them f x f on the GPU (after the conversion,
        ahead of CLAHE) and works on the `width` x `height` = processed image with the calibration of `downscaled_config(config)`.
        `read_image` returns that frame and `read_grid` pixel coordinates are its pixels; the published message is in normalised
        coordinates and needs no change downstream.

        config.cam0_mask / config.cam1_mask (a config object without them has none): the static mask of each camera, for all streams
        -- None, a uint8 / bool array of shape (input_height, input_width) with non-zero = scene, or the path of an 8-bit grey PNG of
        that size; `set_masks` has the rules.  They are read here, so every owner of an engine (the drop-in ImageProcessor, EngineSet,
        the sweep) gets them from its config object.

        config.cam0_response / cam1_response / cam0_vignette / cam1_vignette (a config object without them has none): the photometric
        calibration of each camera, for all streams -- each None, an array or a path as `photometric_tables` takes them.  With any of
        them the engine is created with AV_FE_PHOTOMETRIC and corrects every grey frame, G^-1(p) / V(x) in the integer arithmetic of
        include/airvision.h, after the conversion to grey and ahead of binning and CLAHE; `set_photometric` has the rules.

        config.gray16_scale = 'window' or 'auto' (a config object without the attribute: 'shift'), image_format 'gray16' only: 16-bit
        samples are scaled through config.gray16_window = (lo, hi), or through a range the GPU takes from every stereo pair's own
        histogram (config.gray16_auto_clip ppm at each end, config.gray16_auto_min_span), instead of config.gray16_shift -- `gray16_range`
        is the arithmetic in NumPy, `read_range` returns the ranges of the last step.  Any other image_format with such a scale is a
        ValueError naming both settings.

        config.exposure_reference = t_ref (a config object without the attribute, or None: off): exposure-time normalisation
        ("Exposure-time normalisation" in include/airvision.h).  The engine is created with AV_FE_EXPOSURE, `exposure` is True, and
        `step`, `prestage`, `step_host` and `frames_upload` then REQUIRE the exposure times of the frames they are handed: the keyword
        exposure=(e0, e1), float arrays [n_streams] ([n] for an upload) in the unit of t_ref, one per camera, quantised by
        `quantise_exposure`; or exposure_q=(k0, k1), ready uint16 factors.  A call that needs them and gets neither is a ValueError (a
        `step` with the tensors of the last `prestage` needs none); a keyword on an engine without the switch is a ValueError too.
        `read_exposure` returns the factors a stream's last frame was corrected with."""
        self.config = config
        self.n_streams = int(n_streams)
        self.device = int(device)
        self._cfg = pack_frontend_config(config, max_corners)
        self._cfg.flags |= N.AV_FE_INPUTS_PERSIST if inputs_persist else 0
        self._keep = None
        self._h = C.c_void_p()
        self.generation = np.zeros(self.n_streams, dtype=np.int64)      # restarts of every stream so far (`restart`)
        masks = [check_mask(cam, getattr(config, 'cam%d_mask' % cam, None), self._cfg.height, self._cfg.width) for cam in (0, 1)]      # before any device call
        photo = [photometric_tables(getattr(config, 'cam%d_response' % cam, None), getattr(config, 'cam%d_vignette' % cam, None)) for cam in (0, 1)]
        photo = [check_photometric(cam, r, g, self._cfg.height, self._cfg.width) for cam, (r, g) in enumerate(photo)]
        self.photometric = any(t is not None for pair in photo for t in pair)
        self._exposure_ref = exposure_reference(config)
        self.exposure = self._exposure_ref is not None
        g16 = gray16_scale_settings(config)
        self.gray16_scale = {v: k for k, v in N.GRAY16_SCALES.items()}[g16[0]]
        if self.photometric:
            self._cfg.flags |= N.AV_FE_PHOTOMETRIC
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_create(C.byref(self._cfg), self.n_streams, self.device, C.byref(self._h)))
        self.max_features = N.lib().av_frontend_max_features(self._h)
        self._set_sizes(self._cfg)
        S, cap = self.n_streams, self.max_features
        self._ids = np.zeros((S, cap), np.int64)
        self._uv = np.zeros((S, cap, 4), np.float64)
        self._n = np.zeros(S, np.int32)
        try:
            if masks[0] is not None or masks[1] is not None:
                self.set_masks(*masks)
            if self.photometric:
                self.set_photometric(photo[0][0], photo[0][1], photo[1][0], photo[1][1])
            if g16[0] != N.AV_GRAY16_SHIFT:
                with torch.cuda.device(self.device):
                    N.check(N.lib().av_frontend_set_gray16_scale(self._h, *g16))
        except Exception:
            self.close()
            raise

    def _set_sizes(self, cfg):
        """The sizes that follow from a packed configuration: input_* = the frames the entry points take, width / height = the image
        the engine works on (the input binned by config.image_downscale)."""
        self.downscale = max(1, int(cfg.image_downscale))
        self.input_width, self.input_height = int(cfg.width), int(cfg.height)
        self.width, self.height = self.input_width // self.downscale, self.input_height // self.downscale
        self.pixel_format = int(cfg.pixel_format)
        self._frame_bytes = N.frame_bytes(self.pixel_format, self.input_width, self.input_height)      # img_stride of every entry point

    def close(self):
        if self._h:
            N.lib().av_frontend_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return N.current_stream()

    def push_imu(self, stream, timestamp, gyro):
        g = (C.c_double * 3)(float(gyro[0]), float(gyro[1]), float(gyro[2]))
        N.check(N.lib().av_frontend_push_imu(self._h, int(stream), float(timestamp), g))

    def push_imu_batch(self, stream_idx, timestamps, gyro):
        """stream_idx int32[n], timestamps float64[n], gyro float64[n,3] in one C call."""
        si = np.ascontiguousarray(stream_idx, dtype=np.int32)
        ts = np.ascontiguousarray(timestamps, dtype=np.float64)
        g = np.ascontiguousarray(gyro, dtype=np.float64).reshape(-1, 3)
        assert len(si) == len(ts) == len(g)
        N.check(N.lib().av_frontend_push_imu_batch(self._h, si.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p),
                                                   g.ctypes.data_as(C.c_void_p), len(si)))

    def restart(self, streams):
        """Put the listed streams back to "as created" while the others keep stepping (av_frontend_restart; include/airvision.h,
        "Stream restart"): their next frame is an initialisation, their feature ids begin again at 0, their IMU buffers are emptied.
        Enqueued on the current stream, behind the steps already there; legal between `prestage` and `step`, with a read-back
        pending, and with the frame store.  `generation[s]` counts the restarts of stream s -- ids repeat across lives."""
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(streams, dtype=np.int64)).reshape(-1), dtype=np.int32)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_restart(self._h, idx.ctypes.data_as(C.c_void_p), len(idx), self._stream()))
        if len(idx):
            self.generation[np.unique(idx)] += 1

    def _next_exposure(self, who, n, exposure, exposure_q, needed=True):
        """Hands the factors of the next call's n frames to the engine (av_frontend_next_exposure).  ValueError: a keyword on an engine
        without config.exposure_reference, both keywords, none where the call needs them, a shape other than [n], factors that are not
        uint16 or hold a zero."""
        if not self.exposure:
            if exposure is not None or exposure_q is not None:
                raise ValueError('%s: exposure given to an engine without config.exposure_reference' % who)
            return
        if exposure is not None and exposure_q is not None:
            raise ValueError('%s: exposure= and exposure_q= are alternatives' % who)
        if exposure is None and exposure_q is None:
            if needed:
                raise ValueError('%s: the engine has config.exposure_reference = %r and needs exposure=(e0, e1) (or exposure_q=(k0, k1)) with every frame' % (who, self._exposure_ref))
            return
        if exposure is not None:
            k = [quantise_exposure(np.atleast_1d(np.asarray(e, dtype=np.float64)), self._exposure_ref) for e in exposure]
        else:
            k = [np.atleast_1d(np.asarray(q)) for q in exposure_q]
            for q in k:
                if q.dtype != np.uint16:
                    raise ValueError('%s: exposure_q holds uint16 factors (quantise_exposure makes them), got %s' % (who, q.dtype))
        if len(k) != 2 or any(q.shape != (n,) for q in k):
            raise ValueError('%s: one array of %d exposures per camera is wanted, got shapes %s' % (who, n, [tuple(q.shape) for q in k]))
        if any(int(q.min()) == 0 for q in k):
            raise ValueError('%s: an exposure factor of 0 (1 .. 65535 in Q12)' % who)
        k0, k1 = np.ascontiguousarray(k[0]), np.ascontiguousarray(k[1])
        N.check(N.lib().av_frontend_next_exposure(self._h, k0.ctypes.data_as(C.c_void_p), k1.ctypes.data_as(C.c_void_p), n))

    def read_exposure(self, stream=0):
        """(k0, k1): the Q12 factors the frame of `stream`'s last step was corrected with (av_frontend_read_exposure); through the frame
        store those of the entry it read.  Refused (AirvisionError, AV_E_INVALID) without config.exposure_reference and before a step."""
        out = (C.c_uint16 * 2)()
        N.check(N.lib().av_frontend_read_exposure(self._h, int(stream), out))
        return int(out[0]), int(out[1])

    def step(self, img0, img1, timestamps, exposure=None, exposure_q=None):
        """img0/img1: uint8 cuda tensors [S,h,w] (contiguous); timestamps: S floats.  Enqueues only.  exposure / exposure_q: class
        docstring."""
        S = self.n_streams
        pre = self._pre is not None and self._pre[0].data_ptr() == img0.data_ptr() and self._pre[1].data_ptr() == img1.data_ptr()      # built by `prestage`: the step skips the stage
        if self.pixel_format != N.AV_PIX_GRAY8:
            check_device_frames('step: img0', img0, self.pixel_format, S, self.input_height, self.input_width)
            check_device_frames('step: img1', img1, self.pixel_format, S, self.input_height, self.input_width)
        else:
            assert img0.is_cuda and img1.is_cuda and img0.dtype == torch.uint8 and img1.dtype == torch.uint8
            assert tuple(img0.shape) == (S, self.input_height, self.input_width) == tuple(img1.shape), (img0.shape, img1.shape)
            assert img0.is_contiguous() and img1.is_contiguous()
        ts = (C.c_double * S)(*[float(t) for t in timestamps])
        self._next_exposure('step', S, exposure, exposure_q, needed=not pre)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_step(self._h, N.dptr(img0), N.dptr(img1), self._frame_bytes, ts, self._stream()))
        self._keep = (self._keep[1] if self._keep else None, (img0, img1))       # this frame's and the previous frame's tensors stay alive
        self._pre = None

    def prestage(self, img0, img1, exposure=None, exposure_q=None):
        """Build the pyramids of the NEXT step's images now (av_frontend_prestage): `step` with the same tensors then starts with its
        tracking launch.  Same results; the engine must have been created with inputs_persist=True."""
        S = self.n_streams
        if self.pixel_format != N.AV_PIX_GRAY8:
            check_device_frames('prestage: img0', img0, self.pixel_format, S, self.input_height, self.input_width)
            check_device_frames('prestage: img1', img1, self.pixel_format, S, self.input_height, self.input_width)
        else:
            assert img0.is_cuda and img1.is_cuda and img0.dtype == torch.uint8 and img1.dtype == torch.uint8
            assert tuple(img0.shape) == (S, self.input_height, self.input_width) == tuple(img1.shape) and img0.is_contiguous() and img1.is_contiguous()
        self._next_exposure('prestage', S, exposure, exposure_q)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_prestage(self._h, N.dptr(img0), N.dptr(img1), self._frame_bytes, self._stream()))
        self._pre = (img0, img1)                                                # alive until the step that uses them

    def step_host(self, img0, img1, timestamps, exposure=None, exposure_q=None):
        """numpy uint8 [S,h,w] (or [h,w] when S == 1); frames of config.image_format otherwise (class docstring)."""
        S = self.n_streams
        if self.pixel_format != N.AV_PIX_GRAY8:
            a0 = check_host_frames('step_host: img0', img0, self.pixel_format, S, self.input_height, self.input_width)
            a1 = check_host_frames('step_host: img1', img1, self.pixel_format, S, self.input_height, self.input_width)
        else:
            a0 = np.ascontiguousarray(img0, dtype=np.uint8).reshape(S, self.input_height, self.input_width)
            a1 = np.ascontiguousarray(img1, dtype=np.uint8).reshape(S, self.input_height, self.input_width)
        ts = (C.c_double * S)(*[float(t) for t in np.atleast_1d(timestamps)])
        self._next_exposure('step_host', S, exposure, exposure_q)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_step_host(self._h, a0.ctypes.data_as(C.c_void_p), a1.ctypes.data_as(C.c_void_p),
                                                  self._frame_bytes, ts, self._stream()))

    def set_masks(self, mask0=None, mask1=None):
        """The static masks of cam0 and cam1, shared by all streams (av_frontend_set_masks; "Static masks" in include/airvision.h): what
        is never scene -- outside a fisheye's image circle, airframe in view.  Each is None (all valid), a uint8 / bool array of shape
        (input_height, input_width) with non-zero = scene, or the path of an 8-bit grey PNG of that size; both None clears.  FAST
        corners on a masked cam0 pixel are dropped, tracked points that land on one are dropped, and a stereo match whose cam1 point
        lies on a masked cam1 pixel is no inlier.  With config.image_downscale = f the engine bins them: a pixel is valid iff all f x f
        pixels under it are.  Blocking.  Accepted only before the engine's first frame: after a step, prestage or frames_upload it is
        refused (AirvisionError, AV_E_INVALID).  A wrong dtype or shape is a ValueError before anything reaches the device."""
        m0 = check_mask(0, mask0, self.input_height, self.input_width)
        m1 = check_mask(1, mask1, self.input_height, self.input_width)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_set_masks(self._h, None if m0 is None else m0.ctypes.data_as(C.c_void_p),
                                                  None if m1 is None else m1.ctypes.data_as(C.c_void_p)))

    def read_mask(self, cam=0):
        """The mask of camera `cam` the engine works with: uint8 [height, width] (the processed size) of 0 / 1; refused (AirvisionError,
        AV_E_INVALID) when none is set for that camera."""
        out = np.empty((self.height, self.width), np.uint8)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_mask(self._h, int(cam), out.ctypes.data_as(C.c_void_p)))
        return out

    def set_photometric(self, response0=None, gain0=None, response1=None, gain1=None):
        """The photometric tables of cam0 and cam1, shared by all streams (av_frontend_set_photometric; "Photometric calibration" in
        include/airvision.h): response* uint16[256] in Q8, gain* uint16 [input_height, input_width] in Q12, as `photometric_tables`
        returns them; each may be None = the identity for that part.  Blocking.  The engine must have been created with the
        calibration switched on (one of the four config attributes set), and the call is accepted only before the engine's first
        frame: otherwise AirvisionError, AV_E_INVALID.  A wrong dtype or shape, or a response entry above 65280, is a ValueError before
        anything reaches the device."""
        r0, g0 = check_photometric(0, response0, gain0, self.input_height, self.input_width)
        r1, g1 = check_photometric(1, response1, gain1, self.input_height, self.input_width)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_set_photometric(self._h, ptr(r0), ptr(g0), ptr(r1), ptr(g1)))

    def read_photometric(self, cam=0):
        """The tables of camera `cam` the engine works with: (response uint16[256], gain uint16 [input_height, input_width]); a part that
        was set as None reads back as the identity (p * 256, 4096).  Refused (AirvisionError, AV_E_INVALID) when none are set."""
        r = np.empty(256, np.uint16)
        g = np.empty((self.input_height, self.input_width), np.uint16)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_photometric(self._h, int(cam), r.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)))
        return r, g

    def frames_reserve(self, n_slots):
        """Allocate the shared frame store (av_frontend_frames_reserve): `n_slots` resident stereo frames."""
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_frames_reserve(self._h, int(n_slots)))

    def frames_upload(self, slots, img0, img1, exposure=None, exposure_q=None):
        """Put host frames into the store: slots int32[n], img0 / img1 uint8[n,h,w] (C-contiguous).  Copy, pyramids and FAST of
        every frame happen once, here, on the engine's copy stream; the arrays are free again on return."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(sl)
        if n == 0:
            return
        if self.pixel_format != N.AV_PIX_GRAY8:
            a0 = check_host_frames('frames_upload: img0', img0, self.pixel_format, n, self.input_height, self.input_width)
            a1 = check_host_frames('frames_upload: img1', img1, self.pixel_format, n, self.input_height, self.input_width)
        else:
            a0 = np.ascontiguousarray(img0, dtype=np.uint8).reshape(n, self.input_height, self.input_width)
            a1 = np.ascontiguousarray(img1, dtype=np.uint8).reshape(n, self.input_height, self.input_width)
        self._next_exposure('frames_upload', n, exposure, exposure_q)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_frames_upload(self._h, sl.ctypes.data_as(C.c_void_p), n, a0.ctypes.data_as(C.c_void_p),
                                                      a1.ctypes.data_as(C.c_void_p), self._frame_bytes, self._stream()))

    def step_frames(self, slot_of_stream, timestamps):
        """One step with stream s reading store entry slot_of_stream[s]; < 0 = no frame for that stream in this step."""
        S = self.n_streams
        sl = np.ascontiguousarray(slot_of_stream, dtype=np.int32)
        assert sl.shape == (S,)
        ts = (C.c_double * S)(*[float(t) for t in np.atleast_1d(timestamps)])
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_step_frames(self._h, sl.ctypes.data_as(C.c_void_p), ts, self._stream()))

    def read_features(self):
        """Synchronises; returns [(ids int64[n], uv float64[n,4])] per stream (u0, v0, u1, v1)."""
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_features(self._h, self._ids.ctypes.data_as(C.c_void_p),
                                                      self._uv.ctypes.data_as(C.c_void_p),
                                                      self._n.ctypes.data_as(C.c_void_p), self.max_features, self._stream()))
        return [(self._ids[s, :self._n[s]].copy(), self._uv[s, :self._n[s]].copy()) for s in range(self.n_streams)]

    def read_features_raw(self):
        """Synchronises; returns the engine's own host arrays (ids int64[S,cap], uv float64[S,cap,4],
        n int32[S]) without per-stream copies -- valid until the next read."""
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_features(self._h, self._ids.ctypes.data_as(C.c_void_p),
                                                      self._uv.ctypes.data_as(C.c_void_p),
                                                      self._n.ctypes.data_as(C.c_void_p), self.max_features, self._stream()))
        return self._ids, self._uv, self._n

    def features_dev(self):
        """(ids_ptr, uv_ptr, n_ptr, cap): device addresses of the feature message the last `step` published (int64[S,cap],
        float64[S,cap,4], int32[S]); rewritten by the next step.  For `BatchedMSCKF.submit_dev`."""
        ids, uv, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int(0)
        N.check(N.lib().av_frontend_features_dev(self._h, C.byref(ids), C.byref(uv), C.byref(n), C.byref(cap)))
        return ids, uv, n, int(cap.value)

    def read_features_begin(self, slot=0):
        """Enqueue the device-to-host copy of the features published by the last step into pinned slot 0/1 (returns
        at once).  Call `step` for the next frame before `read_features_end(slot)` to overlap the two."""
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_features_begin(self._h, int(slot), self._stream()))

    def read_features_end(self, slot=0):
        """Wait for the copy begun on `slot` and return NEW host arrays (ids int64[S,cap], uv float64[S,cap,4],
        n int32[S]); entries beyond n[s] are unspecified."""
        ids = np.empty((self.n_streams, self.max_features), np.int64)
        uv = np.empty((self.n_streams, self.max_features, 4), np.float64)
        n = np.empty(self.n_streams, np.int32)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_features_end(self._h, int(slot), ids.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p),
                                                        n.ctypes.data_as(C.c_void_p), self.max_features))
        return ids, uv, n

    def read_grid(self, stream=0):
        cap = self.max_features
        ids = np.zeros(cap, np.int64); life = np.zeros(cap, np.int32); cell = np.zeros(cap, np.int32)
        pts = np.zeros((cap, 4), np.float32)
        n = C.c_int32(0); nid = C.c_int64(0)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_grid(self._h, int(stream), ids.ctypes.data_as(C.c_void_p),
                                                  life.ctypes.data_as(C.c_void_p), cell.ctypes.data_as(C.c_void_p),
                                                  pts.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(nid), self._stream()))
        k = n.value
        return dict(ids=ids[:k], lifetime=life[:k], cell=cell[:k], cam0=pts[:k, :2].copy(), cam1=pts[:k, 2:].copy(),
                    next_feature_id=nid.value)

    def read_counters(self, stream=0):
        out = (C.c_int32 * 8)()
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_counters(self._h, int(stream), C.byref(out), self._stream()))
        return dict(zip(COUNTER_NAMES, [int(v) for v in out]))

    def read_match_counts(self, stream=0):
        """(candidates stereo-matched in round 1, in round 2) of the last step (lazy matching, airvision.h)."""
        out = (C.c_int32 * 2)()
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_match_counts(self._h, int(stream), C.byref(out), self._stream()))
        return int(out[0]), int(out[1])

    def read_ransac_counts(self, stream=0):
        """Outlier rejection of the last step (config.use_ransac): dict(after_ransac, cam0_set, cam1_set, path) with path = cam0
        code | cam1 code << 4 of the AV_RANSAC_PATH_* codes; zeros when the switch is off or nothing was tracked."""
        out = (C.c_int32 * 4)()
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_ransac_counts(self._h, int(stream), C.byref(out), self._stream()))
        return dict(zip(RANSAC_COUNT_NAMES, [int(v) for v in out]))

    def read_image(self, stream=0, cam=0):
        """The level-0 image the last step used for camera `cam` of `stream`, uint8[height, width] (the processed size): the frame
        converted to 8-bit grey (config.image_format other than 'gray8'), photometrically corrected (config.cam*_response /
        cam*_vignette), binned (config.image_downscale 2 or 4), equalised with config.use_clahe.  Refused (AirvisionError,
        AV_E_INVALID) with none of them: level 0 is then the caller's own image."""
        out = np.empty((self.height, self.width), np.uint8)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_image(self._h, int(stream), int(cam), out.ctypes.data_as(C.c_void_p), self._stream()))
        return out

    def read_range(self):
        """int32 [S, 2]: the (lo, hi) the frames of the last step were scaled with (config.gray16_scale 'window' or 'auto'), after
        `step` (prestaged or not) and `step_host`.  Refused (AirvisionError, AV_E_INVALID) with gray16_scale 'shift', before the first
        step and after a `step_frames`: an entry of the frame store is shared by streams and keeps no range."""
        out = np.empty((self.n_streams, 2), np.int32)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_frontend_read_range(self._h, out.ctypes.data_as(C.c_void_p), self._stream()))
        return out

    def enable_timing(self, max_spans):
        """Bracket every launch group with HIP events on the step's stream (bench roofline leg)."""
        N.check(N.lib().av_frontend_enable_timing(self._h, int(max_spans)))

    def read_timing(self):
        """{class: (total_ms, n_launch_groups)} since the last read; synchronises the device."""
        ms = (C.c_double * 4)(); n = (C.c_int32 * 4)()
        N.check(N.lib().av_frontend_read_timing(self._h, C.byref(ms), C.byref(n)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(('pyramid', 'lk', 'fast', 'glue'))}

    def read_all_counters(self):
        return [self.read_counters(s) for s in range(self.n_streams)]
