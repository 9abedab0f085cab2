"""Operator-level Python front of the C ABI: numpy in / numpy out, computed on cuda:<device>.

One function per third-party native call of the reference, with the
argument meaning of the reference call sites so the parity tests read like the reference code.
torch is used only to own device memory and the stream; all arithmetic is in libairvision_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N


def _dev(device):
    return torch.device('cuda', device)


def pyramid_layout(w, h, levels):
    lay = N.PyrLayout()
    N.check(N.lib().av_pyramid_layout(w, h, levels, C.byref(lay)))
    return lay


def build_pyramids(images, levels, device=0, write_level0=True, out=None):
    """images: uint8[n,h,w] (numpy or cuda tensor) -> (uint8 cuda tensor [n, bytes], layout).

    write_level0=False builds levels 1 and up only (av_pyramid_build_levels): the level-0 region keeps what `out` (a uint8 cuda
    tensor [n, bytes], or a fresh uninitialised one) held."""
    t = torch.as_tensor(images)
    if t.dim() == 2:
        t = t[None]
    t = t.to(_dev(device), dtype=torch.uint8).contiguous()
    n, h, w = t.shape
    lay = pyramid_layout(w, h, levels)
    if out is None:
        out = torch.empty((n, lay.bytes), dtype=torch.uint8, device=_dev(device))
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, lay.bytes) or not out.is_contiguous() or out.device != t.device:
        raise ValueError('out must be a contiguous uint8 tensor [%d, %d] on %s' % (n, lay.bytes, t.device))
    build = N.lib().av_pyramid_build if write_level0 else N.lib().av_pyramid_build_levels
    with torch.cuda.device(device):
        N.check(build(N.dptr(t), w * h, n, w, h, levels, N.dptr(out), lay.bytes, N.current_stream()))
    return out, lay


def pyramid_level(pyr_row, lay, level, with_border=False):
    """numpy view of one level of one pyramid (for tests)."""
    a = pyr_row.cpu().numpy()
    B = N.AV_PYR_BORDER
    w, h, pitch, off = lay.w[level], lay.h[level], lay.pitch[level], lay.offset[level]
    full = a[off:off + pitch * (h + 2 * B)].reshape(h + 2 * B, pitch)
    return full[:, :w + 2 * B] if with_border else full[B:B + h, B:B + w]


def calc_optical_flow_pyr_lk(prev_img, next_img, prev_pts, next_pts, winSize=(15, 15), maxLevel=3,
                             criteria=(3, 30, 0.01), flags=4, minEigThreshold=1e-4, device=0, level0_in_place=False):
    """cv2.calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, **lk_params) on the GPU
    (reference: feature_tracker.py:102-108, stereo_matcher.py:64-74, config.py:37-44).
    Returns (next_pts float32[N,2], status uint8[N,1], None).
    level0_in_place: level 0 is read from the images themselves (av_lk_track_images, the engine's way: the level-0 regions of the
    pyramids are left unwritten and unread); the results are the same."""
    if not (flags & 4):
        raise ValueError('only OPTFLOW_USE_INITIAL_FLOW is implemented (the reference always sets it)')
    ctype, max_iter, eps = criteria
    max_iter = int(max_iter) if (ctype & 1) else 30
    eps = float(eps) if (ctype & 2) else 0.01
    prev = np.ascontiguousarray(np.asarray(prev_pts, dtype=np.float32).reshape(-1, 2))
    nxt = np.ascontiguousarray(np.asarray(next_pts, dtype=np.float32).reshape(-1, 2))
    n = prev.shape[0]
    if n == 0:
        return nxt.copy(), np.zeros((0, 1), np.uint8), None
    imgs = np.stack([np.asarray(prev_img, dtype=np.uint8), np.asarray(next_img, dtype=np.uint8)])
    # levels OpenCV would not build are not laid out either (cv::buildOpticalFlowPyramid stops before the first level that is
    # no larger than the window; av_lk_track applies the same rule to whatever it is handed)
    lw, lh, eff = imgs.shape[2], imgs.shape[1], 0
    while eff < maxLevel and (lw + 1) // 2 > winSize[0] and (lh + 1) // 2 > winSize[1]:
        lw, lh, eff = (lw + 1) // 2, (lh + 1) // 2, eff + 1
    maxLevel = eff
    dev = _dev(device)
    d_imgs = torch.from_numpy(imgs).to(dev)
    if level0_in_place:          # levels 1 and up only, over a zeroed buffer: where the library leaves level 0 unwritten it holds no image
        pyr, lay = build_pyramids(d_imgs, maxLevel + 1, device, write_level0=False,
                                  out=torch.zeros((2, pyramid_layout(imgs.shape[2], imgs.shape[1], maxLevel + 1).bytes), dtype=torch.uint8, device=dev))
    else:
        pyr, lay = build_pyramids(d_imgs, maxLevel + 1, device)
    d_prev = torch.from_numpy(prev).to(dev)
    d_next = torch.from_numpy(nxt).to(dev)
    d_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_count = torch.tensor([n], dtype=torch.int32, device=dev)
    h, w = imgs.shape[1:]
    with torch.cuda.device(device):
        tail = (lay.bytes, 1, w, h, maxLevel + 1, N.dptr(d_prev), N.dptr(d_next), N.dptr(d_status), N.dptr(d_count), n,
                int(winSize[0]), max_iter, eps, float(minEigThreshold), N.current_stream())
        if level0_in_place:
            N.check(N.lib().av_lk_track_images(N.dptr(d_imgs[0]), N.dptr(d_imgs[1]), w * h, N.dptr(pyr[0]), N.dptr(pyr[1]), *tail))
        else:
            N.check(N.lib().av_lk_track(N.dptr(pyr[0]), N.dptr(pyr[1]), *tail))
        torch.cuda.synchronize()
    return d_next.cpu().numpy(), d_status.cpu().numpy().reshape(-1, 1), None


KP_RASTER_BITS, KP_RASTER_BITS_WIDE = 19, 24         # av_fast_detect / av_fast_detect_wide (include/airvision.h)


def kp_raster_bits(w, h):
    """Raster bits of the keypoint words of a w x h image: the narrow format wherever it fits, so that sizes up to 2^19 pixels go
    through av_fast_detect as they always did."""
    if w * h > N.AV_MAX_IMAGE_PIXELS:
        raise ValueError('fast_detect: %d x %d exceeds AV_MAX_IMAGE_PIXELS = 2^24 pixels' % (w, h))
    return KP_RASTER_BITS if w * h <= (1 << KP_RASTER_BITS) else KP_RASTER_BITS_WIDE


def pack_keypoints(x, y, score, w, bits):
    """(x, y, score) -> packed words uint32: score << bits | (2^bits - 1 - (y * w + x))."""
    raster = np.asarray(y, np.int64) * int(w) + np.asarray(x, np.int64)
    score = np.asarray(score, np.int64)
    if raster.size and (raster.min() < 0 or raster.max() >= (1 << bits) or score.min() < 0 or (score.max() << bits) >= (1 << 32)):
        raise ValueError('pack_keypoints: raster or score outside the %d-bit format' % bits)
    return ((score << bits) | (((1 << bits) - 1) - raster)).astype(np.uint32)


def unpack_keypoints(words, w, bits):
    """Packed words of either format -> (x, y, score) int arrays in raster order."""
    words = np.asarray(words).view(np.uint32)
    m = np.uint32((1 << bits) - 1)
    raster = (m - (words & m)).astype(np.int64)
    score = (words >> np.uint32(bits)).astype(np.int32)
    order = np.argsort(raster, kind='stable')
    raster, score = raster[order], score[order]
    return (raster % w).astype(np.int32), (raster // w).astype(np.int32), score


def fast_detect(img, threshold, mask=None, cap=1 << 16, device=0):
    """cv2.FastFeatureDetector_create(threshold).detect(img, mask): (x, y, response) int arrays in
    raster order (reference: pipeline.py:23-25, feature_initializer.py:52, feature_adder.py:64).  Images of up to 2^19 pixels go
    through av_fast_detect, larger ones (up to AV_MAX_IMAGE_PIXELS) through av_fast_detect_wide; the result is decoded either way."""
    dev = _dev(device)
    t = torch.as_tensor(np.ascontiguousarray(img, dtype=np.uint8)).to(dev)
    h, w = t.shape
    bits = kp_raster_bits(w, h)
    entry = N.lib().av_fast_detect if bits == KP_RASTER_BITS else N.lib().av_fast_detect_wide
    m = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8)).to(dev)
    kp = torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(device):
        N.check(entry(N.dptr(t), w * h, None if m is None else N.dptr(m), w * h, 1, w, h, int(threshold),
                      N.dptr(kp), N.dptr(cnt), cap, N.current_stream()))
        torch.cuda.synchronize()
    n = int(cnt.item())
    if n > cap:
        raise N.AirvisionError(N.AV_E_CAPACITY, 'FAST found %d keypoints, capacity %d' % (n, cap))
    return unpack_keypoints(kp[:n].cpu().numpy(), w, bits)


def _points_op(fn_name, pts_in, extra, device):
    arr = np.asarray(pts_in)
    out_f32 = arr.dtype == np.float32
    pts = np.ascontiguousarray(arr.reshape(-1, 2), dtype=np.float64)
    n = pts.shape[0]
    if n == 0:
        return pts.astype(np.float32) if out_f32 else pts
    dev = _dev(device)
    d_in = torch.from_numpy(pts).to(dev)
    d_out = torch.empty_like(d_in)
    with torch.cuda.device(device):
        N.check(getattr(N.lib(), fn_name)(N.dptr(d_in), n, *extra, N.dptr(d_out), N.current_stream()))
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return out.astype(np.float32) if out_f32 else out


def undistort_points(pts_in, intrinsics, distortion_coeffs, rectification_matrix=None, device=0, distortion_model='radtan'):
    """cv2.undistortPoints(pts, K, D, None, R, P=I) -- or, for distortion_model 'equidistant', cv2.fisheye.undistortPoints(pts, K,
    D, R, P=I) (reference: camera_model.py:24-47)."""
    R = np.eye(3) if rectification_matrix is None else np.asarray(rectification_matrix, dtype=np.float64)
    extra = (N.darr(intrinsics), N.darr(distortion_coeffs), N.darr(R.reshape(-1)), N.distortion_model_code(distortion_model))
    return _points_op('av_undistort_points_model', pts_in, extra, device)


def distort_points(pts_in, intrinsics, distortion_coeffs, device=0, distortion_model='radtan'):
    """cv2.projectPoints(homogeneous(pts), 0, 0, K, D) -- or cv2.fisheye.distortPoints(pts, K, D) for 'equidistant' (reference:
    camera_model.py:49-75)."""
    extra = (N.darr(intrinsics), N.darr(distortion_coeffs), N.distortion_model_code(distortion_model))
    return _points_op('av_distort_points_model', pts_in, extra, device)


def ransac_num_hypotheses(success_probability=0.99):
    """Hypotheses the two-point RANSAC draws for a success probability (av_ransac_num_hypotheses): 7 at 0.99."""
    return int(N.lib().av_ransac_num_hypotheses(float(success_probability)))


def ransac_hash(seed, frame, camera, k, draw):
    """The draw hash of the two-point RANSAC (include/airvision.h writes it out)."""
    return int(N.lib().av_ransac_hash(int(seed) & 0xFFFFFFFF, int(frame) & 0xFFFFFFFF, int(camera), int(k), int(draw)))


def two_point_ransac_batch(pts1, pts2, R_p_c, intrinsics, distortion_model, distortion_coeffs, inlier_error, success_probability=0.99,
                           seed=0, frames=None, cameras=None, device=0):
    """B problems of one camera model in one launch (av_two_point_ransac): pts1 / pts2 lists of float32[n_b, 2], R_p_c [B, 3, 3],
    frames / cameras int[B] (default 0).  Returns (markers: list of uint8[n_b], info int32[B, 2] = markers set, path code)."""
    B = len(pts1)
    assert len(pts2) == B
    p1 = [np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in pts1]
    p2 = [np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in pts2]
    sizes = [len(p) for p in p1]
    assert sizes == [len(p) for p in p2], 'pts1 and pts2 must pair up'
    if B == 0:
        return [], np.zeros((0, 2), np.int32)
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    total, max_pairs = int(off[-1]), max(sizes)
    if max_pairs > N.AV_RANSAC_MAX_PAIRS:
        raise ValueError('two_point_ransac: %d pairs in one problem, at most %d' % (max_pairs, N.AV_RANSAC_MAX_PAIRS))
    dev = _dev(device)
    cat = lambda ps: np.ascontiguousarray(np.concatenate(ps, axis=0)) if total else np.zeros((1, 2), np.float32)      # noqa: E731
    d1 = torch.from_numpy(cat(p1)).to(dev)
    d2 = torch.from_numpy(cat(p2)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_R = torch.from_numpy(np.ascontiguousarray(np.asarray(R_p_c, dtype=np.float64).reshape(B, 9))).to(dev)
    d_fr = torch.from_numpy(np.ascontiguousarray(np.zeros(B) if frames is None else frames, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)
    d_cam = torch.from_numpy(np.ascontiguousarray(np.zeros(B) if cameras is None else cameras, dtype=np.int32)).to(dev)
    d_mark = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
    d_info = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(device):
        N.check(N.lib().av_two_point_ransac(N.dptr(d1), N.dptr(d2), N.dptr(d_off), B, max_pairs, N.dptr(d_R), N.dptr(d_cam), N.dptr(d_fr),
                                            N.darr(intrinsics), N.darr(distortion_coeffs), N.distortion_model_code(distortion_model),
                                            float(inlier_error), float(success_probability), int(seed) & 0xFFFFFFFF,
                                            N.dptr(d_mark), N.dptr(d_info), N.current_stream()))
        torch.cuda.synchronize()
    mark = d_mark.cpu().numpy()
    return [mark[off[b]:off[b + 1]].copy() for b in range(B)], d_info.cpu().numpy()


def two_point_ransac(pts1, pts2, R_p_c, intrinsics, distortion_model, distortion_coeffs, inlier_error, success_probability=0.99,
                     seed=0, frame=0, camera=0, device=0):
    """Two-point RANSAC on the temporal matches of one camera: pts1 / pts2 float32[n, 2] pixel positions of the same features in the
    previous / current image, R_p_c the rotation previous -> current camera frame (IMUProcessor.integrate_imu_data), inlier_error in
    pixels (config.ransac_threshold).  Returns uint8[n] markers.  This is the step feature_tracker.py:135-136 leaves empty; the
    algorithm is written out in include/airvision.h."""
    marks, _info = two_point_ransac_batch([pts1], [pts2], [R_p_c], intrinsics, distortion_model, distortion_coeffs, inlier_error,
                                          success_probability, seed, [frame], [camera], device)
    return marks[0]


def clahe(img, clip_limit=2.0, tiles=(8, 8), out=None, return_lut=False, device=0):
    """Contrast-limited adaptive histogram equalisation (av_clahe; the definition is written out in include/airvision.h): img uint8
    [n, h, w] or [h, w], a cuda tensor or anything torch.as_tensor takes; tiles = (tiles_x, tiles_y).  Returns a uint8 cuda tensor of
    the same shape -- `out` itself if given (a contiguous uint8 cuda tensor of that shape; out = img works in place) -- and with
    return_lut the look-up tables as well, uint8 [n, tiles_y * tiles_x, 256]."""
    t = torch.as_tensor(img)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError('clahe: uint8 [n, h, w] or [h, w] images, got %s %s' % (t.dtype, tuple(t.shape)))
    t = t.to(_dev(device)).contiguous()
    shape = tuple(t.shape)
    h, w = shape[-2:]
    n = shape[0] if t.dim() == 3 else 1
    if out is None:
        out = torch.empty_like(t)
    elif not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError('clahe: out must be a contiguous uint8 cuda tensor of shape %s' % (shape,))
    tx, ty = [int(v) for v in tiles]
    lut = torch.empty((n, max(tx * ty, 1), 256), dtype=torch.uint8, device=_dev(device)) if return_lut else None
    with torch.cuda.device(device):
        N.check(N.lib().av_clahe(N.dptr(t), w * h, n, w, h, float(clip_limit), tx, ty, N.dptr(out), w * h,
                                 None if lut is None else N.dptr(lut), N.current_stream()))
    return (out, lut) if return_lut else out


def to_gray8(img, pixel_format, shift=8, out=None, device=0):
    """Camera frames of another pixel format to 8-bit grey (av_to_gray8; formats and arithmetic are written out in include/airvision.h).
    pixel_format: 'gray8' | 'gray16' | 'rgb8' | 'bgr8' | 'rgba8' | 'bgra8' | 'bayer_{rggb,bggr,grbg,gbrg}{8,16}' | 'gray{10p,12p,10_csi2,
    12_csi2}' | 'bayer_{rggb,bggr,grbg,gbrg}{10p,12p,10_csi2,12_csi2}' or the AV_PIX_* code.
    img: [n, h, w] or [h, w] for the grey formats and the Bayer mosaics (at least 2 x 2: ValueError otherwise) -- uint16 for 'gray16' and
    'bayer_*16' (a cuda tensor may also be torch.int16 holding the same bits) -- and uint8 [n, h, w, c] or [h, w, c]
    with c = 3 / 4 for the colour ones, and uint8 [n, h, w * d / 8] or [h, w * d / 8] for the packed 10 / 12-bit transports ('gray12p',
    'bayer_rggb10_csi2', ..: w is taken from the last dimension, which must be whole groups of 5 / 3 bytes; shift applies to the sample
    left-justified to 16 bits; a packed MOSAIC is converted in two passes through a scratch that the call allocates and frees, so for
    those formats alone the call waits for the stream and cannot be captured into a graph -- the engine owns its scratch and does neither); a cuda tensor or anything torch.as_tensor takes.  A cuda tensor is read where it lies: each
    image must be contiguous, the images may be any distance apart (a slice of a larger tensor), at any address.  shift: the 16-bit
    formats only, 0 .. 8.  Returns a uint8 cuda tensor [n, h, w] or [h, w] -- `out` itself if given (uint8 cuda, that shape, each image contiguous;
    it must not overlap img)."""
    fmt = N.pixel_format_code(pixel_format)
    shift = N.gray16_shift_value(shift)
    t = torch.as_tensor(img)
    if N.is_packed(fmt):
        return _packed_to_gray8(t, fmt, shift, out, device)
    bpp = N.PIXEL_BYTES[fmt]
    colour = bpp >= 3
    dtypes = (torch.uint16, torch.int16) if N.is_16bit(fmt) else (torch.uint8,)
    core = 3 if colour else 2                                  # dimensions of one image
    if t.dtype not in dtypes or t.dim() not in (core, core + 1) or (colour and t.shape[-1] != bpp):
        raise ValueError('to_gray8: %s images are %s [n, h, w%s] or [h, w%s], got %s %s' % (
            N.PIXEL_FORMAT_NAMES[fmt], ' / '.join(str(d) for d in dtypes), ', %d' % bpp if colour else '', ', %d' % bpp if colour else '', t.dtype, tuple(t.shape)))
    if N.is_bayer(fmt) and (t.shape[-1] < 2 or t.shape[-2] < 2):
        raise ValueError('to_gray8: a Bayer mosaic is at least 2 x 2 samples, got %s' % (tuple(t.shape),))
    t = t.to(_dev(device))
    batched = t.dim() == core + 1
    tb = t if batched else t.unsqueeze(0)
    if not tb[0].is_contiguous():
        tb = tb.contiguous()
    n, h, w = tb.shape[0], tb.shape[1], tb.shape[2]
    if n > 1 and tb.stride(0) < h * w * (bpp if colour else 1):
        tb = tb.contiguous()
    oshape = (n, h, w) if batched else (h, w)
    if out is None:
        out = torch.empty(oshape, dtype=torch.uint8, device=_dev(device))
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == oshape):
        raise ValueError('to_gray8: out must be a uint8 cuda tensor of shape %s' % (oshape,))
    ob = out if batched else out.unsqueeze(0)
    if not ob[0].is_contiguous() or (n > 1 and ob.stride(0) < h * w):
        raise ValueError('to_gray8: every image of out must be contiguous')
    in_stride = (tb.stride(0) if n > 1 else h * w * (bpp if colour else 1)) * tb.element_size()
    out_stride = ob.stride(0) if n > 1 else h * w
    with torch.cuda.device(device):
        N.check(N.lib().av_to_gray8(N.dptr(tb), in_stride, n, w, h, fmt, shift, N.dptr(ob), out_stride, N.current_stream()))
    return out


def _packed_to_gray8(t, fmt, shift, out, device):
    """to_gray8 for the packed transports: t uint8 [n, h, w * d / 8] or [h, w * d / 8]."""
    name, d = N.PIXEL_FORMAT_NAMES[fmt], N.packed_depth(fmt)
    gpx, gb = N.packed_group(fmt)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3) or t.shape[-1] == 0 or t.shape[-1] % gb:
        raise ValueError('to_gray8: %s images are torch.uint8 [n, h, w * %d / 8] or [h, w * %d / 8] with rows of whole %d-byte groups, got %s %s' % (
            name, d, d, gb, t.dtype, tuple(t.shape)))
    wb = int(t.shape[-1])
    w = wb // gb * gpx
    if N.is_bayer(fmt) and (w < 2 or t.shape[-2] < 2):
        raise ValueError('to_gray8: a Bayer mosaic is at least 2 x 2 samples, got %s' % (tuple(t.shape),))
    t = t.to(_dev(device))
    batched = t.dim() == 3
    tb = t if batched else t.unsqueeze(0)
    n, h = tb.shape[0], tb.shape[1]
    if not tb[0].is_contiguous() or (n > 1 and tb.stride(0) < h * wb):
        tb = tb.contiguous()
    oshape = (n, h, w) if batched else (h, w)
    if out is None:
        out = torch.empty(oshape, dtype=torch.uint8, device=_dev(device))
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == oshape):
        raise ValueError('to_gray8: out must be a uint8 cuda tensor of shape %s' % (oshape,))
    ob = out if batched else out.unsqueeze(0)
    if not ob[0].is_contiguous() or (n > 1 and ob.stride(0) < h * w):
        raise ValueError('to_gray8: every image of out must be contiguous')
    in_stride = tb.stride(0) if n > 1 else h * wb
    out_stride = ob.stride(0) if n > 1 else h * w
    with torch.cuda.device(device):
        N.check(N.lib().av_to_gray8(N.dptr(tb), in_stride, n, w, h, fmt, shift, N.dptr(ob), out_stride, N.current_stream()))
    return out


def downscale(img, factor, out=None, device=0):
    """2 x 2 / 4 x 4 binning of 8-bit grey frames (av_downscale; the arithmetic is written out in include/airvision.h):
    out(x, y) = (sum of the f x f block + f * f / 2) >> 2 log2 f.  img: uint8 [n, H, W] or [H, W] with H and W divisible by factor (2 or
    4; ValueError otherwise), a cuda tensor or anything torch.as_tensor takes.  A cuda tensor is read where it lies: each image must be
    contiguous, the images may be any distance apart, at any address.  Returns a uint8 cuda tensor [n, H / f, W / f] or [H / f, W / f]
    -- `out` itself if given (uint8 cuda, that shape, each image contiguous; it must not overlap img)."""
    if isinstance(factor, bool) or factor not in (2, 4):
        raise ValueError('downscale: factor %r is neither 2 nor 4' % (factor,))
    f = int(factor)
    t = torch.as_tensor(img)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError('downscale: images are torch.uint8 [n, H, W] or [H, W], got %s %s' % (t.dtype, tuple(t.shape)))
    H, W = int(t.shape[-2]), int(t.shape[-1])
    if H == 0 or W == 0 or H % f or W % f:
        raise ValueError('downscale: %d x %d is not divisible by the factor %d' % (W, H, f))
    t = t.to(_dev(device))
    batched = t.dim() == 3
    tb = t if batched else t.unsqueeze(0)
    n = tb.shape[0]
    if (n and not tb[0].is_contiguous()) or (n > 1 and tb.stride(0) < H * W):
        tb = tb.contiguous()
    h, w = H // f, W // f
    oshape = (n, h, w) if batched else (h, w)
    if out is None:
        out = torch.empty(oshape, dtype=torch.uint8, device=_dev(device))
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == oshape):
        raise ValueError('downscale: out must be a uint8 cuda tensor of shape %s' % (oshape,))
    ob = out if batched else out.unsqueeze(0)
    if (n and not ob[0].is_contiguous()) or (n > 1 and ob.stride(0) < h * w):
        raise ValueError('downscale: every image of out must be contiguous')
    in_stride = tb.stride(0) if n > 1 else H * W
    out_stride = ob.stride(0) if n > 1 else h * w
    with torch.cuda.device(device):
        N.check(N.lib().av_downscale(N.dptr(tb), in_stride, n, W, H, f, N.dptr(ob), out_stride, N.current_stream()))
    return out


def photometric(images, response=None, gain=None, out=None, device=0, exposure=None):
    """Photometric calibration of 8-bit grey frames (av_photometric; the arithmetic is written out in include/airvision.h):
    out = min(255, (response[p] * gain[x] + 2^19) >> 20).  images: uint8 [n, h, w] or [h, w], a cuda tensor or anything torch.as_tensor
    takes.  A cuda tensor is read where it lies: each image must be contiguous, the images may be any distance apart, at any address.
    response: uint16[256] in Q8 (entries <= 65280) or None; gain: uint16 [h, w] in Q12, one map for all images, or None
    (frontend.photometric_tables makes both); a cuda tensor (torch.uint16, or torch.int16 holding the same bits) is used where it lies.
    At least one of the two.  Returns a uint8 cuda tensor of images' shape -- `out` itself if given (uint8 cuda, that shape, each image
    contiguous); out may be the input itself (in place), any other overlap is refused.
    exposure: the exposure factors of the images ("Exposure-time normalisation" in include/airvision.h; av_photometric_exposure), uint16
    [n] in Q12 as frontend.quantise_exposure makes them -- a host array or a cuda tensor -- image i then goes through the table
    min(65280, (response[p] * k[i] + 2048) >> 12).  With them neither a response nor a gain is required."""
    t = torch.as_tensor(images)
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError('photometric: images are torch.uint8 [n, h, w] or [h, w], got %s %s' % (t.dtype, tuple(t.shape)))
    if response is None and gain is None and exposure is None:
        raise ValueError('photometric: neither a response table nor a gain map nor exposure factors')
    t = t.to(_dev(device))
    batched = t.dim() == 3
    tb = t if batched else t.unsqueeze(0)
    n, h, w = tb.shape
    if (n and not tb[0].is_contiguous()) or (n > 1 and tb.stride(0) < h * w):
        tb = tb.contiguous()

    def table(a, what, shape):
        if isinstance(a, torch.Tensor):
            ok = a.dtype in tuple(d for d in (getattr(torch, 'uint16', None), torch.int16) if d is not None) and tuple(a.shape) == shape
            if not ok or not a.is_cuda or not a.is_contiguous():
                raise ValueError('photometric: %s is a contiguous uint16 cuda tensor of shape %s, got %s %s' % (what, shape, a.dtype, tuple(a.shape)))
            return a
        a = np.asarray(a)
        if a.dtype != np.uint16 or tuple(a.shape) != shape:
            raise ValueError('photometric: %s is uint16 %s, got %s %s' % (what, shape, a.dtype, tuple(a.shape)))
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(_dev(device))
    r = None if response is None else table(response, 'response', (256,))
    g = None if gain is None else table(gain, 'gain', (h, w))
    k = None if exposure is None else table(exposure, 'exposure', (n,))
    oshape = tuple(t.shape)
    if out is None:
        out = torch.empty(oshape, dtype=torch.uint8, device=_dev(device))
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == oshape):
        raise ValueError('photometric: out must be a uint8 cuda tensor of shape %s' % (oshape,))
    ob = out if batched else out.unsqueeze(0)
    if (n and not ob[0].is_contiguous()) or (n > 1 and ob.stride(0) < h * w):
        raise ValueError('photometric: every image of out must be contiguous')
    in_stride = tb.stride(0) if n > 1 else h * w
    out_stride = ob.stride(0) if n > 1 else h * w
    with torch.cuda.device(device):
        if k is None:
            N.check(N.lib().av_photometric(N.dptr(tb), N.dptr(ob), n, w, h, in_stride, out_stride, None if r is None else N.dptr(r),
                                           None if g is None else N.dptr(g), N.current_stream()))
        else:
            N.check(N.lib().av_photometric_exposure(N.dptr(tb), N.dptr(ob), n, w, h, in_stride, out_stride, None if r is None else N.dptr(r),
                                                    None if g is None else N.dptr(g), N.dptr(k), N.current_stream()))
    return out


def to_gray8_range(img, scale='auto', window=None, clip=(100, 100), min_span=256, pool=1, index=None, out=None, work=None, device=0):
    """16-bit grey frames to 8-bit grey through a window instead of a fixed shift (av_to_gray8_range; "Range scaling of 16-bit grey" in
    include/airvision.h has the arithmetic, frontend.gray16_range is its NumPy twin).  img: uint16 [n, h, w] or [h, w] (a cuda tensor may
    also be torch.int16 holding the same bits), read where it lies: each image contiguous, any distance apart, at any address.
    scale 'window': `window` = (lo, hi) for every image.  scale 'auto': every group of `pool` (1 or 2) consecutive images -- 2 = the
    cam0 and cam1 frames of a stereo pair, interleaved -- gets its own range from the group's pooled histogram, with `clip` = (ppm_lo,
    ppm_hi) and `min_span`.  index: one int per group, or None: group g is written to images index[g] * pool .. of `out` (which must then
    be given, uint8 cuda [m, h, w]); a negative entry skips the group, of an entry named twice the last group is written.  work: None, or
    a torch.int32 cuda tensor of at least (n // pool) * AV_GRAY16_WORK_WORDS zeros that 'auto' works in and leaves zero in its histogram
    part, the first 4096 * (n // pool) words (without it the call allocates one and waits for the stream).
    Returns (grey, ranges): the uint8 cuda tensor of img's shape (`out` itself if given) and an int32 cuda tensor [n // pool, 2] of the
    (lo, hi) of every group, (-1, -1) for a group that was not written."""
    mode, lo, hi, ppm_lo, ppm_hi, span = N.gray16_range_settings(scale, window, clip, min_span)
    if mode == N.AV_GRAY16_SHIFT:
        raise ValueError("to_gray8_range: scale is 'window' or 'auto' (ops.to_gray8 is the shift)")
    t = torch.as_tensor(img)
    if t.dtype not in (torch.uint16, torch.int16) or t.dim() not in (2, 3):
        raise ValueError('to_gray8_range: images are torch.uint16 / torch.int16 [n, h, w] or [h, w], got %s %s' % (t.dtype, tuple(t.shape)))
    t = t.to(_dev(device))
    batched = t.dim() == 3
    tb = t if batched else t.unsqueeze(0)
    n, h, w = tb.shape
    if pool not in (1, 2) or n % pool:
        raise ValueError('to_gray8_range: pool is 1 or 2 and divides the number of images (%d), got %r' % (n, pool))
    if (n and not tb[0].is_contiguous()) or (n > 1 and tb.stride(0) < h * w):
        tb = tb.contiguous()
    groups = n // pool
    oshape = tuple(t.shape)
    if out is None:
        if index is not None:
            raise ValueError('to_gray8_range: an index needs `out`')
        out = torch.empty(oshape, dtype=torch.uint8, device=_dev(device))
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and (
            tuple(out.shape) == oshape if index is None else out.dim() == 3 and tuple(out.shape[1:]) == (h, w))):
        raise ValueError('to_gray8_range: out must be a uint8 cuda tensor of shape %s' % (oshape if index is None else ('m', h, w),))
    ob = out if out.dim() == 3 else out.unsqueeze(0)
    if (ob.shape[0] and not ob[0].is_contiguous()) or (ob.shape[0] > 1 and ob.stride(0) < h * w):
        raise ValueError('to_gray8_range: every image of out must be contiguous')
    first = None
    if index is not None:
        idx = [int(v) for v in index]
        if len(idx) != groups or any(e >= 0 and (e + 1) * pool > ob.shape[0] for e in idx):
            raise ValueError('to_gray8_range: index has one entry per group (%d), each negative or inside out (%d images)' % (groups, ob.shape[0]))
        last = {e: g for g, e in enumerate(idx)}
        first = torch.tensor([e if e >= 0 and last[e] == g else -1 for g, e in enumerate(idx)], dtype=torch.int32, device=_dev(device))
    if work is not None and not (isinstance(work, torch.Tensor) and work.is_cuda and work.dtype == torch.int32 and work.is_contiguous()
                                 and work.numel() >= groups * N.AV_GRAY16_WORK_WORDS):
        raise ValueError('to_gray8_range: work is a contiguous torch.int32 cuda tensor of at least %d elements' % (groups * N.AV_GRAY16_WORK_WORDS))
    ranges = torch.full((groups, 2), -1, dtype=torch.int32, device=_dev(device))
    in_stride = (tb.stride(0) if n > 1 else h * w) * tb.element_size()
    out_stride = ob.stride(0) if ob.shape[0] > 1 else h * w
    with torch.cuda.device(device):
        N.check(N.lib().av_to_gray8_range(N.dptr(tb), in_stride, n, w, h, mode, lo, hi, ppm_lo, ppm_hi, span, pool,
                                          None if first is None else N.dptr(first), N.dptr(ob), out_stride, N.dptr(ranges),
                                          None if work is None else N.dptr(work), N.current_stream()))
    return out, ranges
