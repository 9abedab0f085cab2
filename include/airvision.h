/*
 * airvision.h -- C ABI of libairvision_hip.so, the MI355X (gfx950) implementation of
 * UAV-Airvision's per-frame hot path.
 *
 * The reference (BUBLET/uav-airvision) is pure Python; its "FFI" for this path is the set of
 * third-party native calls listed in SURVEY.md section 2.1 (K1-K13) plus the Python call surface of
 * section 8(b).  Each entry point below names the reference interface it replaces (file:line,
 * relative to the reference's src/).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions: every function returns 0 on success and a negative AV_E_*
 * code on error, never throws; `*_dev` pointers are device (HBM) pointers, everything else is host
 * memory owned by the caller and only read/written during the call; the library owns the device
 * memory of a context; there is no process-global state; `stream` is a hipStream_t (NULL = the
 * default stream).  Unless a function says it synchronises, work is only ENQUEUED on `stream`.
 */
#ifndef AIRVISION_H
#define AIRVISION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AV_OK            0
#define AV_E_INVALID    -1   /* bad argument / unsupported shape */
#define AV_E_HIP        -2   /* a HIP runtime call failed (see av_last_error) */
#define AV_E_CAPACITY   -3   /* a device-side capacity was exceeded (e.g. FAST corners > max_corners) */
#define AV_E_NODEVICE   -4   /* no gfx950 device visible */
#define AV_E_NUMERIC    -5   /* a factorisation met a non-positive or non-finite pivot (per-stream: that stream is stopped) */

#define AV_MAX_LEVELS    5   /* pyramid levels 0..4 (the reference uses maxLevel = 3, config.py:34) */
#define AV_PYR_BORDER   16   /* border (pixels) of every padded pyramid level; >= LK win + 1 */
/* The one limit on the size of an image: width * height <= AV_MAX_IMAGE_PIXELS for the front-end engine (every entry path),
 * av_fast_detect_wide and av_clahe; the pyramids and av_lk_track take at least that.  (av_fast_detect alone keeps the 2^19 pixels its
 * word format holds.)  The minimum sizes are each function's own: every pyramid level wider and higher than AV_PYR_BORDER, 7 x 7 for
 * the detector. */
#define AV_MAX_IMAGE_PIXELS (1 << 24)

/* Thread-local text of the last error raised on the calling thread. */
const char* av_last_error(void);
/* Library version / build info string. */
const char* av_version(void);
/* Number of visible HIP devices (does not initialise a context beyond the count). */
int av_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Padded u8 pyramids.  A pyramid is one contiguous device allocation holding levels 0..levels-1,
 * each level stored with an AV_PYR_BORDER-pixel BORDER_REFLECT_101 frame (what OpenCV's
 * buildOpticalFlowPyramid produces internally for calcOpticalFlowPyrLK).
 * ------------------------------------------------------------------------------------------- */
typedef struct av_pyr_layout {
    int32_t levels;
    int32_t w[AV_MAX_LEVELS], h[AV_MAX_LEVELS];      /* interior size of each level                */
    int32_t pitch[AV_MAX_LEVELS];                    /* bytes per padded row                       */
    int64_t offset[AV_MAX_LEVELS];                   /* byte offset of the padded level's (0,0)    */
    int64_t bytes;                                   /* total bytes of one pyramid (16-B multiple) */
} av_pyr_layout;

int av_pyramid_layout(int w, int h, int levels, av_pyr_layout* out);

/* Build n_img pyramids.  Image i is at img_dev + i*img_stride (tightly packed w*h u8), pyramid i
 * at pyr_dev + i*pyr_stride.  Replaces the pyrDown chain inside cv2.calcOpticalFlowPyrLK
 * (reference: image_processing/pyramid_builder.py:22-48 is a pass-through). */
int av_pyramid_build(const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, int levels,
                     uint8_t* pyr_dev, int64_t pyr_stride, void* stream);
/* The same, levels 1 and up only: the level-0 region of every pyramid is left as it is -- for a caller that keeps the image itself as
 * level 0 (what the front-end engine does with resident frames).  That holds where the fused level-0 + level-1 kernel takes the image
 * (w a multiple of 16 with w % 128 == 0 or >= 32, h a multiple of 32, both >= 64, image rows dword-aligned); any other image has its
 * level 1 filtered from the padded level 0, which is then written as by av_pyramid_build. */
int av_pyramid_build_levels(const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, int levels,
                            uint8_t* pyr_dev, int64_t pyr_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * cv2.calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, winSize=(win,win),
 *   maxLevel=levels-1, criteria=(EPS|COUNT, max_iter, eps), flags=OPTFLOW_USE_INITIAL_FLOW)
 * Reference call sites: image_processing/feature_tracker.py:102-108,
 * image_processing/stereo_matcher.py:64-68 and 70-74, parameters config.py:31-44.
 * Batched over n_set point sets: set i tracks count_dev[i] (<= cap) points from pyramid
 * pyrI_dev + i*pyr_stride into pyrJ_dev + i*pyr_stride.  prev/next are float32 (x,y) pairs at
 * [i*cap + k]; next holds the initial guess on entry and the result on return; status is u8.
 * win: 3 .. 31 (config.win_size: the reference's 15 x 15 runs the 16-lanes-per-point kernel, any other size the general
 * one-wavefront-per-point kernel: same arithmetic, same results rule -- bit-identical to the CPU oracle); levels: 1 .. AV_MAX_LEVELS.
 * ------------------------------------------------------------------------------------------- */
int av_lk_track(const uint8_t* pyrI_dev, const uint8_t* pyrJ_dev, int64_t pyr_stride, int n_set,
                int w, int h, int levels,
                const float* prev_dev, float* next_dev, uint8_t* status_dev, const int32_t* count_dev, int cap,
                int win, int max_iter, double eps, double min_eig_threshold, void* stream);
/* The same with level 0 read in place from the images themselves (set i: imgI_dev + i*img_stride into imgJ_dev + i*img_stride, tightly
 * packed w*h u8, BORDER_REFLECT_101 where a window reaches over the border), as the front-end engine tracks its resident frames; the
 * level-0 regions of the two pyramids are not read (av_pyramid_build_levels fills the others).  Same results as av_lk_track. */
int av_lk_track_images(const uint8_t* imgI_dev, const uint8_t* imgJ_dev, int64_t img_stride,
                       const uint8_t* pyrI_dev, const uint8_t* pyrJ_dev, int64_t pyr_stride, int n_set,
                       int w, int h, int levels,
                       const float* prev_dev, float* next_dev, uint8_t* status_dev, const int32_t* count_dev, int cap,
                       int win, int max_iter, double eps, double min_eig_threshold, void* stream);

/* ---------------------------------------------------------------------------------------------
 * cv2.FastFeatureDetector_create(threshold).detect(img, mask)   (TYPE_9_16, NMS on)
 * Reference: image_processing/pipeline.py:23-25, feature_initializer.py:52, feature_adder.py:64.
 * Batched over n_img tightly packed images (and optional masks, NULL = no mask).  For image i the
 * number of keypoints is written to count_dev[i] and keypoint k is packed into
 * kp_dev[i*cap + k] = score << 19 | (2^19 - 1 - (y*w + x)); keypoints are UNORDERED (sort the
 * packed words descending within equal score to recover raster order).  Requires w*h <= 2^19.
 * If more than cap keypoints exist count_dev[i] still reports the true number.
 *
 * av_fast_detect_wide: the same detector, same arguments, for images of up to AV_MAX_IMAGE_PIXELS = 2^24 pixels.  Only the word
 * differs: kp_dev[i*cap + k] = score << 24 | (2^24 - 1 - (y*w + x)).  A score is at most 254, so the word fits 32 bits and orders
 * exactly like the narrow one: by score, then by raster descending.  The two entries return the same keypoints wherever both apply.
 * ------------------------------------------------------------------------------------------- */
int av_fast_detect(const uint8_t* img_dev, int64_t img_stride, const uint8_t* mask_dev, int64_t mask_stride,
                   int n_img, int w, int h, int threshold, uint32_t* kp_dev, int32_t* count_dev, int cap,
                   void* stream);
int av_fast_detect_wide(const uint8_t* img_dev, int64_t img_stride, const uint8_t* mask_dev, int64_t mask_stride,
                        int n_img, int w, int h, int threshold, uint32_t* kp_dev, int32_t* count_dev, int cap,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * cv2.undistortPoints(pts, K, D, None, R, P = identity) for pinhole + radtan
 * (reference: image_processing/camera_model.py:24-47, feature_publisher.py:24-59), and
 * cv2.projectPoints(convertPointsToHomogeneous(pts), 0, 0, K, D)
 * (reference: image_processing/camera_model.py:49-75).  fp64 in, fp64 out; intr = [fx fy cx cy],
 * dist = [k1 k2 p1 p2], R = row-major 3x3 (host pointers, copied by value).
 * ------------------------------------------------------------------------------------------- */
int av_undistort_points(const double* pts_dev, int n, const double* intr, const double* dist, const double* R,
                        double* out_dev, void* stream);
int av_distort_points(const double* pts_dev, int n, const double* intr, const double* dist,
                      double* out_dev, void* stream);

/* The same two operators with the distortion model as an argument (camera_model.py:41-46, 69-74; feature_publisher.py:53-58,
 * 82-87): AV_DISTORTION_RADTAN = the two above; AV_DISTORTION_EQUIDISTANT = cv2.fisheye.undistortPoints(pts, K, D, R, P = identity)
 * and cv2.fisheye.distortPoints(pts, K, D), dist = [k1 k2 k3 k4] of the Kannala-Brandt model.  (Parity of the equidistant branch
 * is unpinned: restated from OpenCV 4.x fisheye.cpp, no cv2 to check against) */
#define AV_DISTORTION_RADTAN 0
#define AV_DISTORTION_EQUIDISTANT 1
int av_undistort_points_model(const double* pts_dev, int n, const double* intr, const double* dist, const double* R, int model,
                              double* out_dev, void* stream);
int av_distort_points_model(const double* pts_dev, int n, const double* intr, const double* dist, int model,
                            double* out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The image front-end as one device-resident engine over n_streams independent stereo streams:
 * ImageProcessingPipeline.__init__ / imu_callback / stereo_callback
 * (reference: image_processing/pipeline.py:15-40, 42-44, 46-150) with all of its feature_* stages
 * (feature_initializer.py:45-85, feature_tracker.py:74-177, stereo_matcher.py:33-115,
 * feature_adder.py:52-108, feature_pruner.py:8-19, feature_publisher.py:90-121,
 * imu_processor.py:22-67).
 * ------------------------------------------------------------------------------------------- */
typedef struct av_frontend_config {
    int32_t width, height;                   /* config.cam0_resolution (config.py:102); width * height <= AV_MAX_IMAGE_PIXELS */
    int32_t grid_row, grid_col;              /* config.py:23-24                                     */
    int32_t grid_min_feature_num;            /* config.py:26                                        */
    int32_t grid_max_feature_num;            /* config.py:27                                        */
    int32_t fast_threshold;                  /* config.py:28                                        */
    int32_t lk_win;                          /* config.patch_size (config.py:35); 3 .. 31           */
    int32_t lk_levels;                       /* config.pyramid_levels + 1 (config.py:34)            */
    int32_t lk_max_iter;                     /* config.max_iteration (config.py:31)                 */
    int32_t max_corners;                     /* capacity for FAST keypoints of one image            */
    int32_t flags;                           /* AV_FE_* bits below                                  */
    double  lk_eps;                          /* config.track_precision (config.py:32)               */
    double  lk_min_eig;                      /* OpenCV default minEigThreshold = 1e-4               */
    double  stereo_threshold;                /* config.py:30                                        */
    double  cam0_intrinsics[4], cam0_distortion[4];   /* config.py:99-101                           */
    double  cam1_intrinsics[4], cam1_distortion[4];   /* config.py:118-120                          */
    double  R_cam0_imu[9], R_cam1_imu[9];    /* inv(T_imu_cam*)[:3,:3] (imu_processor.py:10-16)     */
    double  R0to1[9];                        /* R_cam1_imu.T @ R_cam0_imu (stereo_matcher.py:47)    */
    double  E[9];                            /* skew(t01) @ R0to1 (stereo_matcher.py:90-91)         */
    double  norm_unit;                       /* 4/(2fx+2fy) of cam0 (stereo_matcher.py:103-104)     */
    int32_t cam0_distortion_model;           /* AV_DISTORTION_* (config.py:98); 0 = radtan          */
    int32_t cam1_distortion_model;           /* config.py:117                                       */
    double  ransac_threshold;                /* config.ransac_threshold (config.py:29), pixels; read only with AV_FE_RANSAC */
    double  ransac_success_probability;      /* config.ransac_success_probability, 0 < p < 1 (0.99)  */
    uint32_t ransac_seed;                    /* config.ransac_seed: first word of the draw hash      */
    int32_t reserved0;                       /* keeps the size a multiple of 8; must be 0            */
    double  clahe_clip_limit;                /* config.clahe_clip_limit (2.0); the three are read only with AV_FE_CLAHE */
    int32_t clahe_tiles_x, clahe_tiles_y;    /* config.clahe_tiles (8, 8); 1 .. AV_CLAHE_MAX_TILES    */
    int32_t pixel_format;                    /* config.image_format: AV_PIX_* of the frames handed to every entry path; 0 = 8-bit grey */
    int32_t gray16_shift;                    /* config.gray16_shift: 0 .. 8, read only with the 16-bit formats (checked always)       */
    int32_t image_downscale;                 /* config.image_downscale: 0 / 1 = off, 2 or 4 = bin the grey frames f x f ("Binning" below) */
    int32_t reserved1;                       /* keeps the size a multiple of 8; must be 0            */
} av_frontend_config;

typedef struct av_frontend av_frontend;

/* Any width x height of at most AV_MAX_IMAGE_PIXELS pixels whose pyramid levels are all wider and higher than AV_PYR_BORDER; a larger
 * image is refused here, AV_E_INVALID, before a device is touched.  Capacities that depend on the image: max_corners must hold the
 * corners of a whole first frame (they grow with the area: the Python engine scales its default of 8192 at 752 x 480 by the pixel
 * count); the per-cell lists are sized by the area of a grid cell. */
int  av_frontend_create(const av_frontend_config* cfg, int n_streams, int device, av_frontend** out);
void av_frontend_destroy(av_frontend* fe);

/* ImageProcessingPipeline.imu_callback (pipeline.py:42-44 -> imu_processor.py:22-26).  Only the
 * gyro is used by the front-end.  Thread-safe against av_frontend_step* on other threads. */
int av_frontend_push_imu(av_frontend* fe, int stream, double timestamp, const double gyro[3]);

/* n IMU samples in one call: sample i goes to stream stream_idx[i]; gyro is [n][3]. */
int av_frontend_push_imu_batch(av_frontend* fe, const int32_t* stream_idx, const double* timestamps,
                               const double* gyro, int n);

/* av_frontend_config.flags.  AV_FE_INPUTS_PERSIST: the device images handed to av_frontend_step stay valid and unmodified
 * until the kernels of the NEXT av_frontend_step of this engine have completed.  The engine then reads pyramid level 0 in place
 * (LK and FAST index the caller's image, with BORDER_REFLECT_101 arithmetic at the border) and builds only levels 1..3 -- no
 * padded copy of level 0: 0.8 MB less HBM traffic per stereo frame at 752x480.  Without the flag the inputs are only read during
 * the call's own kernels and level 0 is copied (the round-1/2 behaviour).  av_frontend_step_host always works in place: the
 * images live in the library's own staging slots.  Results are bit-identical either way. */
#define AV_FE_INPUTS_PERSIST 1
/* AV_FE_RANSAC: two-point RANSAC outlier rejection between the stereo re-match and the re-binning of the tracked features (the
 * step feature_tracker.py:135-136 leaves empty: both inlier vectors are all ones there).  A tracked feature survives iff its cam0
 * problem and its cam1 problem (av_two_point_ransac below: previous / current points of that camera, cam*_R_p_c of
 * imu_processor.py:28-67) both mark it; a rejected feature is absent from the published message and keeps no new corner away.  Without
 * the flag the step enqueues exactly what it always did.  Needs grid_num * grid_max <= AV_RANSAC_MAX_PAIRS. */
#define AV_FE_RANSAC 2
/* AV_FE_CLAHE: every frame of both cameras goes through av_clahe (below; clahe_clip_limit, clahe_tiles_x / _y of the configuration)
 * before anything reads it: pyramids, LK and FAST see equalised pixels only, and the published message is that of the unmodified
 * pipeline run on equalised frames.  No counterpart in the reference (pipeline.py:46-150 works on the camera's own pixels).  The
 * caller's images are never written: the engine owns the equalised level 0 -- [3][n_streams][width * height], cam0 of alternating
 * frames and cam1, like the pyramid slots -- and past the stage runs as if those were persisting inputs: level 0 is read in place,
 * only levels 1.. are built.  That holds for av_frontend_step with and without AV_FE_INPUTS_PERSIST, for av_frontend_prestage (the
 * stage runs there, and the step that follows with the same pointers skips both), and for av_frontend_step_host (the stage reads the
 * staging slot).  In the shared frame store av_frontend_frames_upload equalises every entry once, in place in the store, on the copy
 * stream, before the entry's pyramids and FAST pass (one upload must then not name an entry twice: AV_E_INVALID);
 * av_frontend_step_frames is what it was.  The stage's launches count under class 0
 * (pyramid) of av_frontend_enable_timing.  Without the flag the step enqueues exactly what it always did and nothing more is
 * allocated. */
#define AV_FE_CLAHE 4

/* av_frontend_config.pixel_format other than AV_PIX_GRAY8 (av_to_gray8 below has the formats and the arithmetic): the `uint8_t*` image
 * arguments of av_frontend_step, _prestage, _step_host and av_frontend_frames_upload are BYTE pointers to frames of that format, and
 * img_stride is in bytes, at least width * height * bytes per pixel.  Every frame of both cameras is converted to 8-bit grey before
 * anything else reads it, into the engine-owned level 0 that AV_FE_CLAHE uses ([3][n_streams][width * height], allocated when either
 * feature needs it); with AV_FE_CLAHE the grey frames are then equalised there in place; past that the step runs as if those were
 * persisting inputs.  That holds for av_frontend_step with and without AV_FE_INPUTS_PERSIST, for av_frontend_prestage and for
 * av_frontend_step_host (the staging slots and the host-to-device copy carry the raw format).  av_frontend_frames_upload keeps the raw
 * frames in its pinned ring and in a device staging buffer per ring entry and converts them into the store on the copy stream, before
 * CLAHE (if on), the pyramids and FAST; the conversion is not in place, so an upload may name an entry twice when only the format is
 * set (the later frame wins, as with grey frames).  av_frontend_step_frames is what it was.  The conversion counts under class 0 of
 * av_frontend_enable_timing, inside the input stage's span.  The caller's images are never written.  The published message is that
 * of the unmodified pipeline run on the converted frames.  With AV_PIX_GRAY8 nothing is launched and nothing more is allocated.
 * Both cameras have one size and one format.  av_frontend_create refuses an unknown format or a shift outside 0 .. 8, AV_E_INVALID,
 * before a device is touched.
 * Packed 10 / 12-bit transports (AV_PIX_GRAY10P .. AV_PIX_BAYER_GBRG12_CSI2): a frame is av_pixfmt_frame_bytes(pixel_format, width,
 * height) = width * height * d / 8 bytes, and that -- not a number of bytes per pixel -- is what img_stride must at least be and what
 * the staging slots, the pinned ring and the device staging carry: 1.25 or 1.5 bytes per pixel over the host-to-device link instead
 * of 2.  A packed mosaic is converted in two passes through an engine-owned 8-bit mosaic scratch ([2][n_streams][width * height]; the
 * frame store has one of its own, sized by the largest upload), allocated only when such a format is configured.  With binning the
 * chain is raw -> mosaic scratch -> full-size grey scratch -> level 0.  av_frontend_create refuses a width that is not whole groups
 * (4 samples at 10 bits, 2 at 12), AV_E_INVALID with the format's name in the text, before a device is touched. */

/* Binning: av_frontend_config.image_downscale = f = 2 or 4 (av_downscale below has the arithmetic).  width / height stay the size of
 * the frames handed to the entry points and the intrinsics stay those of the full-size camera; the engine works on the binned image
 * of w = width / f by h = height / f pixels (both must divide) and derives its calibration itself, from the pixel-centre map
 * X = f x + (f - 1) / 2, in double precision and in exactly this order:
 *   fx' = fx / f;  fy' = fy / f;  cx' = (cx - (f - 1) / 2) / f;  cy' = (cy - (f - 1) / 2) / f;  norm_unit' = norm_unit * f
 * for both cameras.  Distortion coefficients, extrinsics, R0to1 and E are unchanged; stereo_threshold, ransac_threshold, fast_threshold,
 * the grid, lk_win and max_corners apply to the binned image as they stand.  Order of the input stage: raw frame -> conversion to grey
 * (pixel_format other than AV_PIX_GRAY8) -> binning -> CLAHE (AV_FE_CLAHE, at the binned size) -> pyramids / LK / FAST.  Everything past
 * the stage is sized by w x h: pyramids, tile and cell lists, raster bits, the engine-owned level 0 ([3][n_streams][w * h], which
 * binning always uses) and the frame store's entries.  Only the entry points' image arguments (img_stride >= width * height * bytes per
 * pixel), the staging slots of av_frontend_step_host and the pinned ring and device staging of av_frontend_frames_upload are sized by
 * the input.  With AV_PIX_GRAY8 the binning reads the caller's (or the staging slot's) frames directly; with any other format the
 * conversion writes a full-size grey scratch of the engine's ([2][n_streams][width * height]; the frame store has one of its own, sized by the largest upload)
 * that the binning then reads.  It holds for av_frontend_step with and without AV_FE_INPUTS_PERSIST, av_frontend_prestage (the stage
 * runs there, the step that follows with the same pointers skips it) and av_frontend_step_host: past the stage the step runs as with
 * persisting inputs.  av_frontend_frames_upload copies the full-size frames to its device staging and bins them into the store on the
 * copy stream, after the conversion and before CLAHE, the pyramids and FAST (an entry named twice gets its later frame);
 * av_frontend_step_frames is what it was.  The launches count under class 0 of av_frontend_enable_timing, inside the input stage's
 * span.  The caller's images are never written.  The published message is in normalised undistorted coordinates and is that of the
 * unmodified pipeline run on the binned frames with the calibration above; av_frontend_read_image returns the w x h frame and the
 * pixel coordinates of av_frontend_read_grid are pixels of the binned image.  av_frontend_create refuses a factor outside {0, 1, 2, 4},
 * a non-zero reserved1, a size the factor does not divide and a binned size that fails the size rules (a pyramid level not larger
 * than AV_PYR_BORDER), AV_E_INVALID, before a device is touched.  With 0 or 1 the step enqueues exactly what it always did and nothing
 * more is allocated.  Box filter only; one factor for both cameras; the thresholds are not retuned for the smaller image. */

/* Static masks: the parts of a camera's image that are never scene -- the corners outside a fisheye lens's image circle, an
 * airframe or propeller arcs in view, a sensor's dead border.  No counterpart in the reference, which has only the transient 7 x 7
 * mask around existing features (feature_adder.py:56-62); a static mask is the same detect(img, mask) argument with a second source
 * (OpenVINS use_mask, VINS-Fusion fisheye_mask).
 * One mask per camera, for all streams of an engine: the engine has one calibration, so it has one rig geometry.  A mask is
 * height x width bytes (the size of the frames handed to the entry points), tightly packed: non-zero = scene, 0 = never scene.  Either
 * camera's mask may be absent, which means all valid.  A pixel coordinate (x, y) is mapped to a mask pixel by truncation,
 * m[int(y)][int(x)] -- the reference's own rule for its 7 x 7 mask (feature_adder.py:59-62).
 *  1. Detection (cam0 mask).  A FAST keypoint whose cam0 mask pixel is 0 is dropped after the non-max suppression: detect(img, mask)
 *     with mask = static & 7x7.  It applies on the first frame (feature_initializer.py:52, which has no mask today) and in
 *     add_new_features.  n_fast (av_frontend_read_counters) counts what is left.
 *  2. Temporal tracking (cam0 mask).  A tracked point that passed the LK status and the bounds test (feature_tracker.py:110-121) but
 *     sits on a masked cam0 pixel is dropped there, before the stereo re-match and before RANSAC.  after_tracking counts what is left.
 *  3. Stereo (cam1 mask).  A stereo match (tracked or new candidate, first frame included) that passed the in-image test of
 *     stereo_matcher.py:75-88 but whose cam1 point sits on a masked cam1 pixel is not an inlier.
 *  4. Binning.  With image_downscale = f the masks are given at the input size; the engine works with the binned mask: pixel (x, y)
 *     of it is valid iff all f x f source pixels are non-zero.  Stored bytes are 0 / 1.
 *  5. LK windows, pyramids, CLAHE and RANSAC read masked pixels as they always did.  Only the three gates above change.
 * av_frontend_set_masks takes two tightly packed height x width u8 HOST arrays; either may be NULL (no mask for that camera), both
 * NULL clears.  It is blocking (the masks are binned on the host and copied before it returns; the arrays are free again then) and is
 * accepted only while the engine has not yet been handed a frame: after an av_frontend_step*, _prestage or _frames_upload it returns
 * AV_E_INVALID, because the FAST lists of frames already uploaded would disagree with the mask.  The first call allocates two device
 * buffers of w * h bytes (the processed size); an engine that is never given a mask allocates nothing and enqueues exactly what it
 * always did.  av_frontend_read_mask copies the processed-size 0 / 1 mask of camera `cam` (0 / 1) into out_host (w * h bytes);
 * AV_E_INVALID if none is set for that camera.
 * Not covered: per-stream masks, masks that change during a run, excluding masked pixels from the LK windows, drop counters of their
 * own, two cameras of different sizes. */
int av_frontend_set_masks(av_frontend* fe, const uint8_t* mask0_host, const uint8_t* mask1_host);
int av_frontend_read_mask(av_frontend* fe, int cam, uint8_t* out_host);

/* Photometric calibration: AV_FE_PHOTOMETRIC in av_frontend_config.flags.  A real lens and sensor do not give a linear, spatially
 * uniform measurement of the scene: a wide-angle lens loses half its light or more towards the rim (vignetting) and the sensor's
 * response curve is not a straight line.  No counterpart in the reference, which works on the camera's own pixels; the convention is
 * that of the TUM mono-VO dataset: an inverse response table G^-1 (256 entries, pcalib.txt) and a vignette map V(x) (vignette.png), and
 * the corrected image is I'(x) = G^-1(I(x)) / V(x).  Here in integers only, which makes this text the contract (tests/photometric_ref.py
 * states it in NumPy).  Per camera two optional tables, shared by all streams of an engine (one rig, one calibration):
 *   response  uint16[256] in Q8: entry p is G^-1(p) * 256, every entry <= AV_PHOTOMETRIC_RESPONSE_MAX = 65280 (255 * 256).  Absent means
 *             p * 256.
 *   gain      uint16[height * width] in Q12, at the size of the frames handed to the entry points, tightly packed: 4096 / V(x).  Absent
 *             means 4096 everywhere.  The range covers gains up to 15.9998.
 * For a grey pixel p at x:
 *   out = min(255, (response[p] * gain[x] + (1 << 19)) >> 20)
 * The intermediate fits 32 bits unsigned, 65280 * 65535 + 2^19 < 2^32: that bound is why a response entry above 65280 is refused.
 * With only a response the rule reduces to (response[p] + 128) >> 8, with only a gain to (p * gain[x] + 2048) >> 12 (the min still
 * applies); the kernels compute the one formula.  The float tables are quantised once, on the host, in float64 (the Python
 * frontend.photometric_tables: response floor(clip(U, 0, 255) * 256 + 0.5), gain min(65535, floor(4096 / V + 0.5)), V <= 0 -> 65535);
 * everything after that is integer, so a kernel is either bit-identical to the reference or wrong.
 * Place in the input stage: raw frame -> conversion to grey -> PHOTOMETRIC -> binning -> CLAHE -> pyramids / LK / FAST.  The stage runs
 * at the input size, ahead of the binning: the vignette is a property of the full-size sensor, and binning corrected pixels is the
 * physically right order.  Any pixel_format works: the stage sees the 8-bit grey after the conversion (after the demosaic for a
 * mosaic).  Static masks are independent: a masked pixel is corrected like any other.
 * An engine created with the flag owns level 0 (as with AV_FE_CLAHE) and av_frontend_read_image returns the frame after the whole
 * chain.  After a conversion the stage runs in place on what the conversion wrote; without one it reads the caller's frames (the
 * staging slot's, the upload ring's) and writes the engine's own memory: the caller's frames are never written.  It holds for
 * av_frontend_step with and without AV_FE_INPUTS_PERSIST, av_frontend_prestage (the stage runs there; the step that follows with the same
 * pointers skips it), av_frontend_step_host and av_frontend_frames_upload, which then takes the frames through its device staging into
 * the store entries on the copy stream; an entry named twice in one upload receives its later frame, corrected exactly once (with
 * AV_FE_CLAHE the refusal of duplicates stands).  The launches count under class 0 of av_frontend_enable_timing, inside the input
 * stage's span.  Without the flag the step enqueues exactly what it always did and nothing more is allocated.
 * av_frontend_set_photometric takes HOST arrays: response0 / response1 [256], gain0 / gain1 [height * width] (the input size).  Any
 * pointer may be NULL = the identity for that part; all four NULL is the identity stage.  Blocking (the arrays are free again on
 * return).  It needs the flag, refuses a response entry above 65280, and is accepted only while the engine has not yet been handed a
 * frame (av_frontend_step*, _prestage, _frames_upload), like av_frontend_set_masks and for the same reason: frames already in the engine
 * would disagree with the new tables.  All of these are AV_E_INVALID with a text.  An engine with the flag that has not been given
 * its tables refuses every step, prestage and upload, AV_E_INVALID, with a text that names av_frontend_set_photometric.
 * av_frontend_read_photometric copies the tables of camera `cam` (0 / 1) back: response_out_host [256], gain_out_host
 * [height * width]; either may be NULL; a part that was given as NULL reads back as the identity (p * 256, 4096).
 * Not covered: per-stream tables, tables that change during a run, a per-pixel dark frame, fusing the stage into the conversion / Bayer / unpack kernels, gains of 16 and above, estimating the calibration itself,
 * two cameras of different sizes; fast_threshold and the LK thresholds are not retuned for corrected images. */
#define AV_FE_PHOTOMETRIC 8
#define AV_PHOTOMETRIC_RESPONSE_MAX 65280
int av_frontend_set_photometric(av_frontend* fe, const uint16_t* response0_host, const uint16_t* gain0_host,
                                const uint16_t* response1_host, const uint16_t* gain1_host);
int av_frontend_read_photometric(av_frontend* fe, int cam, uint16_t* response_out_host, uint16_t* gain_out_host);

/* Exposure-time normalisation: AV_FE_EXPOSURE in av_frontend_config.flags.  The third term of the TUM photometric model
 * I(x) = G(t * V(x) * B(x)): the exposure time t of each frame.  A camera on auto-exposure changes t from frame to frame, and both LK
 * passes assume constant brightness between the two images they compare.  Per frame and per camera one factor
 *   k  uint16 in Q12, 1 <= k <= 65535:  k = min(65535, max(1, floor(4096 * t_ref / t + 0.5)))
 * computed once, on the host, in float64 (the Python frontend.quantise_exposure; t <= 0, t_ref <= 0 or a non-finite value is refused
 * there); the range goes up to 15.9998, as the vignette gain's.  Everything after it is integer, so this text is the contract
 * (tests/exposure_ref.py states it in NumPy).  The effective response table of a frame, for p = 0 .. 255:
 *   r'[p] = min(65280, (response[p] * k + 2048) >> 12)              response absent: response[p] = p << 8
 * (65280 * 65535 + 2048 < 2^32), and the pixel is that of "Photometric calibration" with r' in place of the response:
 *   out = min(255, (r'[p] * gain[x] + (1 << 19)) >> 20)             gain absent: 4096
 * k = 4096 gives r' = response exactly: a frame at the reference exposure is byte for byte what the photometric stage alone makes of it.
 * It IS the photometric stage -- the kernel scales the 256-entry table of its workgroup's image while it stages it, nothing is added per
 * pixel -- so the order of the input stage is unchanged: raw -> conversion to grey -> photometric (with exposure) -> binning -> CLAHE.
 * Either flag turns the stage on and makes the engine own level 0.  With AV_FE_EXPOSURE alone the tables are the identity and
 * av_frontend_set_photometric is neither required nor accepted.
 * av_frontend_next_exposure hands over the factors of the frames of the NEXT call that hands frames over, HOST arrays k0 (cam0) and k1
 * (cam1) of n entries: n = n_streams for av_frontend_step, _step_host and _prestage, the upload's n for av_frontend_frames_upload.
 * AV_E_INVALID with a text: a zero factor, a null pointer, an engine without the flag; a wrong n is found by the call that consumes them.
 * A call that runs the input stage consumes the pending factors; with none pending on an engine with the flag it is refused,
 * AV_E_INVALID, with a text that names av_frontend_next_exposure.  A call that does not run the stage needs none: the step after an
 * av_frontend_prestage of the same pointers (the factors given before the prestage belong to the prestaged frames), and
 * av_frontend_step_frames.  Every call that hands frames over leaves nothing pending when it returns, whatever it returns: factors
 * left pending across a step that skipped the stage are discarded.
 * The factors reach the device on the call's own stream from a pinned ring, as the per-step homographies do (an upload's travel with
 * the upload on the copy stream): no host wait, no synchronisation and no kernel launch are added, and the timing spans are those of
 * an AV_FE_PHOTOMETRIC engine.  In the frame store an entry named twice in one upload gets its later frame with that frame's factor,
 * corrected once (with AV_FE_CLAHE the refusal of duplicates stands).
 * av_frontend_read_exposure: out2 = the factors (cam0, cam1) the frame of stream stream_idx's last step was corrected with; through
 * the frame store, those of the entry it read.
 * Not covered: estimating exposures when the camera does not report them; analogue gain as a separate input (the caller folds it into
 * t); exposure applied ahead of a 16-bit conversion or the range scaling; per-stream reference exposures; retuned thresholds. */
#define AV_FE_EXPOSURE 16
int av_frontend_next_exposure(av_frontend* fe, const uint16_t* k0_host, const uint16_t* k1_host, int n);
int av_frontend_read_exposure(av_frontend* fe, int stream_idx, uint16_t out2[2]);

/* ImageProcessingPipeline.stereo_callback for every stream at once (pipeline.py:46-150).
 * Stream s reads its cam0/cam1 images (tightly packed width*height u8, device memory) at
 * img0_dev + s*img_stride and img1_dev + s*img_stride; timestamps[s] is the frame time.  All
 * kernels are enqueued on `stream`; nothing is synchronised. */
int av_frontend_step(av_frontend* fe, const uint8_t* img0_dev, const uint8_t* img1_dev, int64_t img_stride,
                     const double* timestamps, void* stream);
/* Same with host images (the drop-in boundary hands over numpy arrays): copies H2D, steps. */
/* Builds the pyramids of the images the NEXT av_frontend_step will be given, now, behind whatever is enqueued on `stream` (needs
 * AV_FE_INPUTS_PERSIST; the step that follows with the same pointers skips its own pyramid launch; results are identical -- the
 * launch only changes its place in the stream).  pipeline.py:46-150 builds a frame's pyramids when the frame arrives; a caller
 * that knows its next frame (a replay, a queue of camera frames: streaming/dataset.py:93-158) can have them built while the
 * filter works on the frame before. */
int av_frontend_prestage(av_frontend* fe, const uint8_t* img0_dev, const uint8_t* img1_dev, int64_t img_stride, void* stream);

int av_frontend_step_host(av_frontend* fe, const uint8_t* img0_host, const uint8_t* img1_host, int64_t img_stride,
                          const double* timestamps, void* stream);

/* Shared frame store -- for sweeps that replay the SAME frames on several streams: the reference's run.bat:4-12 runs every
 * sequence from several start offsets, and an offset only moves the start index (streaming/dataset.py:206-214), so every frame
 * of the sequence is read by every offset stream a few steps apart.  A frame put into the store is copied to the device, gets
 * both its pyramids (levels 1.., level 0 is read in place) and its FAST pass ONCE (the detector's lists are independent of the
 * stream: the per-stream mask of feature_adder.py:56-62 is applied when the lists are binned into a stream's cells); the streams
 * only carry an entry number per step.
 *   av_frontend_frames_reserve   allocate n_slots entries (~2 MB each at 752 x 480 and four levels); once per engine.
 *   av_frontend_frames_upload    n host frame pairs (frame i: img0_host + i*img_stride, img1_host + i*img_stride, tightly packed
 *                                width*height u8) into entries slots[i].  The copies and kernels run on the engine's copy stream,
 *                                behind the newest step ENQUEUED so far (the entries must be free as of that step) and beside
 *                                whatever is enqueued afterwards: upload the frames of step k+1 before enqueueing step k to overlap
 *                                the two.  The host arrays are free again when the call returns.
 *   av_frontend_step_frames      av_frontend_step with stream s reading entry slot_of_stream[s] (its previous frame's entry is
 *                                remembered by the engine and must still hold that frame).  A NEGATIVE entry = the stream has no
 *                                frame in this step (its sequence is over): none of its kernels' workgroups do anything, its
 *                                published count reads 0, its state stays as it is.  Results are bit-identical to av_frontend_step
 *                                on the same images. */
int av_frontend_frames_reserve(av_frontend* fe, int n_slots);
int av_frontend_frames_upload(av_frontend* fe, const int32_t* slots, int n, const uint8_t* img0_host, const uint8_t* img1_host,
                              int64_t img_stride, void* stream);
int av_frontend_step_frames(av_frontend* fe, const int32_t* slot_of_stream, const double* timestamps, void* stream);

/* Host-side staging for sweeps: decode n 8-bit greyscale, non-interlaced PNG files of width x height (the EuRoC camera
 * frames; reference: streaming/dataset.py:101 `cv2.imread(path, -1)` on the reader threads of dataset.py:93-158) on
 * `threads` host threads, file i into out + i*out_stride -- e.g. straight into the [S][h][w] batches handed to
 * av_frontend_step_host, one step ahead of the GPU.  status[i] (optional) = 0 ok, 1 unsupported flavour of PNG (other depth /
 * colour type / size / interlaced: the caller may decode that file by other means), 2 unreadable or corrupt.  Returns AV_OK,
 * AV_E_CAPACITY if the worst status is 1, AV_E_INVALID if any file was unreadable.  Pure host function. */
int av_png_decode_gray8(const char* const* paths, int n, int width, int height, uint8_t* out, int64_t out_stride, int threads, int32_t* status);
/* The same for the PNG flavour that holds pixel_format: AV_PIX_GRAY8 = colour type 0 at depth 8, AV_PIX_GRAY16 = colour type 0 at depth
 * 16 (the file's big-endian samples are swapped to host byte order), AV_PIX_RGB8 = colour type 2 at depth 8, AV_PIX_RGBA8 = colour type
 * 6 at depth 8; non-interlaced.  (PNG stores no BGR order, no palette-free 16-bit colour is taken: AV_E_INVALID for the other formats.)
 * File i lands in out + i * out_stride_bytes as width * height * bytes-per-pixel tightly packed bytes.  A file of another flavour than
 * the one asked for gets status 1.  Status and return codes as above.  Pure host function. */
int av_png_decode(const char* const* paths, int n, int width, int height, int pixel_format, void* out, int64_t out_stride_bytes, int threads,
                  int32_t* status);
/* Size and flavour of one PNG file from its IHDR alone: *pixel_format = the AV_PIX_* av_png_decode would take for it, or -1 for a
 * flavour it does not decode (palette, 16-bit colour, grey + alpha, depth below 8, interlaced): AV_OK either way.  AV_E_INVALID for a
 * file that cannot be opened or does not begin with a PNG signature and an IHDR chunk.  Pure host function. */
int av_png_probe(const char* path, int32_t* width, int32_t* height, int32_t* pixel_format);

/* Capacity (features per stream) of the published feature message = grid_num * grid_max. */
int av_frontend_max_features(const av_frontend* fe);

/* The feature_msg of the last step (feature_publisher.py:109-121), synchronising `stream` first.
 * For stream s: n_out[s] features; ids at ids_out[s*cap + k]; (u0,v0,u1,v1) at uv_out[(s*cap+k)*4].
 * cap must be >= av_frontend_max_features.  Returns AV_E_CAPACITY if any stream overflowed a
 * device-side buffer during the step (results of that stream are then not parity-exact). */
int av_frontend_read_features(av_frontend* fe, int64_t* ids_out, double* uv_out, int32_t* n_out, int cap, void* stream);
/* The same read-back in two halves: _begin enqueues the device-to-host copies into pinned slot 0/1 behind the work
 * already on `stream` and returns; _end waits for those copies only and unpacks them.  Enqueueing the next
 * av_frontend_step between the two overlaps it with the consumption of this frame's features. */
int av_frontend_read_features_begin(av_frontend* fe, int slot, void* stream);
int av_frontend_read_features_end(av_frontend* fe, int slot, int64_t* ids_out, double* uv_out, int32_t* n_out, int cap);
/* The same feature_msg where the last step left it, ON THE DEVICE: ids int64[S][cap], uv double[S][cap][4], n int32[S] with
 * cap = av_frontend_max_features.  The buffers are rewritten by the next av_frontend_step; consume them with work enqueued on the
 * stream the step ran on (av_msckf_batch_submit_dev copies them there).  This is the hand-over of pipeline.py:131-143 ->
 * modules/vio.py:34-36,46-51 (feature_queue) without the host in between. */
int av_frontend_features_dev(av_frontend* fe, const int64_t** ids_dev, const double** uv_dev, const int32_t** n_dev, int* cap);

/* Pipeline state visible to callers (pipeline.py:33-40): the grid of the frame just published
 * (= prev_features after the callback returns).  Per feature k of stream `stream`:
 * ids[k], lifetime[k], cell[k], pts[k*4] = cam0 x,y, cam1 x,y (pixels, float32; with image_downscale = 2 or 4: pixels of the
 * binned image the engine works on).  Synchronises. */
int av_frontend_read_grid(av_frontend* fe, int stream_idx, int64_t* ids, int32_t* lifetime, int32_t* cell,
                          float* pts, int cap, int32_t* n_out, int64_t* next_feature_id, void* stream);

/* Stage counters of the last step for one stream (feature_tracker.py:96,123,133,157 and the
 * adder): [before_tracking, after_tracking, after_matching, n_fast_corners, n_candidates, n_new,
 * n_published, overflow_flags].  Synchronises. */
int av_frontend_read_counters(av_frontend* fe, int stream_idx, int32_t out[8], void* stream);
/* New-feature candidates are stereo-matched lazily (feature_adder.py:80-108 matches all of them and keeps the grid_min
 * best inliers per cell; the first grid_min + 2 candidates of a cell decide that unless too few of them are inliers):
 * [candidates matched in round 1, in round 2] of the last step, i.e. the LK point passes actually run.  Synchronises. */
int av_frontend_read_match_counts(av_frontend* fe, int stream_idx, int32_t out[2], void* stream);

/* [after_ransac, cam0 markers set, cam1 markers set, path bits] of the last step for one stream of an engine created with
 * AV_FE_RANSAC (zeros otherwise, and on a step that tracked nothing).  path bits = cam0 path | cam1 path << 4 with the
 * AV_RANSAC_PATH_* codes below.  Synchronises. */
int av_frontend_read_ransac_counts(av_frontend* fe, int stream_idx, int32_t out[4], void* stream);

/* The level-0 image the last step used for camera `cam` (0 / 1) of one stream of an engine created with AV_FE_CLAHE, with a
 * pixel_format other than AV_PIX_GRAY8, with AV_FE_PHOTOMETRIC or with image_downscale = 2 or 4, i.e. the grey frame the step
 * worked on, photometrically corrected if AV_FE_PHOTOMETRIC is set, binned if image_downscale is set and equalised if AV_FE_CLAHE
 * is set: (width / f) * (height / f) bytes, the processed size, into out_host
 * (width * height without binning).  AV_E_INVALID with none of the four (level 0 is then the caller's own image),
 * before the first step, and for a stream whose av_frontend_step_frames entries were negative from the start.  The image comes from where
 * the LAST step read it: the frame store after av_frontend_step_frames, the engine's own buffer after the other steps.  Between an
 * av_frontend_prestage and the step it serves the cam1 image of the last step is gone (its slot holds the next frame's): cam 1 is then
 * refused, AV_E_INVALID; cam 0 is still the last step's.  Synchronises. */
int av_frontend_read_image(av_frontend* fe, int stream_idx, int cam, uint8_t* out_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Contrast-limited adaptive histogram equalisation of n_img 8-bit images (tightly packed w * h, image i at img_dev + i * img_stride,
 * result at out_dev + i * out_stride; out_dev == img_dev with equal strides works in place).  No counterpart in the reference; the
 * definition restates cv::CLAHE::apply of OpenCV 4.x for 8-bit input.  Its parity with cv2 is unpinned (there is no cv2 to check
 * against), so this text is the contract.  One difference is known: OpenCV pads both axes as soon as one of them is ragged, here
 * each axis is padded only if it is ragged itself.
 *   Geometry.  w % tiles_x != 0: the image is extended on the right by tiles_x - w % tiles_x columns, BORDER_REFLECT_101; the same at
 *     the bottom with tiles_y.  tw, th = padded size / tiles; area = tw * th.
 *   Look-up table of a tile.
 *     1. hist = 256-bin histogram of the tile's pixels of the padded image
 *     2. clip_limit > 0: clip = max(1, (int)(clip_limit * area / 256)), the product in double;
 *        clipped = sum over bins of max(hist - clip, 0), those bins are set to clip;
 *        batch = clipped / 256, residual = clipped - 256 batch; every bin gets + batch;
 *        residual != 0: step = max(256 / residual, 1); bins 0, step, 2 step, .. get + 1 while residual-- > 0 and the index is < 256
 *     3. scale = 255.0f / area (float32)
 *     4. lut[i] = saturate_u8(round_half_even((float)(hist[0] + .. + hist[i]) * scale))
 *   Interpolation.  Pixel (x, y) of the unpadded image with value v:
 *     txf = x * (1.0f / tw) - 0.5f; tx1 = floor(txf); tx2 = tx1 + 1; xa = txf - tx1; xa1 = 1.0f - xa; then tx1 = max(tx1, 0),
 *     tx2 = min(tx2, tiles_x - 1); ty1, ty2, ya, ya1 the same from y and th;
 *     res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya
 *     in float32, in exactly this order, without fused multiply-add; out = saturate_u8(round_half_even(res)).
 * Limits: 1 <= tiles_x, tiles_y <= AV_CLAHE_MAX_TILES, clip_limit >= 0 (0 = no clipping), w * h <= AV_MAX_IMAGE_PIXELS (a tile then has at most
 * 2^24 pixels: every count and prefix sum is exact in int32 and in float32); anything else is AV_E_INVALID with text.  lut_dev (optional): the tables, uint8 [n_img][tiles_y * tiles_x][256], 16-byte aligned (the images may lie
 * at any address and stride: unaligned ones are read and written byte by byte).
 * ------------------------------------------------------------------------------------------- */
#define AV_CLAHE_MAX_TILES 16
int av_clahe(const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, double clip_limit, int tiles_x, int tiles_y,
             uint8_t* out_dev, int64_t out_stride, uint8_t* lut_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pixel formats of camera frames and their conversion to 8-bit grey.  No counterpart in the reference (streaming/dataset.py:101 hands
 * on whatever cv2.imread(path, -1) returns, and the pipeline assumes 8-bit grey).  Parity with cv2.cvtColor is unpinned (there is no
 * cv2 to check against), so this text is the contract; tests/pixfmt_ref.py states it in NumPy.
 *   format          bytes per pixel   layout
 *   AV_PIX_GRAY8    1                 one sample
 *   AV_PIX_GRAY16   2                 one 16-bit sample in host byte order
 *   AV_PIX_RGB8     3                 R G B interleaved            AV_PIX_BGR8   3   B G R
 *   AV_PIX_RGBA8    4                 R G B A interleaved          AV_PIX_BGRA8  4   B G R A
 *   GRAY16 to grey:  min(255, v >> shift), shift in 0 .. 8, default 8 (the high byte).  It truncates, it does not round.  A sensor with
 *                    10, 12 or 14 significant bits uses shift 2, 4 or 6.
 *   colour to grey:  (9798 R + 19235 G + 3735 B + 16384) >> 15 in integer arithmetic.  The coefficients sum to 2^15, so R = G = B = g
 *                    gives g exactly and the result never exceeds 255.  Alpha is ignored.
 *   GRAY8:           the identity.
 * Not covered: 16-bit colour, cameras of two sizes or formats.  (A window or an automatic range instead of the shift: "Range scaling of
 * 16-bit grey" below, AV_PIX_GRAY16 only.)
 *
 * Bayer mosaics: the raw colour-filter-array frame of a colour machine-vision camera, one sample per pixel.  A pattern is named by the
 * colours of the TOP-LEFT 2 x 2 block in reading order (OpenCV's BayerBG .. BayerGR name another corner: do not carry those names over).
 *   format                     code   sample                      colours of pixels (0,0) (1,0) / (0,1) (1,1), as (x, y)
 *   AV_PIX_BAYER_RGGB8  / 16   16/20  u8 / u16, host byte order   R G / G B
 *   AV_PIX_BAYER_BGGR8  / 16   17/21                              B G / G R
 *   AV_PIX_BAYER_GRBG8  / 16   18/22                              G R / B G
 *   AV_PIX_BAYER_GBRG8  / 16   19/23                              G B / R G
 * Bytes per pixel are 1 and 2.  The image has w >= 2 and h >= 2 samples (smaller: AV_E_INVALID).  Parity with cv2 is unpinned like the
 * other formats' (OpenCV's own Bayer-to-grey is another filter and does not interpolate its border): this text is the contract,
 * tests/bayer_ref.py states it in NumPy.
 *   1. reduce    8-bit: s = v.  16-bit: s = min(255, v >> shift) for every sample before anything else (the GRAY16 rule; sensors with
 *                10, 12 or 14 significant bits use shift 2, 4 or 6).
 *   2. extend    BORDER_REFLECT_101 beyond the border: index -1 reads 1, index w reads w - 2.  Reflection keeps parity, so every
 *                sample keeps its colour.
 *   3. channels  at (x, y), each times four (plain bilinear demosaicing, no division yet): c = s(x, y), hs = s(x-1, y) + s(x+1, y),
 *                vs = s(x, y-1) + s(x, y+1), ds = the sum of the four diagonal neighbours.
 *                  R site:                             R4 = 4c,  G4 = hs + vs,  B4 = ds
 *                  B site:                             B4 = 4c,  G4 = hs + vs,  R4 = ds
 *                  G site whose row neighbours are R:  G4 = 4c,  R4 = 2 hs,     B4 = 2 vs
 *                  G site whose row neighbours are B:  G4 = 4c,  B4 = 2 hs,     R4 = 2 vs
 *   4. grey      (9798 R4 + 19235 G4 + 3735 B4 + 65536) >> 17 in integer arithmetic (at most 32768 * 1020 + 65536: it fits 32 bits).
 *                The coefficients are the colour formats' own: a uniform mosaic of value g gives g exactly, nothing exceeds 255.
 * Example: the RGGB image [[10, 200], [30, 90]] gives [[81, 131], [31, 81]].
 * Not covered for mosaics: edge-aware demosaicing, white balance beyond the fixed luma weights, two cameras of different patterns.
 *
 * Packed 10 / 12-bit transports: how USB3 Vision / GigE cameras (PFNC Mono10p, Mono12p, BayerRG12p ..) and MIPI CSI-2 sensors (RAW10,
 * RAW12) deliver 10- and 12-bit data.  A packed frame is a pure TRANSPORT of a 16-bit frame: w x h samples of depth d = 10 or 12 bits,
 * rows tightly packed, no padding at line ends.  w % 4 == 0 is required for d = 10 and w % 2 == 0 for d = 12, so an image is a run of
 * whole groups and is w * h * d / 8 bytes long (av_pixfmt_frame_bytes).  tests/packed_ref.py states all of this in NumPy.
 *   packing                                     group        bytes of a group (p0, p1, .. are its samples, bit ranges inclusive)
 *   10p      PFNC Mono10p: a little-endian      4 px = 5 B   p0[7:0],  p1[5:0]<<2 | p0[9:8],  p2[3:0]<<4 | p1[9:6],  p3[1:0]<<6 | p2[9:4],  p3[9:2]
 *            bit stream, LSB first
 *   12p      PFNC Mono12p                       2 px = 3 B   p0[7:0],  p1[3:0]<<4 | p0[11:8],  p1[11:4]
 *   10_csi2  MIPI CSI-2 RAW10                   4 px = 5 B   p0[9:2],  p1[9:2],  p2[9:2],  p3[9:2],  p3[1:0]<<6 | p2[1:0]<<4 | p1[1:0]<<2 | p0[1:0]
 *   12_csi2  MIPI CSI-2 RAW12                   2 px = 3 B   p0[11:4],  p1[11:4],  p1[3:0]<<4 | p0[3:0]
 * Examples: the samples 0xABC, 0x123 are the bytes BC 3A 12 as 12p and AB 12 3C as 12_csi2; the samples 0x2A5, 0x13C, 0x3FF, 0x001 are
 * A5 F2 F4 7F 00 as 10p and A9 4F FF 00 71 as 10_csi2.
 *   value rule   for every sample v before anything else: s = min(255, (v << (16 - d)) >> shift) with shift = gray16_shift (0 .. 8), in
 *                32-bit integers.  Unpacking left-justifies the sample to 16 bits and the GRAY16 rule applies unchanged, so the default
 *                shift 8 gives the top eight bits of a 10- or 12-bit sample.  With shift 8 the examples give 171, 18 and 169, 79, 255, 0;
 *                with shift 6 the 12-bit pair gives 255, 72.
 *   grey         AV_PIX_GRAY10P .. AV_PIX_GRAY12_CSI2 stop there: s is the grey value.
 *   mosaics      AV_PIX_BAYER_*10P .. AV_PIX_BAYER_*12_CSI2 continue with steps 2 - 4 of the Bayer definition above on the reduced
 *                samples s: a packed mosaic equals the 8-bit mosaic of its s values.  The pattern is code & 3, in the order above.
 *                Two passes: the reduced 8-bit mosaic goes to a scratch, then the 8-bit Bayer kernels run on it unchanged.
 *   format                                      code
 *   AV_PIX_GRAY10P / 12P / 10_CSI2 / 12_CSI2    32 / 33 / 34 / 35
 *   AV_PIX_BAYER_{RGGB,BGGR,GRBG,GBRG}10P       40 .. 43        AV_PIX_BAYER_{..}12P       44 .. 47
 *   AV_PIX_BAYER_{RGGB,BGGR,GRBG,GBRG}10_CSI2   48 .. 51        AV_PIX_BAYER_{..}12_CSI2   52 .. 55
 * Frames of a packed format are BYTE arrays of h rows of w * d / 8 bytes.  No PNG flavour holds one: av_png_decode refuses these codes
 * and av_png_probe never returns them.
 * Not covered for packed transports: line padding or a row stride; GigE Vision's Mono12Packed / Mono10Packed (another bit order);
 * 14-bit packings; widths that are not whole groups; two cameras of different formats; a fused unpack-and-demosaic kernel.
 *
 * av_to_gray8: n_img images of w x h pixels, image i at img_dev + i * img_stride_bytes (tightly packed rows), to tightly packed u8 at
 * out_dev + i * out_stride.  Images at 16-byte aligned addresses and strides (the strides count only when n_img > 1) go through as whole
 * vectors with the last w * h % 16 pixels byte by byte; a launch with any other address or stride goes byte by byte altogether.
 * A Bayer mosaic goes 16 columns per lane when w % 16 == 0 and the addresses and strides are aligned as above, one pixel per lane
 * otherwise.  A packed frame goes 32 (12-bit) or 64 (10-bit) samples per lane as whole vectors when aligned as above, with the ragged
 * end of an image group by group in one lane, and group by group altogether otherwise; img_stride_bytes is at least
 * av_pixfmt_frame_bytes, and a width that is not whole groups is AV_E_INVALID with the format's name in the text.  A packed mosaic
 * allocates its 8-bit mosaic scratch (n_img frames of w * h bytes, 16-byte aligned strides) for the call and waits for the stream before
 * freeing it: for these formats alone the operator blocks the host and cannot be captured into a graph (the engine owns its scratch and does neither).  shift is read for AV_PIX_GRAY16, the 16-bit Bayer formats and the packed formats only but checked always.  AV_E_INVALID with text for an unknown format, a shift outside 0 .. 8,
 * w * h > AV_MAX_IMAGE_PIXELS, strides smaller than an image, and out_dev overlapping the input.  The one exception: AV_PIX_GRAY8 with
 * out_dev == img_dev and equal strides is the identity in place and does nothing (any other AV_PIX_GRAY8 call is a strided copy, and
 * an overlap is refused like for the other formats).  Codes 6 .. 15, 24 .. 31, 36 .. 39 and 56 upwards are unknown formats.
 * ------------------------------------------------------------------------------------------- */
#define AV_PIX_GRAY8  0
#define AV_PIX_GRAY16 1
#define AV_PIX_RGB8   2
#define AV_PIX_BGR8   3
#define AV_PIX_RGBA8  4
#define AV_PIX_BGRA8  5
#define AV_PIX_BAYER_RGGB8  16
#define AV_PIX_BAYER_BGGR8  17
#define AV_PIX_BAYER_GRBG8  18
#define AV_PIX_BAYER_GBRG8  19
#define AV_PIX_BAYER_RGGB16 20
#define AV_PIX_BAYER_BGGR16 21
#define AV_PIX_BAYER_GRBG16 22
#define AV_PIX_BAYER_GBRG16 23
#define AV_PIX_GRAY10P      32
#define AV_PIX_GRAY12P      33
#define AV_PIX_GRAY10_CSI2  34
#define AV_PIX_GRAY12_CSI2  35
#define AV_PIX_BAYER_RGGB10P     40
#define AV_PIX_BAYER_BGGR10P     41
#define AV_PIX_BAYER_GRBG10P     42
#define AV_PIX_BAYER_GBRG10P     43
#define AV_PIX_BAYER_RGGB12P     44
#define AV_PIX_BAYER_BGGR12P     45
#define AV_PIX_BAYER_GRBG12P     46
#define AV_PIX_BAYER_GBRG12P     47
#define AV_PIX_BAYER_RGGB10_CSI2 48
#define AV_PIX_BAYER_BGGR10_CSI2 49
#define AV_PIX_BAYER_GRBG10_CSI2 50
#define AV_PIX_BAYER_GBRG10_CSI2 51
#define AV_PIX_BAYER_RGGB12_CSI2 52
#define AV_PIX_BAYER_BGGR12_CSI2 53
#define AV_PIX_BAYER_GRBG12_CSI2 54
#define AV_PIX_BAYER_GBRG12_CSI2 55
int av_to_gray8(const void* img_dev, int64_t img_stride_bytes, int n_img, int w, int h, int pixel_format, int shift,
                uint8_t* out_dev, int64_t out_stride, void* stream);
/* Bytes of one tightly packed w x h frame of a pixel format: w * h * bytes per pixel, or w * h * d / 8 for a packed transport.  0 for an
 * unknown format, for w or h below 1, and for a packed width that is not whole groups.  Host only. */
int64_t av_pixfmt_frame_bytes(int pixel_format, int w, int h);

/* ---------------------------------------------------------------------------------------------
 * Range scaling of 16-bit grey: a window (lo, hi) instead of the fixed shift of av_to_gray8, for sources whose signal does not fill its
 * container -- a thermal core whose scene occupies a few hundred counts around a drifting offset, a machine-vision camera in low light.
 * No counterpart in the reference; this text is the contract, tests/range16_ref.py states it in NumPy and frontend.gray16_range is the
 * same arithmetic as product code.  AV_PIX_GRAY16 only.  Integer arithmetic throughout; every quantity fits an unsigned 32-bit register.
 *   mapping   given 0 <= lo < hi <= 65535 and span = hi - lo:
 *                 m   = ((255 << 16) + span / 2) / span          once per range, <= 255 << 16   (integer divisions)
 *                 d   = min(max(v, lo), hi) - lo                 0 .. span
 *                 out = min(255, (d * m + 32768) >> 16)
 *             For every span in 1 .. 65535: out(lo) = 0, out(hi) = 255, out is monotone in v, d * m + 32768 < 2^24 + 2^16, and out is less
 *             than one grey level from 255 d / span.  The formula is the definition, the exact quotient is not.
 *   window    AV_GRAY16_WINDOW: one (lo, hi) for every image (config.gray16_window).  No reduction.
 *   auto      AV_GRAY16_AUTO: every range GROUP gets its own (lo, hi) from a 4,096-bin histogram of v >> 4.
 *     group     the two images of one stereo pair -- cam0 and cam1 of one stream-frame -- POOLED: stereo LK assumes the same brightness in
 *               both views, so both images of a pair share one mapping.  av_to_gray8_range pools `pool` = 1 or 2 consecutive images.
 *               The range depends on the group alone, never on a stream's past (the frame store converts a frame once for all the
 *               offset streams that read it): there is no temporal damping.
 *     N         the samples of the group, w * h * images.
 *     clip      (ppm_lo, ppm_hi), default (100, 100): integers >= 0 whose sum is at most AV_GRAY16_MAX_CLIP_PPM = 500000, the share of
 *               samples that may saturate at each end in parts per million.  k_lo = N * ppm_lo / 10^6 and k_hi = N * ppm_hi / 10^6
 *               (integer division, 64 bits, on the host).
 *     bins      b_lo = the smallest bin b with hist[0 .. b].sum() > k_lo; b_hi = the largest bin b with hist[b .. 4095].sum() > k_hi.
 *               A cumulative count exactly equal to k moves on to the next bin.  k_lo + k_hi < N, so b_lo <= b_hi.
 *     range     lo = 16 b_lo, hi = 16 b_hi + 15.
 *     min span  min_span, default 256, 16 .. 65535 (with 256 no count becomes more than one grey level: a lens cap or an empty sky is
 *               not turned into amplified noise).  If hi - lo < min_span:
 *                 need = min_span - (hi - lo);  lo = max(0, min(lo - need / 2, 65535 - min_span));  hi = lo + min_span
 *               The new range always contains the old one.
 *   Histogram counts are integers added with integer atomics: the result does not depend on their order and is bit-identical from run
 *   to run.
 * The engine: av_frontend_set_gray16_scale(fe, scale, lo, hi, clip_lo_ppm, clip_hi_ppm, min_span) -- config.gray16_scale as
 * AV_GRAY16_SHIFT / _WINDOW / _AUTO, config.gray16_window, config.gray16_auto_clip, config.gray16_auto_min_span; each is checked for the
 * scale that reads it -- chooses the scale of an engine before its first frame, like av_frontend_set_masks (after a step, a prestage or
 * an upload: AV_E_INVALID, the frames in the engine would disagree with the new scale).  av_frontend_config is unchanged, so a caller that
 * never makes the call has the shift.  A scale other than AV_GRAY16_SHIFT needs pixel_format = AV_PIX_GRAY16 (any other format:
 * AV_E_INVALID with both settings in the text; the Python engine refuses it when it is created) and replaces the shift conversion, at its
 * place in the input chain, in all entry paths and in av_frontend_frames_upload; gray16_shift is then not read.  Everything downstream -- photometric calibration, binning,
 * CLAHE, masks -- is unchanged, and av_frontend_read_image returns the grey frame the step used.  With AV_GRAY16_AUTO the engine owns a
 * histogram and a record per stream (the frame store: per frame of one upload), allocated by that call and only then; the three launches go on the
 * stream of the step (the copy stream for an upload), with no host wait and no read-back inside a step.  With AV_GRAY16_SHIFT nothing is
 * launched and nothing more is allocated.
 * av_frontend_read_range: int32 [n_streams][2], the (lo, hi) the frames of the last step were scaled with, for av_frontend_step (with or
 * without persisting inputs, prestaged or not) and av_frontend_step_host.  AV_E_INVALID with text before the first step, after an
 * av_frontend_step_frames (a store entry is shared by streams and keeps no range) and with AV_GRAY16_SHIFT.
 * av_to_gray8_range: n_img images of w x h uint16 samples, image i at img_dev + i * img_stride_bytes, in groups of `pool` (1 or 2;
 * n_img % pool == 0) consecutive images, to tightly packed u8.  index_dev (or null) is a device list of one int per GROUP: group g is
 * written to the output images (index[g] * pool + c) * out_stride, c < pool; a negative entry skips the group -- no histogram, no range, no
 * pixel -- and the caller names no entry twice (null: group g goes to entry g; with a list the overlap of input and output is the
 * caller's to avoid).  range_dev (or null): int32 [n_img / pool][2], (lo, hi) of every group written.  AV_GRAY16_AUTO works in work_dev,
 * AV_GRAY16_WORK_WORDS uint32 per group, ZERO before the first call and left zero in its histogram part by every call (records: the words
 * behind the n_img / pool histograms of 4096); with work_dev null the operator allocates it for the call and waits for the stream before
 * freeing it (it then blocks the host and cannot be captured into a graph).  Alignment as av_to_gray8: 16-byte aligned addresses and
 * strides go as whole vectors, the ragged end and any other launch sample by sample.  AV_E_INVALID with text for a mode other than 1 or 2,
 * a window outside 0 <= lo < hi <= 65535, a clip below 0 or above 500000 in sum, a minimum span outside 16 .. 65535 (each checked for the
 * mode that reads it), pool other than 1 or 2, strides smaller than an image, and out_dev overlapping the input.
 * Not covered: temporal damping of the range (see "group"); finer than 16-count granularity of lo and hi; 16-bit mosaics and packed
 * transports; per-camera ranges; a region of interest for the statistics; fusion with the histograms CLAHE builds.
 * ------------------------------------------------------------------------------------------- */
#define AV_GRAY16_SHIFT  0
#define AV_GRAY16_WINDOW 1
#define AV_GRAY16_AUTO   2
#define AV_GRAY16_MAX_CLIP_PPM 500000
#define AV_GRAY16_WORK_WORDS 4100
int av_to_gray8_range(const void* img_dev, int64_t img_stride_bytes, int n_img, int w, int h, int mode, int lo, int hi,
                      int ppm_lo, int ppm_hi, int min_span, int pool, const int32_t* index_dev,
                      uint8_t* out_dev, int64_t out_stride, int32_t* range_dev, uint32_t* work_dev, void* stream);
int av_frontend_set_gray16_scale(av_frontend* fe, int scale, int lo, int hi, int clip_lo_ppm, int clip_hi_ppm, int min_span);
int av_frontend_read_range(av_frontend* fe, int32_t* range_out_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Binning of 8-bit grey frames by f = 2 or 4.  No counterpart in the reference (other VIO stacks run their front-end on a reduced
 * image with scaled intrinsics -- OpenVINS' downsample_cameras -- and most sensors bin 2 x 2 themselves); this text is the contract,
 * tests/downscale_ref.py states it in NumPy.
 *   input    W x H samples with W % f == 0 and H % f == 0; output w x h with w = W / f, h = H / f
 *   pixel    out(x, y) = (sum of the f x f input block at (f x .. f x + f - 1, f y .. f y + f - 1) + f * f / 2) >> (2 log2 f):
 *            (a + b + c + d + 2) >> 2 for f = 2, (sum of 16 + 8) >> 4 for f = 4.  Integers only, no border rule.
 *   camera   output pixel x covers input pixels f x .. f x + f - 1, centre X = f x + (f - 1) / 2: a pinhole camera of the binned image
 *            has fx' = fx / f, fy' = fy / f, cx' = (cx - (f - 1) / 2) / f, cy' = (cy - (f - 1) / 2) / f and the distortion coefficients
 *            of the full-size one (av_frontend_config.image_downscale applies exactly these).
 * Example: f = 2 on [[1, 2], [3, 5]] gives [[3]] (13 >> 2); a uniform image of value g gives g.
 * av_downscale: n_img images, image i at img_dev + i * img_stride (tightly packed W * H u8), to tightly packed w * h u8 at
 * out_dev + i * out_stride.  With w % 16 == 0 and 16-byte aligned addresses and strides (the strides count only when n_img > 1) a lane
 * takes 16 output pixels from f rows of f 16-byte vectors; anything else goes one output pixel per lane.  AV_E_INVALID with text for a
 * factor other than 2 or 4, W or H the factor does not divide, W * H > AV_MAX_IMAGE_PIXELS, strides smaller than an image, null
 * pointers, n_img < 0 and out_dev overlapping the input (never in place).  n_img == 0 is AV_OK.
 * Not covered: Gaussian / pyrDown filtering, odd factors, cropping, a fused convert-and-bin pass.
 * ------------------------------------------------------------------------------------------- */
int av_downscale(const uint8_t* img_dev, int64_t img_stride, int n_img, int W, int H, int factor,
                 uint8_t* out_dev, int64_t out_stride, void* stream);
/* TEST-ONLY observable, not part of the supported interface (it may change or go without notice): 1 if av_downscale with these
 * arguments takes 16 output pixels per lane, 0 if one (or if the arguments are not a valid call).  It is the launcher's own rule,
 * exported so that tests/test_gpu_downscale_op.py can assert which kernel a case reached.  Pure host function. */
int av_downscale_vector_path(const uint8_t* img_dev, int64_t img_stride, int n_img, int W, int factor, const uint8_t* out_dev, int64_t out_stride);

/* ---------------------------------------------------------------------------------------------
 * Photometric calibration of 8-bit grey frames ("Photometric calibration" above has the definition):
 *   out = min(255, (response[p] * gain[x] + (1 << 19)) >> 20)
 * av_photometric: n images, image i at in_dev + i * in_stride (tightly packed w * h u8), to out_dev + i * out_stride.  response_dev:
 * uint16[256] Q8 on the device or NULL (p * 256); gain_dev: uint16[w * h] Q12 on the device or NULL (4096), one map for all n images.
 * out_dev == in_dev with equal strides (they count only when n > 1) works in place; any other overlap of the two spans is refused.  With 16-byte aligned image
 * addresses, strides (they count only when n > 1) and gain address a lane takes 16 pixels from whole vectors, and the last w * h % 16
 * pixels of every image go byte by byte; anything else goes one pixel per lane.  AV_E_INVALID with text for w * h outside
 * 1 .. AV_MAX_IMAGE_PIXELS, strides smaller than an image, null images, n < 0, both tables NULL, a partially overlapping output and
 * a response entry above AV_PHOTOMETRIC_RESPONSE_MAX (the call reads the 512-byte table back to check it, so it waits for the stream
 * when a response is given; the engine checks its tables once, when they are set).  n == 0 is AV_OK.
 * ------------------------------------------------------------------------------------------- */
int av_photometric(const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                   const uint16_t* response_dev, const uint16_t* gain_dev, void* stream);
/* The same with per-image exposure factors ("Exposure-time normalisation" above): k_dev uint16[n] Q12 on the device, image i with
 * r'[p] = min(65280, (response[p] * k_dev[i] + 2048) >> 12) in place of response[p]; NULL = none (then exactly av_photometric).  All
 * three of response_dev, gain_dev and k_dev are optional, but not all three NULL; the other checks are av_photometric's.  A factor of 0
 * is not refused here (it blacks the image out); the engine refuses it. */
int av_photometric_exposure(const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                            const uint16_t* response_dev, const uint16_t* gain_dev, const uint16_t* k_dev, void* stream);
/* TEST-ONLY observable, not part of the supported interface (it may change or go without notice): 1 if av_photometric with these
 * arguments takes 16 pixels per lane, 0 if one (or if the arguments are not a valid call).  The launcher's own rule, exported so that
 * tests/test_gpu_photometric_op.py can assert which body a case reached.  Pure host function. */
int av_photometric_vector_path(const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                               const uint16_t* response_dev, const uint16_t* gain_dev);

/* ---------------------------------------------------------------------------------------------
 * Two-point RANSAC on the temporal matches of ONE camera (no counterpart in the reference: feature_tracker.py:135-136 is where
 * it would run; the stereo MSCKF the reference descends from has it).  The IMU gives the rotation, so two point pairs fix the
 * translation direction.  One problem: n pairs (p1_i, p2_i) of float32 pixel positions of the same feature in the previous and the
 * current image, R = rotation previous -> current camera frame, the camera's model, thr (pixels), success probability p.
 * Output: one marker (0 / 1) per pair.  All arithmetic in fp64, products summed left to right, no contraction:
 *   1. u1_i = undistort(p1_i), u2_i = undistort(p2_i): normalised coordinates, identity rectification (av_undistort_points_model)
 *   2. h = R (u1_i.x, u1_i.y, 1);  u1_i = (h.x / h.z, h.y / h.z)
 *   3. s = sqrt(2) * 2n / sum_i (|u1_i| + |u2_i|);  u1_i *= s, u2_i *= s;  unit = s * 2 / (fx + fy)
 *   4. d_i = u1_i - u2_i.  |d_i| > 50 unit: marker 0.  The others are the raw set (index order), m of them, mean |d_i| = mean
 *   5. m < 3: all markers 0                                                              (AV_RANSAC_PATH_FEW)
 *   6. mean < unit (standstill / pure rotation): raw pairs with |d_i| > thr unit get 0, the others 1   (AV_RANSAC_PATH_STILL)
 *   7. c_i = (d_i.y, -d_i.x, u1_i.x u2_i.y - u1_i.y u2_i.x): a translation direction t consistent with pair i has c_i . t = 0
 *   8. N = av_ransac_num_hypotheses(p).  Hypothesis k: r0 = av_ransac_hash(seed, frame, camera, k, 0), r1 = (.., k, 1);
 *      a = r0 mod m, b = (a + 1 + r1 mod (m - 1)) mod m index the raw set.  The column of [c_a; c_b] with the smallest L1 norm
 *      (first on ties) is the base j: t_j = 1, the other two (p < q) solve the 2 x 2 system: det = c_a[p] c_b[q] - c_a[q] c_b[p],
 *      t_p = (c_a[q] c_b[j] - c_a[j] c_b[q]) / det, t_q = (c_a[j] c_b[p] - c_a[p] c_b[j]) / det.  det == 0 or a non-finite t skips
 *      the hypothesis.  A raw pair is an inlier if |c_i . t| < thr unit.  Fewer inliers than 0.2 n skips the hypothesis.  The
 *      hypothesis with strictly more inliers than the best so far becomes the best.                  (AV_RANSAC_PATH_MODEL)
 *   9. markers = the best inlier set; all 0 if no hypothesis qualified                    (.. | AV_RANSAC_PATH_NONE)
 * The draws are a stateless hash of (seed, the stream's own frame number, camera, k, draw) and of nothing else, so a problem gives
 * the same markers alone, anywhere in a batch and in any launch shape:
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16          (uint32, wrapping)
 *   av_ransac_hash(seed, frame, camera, k, draw) = mix(mix(mix(seed + 0x9e3779b9) ^ frame) ^ (camera << 16 | k << 1 | draw))
 * av_ransac_hash and av_ransac_num_hypotheses are pure host functions (the kernels inline the same code):
 *   N = ceil(log(1 - p) / log(1 - 0.7^2)) clamped to 1 .. AV_RANSAC_MAX_HYPOTHESES; 7 at p = 0.99; 0 if p is outside (0, 1).
 *
 * av_two_point_ransac runs n_problems problems in one launch (one wavefront each).  Problem b owns the pairs off_dev[b] ..
 * off_dev[b + 1] - 1 of pts1_dev / pts2_dev (float32 x, y), at most max_pairs <= AV_RANSAC_MAX_PAIRS of them; R_dev[9 b ..] is its
 * rotation (row-major), camera_dev[b] and frame_dev[b] its hash words (NULL = all 0).  intr / dist / model as in
 * av_undistort_points_model (host pointers, one camera model per call).  markers_dev: uint8 per pair.  info_dev (optional):
 * int32 [n_problems][2] = {markers set, AV_RANSAC_PATH_* code}; {-1, -1} for a problem with more than max_pairs pairs (its markers
 * are not written).
 * ------------------------------------------------------------------------------------------- */
#define AV_RANSAC_MAX_PAIRS       1920     /* per problem: the pairs of a problem live in one workgroup's LDS (33 B each) */
#define AV_RANSAC_MAX_HYPOTHESES  64
#define AV_RANSAC_PATH_FEW    1
#define AV_RANSAC_PATH_STILL  2
#define AV_RANSAC_PATH_MODEL  4
#define AV_RANSAC_PATH_NONE   8
uint32_t av_ransac_hash(uint32_t seed, uint32_t frame, uint32_t camera, uint32_t k, uint32_t draw);
int av_ransac_num_hypotheses(double success_probability);
int av_two_point_ransac(const float* pts1_dev, const float* pts2_dev, const int32_t* off_dev, int n_problems, int max_pairs,
                        const double* R_dev, const int32_t* camera_dev, const int32_t* frame_dev,
                        const double* intr, const double* dist, int model, double inlier_error, double success_probability,
                        uint32_t seed, uint8_t* markers_dev, int32_t* info_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MSCKF back-end: the batched small-dense fp64 linear algebra of MSCKF.feature_callback
 * (reference: msckf.py:177-228).  The covariance P lives on the device inside the context (row-major,
 * leading dimension av_msckf_ld); state vectors and the feature/camera bookkeeping stay with the
 * caller (the Python MSCKF class mirrors the reference's dict bookkeeping).  Per-feature inputs are
 * CSR-style: observations of feature f are obs_off[f] .. obs_off[f+1]-1, each with the index of its
 * camera state (position in the cam_states dict) and z = (u0, v0, u1, v1).
 * ------------------------------------------------------------------------------------------- */
typedef struct av_msckf av_msckf;

/* chi2_table_100[d] = chi2.ppf(0.05, d) for d = 1..99 (msckf.py:111-113); rows_cap = capacity of the
 * stacked Jacobian in rows (the prune path of the reference is uncapped). */
int  av_msckf_create(int max_cam_states, int rows_cap, const double* chi2_table_100, int device, av_msckf** out);
void av_msckf_destroy(av_msckf* ctx);
int  av_msckf_ld(const av_msckf* ctx);
int  av_msckf_dim(const av_msckf* ctx);
/* state_cov <- host matrix n x n (reset_state_cov msckf.py:788-798, online_reset :843); / read back. */
int  av_msckf_set_cov(av_msckf* ctx, const double* P_host, int n, void* stream);
int  av_msckf_get_cov(av_msckf* ctx, double* P_host, int n, void* stream);
/* MSCKF.process_model covariance part (msckf.py:282-335) for one IMU sample: builds F, G, Phi (3rd
 * order), applies the observability fix with the null-space states, Q = Phi G Qc G^T Phi^T dt,
 * P11 <- Phi P11 Phi^T + Q, P12 <- Phi P12, symmetrise.  gyro/acc are bias-corrected; q_old is the
 * orientation before predict_new_state, q_new/v_new/p_new after; noise = continuous variances
 * [gyro, gyro_bias, acc, acc_bias] (msckf.py:123-127). */
int  av_msckf_propagate(av_msckf* ctx, double dt, const double gyro[3], const double acc[3], const double q_old[4],
                        const double q_new[4], const double q_null[4], const double v_null[3], const double p_null[3],
                        const double v_new[3], const double p_new[3], const double gravity[3], const double noise[4],
                        void* stream);
/* MSCKF.state_augmentation covariance part (msckf.py:407-423): J = [R_i_c 0 0 0 0 I 0; skew(R_w_i^T t_c_i) 0 0 0 I 0 I]. */
int  av_msckf_augment(av_msckf* ctx, const double R_imu_cam0[9], const double skew_Rt_t[9], void* stream);
/* prune_cam_state_buffer (msckf.py:774-786): drop the 6 rows/cols of camera state #cam_index. */
int  av_msckf_remove_cam(av_msckf* ctx, int cam_index, void* stream);
/* Feature.initialize_position (feature/feature_position_initializer.py:6-76) for n_feat features.
 * opt5 = [huber_epsilon, estimation_precision, initial_damping, outer_loop_max, inner_loop_max]
 * (config.py:7-17); max_views = 2 * (largest observation count) <= 64. */
int  av_msckf_triangulate(av_msckf* ctx, int n_feat, const int32_t* obs_off_dev, const int32_t* obs_cam_dev, const double* obs_z_dev,
                          const double* cam_q_dev, const double* cam_p_dev, const double* T_cam0_cam1_rowmajor44,
                          const double* opt5, int max_views, double* pos_dev, int32_t* valid_dev, void* stream);
/* MSCKF.feature_jacobian + gating_test (msckf.py:509-546, 604-612) for n_feat features: writes the
 * null-space-projected rows (4M-3 per feature, starting at row_off[f]) into the context's block
 * buffer and gamma / pass per feature.  dof[f] = chi^2 degrees of freedom (msckf.py:662, 761). */
int  av_msckf_feature_blocks(av_msckf* ctx, int n_feat, int n_cam, int max_obs, const int32_t* obs_off_dev, const int32_t* obs_cam_dev,
                             const double* obs_z_dev, const double* pos_dev, const int32_t* dof_dev, const int32_t* row_off_dev, int total_rows,
                             const double* cam_q_dev, const double* cam_p_dev, const double* cam_qn_dev, const double* cam_pn_dev,
                             const double* T_cam0_cam1_rowmajor44, const double gravity[3], double obs_noise,
                             double* gamma_dev, int32_t* pass_dev, void* stream);
/* Parity-test tap (tests only): rows row0 .. row0 + n_rows - 1 of the block buffer av_msckf_feature_blocks filled -- H_host gets
 * n_rows x av_msckf_ld doubles (full-width rows: IMU columns and the columns of cameras the feature was not seen from read zero),
 * r_host n_rows.  Synchronises.  row0 + n_rows <= rows_cap, else AV_E_CAPACITY. */
int  av_msckf_read_blocks(av_msckf* ctx, int row0, int n_rows, double* H_host, double* r_host, void* stream);
/* MSCKF.measurement_update (msckf.py:548-602) on the blocks (first row, length) selected by the
 * caller after gating: thin QR when rows > n, S, gain, P <- sym((I-KH)P).  Synchronises and returns
 * delta_x (n doubles) for the caller's state injection (msckf.py:568-595). */
int  av_msckf_update(av_msckf* ctx, const int32_t* blk_row_dev, const int32_t* blk_len_dev, int n_blk, int total_rows,
                     double obs_noise, double* dx_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Quaternion / rotation helpers of the filter, for host callers (replaces the functions of src/utils.py; JPL
 * quaternions [x, y, z, w]).  Pure host functions (no device needed); rotation matrices are 9 doubles, row-major.
 *   av_quat_to_rotation       to_rotation(q)                   utils.py:12-23   (normalises q first)
 *   av_rotation_to_quat       to_quaternion(R)                 utils.py:25-47
 *   av_quat_multiply          quaternion_multiplication(a, b)  utils.py:61-76   (normalises inputs and output)
 *   av_quat_small_angle       small_angle_quaternion(dtheta)   utils.py:79-93   (|dtheta/2|^2 <= 1 branch rule)
 *   av_quat_from_two_vectors  from_two_vectors(v0, v1)         utils.py:96-120  (antiparallel / parallel fallbacks)
 * ------------------------------------------------------------------------------------------- */
int  av_quat_to_rotation(const double q[4], double R_rowmajor9[9]);
int  av_rotation_to_quat(const double R_rowmajor9[9], double q[4]);
int  av_quat_multiply(const double q1[4], const double q2[4], double out[4]);
int  av_quat_small_angle(const double dtheta[3], double q[4]);
int  av_quat_from_two_vectors(const double v0[3], const double v1[3], double q[4]);

/* ---------------------------------------------------------------------------------------------
 * n_streams independent MSCKF filters stepped together (the throughput path of the back-end).  The
 * whole of MSCKF.feature_callback (msckf.py:177-228) runs inside the library for all streams: state,
 * observation map, selections and state injection live on the device, and a step is one fixed sequence
 * of batched launches over all streams (the numeric kernels are those of av_msckf_*).
 *   R_imu_cam0_t_cam0_imu12 = [inv(T_imu_cam0)[:3,:3].T (9, row-major), inv(T_imu_cam0)[:3,3] (3)] (msckf.py:132-134)
 *   cov_init5 = [gyro_bias_cov, velocity_cov, acc_bias_cov, extrinsic_rotation_cov, extrinsic_translation_cov]
 *   noise4    = [gyro_noise, gyro_bias_noise, acc_noise, acc_bias_noise]        (config.py:71-75)
 *   opt6      = [huber_epsilon, estimation_precision, initial_damping, outer_max, inner_max, translation_threshold]
 * ------------------------------------------------------------------------------------------- */
typedef struct av_msckf_batch av_msckf_batch;
int  av_msckf_batch_create(int n_streams, int max_cam_states, int rows_cap, const double* chi2_table_100, const double gravity[3],
                           const double* T_cam0_cam1_rowmajor44, const double* R_imu_cam0_t_cam0_imu12, const double cov_init5[5],
                           const double noise4[4], double obs_noise, double position_std_threshold, const double velocity0[3],
                           const double* opt6, int device, av_msckf_batch** out);
void av_msckf_batch_destroy(av_msckf_batch* b);
/* MSCKF.imu_callback for n samples (msckf.py:162-175 incl. initialize_gravity_and_bias); gyro/acc are [n][3]. */
int  av_msckf_batch_push_imu(av_msckf_batch* b, const int32_t* stream_idx, const double* timestamps, const double* gyro, const double* acc, int n);
/* MSCKF.feature_callback for every stream.  Host inputs: stream s has n_feat[s] features, ids[s*cap+k],
 * uv[(s*cap+k)*4..] = u0 v0 u1 v1.  out[s*12..] = {published (0/1; -1 = stream stopped, av_msckf_batch_stream_status),
 * t, p[3], q[4] (JPL xyzw), v[3]}.
 * A stream is live for a frame iff its gravity initialisation was completed by an IMU sample not newer than the frame
 * (msckf.py:182-183 under the deterministic replay); timestamps[s] < 0 means "no frame for stream s in this
 * step" (sequences of different lengths stepped together): the stream idles and reports published = 0.
 * The first step fixes the message capacity `cap` the device buffers are sized for; rows_cap must be >= 5*cap
 * (camera-pruning update) and >= 1664 (lost-feature update: 1500-row cut + one block), else AV_E_CAPACITY;
 * rows_cap = 0 at create sizes the block buffers from that first `cap` (max(2048, 5*cap + 64) rows).  A later step with a larger
 * cap REBUILDS them (and the observation store) for the wider message: the batch is drained and the device
 * synchronised, the capacity grows geometrically (x1.5 at least) and the outgrown allocations stay parked until destroy -- pass
 * the largest cap at the first step (BatchedMSCKF(max_features=...)) when the width of the messages varies.  An explicit
 * rows_cap is never grown: a wider message than it can hold fails with AV_E_CAPACITY.
 * rows_cap rows are what each stream owns.  The lost features of one frame may need more (a blank frame drops every track at once:
 * ~4,500 rows at 150 tracks): the filter then takes the rows from a pool all streams share, allocated behind the
 * last stream's region -- max(131,072, n_streams * rows_cap) rows of ld doubles, AV_MSCKF_POOL_ROWS overrides -- and stops a
 * stream that finds the pool exhausted with AV_E_CAPACITY (av_msckf_batch_stream_status).
 * max_cam_states <= 24 (one back-end pass holds 144 columns = 6 per camera state); the reference's value is 20. */
int  av_msckf_batch_step(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                         const double* timestamps, double* out, void* stream);
/* The same step, queued: returns at once; the stream groups of the batch consume their queues independently (a group
 * that is done with frame k starts frame k+1 without waiting for the slowest group, the way the reference's VIO
 * thread runs behind a queue, modules/vio.py:46-58).  All buffers of a submitted step, inputs and `out`, must stay
 * valid until av_msckf_batch_wait has let it retire.  Steps retire in submission order.
 * av_msckf_batch_wait blocks until at most max_pending submitted steps are unfinished (0 = drain) and returns the
 * first error any of them raised (later queued steps are then skipped).  av_msckf_batch_get_cov / _sizes / _push_imu for
 * a frame whose step is already queued must not race with pending steps: drain (wait 0) before reading state. */
int  av_msckf_batch_submit(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                           const double* timestamps, double* out, void* stream);
int  av_msckf_batch_wait(av_msckf_batch* b, int max_pending);
/* av_msckf_batch_submit with the feature message in DEVICE arrays (av_frontend_features_dev): the three arrays are consumed by
 * copies enqueued on msg_stream -- the stream that produced them -- before the call returns, so the producer may overwrite them
 * at once; the filter's kernels run on the stream groups' own streams (a batch of one group: on `stream`) behind an event.
 * timestamps and out are host arrays and must stay valid until av_msckf_batch_wait has let the step retire.  Blocks while
 * more than two earlier steps are unfinished. */
int  av_msckf_batch_device_resident(const av_msckf_batch* b);     /* always 1: state + observation map live on the device (kept for callers that ask) */
int  av_msckf_batch_submit_dev(av_msckf_batch* b, const int64_t* ids_dev, const double* uv_dev, const int32_t* n_feat_dev, int cap,
                               const double* timestamps, double* out, void* msg_stream, void* stream);
int  av_msckf_batch_get_cov(av_msckf_batch* b, int stream_idx, double* P_host, int n, void* stream);
/* Odometry covariance: the uncertainty of what a step publishes, per stream and step, riding the step's one read-back.
 * The record is the 15 x 15 symmetric matrix C = J P[0:21, 0:21] J^T, P = state_cov AT THE MOMENT OF publish (msckf.py:845-867): the
 * pruning update and the removal of its two camera states are in, online_reset (:821-843) has not taken effect -- on a reset step
 * av_msckf_batch_get_cov returns the re-initialised matrix, this record the one the pose was published with.
 * Error coordinates, in this order:
 *   rows  0:3   p        IMU position in the world frame
 *   rows  3:6   theta    rotation error of R_wb = to_rotation(q)^T applied on the RIGHT (body frame): R_wb,true = R_wb (I + [theta]x);
 *                        this is the filter's own error state delta-theta (q <- dq (x) q, msckf.py:576-579)
 *   rows  6:9   v        velocity in the world frame (what the reference publishes as body_velocity with T_imu_body = I)
 *   rows  9:12  p_c      position of cam0 in the world frame, t_c_w = p + R_wb t_cam0_imu
 *   rows 12:15  theta_c  rotation error of R_wc = (R_imu_cam0 R_wb^T)^T, applied on the right (cam0 frame)
 * With the reference's error-state order (theta 0:3, b_g 3:6, v 6:9, b_a 9:12, p 12:15, theta_ext 15:18, t_ext 18:21), R_ic = R_imu_cam0
 * and t_ci = t_cam0_imu as published with the pose, the non-zero blocks of J are
 *   J[0:3, 12:15] = I;  J[3:6, 0:3] = I;  J[6:9, 6:9] = I;
 *   J[9:12, 12:15] = I;  J[9:12, 0:3] = -R_wb [t_ci]x;  J[9:12, 18:21] = R_wb;
 *   J[12:15, 0:3] = R_ic;  J[12:15, 15:18] = I
 * (from the injection rules q <- dq (x) q, R_ic <- R(dq_ext) R_ic, t_ci += dt, msckf.py:568-595; checked against central differences of
 * those maps, tests/test_odom_cov_ref.py).  Entries of rows and columns 0:9 are the selected entries of P, bit for bit.
 * On the wire: the upper triangle, row-major, AV_ODOM_COV_DOUBLES = 120 doubles per stream ((0,0) .. (0,14), (1,1) .. (14,14)).  Where
 * the step's `published` is not 1 (no gravity yet, no frame, a stopped stream) all 120 are NaN.
 * av_msckf_batch_set_odom_cov(b, enable): before the batch's first step (AV_E_INVALID afterwards).  Off (the default) the step launches
 * and reads back exactly what it did without the feature; on, the last per-stream kernel of the step is the instance that also writes
 * the records (no launch more) and one more asynchronous copy brings them to a pinned buffer of the step's ring slot: no wait and no
 * allocation inside a step.
 * av_msckf_batch_next_odom_cov(b, cov_host): hands over the destination, n_streams * AV_ODOM_COV_DOUBLES doubles, of the records of
 * the NEXT av_msckf_batch_step / _submit / _submit_dev; it is filled when that step retires (step: on return; submit: once
 * av_msckf_batch_wait has let it retire) and must stay valid until then.  Stream groups each fill their own part.  AV_E_INVALID while
 * the feature is off.  A step without a destination computes its records and drops them.
 * Known limits: no conjugation for T_imu_body != I; the right (body-frame) rotation convention only -- the world-frame one is the
 * similarity by R_wb; no bias or extrinsic blocks; no innovation statistics. */
#define AV_ODOM_COV_DOUBLES 120
int  av_msckf_batch_set_odom_cov(av_msckf_batch* b, int enable);
int  av_msckf_batch_next_odom_cov(av_msckf_batch* b, double* cov_host);
/* Landmark map: the 3-D positions of the features a step triangulates and uses, per stream and step, riding the step's read-back.
 * Off by default.  On, every step yields for every stream a count pair n[s][2] and up to `cap` records of AV_LANDMARK_BYTES = 40 bytes:
 *   id      the feature id of the front-end message
 *   p       its position in the filter's world frame, exactly the doubles the filter used: what the triangulation wrote for a feature
 *           triangulated in this step, the stored position of one fixed in an earlier step.  Positions are never re-estimated after the
 *           update (as in the reference).
 *   n_obs   camera states that observed the feature when it was evaluated
 *   flags   AV_LM_USED      its rows went into the update
 *           AV_LM_REJECTED  it was evaluated and the chi-square gate rejected it.  Neither bit: the feature lies beyond the 1,500-row cut
 *                           of the lost-feature update (msckf.py:667-668), where the reference never evaluates it; the feature whose
 *                           rows take the running sum over 1,500 is still USED.
 *           AV_LM_TRACKED   the record comes from the pruning update and the feature stays in the map
 *           AV_LM_NEW       the position was triangulated in this step
 * Records of the lost-feature update (msckf.py:614-676) come first, in map (dict) order: every candidate whose position is valid (the
 * reference's `processed` list).  These features leave the map in this step: the positions are final.  Records of the pruning update
 * (msckf.py:712-786) follow, in map order: only the candidates whose position was first obtained in this step (TRACKED | NEW).  A feature
 * fixed in an earlier pruning step is not republished; when it is lost it appears once more among the lost-feature records, with the same
 * position bits and without NEW.  Not published: candidates check_motion held back, candidates whose triangulation failed, pruning
 * candidates with a single removed observation.
 * Counts: n[s][0] = records the step had, n[s][1] = records written = min(n[s][0], cap); on overflow the first `cap` records in the order
 * above are written and the rest dropped; records past n[s][1] are unspecified.  A stream that is inactive, failed or stopped in this
 * step has n = {0, 0}.  A step that ends in online_reset still publishes what its two updates used.
 * av_msckf_batch_set_landmarks(b, cap): cap records per stream and step, 0 = off; before the batch's first step (AV_E_INVALID afterwards).
 * Off, the step launches and reads back exactly what it did without the feature; on, two per-stream kernels of the step are the instances
 * that also write the records (no launch more) and two more asynchronous copies bring records and counts to pinned buffers of the step's
 * ring slot: no wait and no allocation inside a step.
 * av_msckf_batch_next_landmarks(b, rec, n): hands over the destination -- n_streams * cap records and n_streams * 2 counts -- of the NEXT
 * av_msckf_batch_step / _submit / _submit_dev; it is filled when that step retires and must stay valid until then.  A queued step keeps
 * its own destination.  Stream groups each fill their own part.  AV_E_INVALID while the feature is off.  A step without a destination
 * computes its records and drops them.
 * Known limits: positions as triangulated, not refined by the update; no per-landmark covariance; carried pruning features are not
 * republished. */
#define AV_LANDMARK_BYTES 40
#define AV_LM_USED     1
#define AV_LM_REJECTED 2
#define AV_LM_TRACKED  4
#define AV_LM_NEW      8
typedef struct av_landmark { int64_t id; double p[3]; int32_t flags; int32_t n_obs; } av_landmark;
int  av_msckf_batch_set_landmarks(av_msckf_batch* b, int cap);
int  av_msckf_batch_next_landmarks(av_msckf_batch* b, av_landmark* rec, int32_t* n);
/* Innovation statistics: what the chi-square gates of a step's two measurement updates decided and how large the corrections were, per
 * stream and step, riding the step's read-back.  Off by default.  On, every step yields for every stream one av_filter_stats of
 * AV_FILTER_STATS_BYTES = 128 bytes: two blocks of 64 bytes, upd[0] the lost-feature update (remove_lost_features, msckf.py:614-676),
 * upd[1] the pruning update (prune_cam_state_buffer, msckf.py:712-786).  Per block, over the update's candidates in map (dict) order:
 *   n_cand      candidates of the update: lost features with at least three observations; features seen from both camera states that go
 *   n_pos       ... of them with a valid position (triangulated in this step or in an earlier one; check_motion or a failed
 *               triangulation leave none)
 *   n_eval      ... of them the reference would have gated.  Lost-feature update: those its loop reaches before msckf.py:667-668 breaks
 *               it, i.e. the candidates ahead of which at most 1,500 accepted rows are stacked (the candidate whose rows take the sum
 *               over 1,500 is still evaluated and, if accepted, used).  Pruning update: n_eval = n_pos.
 *   n_pass      evaluated and accepted by the gate (gamma < chi2.ppf(0.05, dof)): the features whose rows the update used
 *   dof_eval    sum of the gate's dof over the evaluated;  dof_pass  over the accepted
 *   gamma_eval  sum of the Mahalanobis values gamma = r^T (H P H^T + observation_noise I)^-1 r over the evaluated;  gamma_pass  over the accepted
 *   rows        rows of the stacked update as applied (before any compression), 0 if none was applied
 *   flags       AV_FS_RAN  an update was applied to the state;  AV_FS_CUT  the 1,500-row cut left candidates unevaluated (n_eval < n_pos)
 *   dx_pos      |delta_x[12:15]| of the applied update, the position correction in metres; 0 if none
 *   dx_rot      |delta_x[0:3]|, the orientation correction in radians; 0 if none
 * The gate's dof is the reference's, not the residual's dimension: a feature seen from M camera states has a residual of 4 M - 3 rows
 * (stereo observations, three dimensions projected out) and is gated with dof = M - 1 in the lost-feature update and with dof = the
 * number of involved camera states (always 2) in the pruning update.  The residual dimension follows from the record: over n features
 * with dof sum d it is 4 d + n for the lost-feature update (M = dof + 1) and 4 d - 3 n for the pruning update (M = dof); for the
 * accepted features that is `rows`.  gamma_pass is a sum over a distribution the gate has truncated; gamma_eval is not.
 * Values are those of the device's evaluation: every candidate is gated against the covariance before the update, as in the reference.
 * A stream that takes no part in the step -- inactive, no frame, failed, or stopped in this step -- gets 128 zero bytes; on a step without
 * camera pruning upd[1] is zero.  The sums are formed in a fixed order: the same bytes at every launch shape and in every run.
 * av_msckf_batch_set_stats(b, enable): before the batch's first step (AV_E_INVALID afterwards).  Off, the step launches and reads back
 * exactly what it did without the feature; on, two per-stream kernels of the step are the instances that also write the blocks (no
 * launch more) and one more asynchronous copy brings them to a pinned buffer of the step's ring slot: no wait and no allocation inside a
 * step.
 * av_msckf_batch_next_stats(b, rec_host): hands over the destination -- n_streams records -- of the NEXT av_msckf_batch_step / _submit /
 * _submit_dev; it is filled when that step retires and must stay valid until then.  A queued step keeps its own destination.  Stream
 * groups each fill their own part.  AV_E_INVALID while the feature is off.  A step without a destination computes its records and drops them.
 * Known limits: sums only, no per-feature values; the gate's dof is the reference's; positions and rows are those of the device's
 * evaluation. */
#define AV_FILTER_STATS_BYTES 128
#define AV_FS_RAN 1
#define AV_FS_CUT 2
typedef struct av_update_stats {
    int32_t n_cand, n_pos, n_eval, n_pass, dof_eval, dof_pass, rows, flags;
    double gamma_eval, gamma_pass, dx_pos, dx_rot;
} av_update_stats;
typedef struct av_filter_stats { av_update_stats upd[2]; } av_filter_stats;
int  av_msckf_batch_set_stats(av_msckf_batch* b, int enable);
int  av_msckf_batch_next_stats(av_msckf_batch* b, av_filter_stats* rec_host);
/* IMU-rate odometry: the state after every IMU sample the step's prediction integrated, per stream and step, riding the step's read-back.
 * The published pose comes once per camera frame; these come at the rate of the IMU, for a control loop, for motion compensation of a
 * lidar or an event camera, for a comparison with a 200 Hz ground truth.  Off by default.  On, every step yields for every stream a count
 * pair n[s][2] = (had, written) and up to `cap` records av_imu_state of AV_IMU_STATE_BYTES = 112 bytes.  Record k describes the k-th IMU
 * sample the prediction of THIS step integrated for the stream -- the samples with imu_state.timestamp <= t <= frame time, in order
 * (batch_imu_processing, msckf.py:251-273):
 *   t        the sample's time stamp
 *   p, q, v  position, orientation (JPL xyzw) and velocity right after predict_new_state (msckf.py:341-388) for that sample: exactly the
 *            doubles the filter holds then, in the filter's own frame and conventions, the same as the published twelve
 *   w        the bias-corrected angular rate the sample was integrated with, gyro - gyro_bias, in the IMU frame
 * The records are PREDICTIONS from the previous step's updated state: no measurement update lies between them.  The correction of this
 * step's updates shows as the difference between the last record (the sample at or just before the frame time) and the step's
 * published pose; a consumer that wants a continuous trajectory splices records and published poses in time order.
 * Counts: had = samples integrated, written = min(had, cap).  On overflow the LAST cap samples are kept, in time order, so the record at
 * the frame's time always survives; records past `written` are unspecified.  A sample that repeats its predecessor's stamp (dt = 0)
 * still gets a record.  A stream with nothing to integrate in this step has n = {0, 0}: inactive, no frame, failed or stopped, its
 * window full, or before its gravity initialisation.  A stream that stops DURING a step (a capacity limit met by one of its updates)
 * still has that step's records: the prediction ran before the limit was met; from the next step on it reads {0, 0}.
 * av_msckf_batch_set_imu_rate(b, cap): cap records per stream and step, 0 = off, at most 4096 (AV_E_INVALID outside 0 .. 4096); before
 * the batch's first step (AV_E_INVALID afterwards).  Off, the step launches and reads back exactly what it did without the feature; on,
 * one small kernel behind the first kernel of the step gathers the records from what that kernel leaves for the covariance propagation
 * (one launch more; no kernel of the step changes) and two more asynchronous copies bring records and counts to pinned buffers of the
 * step's ring slot: no wait and no allocation inside a step.  The records are the same bytes at every launch shape of the step.  The
 * whole n_streams * cap * 112-byte buffer is copied whatever the counts are.
 * av_msckf_batch_next_imu_rate(b, rec, n): hands over the destination -- n_streams * cap records and n_streams * 2 counts -- of the NEXT
 * av_msckf_batch_step / _submit / _submit_dev; it is filled when that step retires and must stay valid until then.  A queued step keeps
 * its own destination.  Stream groups each fill their own part.  AV_E_INVALID while the feature is off.  A step without a destination
 * computes its records and drops them.
 * Known limits: no propagation past the frame time through samples the filter has not consumed yet ("pose now") and no covariance per
 * record here -- both are the "Forecast" below; no biases in the record; records arrive with the step's read-back, not earlier. */
#define AV_IMU_STATE_BYTES 112
typedef struct av_imu_state { double t, p[3], q[4], v[3], w[3]; } av_imu_state;
int  av_msckf_batch_set_imu_rate(av_msckf_batch* b, int cap);
int  av_msckf_batch_next_imu_rate(av_msckf_batch* b, av_imu_state* rec, int32_t* n);
/* Forecast: the pose a step leaves, carried forward to the newest IMU sample the caller has pushed, with its covariance ("pose now").
 * A step's published pose is the state at the camera frame's time; by the time it is read the vehicle has moved on by the front-end's
 * latency, the queue and the step.  The IMU samples of that interval are already in the stream's buffer -- pushed, not consumed, since a
 * step takes only samples with t <= frame time.  Off by default.  On, every step yields for every stream a count pair n[s][2] =
 * (had, written), up to `cap` records av_imu_state, and one covariance record cov[s][AV_ODOM_COV_DOUBLES].
 *   Pending samples  When a step is submitted for a stream with frame time t_f it takes its own samples first, exactly as without the
 *            feature; what the stream's buffer then holds has t > t_f: the pending samples, in push order, `had` of them.  The
 *            selection is made under the stream's lock in the same pass.  They are NOT removed: the next step consumes them as it always
 *            would.  The forecast integrates the first written = min(had, cap) of them -- the FIRST cap, not the last: the chain cannot skip
 *            samples, and pushing seconds of IMU ahead must not buy unbounded work per step.  had > written says "now" was not reached.
 *            (written can fall short of min(had, cap) only when samples arrive while the step is being staged, beyond the staging's slack.)
 *            "Submitted" is the moment the step's own samples are selected: inside the call for a batch of one stream group; for stream
 *            groups, by each group's worker when it launches the step -- inside av_msckf_batch_step, and for _submit / _submit_dev
 *            possibly a moment after the call returns, so samples pushed meanwhile count as pending.
 *   Start    the state and covariance the step leaves on the device, exactly what the next step's prediction starts from: after both
 *            updates and the camera removal; after online_reset on a reset step (the covariance then starts from the re-initialised
 *            block; the odometry-covariance record of that step does not); with the updated biases and the null states as the update
 *            left them.
 *   Per sample  the state by predict_new_state (msckf.py:341-388); the 21 x 21 IMU block of the covariance by process_model's formula
 *            (msckf.py:275-339), observability patches and symmetrisation included, with a private copy of the null states advanced as
 *            process_model advances them.  The camera blocks of P play no part: the IMU block depends on nothing else.
 *   Records  record k: the k-th pending sample's stamp t; p, q, v right after predict_new_state for it, in the filter's own frame;
 *            w = gyro - gyro_bias with the updated bias.  The first record's dt is t - imu_state.timestamp as the step left it; the
 *            forecast's reached time is the last written record's t.  Records past `written` are unspecified.
 *   cov      the odometry covariance, in the layout and error coordinates of "Odometry covariance": the same J, at q of the LAST WRITTEN
 *            record with R_ic and t_ci as the step leaves them, applied to the propagated block.  written = 0: that map of the state and
 *            block the step leaves.
 *   Read-only  The forecast writes nothing the filter reads: a run with it on is bit for bit the run with it off in every other output
 *            and in the final state.
 * A stream that does not publish in the step -- no frame, no gravity yet, stopped, stopped during this step -- reads n = {0, 0} and 120 NaNs.
 * av_msckf_batch_set_forecast(b, cap): cap records per stream and step, 0 = off, at most 4096 (AV_E_INVALID outside 0 .. 4096); before the
 * batch's first step (AV_E_INVALID afterwards).  Off, the step launches, uploads and reads back exactly what it did without the feature.
 * On: the pending samples ride in the upload of the step's own samples, one small upload addresses them; two kernels behind the step's last
 * one (the state chain a lane per stream, then covariance, records and counts one wavefront per stream at every launch shape; no kernel of
 * the step changes); three more asynchronous copies bring the arrays to pinned buffers of the step's ring slot.  No wait and no allocation
 * inside a step: the IMU staging is sized for n_streams * cap pending samples when it is first built.  The same bytes at every launch shape.
 * av_msckf_batch_next_forecast(b, rec, n, cov): hands over the destination -- n_streams * cap records, n_streams * 2 counts, n_streams *
 * AV_ODOM_COV_DOUBLES doubles -- of the NEXT av_msckf_batch_step / _submit / _submit_dev; filled when that step retires, valid until then.
 * A queued step keeps its own destination.  Stream groups each fill their own part.  AV_E_INVALID while the feature is off.  A step
 * without a destination computes its arrays and drops them.
 * Known limits: no forecast for a stream without a frame in the step; no call of its own outside a step; no biases in the record. */
int  av_msckf_batch_set_forecast(av_msckf_batch* b, int cap);
int  av_msckf_batch_next_forecast(av_msckf_batch* b, av_imu_state* rec, int32_t* n, double* cov);
/* Zero-velocity update: a stream that stands still has its velocity pinned to zero.  At rest the stereo features carry no temporal
 * parallax, so nothing in the filter observes the velocity and the accelerometer bias: both random-walk until the vehicle moves.  Off by
 * default; off, a step launches exactly what it launched without the feature.  On, every step runs two more kernels, one wavefront per
 * stream at every launch shape, with no wait, no allocation and no read-back inside the step.
 *   Detector  behind the prediction, ahead of the lost-feature update; read-only for the filter.
 *            IMU test   over the bias-corrected samples the step consumed (n_imu of them): w_max = max |gyro|, a_dev_max =
 *                       max | |acc| - |gravity| |.  imu_ok iff n_imu >= 1, w_max <= gyro_max and a_dev_max <= acc_dev_max.
 *            Vision test  over the entries of the frame the step appended: an entry is tracked if the previous frame observed its
 *                       feature, and still if (u0 - u0')^2 + (v0 - v0')^2 <= disparity_max^2 against that observation (cam0, normalised
 *                       coordinates).  vis_ok iff n_tracked >= min_tracks and 100 n_still >= still_percent n_tracked.  The first live
 *                       frame and the frame after an online reset have n_tracked = 0.
 *            DETECTED = imu_ok and vis_ok.  Both are needed: a gently flying vehicle passes the IMU test.
 *   Update   behind the step's last kernel, ahead of the forecast, for streams that are active, not stopped and DETECTED: the
 *            reference's measurement_update (msckf.py:548-602) with H selecting state columns 6..8, r = -v and velocity_sigma^2 in
 *            place of observation_noise.  S = P[6:9, 6:9] + sigma^2 I is inverted explicitly through its 3 x 3 Cholesky factor, S^-1 =
 *            L^-T L^-1; gamma = r^T S^-1 r.  gate > 0 and gamma > gate: AV_ZU_GATED, nothing is touched.  S not finite or not positive
 *            definite: AV_ZU_BAD, nothing is touched, the stream is NOT stopped.  Otherwise delta_x = P[:, 6:9] S^-1 r is injected as
 *            every update's is (null-state aliasing included), P[i][j] -= c_i^T S^-1 c_j is computed for i <= j and mirrored -- P stays
 *            bit-symmetric, nothing outside the n x n block is touched --, AV_ZU_APPLIED is set.
 *   One-step lag  The update acts on the state the step LEAVES.  The 12 published doubles of the step (and its odometry covariance,
 *            landmarks, statistics, IMU-rate records) are NOT rewritten: the pose of step k is the pre-update one.  av_msckf_batch_get_state,
 *            av_msckf_batch_get_cov, the forecast of step k and everything in step k + 1 see the corrected state.  In the reference's
 *            terms: feature_callback(msg), then the update.  No existing kernel of the step changes.
 *   Record   av_zupt, one per stream, in ONE device array that every step overwrites; it is NOT delivered with the step's read-back but
 *            read on demand.  flags, n_imu, n_tracked, n_still, w_max, a_dev_max are the detector's; v_norm (|v| before the update),
 *            gamma and dx_pos (|delta_x[12:15]|) the update's, 0 where it did not run.  detected_total / applied_total count over the
 *            stream's life, so a consumer that polls misses nothing.  A stream that takes no part in a step, or that stopped in it,
 *            reads a zero record for the step; its totals stay.  av_msckf_batch_restart clears the record and the totals.
 * av_msckf_batch_set_zupt(b, p): p = NULL switches the update off.  Before the batch's first step only (AV_E_INVALID afterwards).
 * AV_E_INVALID unless gyro_max, acc_dev_max, disparity_max >= 0, velocity_sigma > 0, gate >= 0 (0 = no gate), all finite, min_tracks >= 0
 * and 0 <= still_percent <= 100.
 * av_msckf_batch_read_zupt(b, out): drains the queue, like av_msckf_batch_launch_shape, then copies n_streams records.  Off, or before the
 * first step: zeros.
 * Known limits: the thresholds' defaults (config.py) are starting values against the synthetic sensors, not tuned on flight data; no caller
 * override ("landed, disarmed"); no zero-rotation or position-hold measurement; a moving scene in front of a resting camera vetoes the
 * update; constant-velocity flight over a scene with fewer than min_tracks tracks is never declared still. */
#define AV_ZUPT_BYTES 64
enum { AV_ZU_IMU_OK = 1, AV_ZU_VIS_OK = 2, AV_ZU_DETECTED = 4, AV_ZU_APPLIED = 8, AV_ZU_GATED = 16, AV_ZU_BAD = 32 };
typedef struct av_zupt {
    int32_t flags, n_imu, n_tracked, n_still, detected_total, applied_total;
    double w_max, a_dev_max, v_norm, gamma, dx_pos;
} av_zupt;
typedef struct av_zupt_params {
    double gyro_max, acc_dev_max, disparity_max, velocity_sigma, gate;      /* rad/s, m/s^2, normalised image units, m/s, chi^2 (0: none) */
    int32_t min_tracks, still_percent;
} av_zupt_params;
int  av_msckf_batch_set_zupt(av_msckf_batch* b, const av_zupt_params* p);
int  av_msckf_batch_read_zupt(av_msckf_batch* b, av_zupt* out);
int  av_msckf_batch_sizes(av_msckf_batch* b, int stream_idx, int32_t out3[3]);     /* [state dim, camera states, map features] */
/* Full host-side state of one stream -- every target of measurement_update's injection (msckf.py:568-595), for parity tests
 * (SURVEY 8b get_state): imu32 = [imu_state.timestamp, orientation q(4, JPL xyzw), position(3), velocity(3), gyro_bias(3),
 * acc_bias(3), R_imu_cam0 (9, row-major), t_cam0_imu(3), IMUState.gravity(3)]; the camera states of the window in
 * state_server.cam_states order: cam_ids[k] and cam_qp7[7k..] = orientation(4), position(3).  *n_cam = their number;
 * cam_cap = 0 only asks for imu32 and the count.  Drain (wait 0) first. */
int  av_msckf_batch_get_state(av_msckf_batch* b, int stream_idx, double imu32[32], int64_t* cam_ids, double* cam_qp7, int cam_cap, int32_t* n_cam);
/* A failure that concerns ONE stream (its camera window or the block list of one of its updates outgrew a fixed capacity)
 * stops that stream only: from then on (until av_msckf_batch_restart) it idles and its out[s*12] reads -1; the other streams of the batch keep stepping
 * (the reference's sequences are separate processes, run.bat:4-12).  *status = 0 while the stream runs, else the
 * AV_E_* code that stopped it, with the reason in msg.  Configuration errors (rows_cap vs cap, LDS limits) and HIP errors
 * concern the whole batch and are returned by the step / wait as before. */
int  av_msckf_batch_stream_status(av_msckf_batch* b, int stream_idx, int32_t* status, char* msg, int msg_cap);
/* Stream restart: one stream back to "as created" while its neighbours keep stepping.  After a restart of stream s, s is bit for bit a
 * stream of a freshly created batch / engine that is fed the same inputs from then on, and every other stream is bit for bit what it would
 * have been without the call.  Nothing is allocated or freed.  Use it when out[s*12] reads -1 (the stream stopped), when a sequence has
 * ended and its slot is to take the next one, or when a consumer judges from the published covariance or statistics that a stream has
 * diverged.  A vehicle has a stream in the engine and one in the filter: restart both.
 * av_msckf_batch_restart(b, stream_idx, n): n stream indices of the batch (of the whole batch, whatever its stream groups).  Legal at any
 * time: before the first step (host state only: there is no device state yet) and with steps queued -- it then drains the queue first,
 * like av_msckf_batch_launch_shape; the queued steps retire as steps of the old life and their outputs are delivered.  n = 0 is a
 * no-op, an index listed twice counts once, an index out of range is AV_E_INVALID with nothing touched.  Returns when the device state
 * is reset.
 *   Reset, host:   the IMU buffer is EMPTIED -- samples pushed before the call belong to the old life, and the stream goes live again
 *                  only after initialize_gravity_and_bias has seen 200 new samples (msckf.py:230-249); the gravity / first-image /
 *                  initialisation-sent flags, the camera-state id counter, state and extrinsics (the batch's create-time values);
 *                  the failure code and text (av_msckf_batch_stream_status reads 0, ""); the parity-test tap's captures.
 *   Reset, device: the IMU state record, state dimension 21, no camera states, the stream's whole covariance region (create-time
 *                  diagonal, zero elsewhere), the observation store (empty, insertion counter 0, header clear, arrays as allocated), the
 *                  stream's rows of the pose, odometry-covariance, landmark, statistics, IMU-rate and forecast buffers, its zero-velocity record and
 *                  totals.  Camera-state ids and the map's
 *                  insertion order begin again at 0.
 *   Not reset:     av_msckf_batch_counters and av_msckf_batch_work keep accumulating over all lives; the batch's configuration, its
 *                  output switches and capacities; every other stream.
 * av_frontend_restart(fe, stream_idx, n, stream): the same for streams of a front-end engine.  The host state is reset at once (it is
 * consumed inside the step calls); the device state by a small kernel on `stream`, behind what is enqueued there and ahead of the next
 * step.  Legal between av_frontend_prestage and the step (prestaged pyramids are of images, not of stream state), with a feature
 * read-back pending (it still delivers the old life's features), on every entry path and with the frame store.
 *   Reset:         the stream's IMU buffer, previous time stamp, first-frame flag and frame number (AV_FE_RANSAC's draws hash it); its
 *                  previous entry of the frame store; on the device first-frame flag, id counter (feature ids begin again at 0), both
 *                  grids' counts, the counters of av_frontend_read_counters and av_frontend_read_ransac_counts.
 *   Not reset:     masks, photometric tables, exposure factors, range settings and records, the frame store's frames and everything else
 *                  that belongs to the engine and not to the stream; the message of the last step (av_frontend_features_dev) until the
 *                  next step replaces it.
 * Ids repeat across lives: a consumer that keys on feature or camera-state ids keeps a generation count per stream (the Python classes
 * do: `generation`).  Known limits: the filter's restart drains the queue; no save or restore of a stream's state. */
int  av_msckf_batch_restart(av_msckf_batch* b, const int32_t* stream_idx, int n);
int  av_frontend_restart(av_frontend* fe, const int32_t* stream_idx, int n, void* stream);
/* Run statistics over all streams (drain first): [steps, stream-steps that ran prune_cam_state_buffer (msckf.py:712-786),
 * stream-steps whose lost-feature candidates outgrew rows_cap (rows taken from the shared overflow pool), device-buffer
 * reallocations after the first step (0 in a correctly pre-sized run), min camera states, max camera states,
 * min map features, max map features].  bench.py uses it to prove that the timed region is the steady state. */
int  av_msckf_batch_counters(av_msckf_batch* b, int64_t out8[8]);
/* What the batch really launched (no reference counterpart; drains the queue first): out17[0] = number of stream groups (a batch
 * without sub-batches reports 1; at most 8), and for group g out17[1 + 2g] = its stream count, out17[2 + 2g] = the workgroup size the
 * per-stream filter kernels (dk_begin4 / dk_cov / dk_mid / dk_finish) were launched with in the group's LAST enqueued step: 64 (one
 * wavefront per stream) or 256 (four); 0 before the group's first step.  The value is recorded at
 * the launch, not recomputed here.  The rule it reports is per GROUP, not per batch: a batch of n_streams >= 1,024 is
 * split into 2 groups of ceil(n_streams / 2) streams (the last one holds the remainder; AV_MSCKF_GROUPS overrides the count), and
 * each group takes 64 when ITS stream count is >= 1,024, else 256 (AV_DK_WG=64|256 forces one for all groups).  So 1,023 streams run as
 * [(1023, 256)], 1,024 as [(512, 256), (512, 256)], 2,047 as [(1024, 64), (1023, 256)], and only from 2,048 streams up --
 * [(1024, 64), (1024, 64)] -- is a batch "two groups, one wavefront per stream" throughout. */
int  av_msckf_batch_launch_shape(av_msckf_batch* b, int32_t out17[17]);
/* Parity-test tap (SURVEY 8b "get_state / get_cov for parity tests"): the values the reference computes inside gating_test and
 * measurement_update (msckf.py:604-612, 548-602) but never returns.  After av_msckf_batch_debug_capture(b, 1) every stream keeps
 * them for the two update phases of its LAST step: phase 0 = remove_lost_features, 1 = prune_cam_state_buffer.  debug_read:
 * gamma[*n_gamma] in the reference's evaluation order (features behind the > 1500-row cut are not evaluated, msckf.py:667-668);
 * *rows = stacked rows of the phase's update (0: no update ran, dx / P_after untouched); dx[*n_state]; P_after[*n_state ** 2]
 * = state_cov right after the update (before the pruning phase removes its two camera states).  P_after rows have pitch
 * *n_state; n_cap = capacity of dx (n_cap doubles) and P_after (n_cap * n_cap).  Synchronous copies per step: tests only. */
int  av_msckf_batch_debug_capture(av_msckf_batch* b, int enable);
int  av_msckf_batch_debug_read(av_msckf_batch* b, int stream_idx, int phase, double* gamma, int gamma_cap, int32_t* n_gamma,
                               double* dx, double* P_after, int n_cap, int32_t* n_state, int32_t* rows);
/* Parity-test entry (tests only; no step of the filter calls it): the per-feature kernels in the launch shapes of the device-resident
 * filter, on the caller's device arrays.  Feature.initialize_position for the features tri_list_dev[0 .. *n_tri_dev) (triangulation
 * kernel in list form, one wavefront per workgroup; NULL list: skipped, pos_dev / valid_dev are then inputs), then feature_jacobian +
 * gating_test for feat_list_dev[0 .. *n_feat_dev) (NULL list: skipped) the way the filter's update phases launch them: both counts are
 * read ON THE DEVICE, both kernels stride over their lists with a grid sized for `teams` features in flight (teams of 8 lanes -- max_obs
 * <= 2 -- come eight to a workgroup, longer tracks one team per workgroup; the triangulation gets `teams` workgroups), a feature with
 * valid_dev[f] = 0 is not evaluated and reads gamma = 0, pass = 0.  Feature f belongs to stream f / fs_stride of n_streams: its cameras
 * are cam_*[stream * cam_stride + obs_cam], its covariance P_dev + stream * p_stride (row-major, leading dimension ld >= 21 + 6 *
 * cam_stride), its gravity gravity_dev[3 * stream ..], its rows H_dev + stream * h_stride / r_dev + stream * r_stride, first row
 * row_off_dev[f] (< 0: gate only).  compact = 0: rows of ld doubles (zero_fill = 1 clears them first, 0 writes only the feature's own
 * camera columns); compact = c >= 6 * max_obs: rows of c doubles that hold ONLY the feature's own camera columns in observation order
 * (zero_fill must be 0).  max_obs <= 2 evaluates two-observation features only (others read pass = 0); max_obs <= 32, else
 * AV_E_CAPACITY before any launch.  The other arguments are those of av_msckf_triangulate / av_msckf_feature_blocks; ctx lends its
 * chi^2 table and its device.  Nothing is synchronised. */
int  av_msckf_feature_ops_dev(av_msckf* ctx, int n_streams, int fs_stride, int cam_stride, int max_obs, int compact, int zero_fill, int teams,
                              const int32_t* tri_list_dev, const int32_t* n_tri_dev, const int32_t* feat_list_dev, const int32_t* n_feat_dev,
                              const int32_t* obs_off_dev, const int32_t* obs_cam_dev, const double* obs_z_dev, const int32_t* dof_dev, const int32_t* row_off_dev,
                              const double* cam_q_dev, const double* cam_p_dev, const double* cam_qn_dev, const double* cam_pn_dev,
                              const double* P_dev, int ld, int64_t p_stride, const double* gravity_dev,
                              const double* T_cam0_cam1_rowmajor44, const double* opt5, double obs_noise,
                              double* pos_dev, int32_t* valid_dev, double* H_dev, int64_t h_stride, double* r_dev, int64_t r_stride,
                              double* gamma_dev, int32_t* pass_dev, void* stream);
/* Parity-test entry (tests only; no step of the filter calls it): the prediction of the device-resident filter -- batch_imu_processing
 * with predict_new_state and process_model, then state_augmentation (msckf.py:251-423) -- for n_streams streams in ONE launch sequence,
 * exactly the one a filter step begins with: the state kernel (a lane per stream), then the covariance kernel with wg = 64 (one
 * wavefront per stream) or 256 threads per stream, through the helper the step itself launches them with.  The streams are described by
 * flat HOST arrays, per stream:
 *   state_io[43]     ts, q[4], p[3], v[3], bg[3], ba[3], R_imu_cam0[9], t_cam0_imu[3], q_null[4], p_null[3], v_null[3], gravity[3],
 *                    tracking_rate (read and written back)
 *   state_int_io[6]  n_state, n_cam, failed, null_aliased, first_img (read and written back), active (written)
 *   t_frame[1]       the frame's time stamp
 *   ctl[6]           active, first IMU sample, number of IMU samples, ops, rm0, rm1
 *   imu[n_imu][7]    t, gyro[3], acc[3] per sample (raw: the biases are the state's)
 * and by DEVICE arrays the kernels work on in place: camera states cam_q / cam_p / cam_qn at [stream * cam_stride + k], covariances at
 * P_dev + stream * p_stride, row-major with leading dimension ld.  A stream with active = 0 or failed != 0 is left alone; one whose window
 * is full (n_cam == cam_stride) comes back with failed = 1 (no room for the new camera state) and nothing else of it touched.
 * ops (applied after the prediction, to the window as it then stands, through a probe kernel only this entry launches): bit 0 =
 * find_redundant_cam_states (msckf.py:678-709) with the state's tracking_rate -> redundant_out[2] (window positions, ascending; -1 where
 * not asked for); bit 1 = removal of the camera states at window positions rm0 < rm1 from the covariance (msckf.py:774-786), both in one
 * pass, at wg threads.  Checked before anything is launched (AV_E_INVALID, or AV_E_CAPACITY for n_cam > cam_stride): wg, the counts,
 * ld >= 21 + 6 * cam_stride, p_stride >= ld * ld, n_state == 21 + 6 * n_cam, samples inside imu[], four camera states for the redundancy
 * rule, removal positions ascending and inside the window.  noise4 = continuous variances [gyro, gyro_bias, acc, acc_bias]; ctx lends
 * its device.  Synchronises. */
int  av_msckf_predict_ops_dev(av_msckf* ctx, int n_streams, int wg, int cam_stride, int ld, int64_t p_stride,
                              double* state_io, int32_t* state_int_io, const double* t_frame, const int32_t* ctl,
                              const double* imu, int n_imu, const double noise4[4],
                              double* cam_q_dev, double* cam_p_dev, double* cam_qn_dev, double* P_dev,
                              int32_t* redundant_out, void* stream);
/* The same entry with the IMU-rate odometry on (tests only): the launch sequence is then the one a step begins with when
 * av_msckf_batch_set_imu_rate is on, the record kernel behind the state kernel.  cap = 1 .. 4096 records per stream; rec_out[n_streams][cap] and n_out[n_streams][2] are HOST
 * arrays, uploaded as the caller filled them (a pre-fill shows what the kernel did not write) and read back.  Everything else, and
 * every result the two entries share, is as above. */
int  av_msckf_predict_ops_dev_rate(av_msckf* ctx, int n_streams, int wg, int cam_stride, int ld, int64_t p_stride,
                                   double* state_io, int32_t* state_int_io, const double* t_frame, const int32_t* ctl,
                                   const double* imu, int n_imu, const double noise4[4],
                                   double* cam_q_dev, double* cam_p_dev, double* cam_qn_dev, double* P_dev,
                                   int32_t* redundant_out, void* stream, int cap, av_imu_state* rec_out, int32_t* n_out);
/* The forecast's two kernels (tests only; "Forecast"), launched through the helper a step launches them through.  Streams are described by
 * the flat host arrays of av_msckf_predict_ops_dev, state_io[43] and state_int_io[6]; `active` is an INPUT here: the arrays hold the state
 * a step LEAVES.  P_dev: the device covariances [n_streams][p_stride], leading dimension ld.  imu[n_imu][7]; pend[n_streams][2] = (first,
 * count) of every stream's pending samples in it.  cap = 1 .. 4096.  rec_out[n_streams][cap], n_out[n_streams][2] and
 * cov_out[n_streams][AV_ODOM_COV_DOUBLES] are HOST arrays, uploaded as the caller filled them (a pre-fill shows what the kernels did not
 * write) and read back; state_io and state_int_io come back as the kernels left them: unchanged.  Synchronises. */
int  av_msckf_forecast_ops_dev(av_msckf* ctx, int n_streams, int ld, int64_t p_stride, double* state_io, int32_t* state_int_io,
                               const double* imu, int n_imu, const int32_t* pend, const double noise4[4], double* P_dev, void* stream,
                               int cap, av_imu_state* rec_out, int32_t* n_out, double* cov_out);
/* The zero-velocity update's kernel (tests only; "Zero-velocity update"), launched through the helper a step launches it through.  Streams
 * are described by the flat host arrays of av_msckf_predict_ops_dev, state_io[43] and state_int_io[6]; `active` is an INPUT here: the
 * arrays hold the state a step LEAVES, and come back as the kernel left them.  cam_q_dev / cam_p_dev: the device camera states
 * [n_streams][cam_stride][4 | 3], P_dev: the device covariances [n_streams][p_stride], leading dimension ld, all updated in place.
 * rec_io[n_streams]: HOST records, uploaded as the caller filled them -- flags carries the detector's verdict, AV_ZU_DETECTED, per stream;
 * the totals count on from what they hold -- and read back.  Checked before anything is launched: n == 21 + 6 n_cam <= ld, n_cam <=
 * cam_stride <= 64, p_stride >= ld * ld, the parameters as av_msckf_batch_set_zupt checks them.  Synchronises. */
int  av_msckf_zupt_ops_dev(av_msckf* ctx, int n_streams, int cam_stride, int ld, int64_t p_stride, double* state_io, int32_t* state_int_io,
                           double* cam_q_dev, double* cam_p_dev, double* P_dev, const av_zupt_params* params, av_zupt* rec_io, void* stream);
/* Parity-test entry (tests only; no step of the filter calls it): the batched measurement update (msckf.py:548-602 with the stacking
 * loops of :658-668 and :759-763) for n_streams streams in ONE launch sequence, exactly the one a phase of a filter step runs from the
 * stacking decisions to the covariance update, through the helper the step itself launches it with.  phase 0 = the lost-feature phase
 * (the `> 1500 rows` cut, Cholesky back end for every stream, streams that stack more than kch rows compressed through their Gram
 * matrix first; kch = 0 means the filter's own, min(136, ld)), phase 1 = the pruning phase (no cut, information form for the streams that touch at
 * most 24 columns; hld > 0: the block rows are compact, hld doubles each, and no Cholesky back end is launched, as in a step).
 * HOST arrays, per stream s: stream_n (state dimension), stream_mode (1 = information form allowed, 2 = stopped: no update), n_cand;
 * per candidate slot i in [s * fs_stride, s * fs_stride + n_cand[s]): obs_off[i] .. obs_off[i + 1] (n_streams * fs_stride + 1 entries)
 * index obs_cam[n_obs] (the camera slot of every observation), pass[i] the gate flag, row_off[i] the first of its 4 M - 3 rows in the
 * stream's region of the DEVICE block buffers: H_dev + s * h_stride (rows of hld > 0 ? hld : ld doubles) and r_dev + s * r_stride,
 * rows_cap rows each.  P_dev: the device covariances, updated in place at P_dev + s * p_stride with leading dimension ld.  The work
 * buffers are sized as the batched filter sizes them and released before the call returns.  Results, HOST arrays: dx_io[n_streams][ld]
 * (uploaded as the caller filled it: a pre-fill shows what was not written), stacked_out[n_streams] (rows stacked, 0 = no update, -1 =
 * stopped or more than 4096 blocks, -2 = a factorisation met a pivot that is not positive and finite: the update was a no-op),
 * cols_out[n_streams][6 * cam_stride] (the touched state columns, ascending, -1 behind them) and rec_out[n_streams][5] = m, nc, mode
 * (1 = information form), kdir (> 0: rows kept without compression), n_blk as the stacking kernel wrote them.  Checked before anything
 * is launched (AV_E_INVALID / AV_E_CAPACITY), so that no input can send a kernel out of bounds: the counts, n <= ld, n == 21 + 6 n_cam,
 * camera slots inside the stream's window (cam_stride <= 64), at most fs_stride candidates, observations inside obs_cam, stacked rows
 * inside the block buffer and m <= rows_cap, at most 256 touched columns, at most 144 and at most ld rows kept by one pass, hld either
 * 0 or >= the columns of every stream (and every updating stream then in information form), the information form's LDS <= 160 KB.
 * ctx lends its device.  Synchronises. */
int  av_msckf_update_ops_dev(av_msckf* ctx, int n_streams, int phase, int kch, int fs_stride, int cam_stride, int hld,
                             const int32_t* stream_n, const int32_t* stream_mode, const int32_t* n_cand,
                             const int32_t* obs_off, const int32_t* obs_cam, int n_obs, const int32_t* pass, const int32_t* row_off,
                             const double* H_dev, int64_t h_stride, const double* r_dev, int64_t r_stride, int rows_cap,
                             double* P_dev, int ld, int64_t p_stride, double obs_noise,
                             double* dx_io, int32_t* stacked_out, int32_t* cols_out, int32_t* rec_out, void* stream);
/* Work done so far, for the filter stage's roofline (drain first): out8 = [algorithmic fp64 flops of the gating tests
 * (per feature with r = 4M-3 rows, n columns: 2rn^2 + 2r^2n + r^3/3; msckf.py:604-612), of the measurement updates on the
 * k = min(m, n) rows kept (S 2kn^2 + 2k^2n, Cholesky k^3/3, solve 2k^2n, (I-KH)P 4kn^2; msckf.py:562-602), of the reference's
 * thin QR by the survey's formula (2mn^2 - 2/3 n^3 when m > n, msckf.py:554-557 -- reported apart: the column-compressed update
 * never runs a QR of that size), features gated, updates run, rows stacked, milliseconds the phase chains (triangulation ..
 * covariance update) spent on the device summed over stream groups, 0].  The time needs enable = 1 on an earlier call (two HIP
 * events per phase and group); enable = 0 switches it off, enable < 0 only reads. */
int  av_msckf_batch_work(av_msckf_batch* b, int enable, double out8[8]);
/* The same two stages counted as the kernels EXECUTE them (drain first; zeros before the first step): out2 = [fp64 flops of
 * the gating tests on the block-sparse shapes -- H_x as 4 x 6 blocks, the gate matrix from the M^2 6 x 6 blocks of P, reflectors applied
 * to it from both sides: ~0.6 MFLOP for a 21-observation track where the dense formula above says 5.5 --, fp64 flops of the updates
 * over the touched columns -- Gram compression m (nc+1)^2 + (nc+1)^3/3 where a stream stacks more rows than one pass, T^T 2 n nc k,
 * S k^2 nc, Cholesky k^3/3, substitution k^2 (n+1), P - Y^T Y n^2 k; information form m nc^2 + 4 nc^3 + 2 n nc^2 + 2 n^2 nc].
 * Analytic per gated feature / per update (upd_stack_kernel), tile padding not counted.  No reference counterpart: bench.py's
 * roofline_msckf.executed. */
int  av_msckf_batch_work_executed(av_msckf_batch* b, double out2[2]);
/* Lifecycle-test entry (tests only; needs no GPU): what the objects of this process hold at this moment, out4 = [bytes of device memory,
 * bytes of pinned host memory, events, streams].  Every acquisition and release of the library passes through these counts (the
 * process-lifetime diagnostics behind AV_LK_PROF / AV_DEV_FPROF / AV_DEV_UPROF excepted): all four are zero once every object is destroyed. */
int  av_debug_live_resources(int64_t out4[4]);

/* Measurement hooks (bench.py's roofline leg; no reference counterpart): when enabled, every
 * launch group of av_frontend_step is bracketed by a HIP event pair ON THE STEP'S STREAM.
 * max_spans = capacity in event pairs (0 disables).  av_frontend_read_timing synchronises the
 * device and returns, per kernel class [0 pyramid, 1 LK, 2 FAST, 3 glue], the summed elapsed
 * milliseconds and the number of launch groups measured since the last read. */
int av_frontend_enable_timing(av_frontend* fe, int max_spans);
int av_frontend_read_timing(av_frontend* fe, double ms_out[4], int32_t spans_out[4]);

#ifdef __cplusplus
}
#endif
#endif /* AIRVISION_H */
