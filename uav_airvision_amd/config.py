"""Configuration bag for the hot path.

Mirrors the attribute surface of the reference's ``ConfigEuRoC`` / ``OptimizationConfigEuRoC``
(reference: src/config.py:7-17, 19-123) so that objects of either class can be handed to
``ImageProcessor(config)`` / ``MSCKF(config)``.  The reference module imports ``cv2`` only for
three integer constants (config.py:41,44); they are spelled out here so no OpenCV is needed.
"""
import numpy as np

# cv2 constants used by config.py:37-44
TERM_CRITERIA_COUNT = 1
TERM_CRITERIA_EPS = 2
OPTFLOW_USE_INITIAL_FLOW = 4


class OptimizationConfigEuRoC(object):
    """LM triangulation knobs (reference: src/config.py:7-17)."""

    def __init__(self):
        self.translation_threshold = -1.0
        self.huber_epsilon = 0.01
        self.estimation_precision = 5e-7
        self.initial_damping = 1e-3
        self.outer_loop_max_iteration = 5
        self.inner_loop_max_iteration = 5


class ConfigEuRoC(object):
    """EuRoC calibration + tunables (reference: src/config.py:19-123)."""

    def __init__(self, grid_row=4, grid_col=5, grid_min_feature_num=3, grid_max_feature_num=5):
        self.optimization_config = OptimizationConfigEuRoC()

        # front-end (config.py:23-35)
        self.grid_row = grid_row
        self.grid_col = grid_col
        self.grid_num = self.grid_row * self.grid_col
        self.grid_min_feature_num = grid_min_feature_num
        self.grid_max_feature_num = grid_max_feature_num
        self.fast_threshold = 15
        self.ransac_threshold = 3      # pixels; the reference stores it and never reads it; read here when use_ransac is set
        # two-point RANSAC on the tracked features (no counterpart in the reference: feature_tracker.py:135-136 is the empty step).
        # Off by default: with it off the front-end is the reference's, bit for bit.
        self.use_ransac = False
        self.ransac_success_probability = 0.99
        self.ransac_seed = 0
        # contrast-limited adaptive histogram equalisation of every frame ahead of the pyramids, LK and FAST (no counterpart in the
        # reference; av_clahe in include/airvision.h).  Off by default: with it off the front-end is the reference's, bit for bit.
        # fast_threshold and the LK thresholds are not retuned for equalised images.
        self.use_clahe = False
        self.clahe_clip_limit = 2.0
        self.clahe_tiles = (8, 8)       # (tiles_x, tiles_y)
        # pixel format of the camera frames handed to the front-end (no counterpart in the reference, which assumes 8-bit grey):
        # 'gray8' | 'gray16' | 'rgb8' | 'bgr8' | 'rgba8' | 'bgra8' | 'bayer_{rggb,bggr,grbg,gbrg}{8,16}' (a raw Bayer mosaic, named by the
        # colours of its top-left 2 x 2 block; gray16_shift applies to the 16-bit ones).  Anything but 'gray8' is converted to 8-bit grey on the GPU ahead of
        # everything else (av_to_gray8 in include/airvision.h).  gray16_shift: a 16-bit sample v becomes min(255, v >> shift); 8 = the
        # high byte, a sensor with 10 / 12 / 14 significant bits uses 2 / 4 / 6.
        # Packed 10 / 12-bit transports, unpacked on the GPU: 'gray10p' | 'gray12p' (PFNC Mono10p / Mono12p) | 'gray10_csi2' | 'gray12_csi2'
        # (MIPI CSI-2 RAW10 / RAW12) and 'bayer_{rggb,bggr,grbg,gbrg}{10p,12p,10_csi2,12_csi2}'.  Frames are uint8 [n, h, w * d / 8] (rows
        # tightly packed, the width whole groups: a multiple of 4 at 10 bits, of 2 at 12).  A sample is left-justified to 16 bits before
        # gray16_shift applies, so the default 8 gives its top eight bits.  No line stride, no Mono12Packed, no PNG or sweep source.
        self.image_format = 'gray8'
        self.gray16_shift = 8
        # 2 x 2 / 4 x 4 binning of every (grey) frame on the GPU ahead of CLAHE and the pyramids (no counterpart in the reference;
        # av_downscale in include/airvision.h): 1 = off, 2 or 4.  cam*_resolution and cam*_intrinsics stay those of the full-size camera;
        # the engine works on the binned image with the calibration of frontend.downscaled_config.  The thresholds below, the grid
        # and patch_size apply to the binned image as they stand.
        self.image_downscale = 1
        # static masks of the two cameras, for every stream of an engine (no counterpart in the reference; "Static masks" in
        # include/airvision.h): what is never scene -- the corners outside a fisheye's image circle, airframe in view.  None, a uint8 /
        # bool array of shape (height, width) of cam*_resolution with non-zero = scene, or the path of an 8-bit grey PNG of that size
        # (frontend.circle_mask builds the circle).  None: the front-end is the reference's, bit for bit.
        self.cam0_mask = None
        self.cam1_mask = None
        # photometric calibration of the two cameras, for every stream of an engine (no counterpart in the reference; "Photometric
        # calibration" in include/airvision.h; the TUM mono-VO convention): cam*_response = the inverse response G^-1, 256 floats in
        # [0, 255] or the path of a pcalib.txt-style text file of 256 numbers; cam*_vignette = V(x), a float array of shape (height, width)
        # of cam*_resolution with values in (0, 1] or the path of a 16-bit grey PNG of that size (normalised by its maximum).  Every grey
        # pixel becomes G^-1(p) / V(x) on the GPU, after the conversion to grey and ahead of binning and CLAHE
        # (frontend.photometric_tables quantises the tables).  All four None: the front-end is the reference's, bit for bit.
        self.cam0_response = None
        self.cam1_response = None
        self.cam0_vignette = None
        self.cam1_vignette = None
        # exposure-time normalisation between frames (no counterpart in the reference; "Exposure-time normalisation" in
        # include/airvision.h): the reference exposure time t_ref, a float in the unit of the exposures the entry points are then
        # handed with every frame (FrontendEngine.step(..., exposure=(e0, e1)); the drop-in reads `exposure` off the image messages).
        # Every frame is scaled by t_ref / t inside the photometric stage.  None: off, and the front-end is the reference's, bit for bit.
        self.exposure_reference = None
        # scaling of 16-bit grey samples (image_format 'gray16' only; no counterpart in the reference; "Range scaling of 16-bit grey" in
        # include/airvision.h): 'shift' = min(255, v >> gray16_shift), 'window' = gray16_window = (lo, hi) mapped to 0 .. 255 for every
        # image, 'auto' = a range per stereo pair from the pair's own histogram on the GPU: gray16_auto_clip = the parts per million of
        # samples that may saturate at the low / high end, gray16_auto_min_span = the smallest hi - lo (16 .. 65535; 256 keeps one count
        # at most one grey level).  A thermal core or a low-light camera whose signal does not fill its container wants 'auto'.
        self.gray16_scale = 'shift'
        self.gray16_window = None
        self.gray16_auto_clip = (100, 100)
        self.gray16_auto_min_span = 256
        self.stereo_threshold = 5
        self.max_iteration = 30
        self.track_precision = 0.01
        self.pyramid_levels = 3
        self.patch_size = 15
        self.win_size = (self.patch_size, self.patch_size)
        self.lk_params = dict(
            winSize=self.win_size,
            maxLevel=self.pyramid_levels,
            criteria=(TERM_CRITERIA_EPS | TERM_CRITERIA_COUNT, self.max_iteration, self.track_precision),
            flags=OPTFLOW_USE_INITIAL_FLOW)

        # filter (config.py:47-88)
        self.gravity_acc = 9.81
        self.gravity = np.array([0.0, 0.0, -self.gravity_acc])
        self.frame_rate = 20
        self.max_cam_state_size = 20
        self.position_std_threshold = 2.0
        self.rotation_threshold = 0.15
        self.translation_threshold = 0.2
        self.tracking_rate_threshold = 0.5
        self.gyro_noise = 0.005 ** 2
        self.acc_noise = 0.05 ** 2
        self.gyro_bias_noise = 0.001 ** 2
        self.acc_bias_noise = 0.01 ** 2
        self.observation_noise = 0.035 ** 2
        self.velocity = np.zeros(3)
        self.velocity_cov = 0.25
        self.gyro_bias_cov = 0.01
        self.acc_bias_cov = 0.01
        self.extrinsic_rotation_cov = 3.0462e-4
        self.extrinsic_translation_cov = 2.5e-5

        # calibration (config.py:93-123)
        self.T_imu_cam0 = np.array([
            [0.014865542981794, 0.999557249008346, -0.025774436697440, 0.065222909535531],
            [-0.999880929698575, 0.014967213324719, 0.003756188357967, -0.020706385492719],
            [0.004140296794224, 0.025715529947966, 0.999660727177902, -0.008054602460030],
            [0, 0, 0, 1.000000000000000]])
        self.cam0_camera_model = 'pinhole'
        self.cam0_distortion_model = 'radtan'
        self.cam0_distortion_coeffs = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05])
        self.cam0_intrinsics = np.array([458.654, 457.296, 367.215, 248.375])
        self.cam0_resolution = np.array([752, 480])

        self.T_imu_cam1 = np.array([
            [0.012555267089103, 0.999598781151433, -0.025389800891747, -0.044901980682509],
            [-0.999755099723116, 0.013011905181504, 0.017900583825251, -0.020569771258915],
            [0.018223771455443, 0.025158836311552, 0.999517347077547, -0.008638135126028],
            [0, 0, 0, 1.000000000000000]])
        self.T_cn_cnm1 = np.array([
            [0.999997256477881, 0.002312067192424, 0.000376008102415, -0.110073808127187],
            [-0.002317135723281, 0.999898048506644, 0.014089835846648, 0.000399121547014],
            [-0.000343393120525, -0.014090668452714, 0.999900662637729, -0.000853702503357],
            [0, 0, 0, 1.000000000000000]])
        self.cam1_camera_model = 'pinhole'
        self.cam1_distortion_model = 'radtan'
        self.cam1_distortion_coeffs = np.array([-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05])
        self.cam1_intrinsics = np.array([457.587, 456.134, 379.999, 255.238])
        self.cam1_resolution = np.array([752, 480])

        self.T_imu_body = np.identity(4)

        # no reference counterpart: the drop-in MSCKF keeps the 15 x 15 odometry covariance of its last published result in
        # `last_covariance` (needs T_imu_body = identity; include/airvision.h, "Odometry covariance")
        self.publish_covariance = False
        # no reference counterpart: the drop-in MSCKF keeps the landmark records of its last feature_callback in `last_landmarks`
        # (up to landmark_cap per frame, positions in the world frame of the published pose; include/airvision.h, "Landmark map")
        self.publish_landmarks = False
        self.landmark_cap = 256
        # no reference counterpart: the drop-in MSCKF keeps the innovation statistics of its last feature_callback in `last_innovation`
        # (msckf_ops.FILTER_STATS_DTYPE[2]: the lost-feature and the pruning update; include/airvision.h, "Innovation statistics")
        self.publish_innovation = False
        # no reference counterpart: the drop-in MSCKF keeps the IMU-rate records of its last feature_callback in `last_imu_states` (the
        # state after every IMU sample of the frame, the last imu_rate_cap of them; include/airvision.h, "IMU-rate odometry")
        self.publish_imu_rate = False
        self.imu_rate_cap = 32
        # no reference counterpart: the drop-in MSCKF keeps the forecast of its last feature_callback in `last_forecast` -- the pose the step
        # leaves carried through the IMU samples pushed beyond the frame's time (the first forecast_cap of them), with its covariance
        # (include/airvision.h, "Forecast")
        self.publish_forecast = False
        self.forecast_cap = 32
        # no reference counterpart: the zero-velocity update (include/airvision.h, "Zero-velocity update").  A stream that passes the IMU
        # test (gyro and | |acc| - g | below the thresholds over the frame's samples) and the vision test (at least zupt_min_tracks
        # tracked features, zupt_still_percent of them displaced by at most zupt_max_disparity pixels against the previous frame) gets
        # velocity = 0 as a measurement of deviation zupt_velocity_sigma, gated at zupt_gate (the 95 % quantile of chi^2 with three
        # degrees of freedom; 0: no gate).  The thresholds are starting values against the synthetic sensors (gyro sigma 0.005 rad/s,
        # accelerometer sigma 0.05 m/s^2), not tuned on flight data.  The drop-in MSCKF keeps the record in `last_zupt`.
        self.use_zupt = False
        self.zupt_gyro_threshold = 0.1
        self.zupt_acc_threshold = 0.5
        self.zupt_max_disparity = 0.5
        self.zupt_min_tracks = 10
        self.zupt_still_percent = 90
        self.zupt_velocity_sigma = 0.05
        self.zupt_gate = 7.815
