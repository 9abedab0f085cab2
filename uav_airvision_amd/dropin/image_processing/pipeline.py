"""ImageProcessingPipeline on the MI355X engine (reference: src/image_processing/pipeline.py:14-150).

Same constructor argument and callbacks as the reference class; the work is done by one
device-resident `FrontendEngine` with a single stream (the throughput path batches S streams through
the same kernels, see uav_airvision_amd/frontend.py).  There is no CPU path.
"""
from collections import defaultdict, namedtuple

import numpy as np

from uav_airvision_amd.frontend import FrontendEngine

from .feature_measurment import FeatureMeasurement
from .feature_meta_data import FeatureMetaData

_feature_msg = namedtuple('feature_msg', ['timestamp', 'features'])


class ImageProcessingPipeline(object):
    def __init__(self, config, device=0, max_corners=None):
        self.config = config
        self.prev_cam0_msg = None
        self._engine = FrontendEngine(config, n_streams=1, device=device, max_corners=max_corners)
        self.first_frame = True
        self.prev_pyr0 = None
        self.curr_features = [[] for _ in range(config.grid_num)]
        # config.use_clahe (no counterpart in the reference): the engine equalises every frame ahead of everything else; a viewer set
        # here is shown the image the front-end actually worked on (update_image, the hook of viewer.py:45-49)
        # config.image_downscale 2 / 4: the callbacks still take full-size frames; the same hook shows the binned frame
        # config.cam*_response / cam*_vignette: the engine reads them from the config object; the same hook shows the corrected frame
        # config.gray16_scale 'window' / 'auto' (image_format 'gray16'): likewise; gray16_range() returns the (lo, hi) of the last frame
        # config.exposure_reference: both image messages then carry an attribute `exposure`, the frame's exposure time in the unit of the
        # reference (a ValueError names the message that has none); without the setting the attribute is never read
        self.use_clahe = bool(getattr(config, 'use_clahe', False))
        self.downscale = self._engine.downscale
        self.viewer = None

    def gray16_range(self):
        """(lo, hi) the last stereo frame was scaled with (config.gray16_scale 'window' or 'auto'; refused with 'shift')."""
        lo, hi = self._engine.read_range()[0]
        return int(lo), int(hi)

    # ---- reference callbacks -----------------------------------------------------------------
    def imu_callback(self, imu_msg):
        """pipeline.py:42-44 -> imu_processor.py:22-26 (thread-safe against stereo_callback)."""
        self._engine.push_imu(0, imu_msg.timestamp, imu_msg.angular_velocity)

    def stereo_callback(self, stereo_msg):
        """pipeline.py:46-150: returns feature_msg(timestamp, [FeatureMeasurement])."""
        cam0_msg, cam1_msg = stereo_msg.cam0_msg, stereo_msg.cam1_msg
        kw = {}
        if self._engine.exposure:
            for name, msg in (('cam0_msg', cam0_msg), ('cam1_msg', cam1_msg)):
                if getattr(msg, 'exposure', None) is None:
                    raise ValueError('config.exposure_reference is set and %s carries no attribute `exposure`' % name)
            kw['exposure'] = ([float(cam0_msg.exposure)], [float(cam1_msg.exposure)])
        if self._engine.pixel_format != 0:
            # config.image_format (no counterpart in the reference): colour, 16-bit, mosaic or packed 10 / 12-bit frames (uint8 [h, w * d / 8])
            # go to the engine as they are and are converted to 8-bit grey on the GPU; step_host refuses a wrong dtype or shape with a ValueError naming both
            self._engine.step_host(cam0_msg.image, cam1_msg.image, [cam0_msg.timestamp], **kw)
        else:
            img0 = np.ascontiguousarray(cam0_msg.image, dtype=np.uint8)
            img1 = np.ascontiguousarray(cam1_msg.image, dtype=np.uint8)
            if img0.ndim != 2 or img0.shape != (self._engine.input_height, self._engine.input_width) or img1.shape != img0.shape:
                raise ValueError('expected two uint8[%d,%d] images' % (self._engine.input_height, self._engine.input_width))
            self._engine.step_host(img0, img1, [cam0_msg.timestamp], **kw)
        (ids, uv), = self._engine.read_features()
        feats = []
        for k in range(len(ids)):
            fm = FeatureMeasurement()
            fm.id = int(ids[k])
            fm.u0, fm.v0, fm.u1, fm.v1 = uv[k, 0], uv[k, 1], uv[k, 2], uv[k, 3]
            feats.append(fm)
        self.prev_cam0_msg = cam0_msg
        self.prev_pyr0 = cam0_msg.image
        self.first_frame = False
        if (self.use_clahe or self.downscale > 1 or self._engine.photometric) and self.viewer is not None:
            self.viewer.update_image(self.equalized_image(0))
        return _feature_msg(cam0_msg.timestamp, feats)

    # ---- pipeline state visible to callers (pipeline.py:33-40,145-148) -----------------------
    @property
    def prev_features(self):
        g = self._engine.read_grid(0)
        grid = [[] for _ in range(self.config.grid_num)]
        for k in range(len(g['ids'])):
            f = FeatureMetaData()
            f.id = int(g['ids'][k]); f.lifetime = int(g['lifetime'][k])
            f.cam0_point = g['cam0'][k]; f.cam1_point = g['cam1'][k]
            grid[int(g['cell'][k])].append(f)
        return grid

    @property
    def next_feature_id(self):
        return self._engine.read_grid(0)['next_feature_id']

    @property
    def num_features(self):
        c = self._engine.read_counters(0)
        # after_ransac: the engine's own count when config.use_ransac is set; the reference's tracker has no such step and reports
        # after_matching again (feature_tracker.py:135-136, 157)
        ransac = getattr(self.config, 'use_ransac', False) and c['after_matching'] > 0
        d = defaultdict(int)
        d.update(before_tracking=c['before_tracking'], after_tracking=c['after_tracking'], after_matching=c['after_matching'],
                 after_ransac=self._engine.read_ransac_counts(0)['after_ransac'] if ransac else c['after_matching'])
        return d

    def equalized_image(self, cam=0):
        """The grey frame of camera `cam` the last stereo_callback worked on, at the processed size: converted from
        config.image_format, binned (config.image_downscale) and / or equalised (config.use_clahe); refused with none of them."""
        return self._engine.read_image(0, cam)

    def restart(self):
        """No counterpart in the reference: the pipeline back to "as constructed" without rebuilding the engine (FrontendEngine.restart).
        The next stereo_callback is an initialisation and feature ids begin again at 0; `generation` counts the restarts."""
        self._engine.restart([0])
        self.prev_cam0_msg = None
        self.prev_pyr0 = None
        self.first_frame = True

    @property
    def generation(self):
        return int(self._engine.generation[0])

    def close(self):
        self._engine.close()
