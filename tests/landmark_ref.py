"""The landmark map of a filter step (include/airvision.h, "Landmark map") stated on the NumPy oracle: LandmarkOracle restates
OracleMSCKF.remove_lost_features and prune_cam_state_buffer with the same arithmetic in the same order and records, for every step, the
list of (id, position, flags, n_obs) the contract defines.  The oracle file itself is not edited; tests/test_landmark_ref.py checks that
the restatement publishes bit for bit what the plain oracle publishes.

Next to every record the geometry of its triangulation is kept (`geom`), for the position bar of tests/test_gpu_landmarks.py:
z = distance from the landmark to its first observing camera, b = the largest distance between two observing camera centres (cam0
and cam1 of every observing state), both taken when the position was triangulated -- a carried feature keeps the geometry it was fixed
with, because its position is the one computed then."""
import numpy as np

from oracle.msckf_np import OracleMSCKF, to_rotation

LM_USED, LM_REJECTED, LM_TRACKED, LM_NEW = 1, 2, 4, 8


class LandmarkOracle(OracleMSCKF):
    def __init__(self, config, next_imu_id=0):
        OracleMSCKF.__init__(self, config, next_imu_id)
        self.landmarks = []          # records of the last feature_callback: dicts id, p, flags, n_obs, z, b
        self.geom = {}               # feature id -> (z, b) of the triangulation that fixed its position

    def feature_callback(self, feature_msg):
        self.landmarks = []
        return OracleMSCKF.feature_callback(self, feature_msg)

    def _geometry(self, feat):
        """(z, b) of a feature that has just been triangulated from the camera states observing it."""
        centres = []
        for cid in feat.observations:
            if cid not in self.cam_states:
                continue
            cs = self.cam_states[cid]
            R_w_c1 = self.R_cam0_cam1 @ to_rotation(cs.orientation)
            centres += [np.array(cs.position), cs.position - R_w_c1.T @ self.t_cam0_cam1]
        z = float(np.linalg.norm(feat.position - centres[0]))
        b = max(float(np.linalg.norm(p - q)) for p in centres for q in centres)
        return z, b

    def _init_recorded(self, feat):
        """_try_init; True in the second place if the position was obtained by this call."""
        was = feat.is_initialized
        ok = self._try_init(feat)
        if ok and not was:
            self.geom[feat.id] = self._geometry(feat)
        return ok, ok and not was

    def _record(self, feat, flags, n_obs):
        z, b = self.geom[feat.id]
        self.landmarks.append(dict(id=feat.id, p=np.array(feat.position), flags=flags, n_obs=n_obs, z=z, b=b))

    def remove_lost_features(self):
        rows = 0
        invalid, processed, new = [], [], set()
        for feat in self.map_server.values():
            if self.imu_state.id in feat.observations:
                continue
            if len(feat.observations) < 3:
                invalid.append(feat.id)
                continue
            ok, fresh = self._init_recorded(feat)
            if not ok:
                invalid.append(feat.id)
                continue
            if fresh:
                new.add(feat.id)
            rows += 4 * len(feat.observations) - 3
            processed.append(feat.id)
        for fid in invalid:
            del self.map_server[fid]
        if not processed:
            return
        H = np.zeros((rows, 21 + 6 * len(self.cam_states)))
        r = np.zeros(rows)
        k = 0
        flags = {fid: 0 for fid in processed}          # beyond the cut: never evaluated
        for fid in processed:
            feat = self.map_server[fid]
            cam_ids = list(feat.observations.keys())
            Hj, rj = self.feature_jacobian(fid, cam_ids)
            if self.gating_test(Hj, rj, len(cam_ids) - 1):
                H[k:k + Hj.shape[0], :Hj.shape[1]] = Hj
                r[k:k + len(rj)] = rj
                k += Hj.shape[0]
                flags[fid] = LM_USED
            else:
                flags[fid] = LM_REJECTED
            if k > 1500:
                break
        for fid in processed:
            feat = self.map_server[fid]
            self._record(feat, flags[fid] | (LM_NEW if fid in new else 0), len(feat.observations))
        self.measurement_update(H[:k], r[:k])
        for fid in processed:
            del self.map_server[fid]

    def prune_cam_state_buffer(self):
        if len(self.cam_states) < self.config.max_cam_state_size:
            return
        rm = self.find_redundant_cam_states()
        rows = 0
        new = set()
        for feat in self.map_server.values():
            inv = [c for c in rm if c in feat.observations]
            if not inv:
                continue
            if len(inv) == 1:
                del feat.observations[inv[0]]
                continue
            ok, fresh = self._init_recorded(feat)
            if not ok:
                for c in inv:
                    del feat.observations[c]
                continue
            if fresh:
                new.add(feat.id)
            rows += 4 * len(inv) - 3
        H = np.zeros((rows, 21 + 6 * len(self.cam_states)))
        r = np.zeros(rows)
        k = 0
        for feat in self.map_server.values():
            inv = [c for c in rm if c in feat.observations]
            if not inv:
                continue
            Hj, rj = self.feature_jacobian(feat.id, inv)
            if self.gating_test(Hj, rj, len(inv)):
                H[k:k + Hj.shape[0], :Hj.shape[1]] = Hj
                r[k:k + len(rj)] = rj
                k += Hj.shape[0]
                used = LM_USED
            else:
                used = LM_REJECTED
            if feat.id in new:                          # a feature fixed in an earlier step has been published with these bits already
                self._record(feat, LM_TRACKED | LM_NEW | used, len(feat.observations))
            for c in inv:
                del feat.observations[c]
        self.measurement_update(H[:k], r[:k])
        for cid in rm:
            i = list(self.cam_states.keys()).index(cid)
            a, b = 21 + 6 * i, 27 + 6 * i
            keep = np.r_[0:a, b:self.state_cov.shape[0]]
            self.state_cov = self.state_cov[np.ix_(keep, keep)].copy()
            del self.cam_states[cid]
