"""Python handle of the MSCKF device context (av_msckf_* C ABI): covariance resident on the GPU, batched
per-feature kernels, stacked update.  Used by dropin/msckf.py and dropin/feature; numpy in, numpy out."""
import collections
import ctypes as C

import numpy as np
import torch
from scipy.stats import chi2

from . import _native as N


def _d(a):
    return (C.c_double * len(a))(*[float(v) for v in a])


class FeatureBatch(object):
    """CSR description of a batch of features on the device."""

    def __init__(self, obs_cam_lists, obs_z_lists, device):
        dev = torch.device('cuda', device)
        counts = [len(c) for c in obs_cam_lists]
        self.n = len(counts)
        self.max_obs = max(counts) if counts else 0
        off = np.zeros(self.n + 1, np.int32)
        off[1:] = np.cumsum(counts)
        cam = np.concatenate([np.asarray(c, np.int32) for c in obs_cam_lists]) if self.n else np.zeros(0, np.int32)
        z = np.concatenate([np.asarray(zz, np.float64).reshape(-1, 4) for zz in obs_z_lists]) if self.n else np.zeros((0, 4))
        self.counts = counts
        self.off = torch.from_numpy(off).to(dev)
        self.cam = torch.from_numpy(np.ascontiguousarray(cam)).to(dev)
        self.z = torch.from_numpy(np.ascontiguousarray(z)).to(dev)


class MsckfDevice(object):
    def __init__(self, max_cam_states=20, rows_cap=8192, device=0):
        self.device = int(device)
        self.dev = torch.device('cuda', self.device)
        table = np.zeros(100)
        table[1:] = [chi2.ppf(0.05, i) for i in range(1, 100)]          # msckf.py:111-113
        self.chi2_table = table
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_create(int(max_cam_states), int(rows_cap), _d(table), self.device, C.byref(self._h)))
        self.rows_cap = rows_cap

    def close(self):
        if self._h:
            N.lib().av_msckf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dim(self):
        return N.lib().av_msckf_dim(self._h)

    def _st(self):
        return N.current_stream()

    def set_cov(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_set_cov(self._h, P.ctypes.data_as(C.c_void_p), P.shape[0], self._st()))

    def get_cov(self):
        n = self.dim
        P = np.empty((n, n), np.float64)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_get_cov(self._h, P.ctypes.data_as(C.c_void_p), n, self._st()))
        return P

    def propagate(self, dt, gyro, acc, q_old, q_new, q_null, v_null, p_null, v_new, p_new, gravity, noise):
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_propagate(self._h, float(dt), _d(gyro), _d(acc), _d(q_old), _d(q_new), _d(q_null), _d(v_null),
                                               _d(p_null), _d(v_new), _d(p_new), _d(gravity), _d(noise), self._st()))

    def augment(self, R_imu_cam0, skew_Rt_t):
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_augment(self._h, _d(np.asarray(R_imu_cam0).reshape(-1)), _d(np.asarray(skew_Rt_t).reshape(-1)), self._st()))

    def remove_cam(self, idx):
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_remove_cam(self._h, int(idx), self._st()))

    def _cams(self, cam_q, cam_p):
        q = torch.from_numpy(np.ascontiguousarray(cam_q, dtype=np.float64).reshape(-1, 4)).to(self.dev)
        p = torch.from_numpy(np.ascontiguousarray(cam_p, dtype=np.float64).reshape(-1, 3)).to(self.dev)
        return q, p

    def triangulate(self, batch, cam_q, cam_p, T_cam0_cam1, opt):
        """-> (positions float64[n,3], valid bool[n])."""
        if batch.n == 0:
            return np.zeros((0, 3)), np.zeros(0, bool)
        q, p = self._cams(cam_q, cam_p)
        pos = torch.empty((batch.n, 3), dtype=torch.float64, device=self.dev)
        valid = torch.empty(batch.n, dtype=torch.int32, device=self.dev)
        opt5 = _d([opt.huber_epsilon, opt.estimation_precision, opt.initial_damping,
                   opt.outer_loop_max_iteration, opt.inner_loop_max_iteration])
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_triangulate(self._h, batch.n, N.dptr(batch.off), N.dptr(batch.cam), N.dptr(batch.z), N.dptr(q), N.dptr(p),
                                                 _d(np.asarray(T_cam0_cam1, dtype=np.float64).reshape(-1)), opt5, 2 * batch.max_obs,
                                                 N.dptr(pos), N.dptr(valid), self._st()))
            torch.cuda.synchronize()
        return pos.cpu().numpy(), valid.cpu().numpy().astype(bool)

    def feature_blocks(self, batch, positions, dofs, cam_q, cam_p, cam_qn, cam_pn, T_cam0_cam1, gravity, obs_noise):
        """Jacobian + null-space projection + gate for the batch.  -> (row_off int[n], gamma[n], pass bool[n])."""
        n_cam = len(cam_q)
        rows = np.array([4 * c - 3 for c in batch.counts], np.int32)
        row_off = np.zeros(batch.n, np.int32)
        if batch.n:
            row_off[1:] = np.cumsum(rows)[:-1]
        total = int(rows.sum())
        if batch.n == 0:
            return row_off, rows, np.zeros(0), np.zeros(0, bool)
        q, p = self._cams(cam_q, cam_p)
        qn, pn = self._cams(cam_qn, cam_pn)
        pos = torch.from_numpy(np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)).to(self.dev)
        dof = torch.from_numpy(np.ascontiguousarray(dofs, dtype=np.int32)).to(self.dev)
        ro = torch.from_numpy(row_off).to(self.dev)
        gamma = torch.empty(batch.n, dtype=torch.float64, device=self.dev)
        ok = torch.empty(batch.n, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_feature_blocks(self._h, batch.n, n_cam, batch.max_obs, N.dptr(batch.off), N.dptr(batch.cam), N.dptr(batch.z),
                                                    N.dptr(pos), N.dptr(dof), N.dptr(ro), total, N.dptr(q), N.dptr(p), N.dptr(qn), N.dptr(pn),
                                                    _d(np.asarray(T_cam0_cam1, dtype=np.float64).reshape(-1)), _d(gravity), float(obs_noise),
                                                    N.dptr(gamma), N.dptr(ok), self._st()))
            torch.cuda.synchronize()
        return row_off, rows, gamma.cpu().numpy(), ok.cpu().numpy().astype(bool)

    def read_blocks(self, row0, n_rows):
        """Parity-test tap (tests only): rows of the block buffer feature_blocks filled -> (H float64[n_rows, ld], r float64[n_rows])."""
        ld = N.lib().av_msckf_ld(self._h)
        H = np.empty((int(n_rows), ld)); r = np.empty(int(n_rows))
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_read_blocks(self._h, int(row0), int(n_rows), H.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), self._st()))
        return H, r

    def feature_ops_dev(self, obs_cam_lists, obs_z_lists, fs_stride, cam_q, cam_p, cam_qn, cam_pn, P, gravity, T_cam0_cam1, opt, obs_noise, dofs,
                        max_obs, teams, tri_list=None, feat_list=None, positions=None, valid=None, compact=0, zero_fill=0):
        """Parity-test entry (av_msckf_feature_ops_dev; tests only): the per-feature kernels in the launch shapes of the device-resident
        filter.  Feature slot f = stream * fs_stride + k (obs_cam_lists / obs_z_lists / dofs have one entry per slot, empty = unused);
        cam_* are [streams * cam_stride] rows, P is [streams, n, n] with n = 21 + 6 * cam_stride, gravity [streams, 3].  tri_list /
        feat_list: slots to triangulate / to evaluate (device lists with device-side counts; None skips the stage); positions / valid
        preset the arrays the triangulation would write.  Every index is checked here, on the host, before anything is launched.
        -> dict(pos, valid, H [streams, rows, ld or compact] (NaN where nothing was written), r, gamma, ok, row_off)."""
        n_slots = len(obs_cam_lists)
        counts = np.array([len(c) for c in obs_cam_lists], np.int64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        S, ld = P.shape[0], P.shape[1]
        cam_q = np.ascontiguousarray(cam_q, dtype=np.float64).reshape(-1, 4)
        cam_stride = len(cam_q) // S
        if fs_stride < 1 or n_slots != S * fs_stride or len(cam_q) != S * cam_stride or P.shape != (S, ld, ld) or ld != 21 + 6 * cam_stride or len(dofs) != n_slots:
            raise ValueError('feature_ops_dev: inconsistent shapes')
        for name, a in (('cam_p', cam_p), ('cam_qn', cam_qn), ('cam_pn', cam_pn)):
            if len(a) != len(cam_q):
                raise ValueError('feature_ops_dev: %s has %d rows, cam_q %d' % (name, len(a), len(cam_q)))
        lists = []
        for lst in (tri_list, feat_list):
            lst = None if lst is None else np.ascontiguousarray(lst, dtype=np.int32)
            if lst is not None and len(lst) and (lst.min() < 0 or lst.max() >= n_slots or counts[lst].min() < 1 or (max_obs > 2 and counts[lst].max() > max_obs)):
                raise ValueError('feature_ops_dev: a listed slot is out of range, empty or longer than max_obs')
            lists.append(lst)
        tri_list, feat_list = lists
        if any(len(c) and (min(c) < 0 or max(c) >= cam_stride) for c in obs_cam_lists) or min(dofs) < 0 or max(dofs) > 99:
            raise ValueError('feature_ops_dev: camera index or dof out of range')
        if not (compact == 0 or (compact >= 6 * max_obs and not zero_fill)) or not 1 <= int(teams) <= 262144:
            raise ValueError('feature_ops_dev: bad compact / zero_fill / teams')
        batch = FeatureBatch([c if len(c) else [] for c in obs_cam_lists], [z if len(z) else np.zeros((0, 4)) for z in obs_z_lists], self.device)
        rows = np.maximum(4 * counts - 3, 0).reshape(S, fs_stride)
        row_off = (np.cumsum(rows, axis=1) - rows).astype(np.int32).reshape(-1)
        rows_cap = max(int(rows.sum(axis=1).max()), 1)
        width = compact if compact > 0 else ld
        dev = self.dev
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        q, p = self._cams(cam_q, cam_p)
        qn, pn = self._cams(cam_qn, cam_pn)
        pos = up(np.zeros((n_slots, 3)) if positions is None else np.asarray(positions).reshape(n_slots, 3), np.float64)
        val = up(np.zeros(n_slots) if valid is None else valid, np.int32)
        H = torch.full((S, rows_cap, width), float('nan'), dtype=torch.float64, device=dev)
        r = torch.full((S, rows_cap), float('nan'), dtype=torch.float64, device=dev)
        gam = torch.full((n_slots,), float('nan'), dtype=torch.float64, device=dev)
        ok = torch.full((n_slots,), -1, dtype=torch.int32, device=dev)
        Pd, grav, dof, ro = up(P, np.float64), up(np.asarray(gravity).reshape(S, 3), np.float64), up(dofs, np.int32), up(row_off, np.int32)
        tl = None if tri_list is None else up(tri_list, np.int32)
        fl = None if feat_list is None else up(feat_list, np.int32)
        nt = up([0 if tri_list is None else len(tri_list)], np.int32)
        nf = up([0 if feat_list is None else len(feat_list)], np.int32)
        opt5 = _d([opt.huber_epsilon, opt.estimation_precision, opt.initial_damping, opt.outer_loop_max_iteration, opt.inner_loop_max_iteration])
        null = C.c_void_p(None)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_feature_ops_dev(
                self._h, S, int(fs_stride), cam_stride, int(max_obs), int(compact), int(zero_fill), int(teams),
                null if tl is None else N.dptr(tl), N.dptr(nt), null if fl is None else N.dptr(fl), N.dptr(nf),
                N.dptr(batch.off), N.dptr(batch.cam), N.dptr(batch.z), N.dptr(dof), N.dptr(ro), N.dptr(q), N.dptr(p), N.dptr(qn), N.dptr(pn),
                N.dptr(Pd), ld, ld * ld, N.dptr(grav), _d(np.asarray(T_cam0_cam1, dtype=np.float64).reshape(-1)), opt5, float(obs_noise),
                N.dptr(pos), N.dptr(val), N.dptr(H), rows_cap * width, N.dptr(r), rows_cap, N.dptr(gam), N.dptr(ok), self._st()))
            torch.cuda.synchronize()
        return dict(pos=pos.cpu().numpy(), valid=val.cpu().numpy(), H=H.cpu().numpy(), r=r.cpu().numpy(), gamma=gam.cpu().numpy(), ok=ok.cpu().numpy(),
                    row_off=row_off, rows=rows.reshape(-1))

    STATE_FIELDS = (('ts', 1), ('q', 4), ('p', 3), ('v', 3), ('bg', 3), ('ba', 3), ('R_ic', 9), ('t_ci', 3), ('qn', 4), ('pn', 3), ('vn', 3),
                    ('gravity', 3), ('tracking_rate', 1))          # state_io of av_msckf_predict_ops_dev, 43 doubles
    STATE_INTS = ('n', 'ncam', 'failed', 'null_aliased', 'first_img', 'active')

    def predict_ops_dev(self, streams, imu, cam_q, cam_p, cam_qn, P, noise, wg, rate_cap=0, rate_fill=np.nan):
        """Parity-test entry (av_msckf_predict_ops_dev; tests only): the prediction of the device-resident filter -- state integration,
        covariance propagation, augmentation -- in the launch sequence a step begins with, for all `streams` at once, at wg = 64 or 256.
        streams: one dict per stream with the STATE_FIELDS (R_ic 3 x 3 or 9), n, ncam, and optionally failed, null_aliased, first_img,
        active (default 1), t_frame (default ts), imu_first / imu_cnt (default 0 / 0), find_redundant (bool), remove ((i0, i1) or None).
        imu: float64[n_imu, 7] (t, gyro, acc).  cam_q / cam_p / cam_qn: [streams, cam_stride, 4 | 3 | 4]; P: [streams, ld, ld] (whatever
        lies outside a stream's own square is the caller's pre-fill and must come back untouched).  The library checks every count and
        position before it launches anything.
        rate_cap >= 1: through av_msckf_predict_ops_dev_rate, the launches a step begins with when the IMU-rate odometry is on; the result
        then also holds imu_rec IMU_STATE_DTYPE[streams, rate_cap], pre-filled with rate_fill in every double, and imu_n int32[streams, 2],
        pre-filled with -1, as the kernel left them.
        -> dict(streams: list of dicts (STATE_FIELDS + STATE_INTS as they come back, redundant: (r0, r1) or None), cam_q, cam_p, cam_qn, P)."""
        S = len(streams)
        cam_q = np.ascontiguousarray(cam_q, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if cam_q.ndim != 3 or cam_q.shape[0] != S or P.ndim != 3 or P.shape[0] != S or P.shape[1] != P.shape[2]:
            raise ValueError('predict_ops_dev: inconsistent shapes')
        cs, ld = cam_q.shape[1], P.shape[1]
        if np.shape(cam_p) != (S, cs, 3) or np.shape(cam_qn) != (S, cs, 4):
            raise ValueError('predict_ops_dev: cam_p / cam_qn do not match cam_q')
        sd, si, tf, ctl = np.zeros((S, 43)), np.zeros((S, 6), np.int32), np.zeros(S), np.zeros((S, 6), np.int32)
        for s, st in enumerate(streams):
            o = 0
            for name, k in self.STATE_FIELDS:
                sd[s, o:o + k] = np.asarray(st[name], dtype=np.float64).reshape(-1)
                o += k
            si[s, :5] = [st['n'], st['ncam'], st.get('failed', 0), st.get('null_aliased', 0), st.get('first_img', 0)]
            tf[s] = st.get('t_frame', st['ts'])
            rm = st.get('remove') or (0, 0)
            ctl[s] = [st.get('active', 1), st.get('imu_first', 0), st.get('imu_cnt', 0), (1 if st.get('find_redundant') else 0) | (2 if st.get('remove') else 0), rm[0], rm[1]]
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        red = np.full((S, 2), -1, np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)
        q, p, qn, Pd = up(cam_q), up(cam_p), up(cam_qn), up(P)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)
        rate = {}
        if rate_cap:
            rec = np.full((S, int(rate_cap), 14), rate_fill, dtype=np.float64)
            rate = dict(imu_rec=rec.view(IMU_STATE_DTYPE).reshape(S, int(rate_cap)), imu_n=np.full((S, 2), -1, np.int32))
        with torch.cuda.device(self.device):
            args = (self._h, S, int(wg), cs, ld, ld * ld, hp(sd), hp(si), hp(tf), hp(ctl), hp(imu), len(imu), _d(noise),
                    N.dptr(q), N.dptr(p), N.dptr(qn), N.dptr(Pd), hp(red), self._st())
            if rate_cap:
                N.check(N.lib().av_msckf_predict_ops_dev_rate(*(args + (int(rate_cap), hp(rec), hp(rate['imu_n'])))))
            else:
                N.check(N.lib().av_msckf_predict_ops_dev(*args))
            torch.cuda.synchronize()
        out = []
        for s, st in enumerate(streams):
            d, o = {}, 0
            for name, k in self.STATE_FIELDS:
                d[name] = sd[s, o:o + k].copy() if k > 1 else float(sd[s, o])
                o += k
            d.update(zip(self.STATE_INTS, (int(v) for v in si[s])))
            d['redundant'] = (int(red[s, 0]), int(red[s, 1])) if st.get('find_redundant') else None
            out.append(d)
        return dict(streams=out, cam_q=q.cpu().numpy(), cam_p=p.cpu().numpy(), cam_qn=qn.cpu().numpy(), P=Pd.cpu().numpy(), **rate)

    def update_ops_dev(self, streams, H, r, P, obs_noise, phase, kch=0, hld=0, cam_stride=None, fs_stride=None, dx_fill=np.nan):
        """Parity-test entry (av_msckf_update_ops_dev; tests only): the batched measurement update -- stacking decisions, information
        form, row compression, Cholesky back end -- in the launch sequence a phase of a step runs, for all `streams` at once.
        streams: one dict per stream with n, optionally mode (1: information form allowed, default; 2: stopped), and feats: the candidate
        features in map order, each a dict(cams: camera slot of every observation, ok: gate flag, row: first of its 4 M - 3 rows in the
        stream's block buffer).  H: [streams, rows_cap, ld] (hld = 0) or [streams, rows_cap, hld] (compact rows), r: [streams, rows_cap],
        P: [streams, ld, ld] (whatever lies outside a stream's n x n square is the caller's pre-fill and must come back untouched).
        phase 0: the lost-feature configuration (cut at 1500 rows, no information form), 1: the pruning configuration; kch: rows one
        back-end pass takes directly (0: the filter's own, min(136, ld)).  The library checks every count and index before it launches anything.
        -> dict(dx [streams, ld] pre-filled with dx_fill, stacked [streams], cols: per stream the touched columns, rec: per stream
        dict(m, nc, mode, kdir, n_blk) as the stacking kernel wrote it, P)."""
        S = len(streams)
        H = np.ascontiguousarray(H, dtype=np.float64)
        r = np.ascontiguousarray(r, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if H.ndim != 3 or r.ndim != 2 or P.ndim != 3 or H.shape[0] != S or r.shape != H.shape[:2] or P.shape[0] != S or P.shape[1] != P.shape[2]:
            raise ValueError('update_ops_dev: inconsistent shapes')
        ld, rows_cap = P.shape[1], H.shape[1]
        if H.shape[2] != (hld if hld > 0 else ld):
            raise ValueError('update_ops_dev: rows of %d doubles, expected %d' % (H.shape[2], hld if hld > 0 else ld))
        cs = int(cam_stride) if cam_stride is not None else max(1, (ld - 21) // 6)
        fs = int(fs_stride) if fs_stride is not None else max([1] + [len(st['feats']) for st in streams])
        n_s = np.array([st['n'] for st in streams], np.int32)
        mode = np.array([st.get('mode', 1) for st in streams], np.int32)
        n_cand = np.array([len(st['feats']) for st in streams], np.int32)
        nf = S * fs
        counts, ok, row = np.zeros(nf, np.int64), np.zeros(nf, np.int32), np.zeros(nf, np.int32)
        cams = []
        for s, st in enumerate(streams):
            for k, f in enumerate(st['feats'][:fs]):
                i = s * fs + k
                counts[i], ok[i], row[i] = len(f['cams']), int(bool(f['ok'])), f['row']
        # (the observation CSR is laid out slot by slot, so a stream with more candidates than fs_stride still describes valid memory:
        #  the library refuses it by its count)
        for s, st in enumerate(streams):
            for f in st['feats'][:fs]:
                cams.extend(int(c) for c in f['cams'])
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        cam = np.array(cams if cams else [0], np.int32)
        dx = np.full((S, ld), dx_fill, dtype=np.float64)
        stacked, cols, rec = np.full(S, -99, np.int32), np.full((S, 6 * cs), -99, np.int32), np.full((S, 5), -99, np.int32)
        up = lambda a: torch.from_numpy(a).to(self.dev)
        Hd, rd, Pd = up(H), up(r), up(P)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_update_ops_dev(
                self._h, S, int(phase), int(kch), fs, cs, int(hld), hp(n_s), hp(mode), hp(n_cand), hp(off), hp(cam), len(cams), hp(ok), hp(row),
                N.dptr(Hd), rows_cap * H.shape[2], N.dptr(rd), rows_cap, rows_cap, N.dptr(Pd), ld, ld * ld, float(obs_noise),
                hp(dx), hp(stacked), hp(cols), hp(rec), self._st()))
            torch.cuda.synchronize()
        return dict(dx=dx, stacked=stacked, cols=[c[c >= 0] for c in cols], P=Pd.cpu().numpy(),
                    rec=[dict(zip(('m', 'nc', 'mode', 'kdir', 'n_blk'), (int(v) for v in q))) for q in rec])

    def forecast_ops_dev(self, streams, imu, P, noise, cap, fill=np.nan):
        """Parity-test entry (av_msckf_forecast_ops_dev; tests only): the forecast's two kernels through the helper a step launches them
        through, for all `streams` at once.  streams: one dict per stream with the STATE_FIELDS, n, ncam, and optionally failed,
        null_aliased, first_img, active (default 1) -- the state a step LEAVES -- and pend_first / pend_cnt (default 0 / 0): its pending
        samples are imu[pend_first : pend_first + pend_cnt].  imu: float64[n_imu, 7]; P: [streams, ld, ld].
        -> dict(streams: the states as they come back, P, rec IMU_STATE_DTYPE[streams, cap] pre-filled with `fill` in every double,
        n int32[streams, 2] pre-filled with -1, cov float64[streams, 120] pre-filled with `fill`, as the kernels left them)."""
        S = len(streams)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if P.ndim != 3 or P.shape[0] != S or P.shape[1] != P.shape[2]:
            raise ValueError('forecast_ops_dev: inconsistent shapes')
        ld = P.shape[1]
        sd, si, pend = np.zeros((S, 43)), np.zeros((S, 6), np.int32), np.zeros((S, 2), np.int32)
        for s, st in enumerate(streams):
            o = 0
            for name, k in self.STATE_FIELDS:
                sd[s, o:o + k] = np.asarray(st[name], dtype=np.float64).reshape(-1)
                o += k
            si[s] = [st['n'], st['ncam'], st.get('failed', 0), st.get('null_aliased', 0), st.get('first_img', 0), st.get('active', 1)]
            pend[s] = [st.get('pend_first', 0), st.get('pend_cnt', 0)]
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        Pd = torch.from_numpy(P).to(self.dev)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)
        rec = np.full((S, int(cap), 14), fill, dtype=np.float64)
        n, cov = np.full((S, 2), -1, np.int32), np.full((S, ODOM_COV_DOUBLES), fill, dtype=np.float64)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_forecast_ops_dev(self._h, S, ld, ld * ld, hp(sd), hp(si), hp(imu), len(imu), hp(pend), _d(noise), N.dptr(Pd), self._st(),
                                                      int(cap), hp(rec), hp(n), hp(cov)))
            torch.cuda.synchronize()
        out = []
        for s in range(S):
            d, o = {}, 0
            for name, k in self.STATE_FIELDS:
                d[name] = sd[s, o:o + k].copy() if k > 1 else float(sd[s, o])
                o += k
            d.update(zip(self.STATE_INTS, (int(v) for v in si[s])))
            out.append(d)
        return dict(streams=out, P=Pd.cpu().numpy(), rec=rec.view(IMU_STATE_DTYPE).reshape(S, int(cap)), n=n, cov=cov)

    def zupt_ops_dev(self, streams, cam_q, cam_p, P, params):
        """Parity-test entry (av_msckf_zupt_ops_dev; tests only): the zero-velocity update's kernel through the helper a step launches it
        through, for all `streams` at once.  streams: one dict per stream with the STATE_FIELDS, n, ncam, and optionally failed,
        null_aliased, first_img, active (default 1) -- the state a step LEAVES -- and zupt_flags (default ZU_DETECTED), detected_total,
        applied_total (default 0): the record as the detector left it.  cam_q / cam_p: [streams, cam_stride, 4 | 3]; P: [streams, ld, ld]
        (whatever lies outside a stream's n x n square is the caller's pre-fill); params: a dict of ZUPT_PARAM_NAMES.
        -> dict(streams: the states as they come back, cam_q, cam_p, P, rec ZUPT_DTYPE[streams])."""
        S = len(streams)
        cam_q = np.ascontiguousarray(cam_q, dtype=np.float64)
        cam_p = np.ascontiguousarray(cam_p, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        if cam_q.ndim != 3 or cam_q.shape[0] != S or cam_q.shape[2] != 4 or cam_p.shape != cam_q.shape[:2] + (3,) or P.ndim != 3 or P.shape[0] != S or P.shape[1] != P.shape[2]:
            raise ValueError('zupt_ops_dev: inconsistent shapes')
        cs, ld = cam_q.shape[1], P.shape[1]
        sd, si, rec = np.zeros((S, 43)), np.zeros((S, 6), np.int32), np.zeros(S, ZUPT_DTYPE)
        for s, st in enumerate(streams):
            o = 0
            for name, k in self.STATE_FIELDS:
                sd[s, o:o + k] = np.asarray(st[name], dtype=np.float64).reshape(-1)
                o += k
            si[s] = [st['n'], st['ncam'], st.get('failed', 0), st.get('null_aliased', 0), st.get('first_img', 0), st.get('active', 1)]
            rec[s]['flags'] = st.get('zupt_flags', ZU_DETECTED)
            rec[s]['detected_total'], rec[s]['applied_total'] = st.get('detected_total', 0), st.get('applied_total', 0)
        up = lambda a: torch.from_numpy(a).to(self.dev)
        q, p, Pd = up(cam_q), up(cam_p), up(P)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)
        zp = _zupt_struct(params)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_zupt_ops_dev(self._h, S, cs, ld, ld * ld, hp(sd), hp(si), N.dptr(q), N.dptr(p), N.dptr(Pd), C.byref(zp), hp(rec), self._st()))
            torch.cuda.synchronize()
        out = []
        for s in range(S):
            d, o = {}, 0
            for name, k in self.STATE_FIELDS:
                d[name] = sd[s, o:o + k].copy() if k > 1 else float(sd[s, o])
                o += k
            d.update(zip(self.STATE_INTS, (int(v) for v in si[s])))
            out.append(d)
        return dict(streams=out, cam_q=q.cpu().numpy(), cam_p=p.cpu().numpy(), P=Pd.cpu().numpy(), rec=rec)

    def update(self, blk_rows, blk_lens, obs_noise):
        """Stacked EKF update on the selected blocks; returns delta_x (n doubles)."""
        n = self.dim
        dx = np.zeros(n)
        total = int(np.sum(blk_lens)) if len(blk_lens) else 0
        if total == 0:
            return dx
        br = torch.from_numpy(np.ascontiguousarray(blk_rows, dtype=np.int32)).to(self.dev)
        bl = torch.from_numpy(np.ascontiguousarray(blk_lens, dtype=np.int32)).to(self.dev)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_update(self._h, N.dptr(br), N.dptr(bl), len(blk_lens), total, float(obs_noise),
                                            dx.ctypes.data_as(C.c_void_p), self._st()))
        return dx


# ---- odometry covariance (include/airvision.h, "Odometry covariance") --------------------------------------------------------
ODOM_COV_DIM = 15
ODOM_COV_DOUBLES = 120             # AV_ODOM_COV_DOUBLES: the upper triangle of the 15 x 15 record, row-major
# error coordinates of the record, in order: (name, slice)
ODOM_COV_FIELDS = (('p', slice(0, 3)), ('theta', slice(3, 6)), ('v', slice(6, 9)), ('p_c', slice(9, 12)), ('theta_c', slice(12, 15)))
_ODOM_IU = np.triu_indices(ODOM_COV_DIM)


def unpack_odom_cov(a):
    """float64[..., 120] records as a step returns them -> exactly symmetric float64[..., 15, 15] (NaN records stay NaN)."""
    a = np.asarray(a, dtype=np.float64)
    assert a.shape[-1] == ODOM_COV_DOUBLES, a.shape
    C_ = np.empty(a.shape[:-1] + (ODOM_COV_DIM, ODOM_COV_DIM))
    C_[..., _ODOM_IU[0], _ODOM_IU[1]] = a
    C_[..., _ODOM_IU[1], _ODOM_IU[0]] = a
    return C_


def pack_odom_cov(Cm):
    """float64[..., 15, 15] -> the wire form float64[..., 120] (the upper triangle, row-major)."""
    Cm = np.asarray(Cm, dtype=np.float64)
    assert Cm.shape[-2:] == (ODOM_COV_DIM, ODOM_COV_DIM), Cm.shape
    return np.ascontiguousarray(Cm[..., _ODOM_IU[0], _ODOM_IU[1]])


# ---- landmark map (include/airvision.h, "Landmark map") ------------------------------------------------------------------------
LANDMARK_DTYPE = np.dtype([('id', np.int64), ('p', np.float64, (3,)), ('flags', np.int32), ('n_obs', np.int32)])      # av_landmark, AV_LANDMARK_BYTES
assert LANDMARK_DTYPE.itemsize == 40
LM_USED, LM_REJECTED, LM_TRACKED, LM_NEW = 1, 2, 4, 8               # AV_LM_*


def unpack_landmarks(rec, n, s):
    """The written records of stream `s`: rec LANDMARK_DTYPE[S, cap] and n int32[S, 2] as a step returns them -> rec[s, :n[s, 1]]
    (n[s, 0] - n[s, 1] records were dropped to the cap)."""
    return rec[s, :int(n[s, 1])]


# ---- innovation statistics (include/airvision.h, "Innovation statistics") ------------------------------------------------------
_FS_INTS = ('n_cand', 'n_pos', 'n_eval', 'n_pass', 'dof_eval', 'dof_pass', 'rows', 'flags')
_FS_DOUBLES = ('gamma_eval', 'gamma_pass', 'dx_pos', 'dx_rot')
FILTER_STATS_DTYPE = np.dtype([(n, np.int32) for n in _FS_INTS] + [(n, np.float64) for n in _FS_DOUBLES])      # av_update_stats; a step's records: [S, 2]
assert FILTER_STATS_DTYPE.itemsize == 64
FILTER_STATS_BYTES = 128                                            # AV_FILTER_STATS_BYTES: block 0 the lost-feature update, block 1 the pruning update
FS_RAN, FS_CUT = 1, 2                                               # AV_FS_*


def filter_stats_rows(rec):
    """(rows of the evaluated features' residuals, rows of the accepted ones) of records FILTER_STATS_DTYPE[..., 2]: the gate's dof is
    M - 1 in the lost-feature update and M in the pruning update, a residual has 4 M - 3 rows -> 4 dof + n and 4 dof - 3 n."""
    rec = np.asarray(rec)
    k = np.array([1, -3], dtype=np.int64)
    return (4 * rec['dof_eval'].astype(np.int64) + k * rec['n_eval'], 4 * rec['dof_pass'].astype(np.int64) + k * rec['n_pass'])


def unpack_filter_stats(rec):
    """Records FILTER_STATS_DTYPE[..., 2] as a step returns them -> a dict of arrays of that shape: every field of the record, and per block
    rows_eval   rows of the residuals of the evaluated features (from the dof sums; for the accepted ones that is `rows`)
    nis_dof     gamma_eval / dof_eval: the normalised innovation in the units of the gate (the reference's dof, not the residual's dimension)
    nis_rows    gamma_eval / rows_eval: the normalised innovation per residual dimension, near 1 for a consistent filter
    reject_rate 1 - n_pass / n_eval
    with NaN where nothing was evaluated."""
    rec = np.asarray(rec)
    out = {n: rec[n] for n in FILTER_STATS_DTYPE.names}
    rows_eval, _ = filter_stats_rows(rec)
    ne = rec['n_eval'].astype(np.float64)
    nothing = rec['n_eval'] <= 0
    with np.errstate(divide='ignore', invalid='ignore'):
        out['rows_eval'] = rows_eval
        out['nis_dof'] = np.where(nothing, np.nan, rec['gamma_eval'] / rec['dof_eval'])
        out['nis_rows'] = np.where(nothing, np.nan, rec['gamma_eval'] / rows_eval)
        out['reject_rate'] = np.where(nothing, np.nan, 1.0 - rec['n_pass'] / ne)
    return out


# ---- IMU-rate odometry (include/airvision.h, "IMU-rate odometry") --------------------------------------------------------------
IMU_STATE_DTYPE = np.dtype([('t', np.float64), ('p', np.float64, (3,)), ('q', np.float64, (4,)), ('v', np.float64, (3,)), ('w', np.float64, (3,))])      # av_imu_state, AV_IMU_STATE_BYTES
assert IMU_STATE_DTYPE.itemsize == 112
IMU_RATE_CAP_MAX = 4096


def unpack_imu_states(rec, n, s):
    """The written records of stream `s`: rec IMU_STATE_DTYPE[S, cap] and n int32[S, 2] as a step returns them -> rec[s, :n[s, 1]], in
    time order (n[s, 0] - n[s, 1] records, the oldest, were dropped to the cap)."""
    return rec[s, :int(n[s, 1])]


# ---- forecast (include/airvision.h, "Forecast") --------------------------------------------------------------------------------
FORECAST_CAP_MAX = 4096


def unpack_forecast(rec, n, cov, s):
    """The forecast of stream `s`: rec IMU_STATE_DTYPE[S, cap], n int32[S, 2] and cov float64[S, 120] as a step returns them ->
    (rec[s, :n[s, 1]], the covariance as 15 x 15, reached_t).  The written records are the FIRST n[s, 1] pending samples in time order
    (n[s, 0] > n[s, 1]: the cap ended the chain before the newest sample); reached_t is the last written record's stamp, None when
    nothing was written -- the covariance is then that of the pose the step leaves, at the step's own time.  A stream that did not
    publish reads no records, a NaN matrix and None."""
    got = rec[s, :int(n[s, 1])]
    return got, unpack_odom_cov(cov[s]), (float(got['t'][-1]) if len(got) else None)


# ---- zero-velocity update (include/airvision.h, "Zero-velocity update") --------------------------------------------------------
_ZU_INTS = ('flags', 'n_imu', 'n_tracked', 'n_still', 'detected_total', 'applied_total')
_ZU_DOUBLES = ('w_max', 'a_dev_max', 'v_norm', 'gamma', 'dx_pos')
ZUPT_DTYPE = np.dtype([(n, np.int32) for n in _ZU_INTS] + [(n, np.float64) for n in _ZU_DOUBLES])      # av_zupt, AV_ZUPT_BYTES
assert ZUPT_DTYPE.itemsize == 64
ZU_IMU_OK, ZU_VIS_OK, ZU_DETECTED, ZU_APPLIED, ZU_GATED, ZU_BAD = 1, 2, 4, 8, 16, 32      # AV_ZU_*
ZUPT_PARAM_NAMES = ('gyro_max', 'acc_dev_max', 'disparity_max', 'velocity_sigma', 'gate', 'min_tracks', 'still_percent')      # av_zupt_params


def zupt_params(config):
    """The av_zupt_params of a config's zupt_* attributes as a dict (ZUPT_PARAM_NAMES): zupt_max_disparity, in pixels, becomes
    normalised image units with 2 / (fx + fy) of cam0."""
    fx, fy = float(config.cam0_intrinsics[0]), float(config.cam0_intrinsics[1])
    return dict(gyro_max=float(config.zupt_gyro_threshold), acc_dev_max=float(config.zupt_acc_threshold),
                disparity_max=float(config.zupt_max_disparity) * 2.0 / (fx + fy), velocity_sigma=float(config.zupt_velocity_sigma),
                gate=float(config.zupt_gate), min_tracks=int(config.zupt_min_tracks), still_percent=int(config.zupt_still_percent))


def _zupt_struct(params):
    if set(params) != set(ZUPT_PARAM_NAMES):
        raise ValueError('zero-velocity parameters are a dict of %s' % ', '.join(ZUPT_PARAM_NAMES))
    return N.ZuptParams(*[(float if i < 5 else int)(params[k]) for i, k in enumerate(ZUPT_PARAM_NAMES)])


def unpack_zupt(rec):
    """Records ZUPT_DTYPE[...] as `read_zupt` returns them -> a dict of arrays of that shape: every field of the record, and the flags
    as booleans imu_ok, vis_ok, detected, applied, gated, bad."""
    rec = np.asarray(rec)
    out = {n: rec[n] for n in ZUPT_DTYPE.names}
    for name, bit in (('imu_ok', ZU_IMU_OK), ('vis_ok', ZU_VIS_OK), ('detected', ZU_DETECTED), ('applied', ZU_APPLIED), ('gated', ZU_GATED), ('bad', ZU_BAD)):
        out[name] = (rec['flags'] & bit) != 0
    return out


# The optional outputs of a step of BatchedMSCKF, one entry each.  kw: the keyword of `step / submit / submit_dev`; ctor_kw: the
# constructor keyword that switches it on; setting: the attribute that holds its setting (falsy: off); fn: the library's
# av_msckf_batch_set_<fn> / av_msckf_batch_next_<fn>; last: the attribute that remembers the arrays of the most recent step that was
# given any; shapes(flt): the (dtype, shape) of every array it takes; fill: what `True` allocates them with; what(flt): its ValueError.
# A sixth output is one more entry here (and its constructor / step keywords), beside the C table (OUTS, csrc/msckf_dev.inc).
StepOutput = collections.namedtuple('StepOutput', 'kw ctor_kw setting fn last shapes fill what')
STEP_OUTPUTS = (
    StepOutput('cov', 'odom_cov', 'odom_cov', 'odom_cov', 'last_cov', lambda f: [(np.float64, (f.S, ODOM_COV_DOUBLES))], np.nan,
               lambda f: 'cov must be a C-contiguous float64[%d, %d] array' % (f.S, ODOM_COV_DOUBLES)),
    StepOutput('landmarks', 'landmarks', 'landmark_cap', 'landmarks', 'last_landmarks',
               lambda f: [(LANDMARK_DTYPE, (f.S, f.landmark_cap)), (np.int32, (f.S, 2))], 0,
               lambda f: 'landmarks must be a pair of C-contiguous arrays LANDMARK_DTYPE[%d, %d], int32[%d, 2]' % (f.S, f.landmark_cap, f.S)),
    StepOutput('stats', 'stats', 'stats', 'stats', 'last_stats', lambda f: [(FILTER_STATS_DTYPE, (f.S, 2))], 0,
               lambda f: 'stats must be a C-contiguous FILTER_STATS_DTYPE[%d, 2] array' % f.S),
    StepOutput('imu_states', 'imu_rate', 'imu_rate_cap', 'imu_rate', 'last_imu_states',
               lambda f: [(IMU_STATE_DTYPE, (f.S, f.imu_rate_cap)), (np.int32, (f.S, 2))], 0,
               lambda f: 'imu_states must be a pair of C-contiguous arrays IMU_STATE_DTYPE[%d, %d], int32[%d, 2]' % (f.S, f.imu_rate_cap, f.S)),
    StepOutput('forecast', 'forecast', 'forecast_cap', 'forecast', 'last_forecast',
               lambda f: [(IMU_STATE_DTYPE, (f.S, f.forecast_cap)), (np.int32, (f.S, 2)), (np.float64, (f.S, ODOM_COV_DOUBLES))], 0,
               lambda f: 'forecast must be a triple of C-contiguous arrays IMU_STATE_DTYPE[%d, %d], int32[%d, 2], float64[%d, %d]' %
               (f.S, f.forecast_cap, f.S, f.S, ODOM_COV_DOUBLES)),
)
_OUTPUT = {o.kw: o for o in STEP_OUTPUTS}


class BatchedMSCKF(object):
    """S independent filters stepped together (av_msckf_batch_* C ABI): C++ bookkeeping inside the
    library, one batched launch per numeric phase.  Mirrors MSCKF.imu_callback / feature_callback
    (reference: src/msckf.py:162-228) for many streams at once."""

    def __init__(self, config, n_streams, device=0, rows_cap=None, max_features=None, odom_cov=False, landmarks=False, landmark_cap=64, stats=False,
                 imu_rate=False, imu_rate_cap=32, forecast=False, forecast_cap=32, zupt=False):
        """rows_cap: rows of the per-stream block buffer.  None = sized by the library from the capacity of the first
        feature message (the camera-pruning update stacks 5 rows per feature, the lost-feature update at most 1500 + one
        block); `max_features`, when given, sizes it up front instead.  With the automatic size a later step with a wider
        `ids.shape[1]` REBUILDS the block buffers and the device-resident observation store for the wider message (drains the
        batch, synchronises the device, grows by at least x1.5, keeps the outgrown allocations until close) -- pass
        max_features when the width of the feature arrays can vary.  An explicit rows_cap is never grown.
        config.max_cam_state_size <= 24 (reference: 20).
        odom_cov=True: every step also computes the covariance of what it publishes (ODOM_COV_FIELDS; `step / submit / submit_dev(...,
        cov=)`, `last_cov`, `unpack_odom_cov`).
        landmarks=True: every step also publishes the features its two updates triangulated, up to landmark_cap records per stream
        (LANDMARK_DTYPE; `step / submit / submit_dev(..., landmarks=)`, `last_landmarks`, `unpack_landmarks`).
        stats=True: every step also publishes the innovation statistics of its two updates, FILTER_STATS_DTYPE[S, 2] (`step / submit /
        submit_dev(..., stats=)`, `last_stats`, `unpack_filter_stats`).
        imu_rate=True: every step also publishes the state after every IMU sample its prediction integrated, the last imu_rate_cap
        (1 .. 4096) of them per stream (IMU_STATE_DTYPE; `step / submit / submit_dev(..., imu_states=)`, `last_imu_states`,
        `unpack_imu_states`).  Predictions from the previous step's state; `w` is in the IMU frame.
        forecast=True: every step also publishes the pose it leaves carried through the IMU samples pushed beyond the frame's time, the
        first forecast_cap (1 .. 4096) of them per stream, with the covariance at the last of them (records IMU_STATE_DTYPE, counts, a
        float64[S, 120] odometry-covariance record; `step / submit / submit_dev(..., forecast=)`, `last_forecast`, `unpack_forecast`).
        Read-only for the filter: every other output and the state are bit for bit what they are without it.
        zupt=True: the zero-velocity update with the config's zupt_* attributes (`zupt_params`), or a dict of ZUPT_PARAM_NAMES: a stream
        detected at rest gets velocity = 0 as a measurement on the state the step leaves -- the step's own published pose is the
        pre-update one; `get_state`, `get_cov`, the forecast and the next step see the corrected state.  `read_zupt()` reads the records."""
        if rows_cap is None:
            rows_cap = 0 if max_features is None else max(2048, 5 * int(max_features) + 64)
        self.rows_cap = int(rows_cap)
        self.config = config
        self.S = int(n_streams)
        self.device = int(device)
        table = np.zeros(100)
        table[1:] = [chi2.ppf(0.05, i) for i in range(1, 100)]
        T_cam0_imu = np.linalg.inv(config.T_imu_cam0)
        rt = np.concatenate([T_cam0_imu[:3, :3].T.reshape(-1), T_cam0_imu[:3, 3]])
        o = config.optimization_config
        self._h = C.c_void_p()
        self._inflight = []
        self.generation = np.zeros(self.S, dtype=np.int64)      # restarts of every stream so far (`restart`)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_batch_create(
                self.S, int(config.max_cam_state_size), int(rows_cap), _d(table), _d(config.gravity),
                _d(np.asarray(config.T_cn_cnm1, dtype=np.float64).reshape(-1)), _d(rt),
                _d([config.gyro_bias_cov, config.velocity_cov, config.acc_bias_cov, config.extrinsic_rotation_cov, config.extrinsic_translation_cov]),
                _d([config.gyro_noise, config.gyro_bias_noise, config.acc_noise, config.acc_bias_noise]),
                float(config.observation_noise), float(config.position_std_threshold), _d(config.velocity),
                _d([o.huber_epsilon, o.estimation_precision, o.initial_damping, o.outer_loop_max_iteration, o.inner_loop_max_iteration, o.translation_threshold]),
                self.device, C.byref(self._h)))
        # the optional outputs: last_* = the arrays of the most recent step that was given any (cov: float64[S, 120]; landmarks: (records
        # LANDMARK_DTYPE[S, cap], counts int32[S, 2]); stats: FILTER_STATS_DTYPE[S, 2]; imu_states: (records IMU_STATE_DTYPE[S, cap], counts
        # int32[S, 2]); forecast: (records IMU_STATE_DTYPE[S, cap], counts int32[S, 2], covariance float64[S, 120]))
        want = {'odom_cov': bool(odom_cov), 'landmark_cap': int(landmark_cap) if landmarks else 0, 'stats': bool(stats),
                'imu_rate_cap': int(imu_rate_cap) if imu_rate else 0, 'forecast_cap': int(forecast_cap) if forecast else 0}
        for o in STEP_OUTPUTS:
            setattr(self, o.setting, want[o.setting])
            setattr(self, o.last, None)
        try:
            if landmarks and want['landmark_cap'] < 1:
                raise ValueError('landmark_cap must be at least 1')
            if imu_rate and not 1 <= want['imu_rate_cap'] <= IMU_RATE_CAP_MAX:
                raise ValueError('imu_rate_cap must be 1 .. %d' % IMU_RATE_CAP_MAX)
            if forecast and not 1 <= want['forecast_cap'] <= FORECAST_CAP_MAX:
                raise ValueError('forecast_cap must be 1 .. %d' % FORECAST_CAP_MAX)
            for o in STEP_OUTPUTS:
                if want[o.setting]:
                    self._set(o, want[o.setting])
            self.zupt = None                                 # the zero-velocity update's parameters (dict of ZUPT_PARAM_NAMES), None: off
            if zupt:
                self.set_zupt(zupt_params(config) if zupt is True else zupt)
        except Exception:
            self.close()
            raise

    def _set(self, o, setting):
        N.check(getattr(N.lib(), 'av_msckf_batch_set_' + o.fn)(self._h, int(setting)))
        setattr(self, o.setting, setting)

    def set_odom_cov(self, enable):
        """av_msckf_batch_set_odom_cov: before the first step only."""
        self._set(_OUTPUT['cov'], bool(enable))

    def set_landmarks(self, cap):
        """av_msckf_batch_set_landmarks: cap records per stream and step (0: off); before the first step only."""
        self._set(_OUTPUT['landmarks'], int(cap))

    def set_stats(self, enable):
        """av_msckf_batch_set_stats: before the first step only."""
        self._set(_OUTPUT['stats'], bool(enable))

    def set_imu_rate(self, cap):
        """av_msckf_batch_set_imu_rate: cap records per stream and step (0: off, at most 4096); before the first step only."""
        self._set(_OUTPUT['imu_states'], int(cap))

    def set_forecast(self, cap):
        """av_msckf_batch_set_forecast: cap records per stream and step (0: off, at most 4096); before the first step only."""
        self._set(_OUTPUT['forecast'], int(cap))

    def set_zupt(self, params):
        """av_msckf_batch_set_zupt: a dict of ZUPT_PARAM_NAMES (`zupt_params(config)` builds one), None: off; before the first step only."""
        p = None if params is None else _zupt_struct(params)
        N.check(N.lib().av_msckf_batch_set_zupt(self._h, None if p is None else C.byref(p)))
        self.zupt = None if params is None else dict(params)

    def read_zupt(self):
        """The zero-velocity records of every stream after the last step, ZUPT_DTYPE[S] (av_msckf_batch_read_zupt; `unpack_zupt`); drains
        the queue first.  Zeros while the update is off or before the first step."""
        self.wait(0)
        rec = np.zeros(self.S, ZUPT_DTYPE)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_batch_read_zupt(self._h, rec.ctypes.data_as(C.c_void_p)))
        return rec

    def _next(self, o, value):
        """The arrays of output `o` for the next step (None: the step has none), handed to the library.  value: None, True (allocate) or
        the caller's C-contiguous array (landmarks, imu_states: pair of arrays; forecast: triple) of o.shapes(self)."""
        if value is None or value is False:
            return None
        if not getattr(self, o.setting):
            raise ValueError('%s= needs BatchedMSCKF(..., %s=True)' % (o.kw, o.ctor_kw))
        shapes = o.shapes(self)
        if value is True:
            arrs = tuple(np.full(shape, o.fill, dtype=dtype) for dtype, shape in shapes)
        else:
            arrs = tuple(value) if len(shapes) > 1 else (value,)
        if len(arrs) != len(shapes) or not all(isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags['C_CONTIGUOUS']
                                               for a, (dtype, shape) in zip(arrs, shapes)):
            raise ValueError(o.what(self))
        N.check(getattr(N.lib(), 'av_msckf_batch_next_' + o.fn)(self._h, *[a.ctypes.data_as(C.c_void_p) for a in arrs]))
        setattr(self, o.last, arrs[0] if len(arrs) == 1 else arrs)
        return getattr(self, o.last)

    def _next_outputs(self, **kw):
        """`step / submit / submit_dev`'s keywords handed to the library; the tuple of arrays the step's entry of _inflight keeps alive."""
        return tuple(self._next(o, kw[o.kw]) for o in STEP_OUTPUTS)

    def close(self):
        if self._h:
            if getattr(self, '_inflight', None):
                N.lib().av_msckf_batch_wait(self._h, 0)          # queued steps still reference the arrays in _inflight
                self._inflight = []
            N.lib().av_msckf_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push_imu(self, stream_idx, timestamps, gyro, acc):
        si = np.ascontiguousarray(stream_idx, dtype=np.int32)
        ts = np.ascontiguousarray(timestamps, dtype=np.float64)
        g = np.ascontiguousarray(gyro, dtype=np.float64).reshape(-1, 3)
        a = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 3)
        N.check(N.lib().av_msckf_batch_push_imu(self._h, si.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p),
                                                g.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), len(si)))

    def step(self, ids, uv, n_feat, timestamps, cov=None, landmarks=None, stats=None, imu_states=None, forecast=None):
        """ids int64[S,cap], uv float64[S,cap,4], n_feat int32[S], timestamps float64[S] (host arrays).
        Returns float64[S,12]: published, t, p(3), q(4), v(3).  cov (odom_cov=True): a float64[S,120] array that takes the step's
        odometry-covariance records, or True to have one allocated; it is `last_cov` afterwards.  landmarks (landmarks=True): a pair of
        arrays (LANDMARK_DTYPE[S, landmark_cap], int32[S, 2]) that takes the step's landmark records and counts, or True to have them
        allocated; the pair is `last_landmarks` afterwards.  stats (stats=True): a FILTER_STATS_DTYPE[S, 2] array that takes the step's
        innovation statistics, or True to have one allocated; it is `last_stats` afterwards.  imu_states (imu_rate=True): a pair of arrays
        (IMU_STATE_DTYPE[S, imu_rate_cap], int32[S, 2]) that takes the step's IMU-rate records and counts, or True to have them allocated;
        the pair is `last_imu_states` afterwards.  forecast (forecast=True): a triple of arrays (IMU_STATE_DTYPE[S, forecast_cap], int32[S, 2],
        float64[S, 120]) that takes the step's forecast records, counts and covariance, or True to have them allocated; the triple is
        `last_forecast` afterwards (`unpack_forecast`)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        nf = np.ascontiguousarray(n_feat, dtype=np.int32)
        ts = np.ascontiguousarray(timestamps, dtype=np.float64)
        cap = ids.shape[1]
        out = np.zeros((self.S, 12))
        self._next_outputs(cov=cov, landmarks=landmarks, stats=stats, imu_states=imu_states, forecast=forecast)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_batch_step(self._h, ids.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p),
                                                nf.ctypes.data_as(C.c_void_p), cap, ts.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p), N.current_stream()))
        return out

    def submit(self, ids, uv, n_feat, timestamps, cov=None, landmarks=None, stats=None, imu_states=None, forecast=None):
        """Queue one step (av_msckf_batch_submit) and return its float64[S,12] output array, which is filled once the
        step has retired -- i.e. after a `wait(k)` that leaves fewer than the steps submitted after it pending.  The
        stream groups of the batch run behind their queues independently of each other.  cov: as in `step`; the array (`last_cov`) is
        filled when the step retires, like the output array; landmarks, stats, imu_states, forecast: likewise."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        nf = np.ascontiguousarray(n_feat, dtype=np.int32)
        ts = np.ascontiguousarray(timestamps, dtype=np.float64)
        out = np.zeros((self.S, 12))
        outs = self._next_outputs(cov=cov, landmarks=landmarks, stats=stats, imu_states=imu_states, forecast=forecast)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_batch_submit(self._h, ids.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p),
                                                  nf.ctypes.data_as(C.c_void_p), ids.shape[1], ts.ctypes.data_as(C.c_void_p),
                                                  out.ctypes.data_as(C.c_void_p), N.current_stream()))
        self._inflight.append((ids, uv, nf, ts, out) + outs)     # the library reads / writes these until the step retires
        return out

    def device_resident(self):
        """Always True: the filter state and the observation map live on the device.  Kept for callers that still ask."""
        return N.lib().av_msckf_batch_device_resident(self._h) == 1

    def submit_dev(self, engine, timestamps, msg_stream=None, cov=None, landmarks=None, stats=None, imu_states=None, forecast=None):
        """Queue one step on the feature message `engine` (a FrontendEngine with the same streams) has just published, read
        where it lies on the device (av_msckf_batch_submit_dev): no host round trip between the front-end and the filter.
        msg_stream: the stream handle the engine's step ran on (default: torch's current stream, i.e. call this right after
        `engine.step` on the same stream).  The filter's kernels run on the current stream / the stream groups' own streams.
        Returns the float64[S,12] output array, filled once a `wait` has let the step retire.  cov, landmarks, stats, imu_states, forecast: as in `submit`."""
        ids, uv, n, cap = engine.features_dev()
        ts = np.ascontiguousarray(timestamps, dtype=np.float64)
        assert ts.shape == (self.S,) and engine.n_streams == self.S
        out = np.zeros((self.S, 12))
        outs = self._next_outputs(cov=cov, landmarks=landmarks, stats=stats, imu_states=imu_states, forecast=forecast)
        with torch.cuda.device(self.device):
            ms = N.current_stream() if msg_stream is None else msg_stream
            N.check(N.lib().av_msckf_batch_submit_dev(self._h, ids, uv, n, cap, ts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                      ms, N.current_stream()))
        self._inflight.append((ts, out) + outs)
        return out

    def wait(self, max_pending=0):
        """Block until at most `max_pending` submitted steps are unfinished; raises the first error of a retired step."""
        N.check(N.lib().av_msckf_batch_wait(self._h, int(max_pending)))
        while len(self._inflight) > max_pending:
            self._inflight.pop(0)

    def restart(self, streams):
        """Put the listed streams back to "as created" while the others keep stepping (av_msckf_batch_restart; include/airvision.h,
        "Stream restart"): from the next step on each of them is bit for bit a stream of a new batch.  Drains the queue first (queued
        steps retire as steps of the old life).  IMU samples pushed before the call are dropped: push the new life's samples after it.
        `generation[s]` counts the restarts of stream s -- camera-state ids and the map's order repeat across lives."""
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(streams, dtype=np.int64)).reshape(-1), dtype=np.int32)
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_batch_restart(self._h, idx.ctypes.data_as(C.c_void_p), len(idx)))
        if len(idx):
            self._inflight = []                              # the queue has been drained
            self.generation[np.unique(idx)] += 1

    def sizes(self, s):
        o = (C.c_int32 * 3)()
        N.check(N.lib().av_msckf_batch_sizes(self._h, int(s), C.byref(o)))
        return int(o[0]), int(o[1]), int(o[2])

    COUNTER_NAMES = ('steps', 'prune_stream_steps', 'two_pass_streams', 'devbuf_growths', 'min_cam_states', 'max_cam_states',
                     'min_map_features', 'max_map_features')

    def counters(self):
        """Run statistics over all streams (av_msckf_batch_counters); drains the queue first.  `two_pass_streams` counts the stream-steps
        whose lost-feature candidates needed more rows than `rows_cap`: the filter serves them from the overflow pool all
        streams share (AV_MSCKF_POOL_ROWS; an exhausted pool stops the stream with AV_E_CAPACITY)."""
        self.wait(0)
        o = (C.c_int64 * 8)()
        N.check(N.lib().av_msckf_batch_counters(self._h, C.byref(o)))
        return dict(zip(self.COUNTER_NAMES, [int(v) for v in o]))

    def launch_shape(self):
        """[(streams, workgroup size), ...] per stream group, as launched (av_msckf_batch_launch_shape); drains the queue first.  The
        workgroup size is what the per-stream kernels of the group's last step ran with: 64 (one wavefront per stream: groups of at least
        1,024 streams, or AV_DK_WG=64), 256 (four), 0 before the first step."""
        self.wait(0)
        o = (C.c_int32 * 17)()
        N.check(N.lib().av_msckf_batch_launch_shape(self._h, C.byref(o)))
        return [(int(o[1 + 2 * g]), int(o[2 + 2 * g])) for g in range(int(o[0]))]

    def get_cov(self, s):
        n = self.sizes(s)[0]
        P = np.empty((n, n))
        with torch.cuda.device(self.device):
            N.check(N.lib().av_msckf_batch_get_cov(self._h, int(s), P.ctypes.data_as(C.c_void_p), n, N.current_stream()))
        return P

    def get_state(self, s):
        """Everything measurement_update injects into (msckf.py:568-595) for stream s: dict(t, q, p, v, bg, ba, R_ic, t_ci,
        gravity, cam_ids, cam_q, cam_p).  Drain (`wait(0)`) first."""
        imu = (C.c_double * 32)()
        n = C.c_int32(0)
        cap = int(self.config.max_cam_state_size) + 1
        ids = np.zeros(cap, np.int64); qp = np.zeros((cap, 7))
        N.check(N.lib().av_msckf_batch_get_state(self._h, int(s), C.byref(imu), ids.ctypes.data_as(C.c_void_p), qp.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        a = np.array(imu[:])
        k = int(n.value)
        return dict(t=a[0], q=a[1:5], p=a[5:8], v=a[8:11], bg=a[11:14], ba=a[14:17], R_ic=a[17:26].reshape(3, 3), t_ci=a[26:29],
                    gravity=a[29:32], cam_ids=ids[:k].copy(), cam_q=qp[:k, :4].copy(), cam_p=qp[:k, 4:].copy())

    def stream_status(self, s):
        """(0, '') while stream s runs; (AV_E_* code, reason) once a per-stream capacity failure stopped it (its step output
        then reads published = -1; the other streams keep running)."""
        st = C.c_int32(0)
        msg = C.create_string_buffer(160)
        N.check(N.lib().av_msckf_batch_stream_status(self._h, int(s), C.byref(st), msg, 160))
        return int(st.value), msg.value.decode()

    WORK_NAMES = ('gate_flops', 'update_flops', 'reference_qr_flops', 'features_gated', 'updates', 'rows_stacked', 'chain_ms', 'chain_timings_dropped')

    def work(self, enable=-1):
        """Algorithmic fp64 flops of the gates / updates run so far and the device time of the phase chains
        (av_msckf_batch_work); enable=1/0 switches the event timing on / off, -1 only reads.  Drains the queue first."""
        self.wait(0)
        o = (C.c_double * 8)()
        N.check(N.lib().av_msckf_batch_work(self._h, int(enable), C.byref(o)))
        return dict(zip(self.WORK_NAMES, [float(v) for v in o]))

    def work_executed(self):
        """fp64 flops the gate / update kernels EXECUTED so far on their block-sparse shapes (av_msckf_batch_work_executed; analytic per
        gated feature / per update): {'gate_flops_executed', 'update_flops_executed'}.  Drains the queue first."""
        self.wait(0)
        o = (C.c_double * 2)()
        N.check(N.lib().av_msckf_batch_work_executed(self._h, C.byref(o)))
        return {'gate_flops_executed': float(o[0]), 'update_flops_executed': float(o[1])}

    def debug_capture(self, enable=True):
        """Parity-test tap: keep gamma / delta_x / P+ of the two update phases of every stream's last step (tests only)."""
        N.check(N.lib().av_msckf_batch_debug_capture(self._h, 1 if enable else 0))

    def debug_read(self, s, phase, gamma_cap=8192):
        """(gamma float64[k], rows, dx float64[n] or None, P_after float64[n,n] or None) of phase 0 (remove_lost_features) or
        1 (prune_cam_state_buffer) of stream s's last step."""
        ncap = 21 + 6 * (int(self.config.max_cam_state_size) + 1)
        g = np.zeros(gamma_cap); dx = np.zeros(ncap); P = np.zeros(ncap * ncap)
        ng, n, rows = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        N.check(N.lib().av_msckf_batch_debug_read(self._h, int(s), int(phase), g.ctypes.data_as(C.c_void_p), gamma_cap, C.byref(ng),
                                                  dx.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), ncap, C.byref(n), C.byref(rows)))
        k = int(n.value)
        if rows.value <= 0:
            return g[:ng.value].copy(), 0, None, None
        return g[:ng.value].copy(), int(rows.value), dx[:k].copy(), P[:k * k].reshape(k, k).copy()
