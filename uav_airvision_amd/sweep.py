"""Sequence x offset sweep runner on the batched throughput path.

The reference's `run.bat:4-12` runs 9 sequences x 7 start offsets serially through `main.py --path DIR --offset S`
(`main.py:10-34`, `streaming/dataset.py:189-214`).  Here every (sequence, offset) pair is one independent stream; the
pairs are partitioned over ranks (`shard.partition`, one process per GPU) and each rank steps ALL of its streams
together: one `FrontendEngine(n_streams=k)` (one batched kernel launch per stage and step for the k streams) feeding one
`BatchedMSCKF(k)` -- the same two objects bench.py times -- driven by the deterministic replay of SURVEY 3.5 (IMU
messages with timestamp <= t before the frame at t).  Sequences end at different frames; a finished stream idles
(blank images, frame timestamp -1 for the filter) until the longest one is done.  Trajectories are gathered at the end
(`shard.gather_trajectories`); there is no per-frame communication.

    python -m uav_airvision_amd.sweep --root /data/euroc --sequences MH_01_easy MH_03_medium --offsets 0 10 20
    python -m torch.distributed.run --nproc-per-node 8 -m uav_airvision_amd.sweep ...
    python -m uav_airvision_amd.sweep --make-synthetic /tmp/syn --sequences SYN_01 SYN_02 --frames 200 ...   (no dataset at hand)
"""
import argparse
import json
import os
import sys

import numpy as np


def run_stream(config, dataset_path, offset, device=0, max_frames=None):
    """ONE (sequence, offset) stream through the single-stream drop-in classes (`ImageProcessor` + `MSCKF`, the objects
    `modules/vio.py` constructs); returns (float64[n, 8] trajectory `t px py pz qx qy qz qw`, dataset).  The sweep itself
    uses `run_batched`; this is the reference-shaped path kept for comparison and for `vio.py`-style callers."""
    here = os.path.dirname(os.path.abspath(__file__))
    dropin = os.path.join(here, 'dropin')
    if dropin not in sys.path:
        sys.path.insert(0, dropin)
    from image_processing import ImageProcessor
    from msckf import MSCKF
    from .euroc import EuRoCDataset, replay
    ds = EuRoCDataset(dataset_path)
    ds.set_starttime(offset)
    ip = ImageProcessor(config, device=device)
    flt = MSCKF(config, device=device, write_trajectory=False)
    traj = []

    def on_stereo(msg):
        feat = ip.stereo_callback(msg)
        if feat and flt.feature_callback(feat) is not None:
            s = flt.state_server.imu_state
            traj.append([s.timestamp, *s.position, *s.orientation])
    replay(ds, [ip.imu_callback, flt.imu_callback], on_stereo, max_frames)
    ip.close(); flt.close()
    return np.array(traj, dtype=np.float64).reshape(-1, 8), ds


class BatchedRunner(object):
    """k streams stepped together on one GPU: `FrontendEngine(n_streams=k)` -> `BatchedMSCKF(k)`.

    `datasets`: objects with `.imu` and `.stereo` iterables of the reference's message namedtuples
    (`euroc.EuRoCDataset` after `set_starttime`, or anything shaped like it).  `run()` returns one float64[n, 8]
    trajectory per stream in the reference's output-line layout (msckf.py:152-158: t = imu_state.timestamp).
    `on_step(step, timestamps, ids, uv, n_feat, out)` -- optional, called once per step with the published feature
    arrays of the front-end and the filter's float64[k, 12] output of the same step (parity tests); without it the
    filter runs one step behind the front-end (queued), the way bench.py pipelines them.
    odom_cov=True: every step also brings the odometry covariance of what it publishes (BatchedMSCKF(odom_cov=True)); after `run`,
    `cov_rows[s]` is float64[n, 121], one row `t` + the 120-double record per row of stream s's trajectory.
    landmark_cap > 0: every step also brings its landmark records (BatchedMSCKF(landmarks=True, landmark_cap=)); after `run`,
    `lm_rows[s]` is (float64[n] pose times, LANDMARK_DTYPE[n] records, records dropped to the cap) of stream s.
    innovation=True: every step also brings its innovation statistics (BatchedMSCKF(stats=True)); after `run`, `nis_rows[s]` is
    (float64[n] pose times, FILTER_STATS_DTYPE[n, 2] records), one per row of stream s's trajectory.
    imu_rate_cap > 0: every step also brings its IMU-rate records (BatchedMSCKF(imu_rate=True, imu_rate_cap=)); after `run`,
    `ir_rows[s]` is (float64[n, 14] lines `t p q v w` -- the records of every publishing step, then that step's published pose with the
    w of its last record --, records among them, records dropped to the cap) of stream s."""

    def __init__(self, config, n_streams, device=0, rows_cap=None, odom_cov=False, landmark_cap=0, innovation=False, imu_rate_cap=0):
        from .frontend import FrontendEngine
        from .msckf_ops import BatchedMSCKF
        self.config, self.S, self.device = config, int(n_streams), int(device)
        self.eng = FrontendEngine(config, n_streams=self.S, device=self.device)
        self.odom_cov = bool(odom_cov)
        self.landmark_cap = int(landmark_cap)
        self.flt = BatchedMSCKF(config, self.S, device=self.device, rows_cap=rows_cap, max_features=self.eng.max_features, odom_cov=self.odom_cov,
                                landmarks=self.landmark_cap > 0, landmark_cap=max(1, self.landmark_cap), stats=bool(innovation),
                                imu_rate=int(imu_rate_cap) > 0, imu_rate_cap=max(1, int(imu_rate_cap)), zupt=bool(getattr(config, 'use_zupt', False)))
        self.zupt_totals = None                           # config.use_zupt: after `run`, int64[S, 2] (detected_total, applied_total) of every stream
        self.imu_rate_cap = int(imu_rate_cap)
        self.ir_rows = None
        self.innovation = bool(innovation)
        self.nis_rows = None
        self.cov_rows = None
        self.lm_rows = None
        self.frames_done = np.zeros(self.S, np.int64)
        self._fstream = None
        self.plan, self.steps_done, self.times = None, 0, None

    def close(self):
        self.eng.close(); self.flt.close()

    def run(self, datasets, max_frames=None, on_step=None, host_threads=16, share_frames=True):
        """share_frames (datasets that list their files): every distinct frame is decoded, uploaded, pyramided and FAST-scanned
        once and kept in the engine's device frame store while any stream still reads it (`euroc.SharedFramePlan`); finished
        streams launch nothing.  False: round 4's per-stream staging (`euroc.FrameStager`), kept for A/B measurements."""
        from .euroc import FrameStager, SharedFramePlan, SharedFrameStager
        staged = all(hasattr(d, 'stereo_files') for d in datasets)
        self.plan = None
        stager = None
        # config.exposure_reference: the exposure of every frame comes from the sequences' times.txt (euroc.ExposureTimes), read -- and
        # checked for every frame of the run -- before the first step; without the setting the files are never opened
        self.times = None
        if self.eng.exposure:
            from .euroc import ExposureTimes
            if not staged:
                raise ValueError('config.exposure_reference needs datasets that list their files (mav0/cam*/times.txt are matched to them by name)')
            self.times = ExposureTimes().check(datasets, max_frames)
        if staged and share_frames:
            self.plan = SharedFramePlan(datasets, max_frames=max_frames)
            self.eng.frames_reserve(self.plan.n_slots)
            stager = SharedFrameStager(self.plan, self.eng.input_height, self.eng.input_width, threads=host_threads, pixel_format=self.eng.pixel_format)
        elif staged:
            stager = FrameStager(datasets, self.eng.input_height, self.eng.input_width, max_frames=max_frames, threads=host_threads, pixel_format=self.eng.pixel_format)
        elif self.eng.pixel_format != 0:
            raise ValueError('datasets that do not list their files are read as 8-bit grey frames: config.image_format must be gray8')
        try:
            return self._run(datasets, stager, max_frames, on_step)
        finally:
            if stager is not None:
                stager.close()

    def _run(self, datasets, stager, max_frames, on_step):
        S = self.S
        assert len(datasets) == S
        eng, flt = self.eng, self.flt
        plan = self.plan
        staged = stager is not None
        # frames: decoded ahead on host threads when the datasets list their files (reference: the reader threads of
        # streaming/dataset.py:93-158); any other dataset-shaped object is read through `.stereo`
        its_img = None if staged else [iter(d.stereo) for d in datasets]
        # IMU: datasets that hold their samples as one array (EuRoCDataset) are sliced per frame; others are iterated
        arr = [getattr(d, '_imu', None) if hasattr(d, 'starttime') else None for d in datasets]
        pos = [0 if a is None else int(np.searchsorted(a[:, 0], d.starttime, 'left')) for a, d in zip(arr, datasets)]
        its_imu = [iter(d.imu) if a is None else None for a, d in zip(arr, datasets)]
        pend = [None if it is None else next(it, None) for it in its_imu]
        img0 = np.zeros((S, eng.input_height, eng.input_width), np.uint8) if plan is None else None
        img1 = np.zeros_like(img0) if plan is None else None
        traj = [[] for _ in range(S)]
        last_t = np.zeros(S)
        inflight = []                                     # outputs of submitted steps that have not been recorded yet
        dev = flt.device_resident()

        covs = [[] for _ in range(S)]
        want = True if self.odom_cov else None

        lms = [[[], [], 0] for _ in range(S)]             # per stream: pose times, record arrays, records dropped to the cap
        want_lm = True if self.landmark_cap > 0 else None

        nis = [[[], []] for _ in range(S)]                # per stream: pose times, the step's two blocks
        want_nis = True if self.innovation else None

        irs = [[[], 0, 0] for _ in range(S)]              # per stream: lines `t p q v w`, records among them, records dropped to the cap
        want_ir = True if self.imu_rate_cap > 0 else None

        def record(out, cov=None, lm=None, fst=None, ir=None):
            for s in np.nonzero(out[:, 0] > 0.5)[0]:
                traj[s].append(out[s, 1:9].copy())
                if ir is not None:                        # the step's records, then its published pose (the update's correction lies between)
                    rec = ir[0][s, :ir[1][s, 1]]
                    rows = np.full((len(rec) + 1, 14), np.nan)
                    rows[:-1] = rec.view(np.float64).reshape(len(rec), 14)
                    rows[-1, :11] = out[s, 1:12]
                    if len(rec):
                        rows[-1, 11:] = rec['w'][-1]
                    irs[s][0].append(rows); irs[s][1] += len(rec); irs[s][2] += int(ir[1][s, 0] - ir[1][s, 1])
                if cov is not None:
                    covs[s].append(np.concatenate([out[s, 1:2], cov[s]]))
                if lm is not None and lm[1][s, 1] > 0:
                    rec = lm[0][s, :lm[1][s, 1]].copy()
                    lms[s][0].append(np.full(len(rec), out[s, 1])); lms[s][1].append(rec)
                if lm is not None:
                    lms[s][2] += int(lm[1][s, 0] - lm[1][s, 1])
                if fst is not None:
                    nis[s][0].append(out[s, 1]); nis[s][1].append(fst[s].copy())

        times, t_ref = self.times, getattr(eng, '_exposure_ref', None)

        def upload(k):                                    # the new frames of step k, each with the exposures of its own two files
            kw = {} if times is None else dict(exposure=([times.of(e[1]) for e in plan.new[k]], [times.of(e[2]) for e in plan.new[k]]))
            eng.frames_upload(*stager.get(k), **kw)

        if plan is not None and plan.n_steps:
            upload(0)
        step = 0
        while True:
            if plan is not None:
                if step >= plan.n_steps:
                    break
                if step + 1 < plan.n_steps:               # the NEXT step's new frames go up before this step is enqueued: copy,
                    upload(step + 1)                      # pyramids and FAST of step k+1 run beside the kernels of step k
                frame_ts = plan.ts[step]
            elif staged:
                nxt = stager.next()
                if nxt is None:
                    break
                frame_ts, img0, img1 = nxt
            else:
                msgs = [next(it, None) for it in its_img] if (max_frames is None or step < max_frames) else [None] * S
                if all(m is None for m in msgs):
                    break
                frame_ts = np.array([-1.0 if m is None else m.timestamp for m in msgs])
                for s, m in enumerate(msgs):
                    if m is None:
                        its_img[s] = iter(())
                        img0[s] = 0; img1[s] = 0
                    else:
                        img0[s] = m.cam0_image; img1[s] = m.cam1_image
            ts_f = np.full(S, -1.0)                       # the filter's frame times: < 0 = no frame for this stream
            ts_e = np.empty(S)
            idx, tt, gy, ac = [], [], [], []
            for s in range(S):
                if frame_ts[s] < 0:                       # finished: idles (shared store: launches nothing) until the longest stream ends
                    last_t[s] += 0.05
                    ts_e[s] = last_t[s]
                    continue
                t = float(frame_ts[s])
                ts_f[s] = ts_e[s] = last_t[s] = t
                self.frames_done[s] += 1
                a = arr[s]
                if a is not None:                         # SURVEY 3.5 / vio.py:43-44: every IMU message with timestamp <= t first
                    e = int(np.searchsorted(a[:, 0], t, 'right'))
                    if e > pos[s]:
                        idx.append(np.full(e - pos[s], s, np.int32)); tt.append(a[pos[s]:e, 0]); gy.append(a[pos[s]:e, 1:4]); ac.append(a[pos[s]:e, 4:7])
                        pos[s] = e
                else:
                    n0 = len(tt)
                    while pend[s] is not None and pend[s].timestamp <= t:
                        tt.append(np.array([pend[s].timestamp])); gy.append(np.asarray(pend[s].angular_velocity, np.float64).reshape(1, 3))
                        ac.append(np.asarray(pend[s].linear_acceleration, np.float64).reshape(1, 3))
                        pend[s] = next(its_imu[s], None)
                    if len(tt) > n0:
                        idx.append(np.full(len(tt) - n0, s, np.int32))
            if idx:
                idx, tt, gy, ac = np.concatenate(idx), np.concatenate(tt), np.concatenate(gy), np.concatenate(ac)
                eng.push_imu_batch(idx, tt, gy)
                flt.push_imu(idx, tt, gy, ac)
            if plan is not None:
                eng.step_frames(plan.slots[step], ts_e)
            elif times is not None:                       # (a finished stream idles on blank images at the reference exposure)
                fl = stager.last_files
                eng.step_host(img0, img1, ts_e, exposure=([t_ref if f is None else times.of(f[0]) for f in fl], [t_ref if f is None else times.of(f[1]) for f in fl]))
            else:
                eng.step_host(img0, img1, ts_e)
            if on_step is not None:
                ids, uv, n = eng.read_features_raw()
                n[ts_f < 0] = 0
                out = flt.step(ids, uv, n, ts_f, cov=want, landmarks=want_lm, stats=want_nis, imu_states=want_ir)
                record(out, flt.last_cov, flt.last_landmarks, flt.last_stats, flt.last_imu_states)
                on_step(step, ts_f, ids, uv, n, out)
            elif dev:
                # the filter reads the published message where it lies on the device; nothing of this step is waited for here:
                # the next frames are decoded, uploaded and tracked while the filter's groups work through their queues
                # (a stream without a frame carries timestamp -1: its message is ignored)
                import torch
                from . import _native as N
                if self._fstream is None:
                    self._fstream = torch.cuda.Stream(device=self.device)
                ms = N.current_stream()                   # the stream the front-end's step was enqueued on
                with torch.cuda.stream(self._fstream):    # the filter's kernels (one group: here) overlap the next frame's front-end
                    inflight.append((flt.submit_dev(eng, ts_f, msg_stream=ms, cov=want, landmarks=want_lm, stats=want_nis, imu_states=want_ir),
                                     flt.last_cov, flt.last_landmarks, flt.last_stats, flt.last_imu_states))
                flt.wait(2)
                while len(inflight) > 2:
                    record(*inflight.pop(0))
            else:
                eng.read_features_begin(step & 1)
                ids, uv, n = eng.read_features_end(step & 1)
                n[ts_f < 0] = 0
                inflight.append((flt.submit(ids, uv, n, ts_f, cov=want, landmarks=want_lm, stats=want_nis, imu_states=want_ir),
                                 flt.last_cov, flt.last_landmarks, flt.last_stats, flt.last_imu_states))
                flt.wait(1)                               # at most one step behind: the next frames are decoded meanwhile
                while len(inflight) > 1:
                    record(*inflight.pop(0))
            step += 1
        flt.wait(0)
        for pair in inflight:
            record(*pair)
        self.steps_done = step
        if flt.zupt is not None:
            z = flt.read_zupt()
            self.zupt_totals = np.stack([z['detected_total'], z['applied_total']], axis=1).astype(np.int64)
        self.cov_rows = [np.array(c, dtype=np.float64).reshape(-1, 121) for c in covs] if self.odom_cov else None
        if self.landmark_cap > 0:
            from .msckf_ops import LANDMARK_DTYPE
            self.lm_rows = [(np.concatenate(t) if t else np.zeros(0), np.concatenate(r) if r else np.zeros(0, LANDMARK_DTYPE), d) for t, r, d in lms]
        if self.innovation:
            from .msckf_ops import FILTER_STATS_DTYPE
            self.nis_rows = [(np.array(t, dtype=np.float64), np.array(r, dtype=FILTER_STATS_DTYPE).reshape(-1, 2)) for t, r in nis]
        if self.imu_rate_cap > 0:
            self.ir_rows = [(np.concatenate(r) if r else np.zeros((0, 14)), n, d) for r, n, d in irs]
        return [np.array(t, dtype=np.float64).reshape(-1, 8) for t in traj]


def run_batched(config, dataset_paths, offsets, device=0, max_frames=None, on_step=None, rows_cap=None, share_frames=True, stats=None, cov_rows=None, lm_rows=None, landmark_cap=64, nis_rows=None,
                ir_rows=None, imu_rate_cap=32, zupt_rows=None):
    """Open (path, offset) pairs as EuRoC datasets and run them as one batch; returns (trajectories, datasets).
    zupt_rows (a list; config.use_zupt): receives, per stream, (detected_total, applied_total) of the zero-velocity update.
    cov_rows (a list): the batch runs with the odometry covariance on and the list receives, per stream, float64[n, 121] rows `t` + record.
    lm_rows (a list): the batch runs with the landmark map on (landmark_cap records per stream and step) and the list receives, per
    stream, (pose times float64[n], records LANDMARK_DTYPE[n], records dropped to the cap).
    nis_rows (a list): the batch runs with the innovation statistics on and the list receives, per stream, (pose times float64[n], records
    FILTER_STATS_DTYPE[n, 2]).
    ir_rows (a list): the batch runs with the IMU-rate odometry on (the last imu_rate_cap records per stream and step) and the list
    receives, per stream, (lines float64[n, 14] `t p q v w`, records among them, records dropped to the cap).
    stats (a dict) receives the batch's stream-frames, steps, distinct frames decoded and the seconds its stepping loop took."""
    import time
    from .euroc import EuRoCDataset
    dss = []
    for p, o in zip(dataset_paths, offsets):
        ds = EuRoCDataset(p)
        ds.set_starttime(o)
        dss.append(ds)
    r = BatchedRunner(config, len(dss), device=device, rows_cap=rows_cap, odom_cov=cov_rows is not None, landmark_cap=landmark_cap if lm_rows is not None else 0,
                      innovation=nis_rows is not None, imu_rate_cap=imu_rate_cap if ir_rows is not None else 0)
    try:
        t0 = time.perf_counter()
        trajs = r.run(dss, max_frames=max_frames, on_step=on_step, share_frames=share_frames)
        if cov_rows is not None:
            cov_rows.extend(r.cov_rows)
        if lm_rows is not None:
            lm_rows.extend(r.lm_rows)
        if nis_rows is not None:
            nis_rows.extend(r.nis_rows)
        if ir_rows is not None:
            ir_rows.extend(r.ir_rows)
        if zupt_rows is not None and r.zupt_totals is not None:
            zupt_rows.extend((int(d), int(a)) for d, a in r.zupt_totals)
        if stats is not None:
            stats['seconds'] = stats.get('seconds', 0.0) + time.perf_counter() - t0
            stats['stream_frames'] = stats.get('stream_frames', 0) + int(r.frames_done.sum())
            stats['steps'] = stats.get('steps', 0) + int(r.steps_done)
            stats['frames_decoded'] = stats.get('frames_decoded', 0) + (r.plan.n_frames_distinct if r.plan is not None else int(r.frames_done.sum()))
            stats['store_entries'] = max(stats.get('store_entries', 0), r.plan.n_slots if r.plan is not None else 0)
    finally:
        r.close()
    return trajs, dss


def batch_pixel_format(dataset_paths, choice='gray8'):
    """The config.image_format of one batch of sequences for --pixel-format `choice`.  'auto' probes the header of the first cam0 file
    of every sequence (av_png_probe); all sequences of a batch must agree, since one engine reads one format: ValueError otherwise."""
    if choice != 'auto':
        return choice
    from .euroc import EuRoCDataset, probe_png
    found = {}
    for p in dataset_paths:
        if p in found:
            continue
        files = EuRoCDataset._list_images(os.path.join(p, 'mav0', 'cam0', 'data'))[0]
        if not files:
            raise ValueError('--pixel-format auto: %s has no cam0 frames to probe' % p)
        fmt = probe_png(files[0])[2]
        if fmt is None:
            raise ValueError('--pixel-format auto: %s is a PNG flavour the decoder does not take (8 / 16-bit grey, RGB, RGBA are)' % files[0])
        found[p] = fmt
    if len(set(found.values())) > 1:
        raise ValueError('--pixel-format auto: the sequences of one batch must share one pixel format, found ' +
                         ', '.join('%s: %s' % (os.path.basename(os.path.normpath(p)), f) for p, f in found.items()))
    return next(iter(found.values()))


BAYER_FORMATS = ['bayer_%s%d' % (p, b) for b in (8, 16) for p in ('rggb', 'bggr', 'grbg', 'gbrg')]


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', help='directory holding the EuRoC sequences')
    ap.add_argument('--make-synthetic', metavar='DIR', help='first write EuRoC-layout synthetic sequences (one per --sequences name) into DIR and use it as --root')
    ap.add_argument('--frames', type=int, default=200, help='frames per synthetic sequence (--make-synthetic)')
    ap.add_argument('--sequences', nargs='+', required=True)
    ap.add_argument('--offsets', nargs='+', type=float, default=[0.0])
    ap.add_argument('--max-frames', type=int, default=None)
    ap.add_argument('--batch', type=int, default=64, help='streams stepped together per GPU (larger sweeps run in several batches)')
    ap.add_argument('--grid', nargs=3, type=int, default=None, metavar=('ROWS', 'COLS', 'MAX'), help='feature grid (default 4 5 5; 10 15 10 = the 1500-feature sweep)')
    ap.add_argument('--out', default='results/txts')
    ap.add_argument('--no-share-frames', action='store_true', help="round 4's per-stream staging instead of the shared frame store (A/B)")
    ap.add_argument('--covariance', action='store_true',
                    help='also write, next to every trajectory file, output_<sequence>_offset<o>_cov.txt: per published pose one line `t` + the 120 numbers of its '
                         'odometry covariance (upper triangle of the 15 x 15 matrix over p, theta, v, p_c, theta_c; include/airvision.h); with ground truth the '
                         'report gains anees_pos, the mean normalised position error squared (3 for a consistent filter)')
    ap.add_argument('--landmarks', action='store_true',
                    help='also write, next to every trajectory file, output_<sequence>_offset<o>_map.txt: the landmark records of every step, one line '
                         '`t id x y z flags n_obs` each (t = the time of the pose of the step; include/airvision.h, "Landmark map"); the report states how many '
                         'records were dropped to the cap')
    ap.add_argument('--innovation', action='store_true',
                    help='also write, next to every trajectory file, output_<sequence>_offset<o>_nis.txt: per published pose one line `t` + the sixteen integers '
                         'and eight doubles of its two innovation-statistics blocks (lost-feature update, pruning update; include/airvision.h, "Innovation '
                         'statistics"); the report of every stream gains nis_rows, the sum of gamma over the residual rows of all evaluated features '
                         '(near 1 for a consistent filter; needs no ground truth), and reject_rate, the share of evaluated features the gate rejected')
    ap.add_argument('--imu-rate', action='store_true',
                    help='also write, next to every trajectory file, output_<sequence>_offset<o>_imu.txt: the state after every IMU sample the filter '
                         'integrated, one line `t p q v w` each (p, q, v in the frame of the trajectory file, w the bias-corrected gyro in the IMU frame; '
                         'include/airvision.h, "IMU-rate odometry"), and after the records of every step the published pose of that step as one more line; '
                         'the report states the records dropped to the cap and, with ground truth, the ATE of this denser trajectory')
    ap.add_argument('--zupt', action='store_true',
                    help='zero-velocity update for streams at rest (config.use_zupt with the config\'s zupt_* thresholds); the report gains '
                         '"zupt": per stream the frames detected at rest and the updates applied')
    ap.add_argument('--imu-rate-cap', type=int, default=32, metavar='N', help='--imu-rate: records per stream and step, the last N samples (default 32, at most 4096)')
    ap.add_argument('--landmark-cap', type=int, default=64, metavar='N', help='--landmarks: records per stream and step (default 64)')
    ap.add_argument('--ransac', action='store_true', help='two-point RANSAC outlier rejection on the tracked features (config.use_ransac; off = the reference front-end)')
    ap.add_argument('--ransac-threshold', type=float, default=None, metavar='T', help='inlier error in pixels (config.ransac_threshold, default 3)')
    ap.add_argument('--clahe', action='store_true', help='equalise every frame (CLAHE) ahead of the pyramids, LK and FAST (config.use_clahe; off = the reference front-end)')
    ap.add_argument('--clahe-clip', type=float, default=None, metavar='C', help='clip limit (config.clahe_clip_limit, default 2.0; 0 = no clipping)')
    ap.add_argument('--clahe-tiles', nargs=2, type=int, default=None, metavar=('X', 'Y'), help='tile grid (config.clahe_tiles, default 8 8)')
    ap.add_argument('--pixel-format', choices=['gray8', 'gray16', 'rgb8', 'rgba8', 'auto'] + BAYER_FORMATS, default='gray8',
                    help='PNG flavour of the camera frames (config.image_format); auto = probe the first cam0 file of every sequence, which must agree within a batch.  '
                         'bayer_<pattern>8 / bayer_<pattern>16 (pattern = the colours of the top-left 2 x 2 block): the files are grey PNGs holding a raw Bayer mosaic, '
                         'demosaiced to grey on the GPU; auto never chooses a Bayer format, since a file cannot say that it is a mosaic')
    ap.add_argument('--downscale', type=int, choices=[1, 2, 4], default=None,
                    help='bin every frame f x f on the GPU ahead of CLAHE and the pyramids and run the front-end on the smaller image with the '
                         'calibration scaled to it (config.image_downscale, default 1 = off); the files stay full size')
    ap.add_argument('--mask0', metavar='PNG', default=None,
                    help='static mask of cam0 for every stream: an 8-bit grey PNG of the frame size, 0 = never scene (outside a fisheye image circle, airframe in view), '
                         'anything else = scene (config.cam0_mask; default: none)')
    ap.add_argument('--mask1', metavar='PNG', default=None, help='the same for cam1 (config.cam1_mask)')
    ap.add_argument('--response0', metavar='TXT', default=None,
                    help='photometric calibration of cam0 for every stream: a pcalib.txt-style text file of 256 numbers in [0, 255], the inverse response G^-1 '
                         '(config.cam0_response; default: none)')
    ap.add_argument('--response1', metavar='TXT', default=None, help='the same for cam1 (config.cam1_response)')
    ap.add_argument('--vignette0', metavar='PNG', default=None,
                    help='vignette map of cam0 for every stream: a 16-bit grey PNG of the frame size, normalised by its maximum; every pixel is divided by it on the GPU '
                         '(config.cam0_vignette; default: none)')
    ap.add_argument('--vignette1', metavar='PNG', default=None, help='the same for cam1 (config.cam1_vignette)')
    ap.add_argument('--exposure-reference', type=float, default=None, metavar='MS',
                    help='exposure-time normalisation: every frame is scaled by MS / its own exposure on the GPU, inside the photometric stage '
                         '(config.exposure_reference; default: off).  The exposures are read from mav0/cam0/times.txt and mav0/cam1/times.txt of every '
                         'sequence: one line per frame, <file stem> <timestamp in s> <exposure in ms>')
    ap.add_argument('--gray16-shift', type=int, default=None, metavar='N',
                    help='16-bit frames, grey or Bayer: sample = min(255, v >> N), 0 .. 8 (config.gray16_shift, default 8)')
    ap.add_argument('--gray16-scale', choices=['shift', 'window', 'auto'], default=None,
                    help="16-bit grey frames (--pixel-format gray16): 'shift' = the fixed shift, 'window' = --gray16-window mapped to 0 .. 255, 'auto' = a range per "
                         "stereo pair from the pair's own histogram on the GPU, for thermal and low-light sources (config.gray16_scale, default shift)")
    ap.add_argument('--gray16-window', type=int, nargs=2, default=None, metavar=('LO', 'HI'),
                    help='--gray16-scale window: 0 <= LO < HI <= 65535 (config.gray16_window)')
    ap.add_argument('--gray16-clip', type=int, nargs=2, default=None, metavar=('PPM_LO', 'PPM_HI'),
                    help='--gray16-scale auto: parts per million of samples that may saturate at the low / high end (config.gray16_auto_clip, default 100 100)')
    ap.add_argument('--gray16-min-span', type=int, default=None, metavar='N',
                    help='--gray16-scale auto: the smallest hi - lo of a range, 16 .. 65535 (config.gray16_auto_min_span, default 256)')
    return ap


def apply_args(cfg, args):
    """The command line's front-end switches on a config object."""
    cfg.use_ransac = bool(args.ransac)
    if args.ransac_threshold is not None:
        cfg.ransac_threshold = args.ransac_threshold
    cfg.use_clahe = bool(args.clahe)
    if args.clahe_clip is not None:
        cfg.clahe_clip_limit = args.clahe_clip
    if args.clahe_tiles is not None:
        cfg.clahe_tiles = (int(args.clahe_tiles[0]), int(args.clahe_tiles[1]))
    if getattr(args, 'pixel_format', 'gray8') != 'auto':          # auto: set per batch (batch_pixel_format)
        cfg.image_format = getattr(args, 'pixel_format', 'gray8')
    if getattr(args, 'gray16_shift', None) is not None:
        cfg.gray16_shift = args.gray16_shift
    for arg, attr in (('gray16_scale', 'gray16_scale'), ('gray16_window', 'gray16_window'), ('gray16_clip', 'gray16_auto_clip'), ('gray16_min_span', 'gray16_auto_min_span')):
        v = getattr(args, arg, None)                            # (a setting already on the config object stays unless the switch is given)
        if v is not None:
            setattr(cfg, attr, tuple(v) if isinstance(v, list) else v)
    if getattr(args, 'exposure_reference', None) is not None:      # (a reference already on the config object stays unless the switch is given)
        cfg.exposure_reference = float(args.exposure_reference)
    if getattr(args, 'downscale', None) is not None:          # (a factor already set on the config object stays unless the switch is given)
        cfg.image_downscale = int(args.downscale)
    for cam in (0, 1):                                         # (a mask already set on the config object stays unless the switch is given)
        if getattr(args, 'mask%d' % cam, None) is not None:
            setattr(cfg, 'cam%d_mask' % cam, getattr(args, 'mask%d' % cam))
        for part in ('response', 'vignette'):                  # (a table already set on the config object stays unless the switch is given)
            if getattr(args, '%s%d' % (part, cam), None) is not None:
                setattr(cfg, 'cam%d_%s' % (cam, part), getattr(args, '%s%d' % (part, cam)))
    if getattr(args, 'zupt', False):                          # (already on the config object: stays on)
        cfg.use_zupt = True
    return cfg


def main(argv=None):
    ap = make_parser()
    args = ap.parse_args(argv)

    import torch
    import torch.distributed as dist
    from . import shard
    from .config import ConfigEuRoC
    from .evaluate import ate, format_state_line, nees, rte
    from .msckf_ops import unpack_odom_cov
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    cfg = ConfigEuRoC(grid_row=args.grid[0], grid_col=args.grid[1], grid_max_feature_num=args.grid[2]) if args.grid else ConfigEuRoC()
    apply_args(cfg, args)
    root = args.root
    if args.make_synthetic:
        root = args.make_synthetic
        if rank == 0:
            from .euroc import write_euroc_layout
            from .synth import SyntheticStream
            for i, seq in enumerate(args.sequences):
                if not os.path.isdir(os.path.join(root, seq, 'mav0')):
                    write_euroc_layout(os.path.join(root, seq), SyntheticStream(cfg, seed=1000 + i, n_frames=args.frames, motion_scale=1.5, t0=1403636580.0 + 1000 * i, rest=1.0))
        if world > 1:
            dist.barrier()
    if not root:
        ap.error('--root or --make-synthetic is required')
    jobs = shard.broadcast_object([(s, o) for s in args.sequences for o in args.offsets] if rank == 0 else None)
    mine = shard.partition(len(jobs), world, rank)
    local_traj, local_cov, local_lm, local_nis, local_ir, report, stats = {}, {}, {}, {}, {}, {}, {}
    local_zupt = {}
    import time
    if world > 1:
        dist.barrier()
    t_all = time.perf_counter()
    for b0 in range(0, len(mine), args.batch):
        chunk = mine[b0:b0 + args.batch]
        cfg.image_format = batch_pixel_format([os.path.join(root, jobs[j][0]) for j in chunk], args.pixel_format)
        cov_rows = [] if args.covariance else None
        lm_rows = [] if args.landmarks else None
        nis_rows = [] if args.innovation else None
        ir_rows = [] if args.imu_rate else None
        zupt_rows = [] if cfg.use_zupt else None
        trajs, dss = run_batched(cfg, [os.path.join(root, jobs[j][0]) for j in chunk], [jobs[j][1] for j in chunk], device=local, max_frames=args.max_frames,
                                 share_frames=not args.no_share_frames, stats=stats, **({'cov_rows': cov_rows} if args.covariance else {}),
                                 **({'lm_rows': lm_rows, 'landmark_cap': args.landmark_cap} if args.landmarks else {}),
                                 **({'nis_rows': nis_rows} if args.innovation else {}),
                                 **({'ir_rows': ir_rows, 'imu_rate_cap': args.imu_rate_cap} if args.imu_rate else {}),
                                 **({'zupt_rows': zupt_rows} if zupt_rows is not None else {}))
        for i, (j, traj, ds) in enumerate(zip(chunk, trajs, dss)):
            local_traj[j] = traj
            if zupt_rows:
                local_zupt[j] = zupt_rows[i]
            if cov_rows is not None:
                local_cov[j] = cov_rows[i]
            if lm_rows is not None:
                local_lm[j] = lm_rows[i]
            if ir_rows is not None:
                local_ir[j] = ir_rows[i]
            gt = ds.groundtruth_array()
            if len(gt) and len(traj) > 20:
                a, r = ate(traj, gt), rte(traj, gt)
                report[j] = dict(sequence=jobs[j][0], offset=jobs[j][1], frames=len(traj), ate_rmse=a['rmse'], ate_mean=a['mean'], rte_rmse=r['rmse'])
                if ir_rows is not None and len(ir_rows[i][0]) > 20:
                    report[j]['ate_rmse_imu_rate'] = ate(ir_rows[i][0], gt)['rmse']
                if cov_rows is not None:
                    report[j]['anees_pos'] = nees(traj, unpack_odom_cov(cov_rows[i][:, 1:])[:, 0:3, 0:3], gt)[1]
            if nis_rows is not None:                      # (needs no ground truth: a stream without one gets its report entry here)
                local_nis[j] = nis_rows[i]
                report.setdefault(j, dict(sequence=jobs[j][0], offset=jobs[j][1], frames=len(traj))).update(innovation_summary(nis_rows[i][1]))
    elapsed = shard.max_over_ranks(time.perf_counter() - t_all)          # barrier before, max over ranks after: the bench contract's clock
    allt = shard.gather_trajectories(local_traj, len(jobs), world, rank)
    per_rank = shard.gather_objects({'rank': rank, 'streams': [jobs[j] for j in mine], 'report': report, 'stats': stats, 'cov': local_cov, 'lm': local_lm, 'nis': local_nis, 'ir': local_ir,
                                     'zupt': local_zupt})
    if rank == 0:
        os.makedirs(args.out, exist_ok=True)
        for j, (seq, off) in enumerate(jobs):
            with open(os.path.join(args.out, 'output_%s_offset%d.txt' % (seq, int(off))), 'w') as f:
                for row in allt[j]:
                    f.write(format_state_line(row[0], row[1:4], row[4:8]))
        for r in per_rank if args.covariance else []:
            for j, rows in r['cov'].items():
                with open(os.path.join(args.out, 'output_%s_offset%d_cov.txt' % (jobs[j][0], int(jobs[j][1]))), 'w') as f:
                    for row in rows:
                        f.write('%.6f ' % row[0] + ' '.join('%.9e' % v for v in row[1:]) + '\n')
        lm_dropped = {}
        for r in per_rank if args.landmarks else []:
            for j, (ts, recs, dropped) in r['lm'].items():
                lm_dropped[j] = (len(recs), int(dropped))
                with open(os.path.join(args.out, 'output_%s_offset%d_map.txt' % (jobs[j][0], int(jobs[j][1]))), 'w') as f:
                    for t, rec in zip(ts, recs):
                        f.write('%.6f %d %.9f %.9f %.9f %d %d\n' % (t, rec['id'], rec['p'][0], rec['p'][1], rec['p'][2], rec['flags'], rec['n_obs']))
        for r in per_rank if args.innovation else []:
            for j, (ts, recs) in r['nis'].items():
                with open(os.path.join(args.out, 'output_%s_offset%d_nis.txt' % (jobs[j][0], int(jobs[j][1]))), 'w') as f:
                    for t, rec in zip(ts, recs):
                        f.write(format_nis_line(t, rec))
        ir_counts = {}
        for r in per_rank if args.imu_rate else []:
            for j, (rows, n_rec, dropped) in r['ir'].items():
                ir_counts[j] = (int(n_rec), int(dropped), len(rows))
                with open(os.path.join(args.out, 'output_%s_offset%d_imu.txt' % (jobs[j][0], int(jobs[j][1]))), 'w') as f:
                    for row in rows:
                        f.write('%.6f ' % row[0] + ' '.join('%.9f' % v for v in row[1:]) + '\n')
        rep = sweep_report(jobs, per_rank, elapsed, world)
        if args.imu_rate:
            rep['imu_rate'] = dict(cap=args.imu_rate_cap, records=[ir_counts.get(j, (0, 0, 0))[0] for j in range(len(jobs))],
                                   dropped_to_cap=[ir_counts.get(j, (0, 0, 0))[1] for j in range(len(jobs))],
                                   lines=[ir_counts.get(j, (0, 0, 0))[2] for j in range(len(jobs))])
        if args.landmarks:
            rep['landmarks'] = dict(cap=args.landmark_cap, records=[lm_dropped.get(j, (0, 0))[0] for j in range(len(jobs))],
                                    dropped_to_cap=[lm_dropped.get(j, (0, 0))[1] for j in range(len(jobs))])
        if cfg.use_zupt:
            zt = {}
            for r in per_rank:
                zt.update(r['zupt'])
            rep['zupt'] = dict(detected_total=[zt.get(j, (0, 0))[0] for j in range(len(jobs))], applied_total=[zt.get(j, (0, 0))[1] for j in range(len(jobs))])
        if cfg.use_clahe:
            rep['clahe'] = dict(clip_limit=cfg.clahe_clip_limit, tiles=list(cfg.clahe_tiles))
        if args.pixel_format != 'gray8':
            rep['pixel_format'] = dict(asked=args.pixel_format, last_batch=cfg.image_format, gray16_shift=cfg.gray16_shift)
        if getattr(cfg, 'gray16_scale', 'shift') != 'shift':
            rep['gray16_scale'] = dict(scale=cfg.gray16_scale, window=cfg.gray16_window, clip=list(cfg.gray16_auto_clip), min_span=cfg.gray16_auto_min_span)
        if getattr(cfg, 'image_downscale', 1) != 1:
            rep['downscale'] = cfg.image_downscale
        if args.mask0 is not None or args.mask1 is not None:
            rep['masks'] = dict(mask0=args.mask0, mask1=args.mask1)
        # every table the sweep ran with, from a switch or already on the config object: its file, or 'array' for one given as values
        photo = {k: getattr(cfg, 'cam%s_%s' % (k[-1], k[:-1]), None) for k in ('response0', 'response1', 'vignette0', 'vignette1')}
        photo = {k: (os.fspath(v) if isinstance(v, (str, os.PathLike)) else 'array') for k, v in photo.items() if v is not None}
        if photo:
            rep['photometric'] = photo
        if getattr(cfg, 'exposure_reference', None) is not None:
            rep['exposure_reference'] = float(cfg.exposure_reference)
        print(json.dumps(rep))
    if world > 1:
        dist.destroy_process_group()


def format_nis_line(t, rec):
    """One line of an _nis file: `t`, then the eight integers of both blocks (lost-feature update first), then the four doubles of both."""
    from .msckf_ops import _FS_DOUBLES, _FS_INTS
    return '%.6f ' % t + ' '.join('%d' % rec[b][n] for b in range(2) for n in _FS_INTS) + ' ' + \
        ' '.join('%.17g' % rec[b][n] for b in range(2) for n in _FS_DOUBLES) + '\n'


def innovation_summary(recs):
    """Run-wide figures of one stream from its records FILTER_STATS_DTYPE[n, 2]: nis_rows = sum of gamma_eval / sum of the evaluated
    features' residual rows, reject_rate = 1 - sum of n_pass / sum of n_eval, both over the two updates of every pose (None: nothing evaluated)."""
    from .msckf_ops import filter_stats_rows
    rows = int(filter_stats_rows(recs)[0].sum()) if len(recs) else 0
    n_eval = int(recs['n_eval'].sum()) if len(recs) else 0
    return dict(nis_rows=float(recs['gamma_eval'].sum()) / rows if rows > 0 else None,
                reject_rate=1.0 - int(recs['n_pass'].sum()) / n_eval if n_eval > 0 else None)


def sweep_report(jobs, per_rank, elapsed, world):
    """ONE line for the whole sweep (BASELINE configs[3] / [4]: "aggregate frames/sec + per-seq ATE"): the stream-frames of all
    ranks over the slowest rank's wall time, and every (sequence, offset) stream's ATE / RTE in job order."""
    rep = {}
    for r in per_rank:
        rep.update(r['report'])
    tot = {k: sum(r['stats'].get(k, 0) for r in per_rank) for k in ('stream_frames', 'steps', 'frames_decoded')}
    return {'metric': 'stream-frames/s of the sequence x offset sweep (decode + front-end + MSCKF, end to end)',
            'value': tot['stream_frames'] / elapsed if elapsed > 0 else None, 'unit': 'stereo frames/s', 'n_gpus': world,
            'streams': [list(j) for j in jobs], 'stream_frames': tot['stream_frames'], 'frames_decoded': tot['frames_decoded'], 'seconds': elapsed,
            'streams_per_rank': [len(r['streams']) for r in per_rank],
            'stepping_seconds_per_rank': [r['stats'].get('seconds', 0.0) for r in per_rank],
            'report': [dict(rep[j]) if j in rep else dict(sequence=jobs[j][0], offset=jobs[j][1], frames=0) for j in range(len(jobs))]}


if __name__ == '__main__':
    main()
