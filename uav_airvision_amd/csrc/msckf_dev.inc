// msckf_dev.inc -- the batched filter with its WHOLE state resident on the device (included at the end of msckf.hip).
//
// What msckf_batch.inc keeps on the host -- the IMU state and the camera states (msckf.py:18-91), the observation map
// (map_server, msckf.py:120), add_feature_observations (:425-441), the selections of remove_lost_features (:614-640) and
// prune_cam_state_buffer (:736-757), find_redundant_cam_states (:678-709), the state injection of measurement_update
// (:568-595), publish / online_reset (:821-867) -- lives here in HBM and is stepped by kernels.  A step of a stream group is one
// fixed sequence of launches with NO host decision and NO device-to-host traffic inside it; the only read-back is the
// published pose of every stream at the end (12 doubles), so the host can queue the next step while this one runs.
//
//   dk_predict   per stream: gravity/bias initialisation record, batch_imu_processing + predict_new_state (RK4, one thread),
//                process_model covariance propagation, state_augmentation
//   dk_append    per stream: add_feature_observations into the frame-major store (msckf_store.h), tracking_rate, lost-feature
//                selection in dict order, their observation CSR / row offsets / launch buckets, deletion of the lost features
//   triangulate_kernel, feature_kernel<16|64|256> (length buckets), upd_stack_kernel, [compression], the back end  -- msckf.hip,
//                driven by device-side lists and counts
//   dk_mid       per stream: state injection of the lost-feature update, find_redundant_cam_states, pruning candidates (features
//                seen from both cameras, dict order), their CSR
//   ... the same chain for the pruning update ...
//   dk_finish    per stream: injection, removal of the two camera states (covariance rows/columns, frames, links), online
//                reset, publish
//   dk_finish_cov  (instead of dk_finish when av_msckf_batch_set_odom_cov is on) the same, and between the publish and the reset the
//                stream's odometry-covariance record (120 doubles), read back next to the pose
//   dk_mid_lm, dk_finish_lm, dk_finish_cov_lm  (instead of dk_mid / dk_finish / dk_finish_cov when av_msckf_batch_set_landmarks is on)
//                the same, and the stream's landmark records: the lost-feature update's ahead of dk_mid's rebuild of the per-phase
//                feature arrays, the pruning update's ahead of dk_finish's camera removal
//   dk_mid_st, dk_mid_lm_st, dk_finish_st, dk_finish_cov_st, dk_finish_lm_st, dk_finish_cov_lm_st  (instead of the six above when
//                av_msckf_batch_set_stats is on) the same, and the stream's innovation statistics of the update that has just run
//   dk_imu_rate  (behind dk_state, the state half of dk_predict, when av_msckf_batch_set_imu_rate is on) per stream: the state after every
//                IMU sample of the frame, gathered from the records dk_state leaves for dk_cov
//   dk_forecast_state, dk_forecast_cov  (behind dk_finish*, when av_msckf_batch_set_forecast is on) per stream: the state the step leaves,
//                carried through the IMU samples the step has NOT consumed, with the covariance of its IMU block; read-only for the filter
//   dk_zupt_detect, dk_zupt_update  (behind dk_cov / behind dk_finish*, when av_msckf_batch_set_zupt is on) per stream: is the stream at rest in
//                this step (IMU samples and the tracks of the appended frame), and if so a velocity = 0 measurement update on the state the step leaves
//
// Per-stream capacity failures are recorded in the stream's state (DState::failed) and stop that stream only.

namespace {

constexpr int DEV_BUCKETS = 2;          // launch buckets of the lost-feature phase (track length <= 8 / longer)
constexpr int DEV_IMU_BATCH = 16;          // IMU samples whose state integration runs ahead of their covariance steps (a frame holds ~10)
constexpr int DEV_LDS_KEYS = 2048;     // sort keys of a stream's candidate list live in LDS up to this message capacity (16 KB)

enum { DFAIL_NONE = 0, DFAIL_CAMS = 1, DFAIL_FRAMES = 2, DFAIL_STACK = 3, DFAIL_PIVOT = 4, DFAIL_TABLE = 5, DFAIL_OBS = 6, DFAIL_ROWS = 7 };

struct DState {                      // IMUState of one stream (msckf.py:18-58) + the step's flags
    double ts;                       // imu_state.timestamp: time of the last IMU sample applied
    double q[4], p[3], v[3], bg[3], ba[3];
    double R_ic[9], t_ci[3];
    double qn[4], pn[3], vn[3];      // orientation_null, position_null, velocity_null
    double gravity[3];
    double tracking_rate;
    long long next_imu_id;
    int n, ncam;
    int active;                      // this step: the stream takes part
    int failed;                      // DFAIL_*: the stream is stopped
    int first_img, null_aliased;
    int prune, rm0, rm1;             // this step: camera pruning runs; window positions of the two camera states that go
    int n_prune_steps;               // counter: steps that ran the camera pruning
    int n_two_pass;                  // counter: lost-feature phases gated in two passes
    int resets;                      // counter: online resets
};
struct DCtl {                        // host -> device, per stream and step
    double t_frame;                  // frame timestamp, < 0: no frame for this stream
    double q0[4], bg0[3], g0[3];     // initialize_gravity_and_bias results (has_init)
    int active, has_init, imu_first, imu_cnt;
};
struct DImu { double t, w[3], a[3]; };
// what dk_begin's state integration leaves for the covariance kernel of the same step (dk_cov): the samples' records are a.prop[first .. first + cnt)
struct DCov { int act, cnt, first, pad; AugArgs aa; };

// everything the dk_* kernels need, by value
struct DevArgs {
    int S, cap, FS, cs, max_cam, ld, rows_cap, obs_stride;
    unsigned long long* prof;        // diagnostic phase stamps of stream 0's workgroups (AV_DEV_UPROF=1), NULL otherwise
    int pool_rows;                   // rows of the overflow pool behind stream S - 1's block-buffer region (msckf_batch.inc: b_pool_rows)
    size_t pstride;
    double* P; double* scratch;
    DState* st; long long* cam_id; double* cam_q; double* cam_p; double* cam_qn; int* ncam; int* nstate; double* grav;
    // observation store, per-stream strides derived from cap / mcap / ns / hcells
    int mcap, ns, hcells;
    long long* fr_id; double* fr_z; int* fr_fslot; int* fr_prev; int* fr_next; int* fr_n; int* pos_of; int* order; int* hdr; long long* births;
    long long* m_id; long long* m_birth; double* m_pos; int* m_init; int* m_nobs; int* m_tail; int* free_stack;
    int* hash_a; int* hash_b; int* hash_c; int* tmp_a; int* tmp_b; int* tmp_c; unsigned long long* keys; int* cand; int* e0; int* e1;
    // per-phase feature arrays (feature f of stream s: s * FS + k)
    int* f_off; int* obs_cam; double* obs_z; double* f_pos; int* f_dof; int* f_rowoff; int* f_valid; int* f_mslot; int* n_cand; int* over;
    int* t_off; int* t_obs_cam; double* t_obs_z;      // triangulation CSR of the pruning phase (all observations of the feature)
    int* blist; int* tlist; int* cnt; int* cnt_next;   // [5][S*cap] bucket lists, [S*cap] triangulation list, [16] counters (8 per phase) of this step / of the next one
    const int* stacked; const double* dx;              // results of the update just run (dk_mid: lost features, dk_finish: pruning)
    // inputs of the step
    const DCtl* ctl; const DImu* imu; const long long* msg_ids; const double* msg_uv; const int* msg_n; int msg_cap;
    PropArgs* prop; DCov* cov;                        // dk_begin -> dk_cov: one record per IMU sample (indexed like imu), one per stream
    double* out;                                       // [S][12]
    double R01[9], t01[3], noise[4], cov0[5];
    double trans_thr, pos_std_thr;
    // dk_begin triangulates the lost features itself (dev_triangulate_own)
    double huber, precision, damping; int outer_max, inner_max;
    double* Hblk; double* rblk; size_t hstride, rstride; const double* chi2; double obs_noise; double* gamma; int* pass;
    const UpdArgs* updbase; UpdArgs* upd; int* cols; int cols_stride; int* blk_row; int* blk_len; int* stacked_out; double* work;
};

// triangulate_kernel's arguments for the candidates of one phase: lost features from their own CSR, pruning candidates from the
// t_* CSR (all observations of the feature) with the position stored in the stream's feature table
__device__ __forceinline__ TriArgs dev_tri_args(const DevArgs& a, bool prune)
{
    TriArgs t;
    t.n_feat = 0; t.obs_off = prune ? a.t_off : a.f_off; t.obs_cam = prune ? a.t_obs_cam : a.obs_cam; t.obs_z = prune ? a.t_obs_z : a.obs_z;
    t.cam_q = a.cam_q; t.cam_p = a.cam_p; t.feat_stream = nullptr; t.cam_stride = a.cs;
    for (int i = 0; i < 9; ++i) t.R01[i] = a.R01[i];
    for (int i = 0; i < 3; ++i) t.t01[i] = a.t01[i];
    t.huber = a.huber; t.precision = a.precision; t.damping = a.damping; t.outer_max = a.outer_max; t.inner_max = a.inner_max;
    t.out_pos = a.f_pos; t.out_valid = a.f_valid; t.list = nullptr; t.n_list_dev = nullptr; t.fs_stride = a.FS;
    t.f_mslot = prune ? a.f_mslot : nullptr; t.meta_pos = prune ? a.m_pos : nullptr; t.meta_init = prune ? a.m_init : nullptr; t.meta_stride = a.mcap;
    return t;
}
// initialize_position of this stream's candidates that have no position yet (flags left by dev_build_candidates in V.tmp_b):
// a wavefront per feature, the workgroup's four wavefronts side by side
__device__ __forceinline__ void dev_triangulate_own(const DevArgs& a, const AvsStore& V, int s, int nc, bool prune)
{
    const TriArgs t = dev_tri_args(a, prune);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t f0 = (size_t)s * a.FS;
    for (int k = wave; k < nc; k += (int)(blockDim.x >> 6)) if (V.tmp_b[k] >= 0) triangulate_one(t, (int)(f0 + k), lane);      // wave-uniform
    __syncthreads();
}

__device__ __forceinline__ AvsStore dev_store(const DevArgs& a, int s)
{
    AvsStore V;
    V.cap = a.cap; V.mcap = a.mcap; V.ns = a.ns; V.hcells = a.hcells;
    const size_t fo = (size_t)s * a.ns * a.cap;
    V.fr_id = a.fr_id + fo; V.fr_z = a.fr_z + 4 * fo; V.fr_fslot = a.fr_fslot + fo; V.fr_prev = a.fr_prev + fo; V.fr_next = a.fr_next + fo;
    V.fr_n = a.fr_n + (size_t)s * a.ns; V.pos_of = a.pos_of + (size_t)s * a.ns; V.order = a.order + (size_t)s * a.ns;
    V.hdr = a.hdr + (size_t)s * AVS_HDR_WORDS; V.births = a.births + s;
    const size_t mo = (size_t)s * a.mcap;
    V.m_id = a.m_id + mo; V.m_birth = a.m_birth + mo; V.m_pos = a.m_pos + 3 * mo; V.m_init = a.m_init + mo; V.m_nobs = a.m_nobs + mo; V.m_tail = a.m_tail + mo;
    V.free_stack = a.free_stack + mo;
    const size_t ho = (size_t)s * a.hcells, to = (size_t)s * a.cap;
    V.hash_a = a.hash_a + ho; V.hash_b = a.hash_b + ho; V.hash_c = a.hash_c + ho;
    V.tmp_a = a.tmp_a + to; V.tmp_b = a.tmp_b + to; V.tmp_c = a.tmp_c + to; V.keys = a.keys + to;
    return V;
}

// predict_new_state (msckf.py:341-388): 4th-order Runge-Kutta with k2 and k3 sharing the half-step rotation (appendix A.13)
__device__ void dev_predict_new_state(DState& S, double dt, const double* gyro, const double* acc)
{
    const double gn = h_norm3(gyro);
    const double Om[16] = {0, gyro[2], -gyro[1], gyro[0], -gyro[2], 0, gyro[0], gyro[1], gyro[1], -gyro[0], 0, gyro[2], -gyro[0], -gyro[1], -gyro[2], 0};
    auto apply = [&](double c, double s_over, double lin, double* out) {
        for (int i = 0; i < 4; ++i) {
            double acc_ = 0;
            for (int j = 0; j < 4; ++j) {
                const double m = (gn > 1e-5) ? ((i == j ? c : 0.0) + s_over * Om[i * 4 + j]) : (c * ((i == j ? 1.0 : 0.0) + Om[i * 4 + j] * lin));
                acc_ += m * S.q[j];
            }
            out[i] = acc_;
        }
    };
    double dq[4], dq2[4];
    if (gn > 1e-5) {
        apply(cos(gn * dt * 0.5), sin(gn * dt * 0.5) / gn, 0, dq);
        apply(cos(gn * dt * 0.25), sin(gn * dt * 0.25) / gn, 0, dq2);
    } else {
        apply(cos(gn * dt * 0.5), 0, dt * 0.5, dq);
        apply(cos(gn * dt * 0.25), 0, dt * 0.25, dq2);
    }
    double R[9], R1[9], R2[9];
    h_to_rotation(S.q, R); h_to_rotation(dq, R1); h_to_rotation(dq2, R2);
    double k1v[3], k2v[3], k4v[3];
    h_mtv(R, acc, k1v); h_mtv(R2, acc, k2v); h_mtv(R1, acc, k4v);
    for (int i = 0; i < 3; ++i) { k1v[i] += S.gravity[i]; k2v[i] += S.gravity[i]; k4v[i] += S.gravity[i]; }
    const double* k3v = k2v;
    double vnew[3], pnew[3];
    for (int i = 0; i < 3; ++i) {
        const double k1p = S.v[i], k2p = S.v[i] + k1v[i] * dt / 2., k3p = S.v[i] + k2v[i] * dt / 2, k4p = S.v[i] + k3v[i] * dt;
        vnew[i] = S.v[i] + (k1v[i] + 2 * k2v[i] + 2 * k3v[i] + k4v[i]) * dt / 6.;
        pnew[i] = S.p[i] + (k1p + 2 * k2p + 2 * k3p + k4p) * dt / 6.;
    }
    const double nq = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int i = 0; i < 4; ++i) S.q[i] = dq[i] / nq;
    for (int i = 0; i < 3; ++i) { S.v[i] = vnew[i]; S.p[i] = pnew[i]; }
}

// state injection of measurement_update (msckf.py:576-595) with the reference's in-place aliasing; camera states by `lanes` threads
__device__ void dev_inject_imu(DState& S, const double* dx)
{
    double dq[4], qo[4];
    h_small_angle(dx, dq); h_quat_mul(dq, S.q, qo);
    for (int i = 0; i < 4; ++i) S.q[i] = qo[i];
    for (int i = 0; i < 3; ++i) {
        S.bg[i] += dx[3 + i]; S.v[i] += dx[6 + i]; S.ba[i] += dx[9 + i]; S.p[i] += dx[12 + i];
        if (S.null_aliased) { S.vn[i] += dx[6 + i]; S.pn[i] += dx[12 + i]; }
    }
    double de[4], Re[9], Rn[9];
    h_small_angle(dx + 15, de); h_to_rotation(de, Re);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = Re[r * 3] * S.R_ic[c] + Re[r * 3 + 1] * S.R_ic[3 + c] + Re[r * 3 + 2] * S.R_ic[6 + c];
    for (int i = 0; i < 9; ++i) S.R_ic[i] = Rn[i];
    for (int i = 0; i < 3; ++i) S.t_ci[i] += dx[18 + i];
}
__device__ void dev_inject_cam(double* cq, double* cp, const double* d)
{
    double q4[4], co[4];
    h_small_angle(d, q4); h_quat_mul(q4, cq, co);
    for (int i = 0; i < 4; ++i) cq[i] = co[i];
    for (int i = 0; i < 3; ++i) cp[i] += d[3 + i];
}
// result of the update that has just run on stream s: failure codes, state injection (thread 0 the IMU part, one thread per camera)
__device__ void dev_apply_update(const DevArgs& a, int s, DState* D)
{
    const int st = a.stacked[s];
    if (threadIdx.x == 0) {
        if (st == UPD_BAD_PIVOT) D->failed = DFAIL_PIVOT;
        else if (st < 0) D->failed = DFAIL_STACK;
        else if (st > 0) { DState L = *D; dev_inject_imu(L, a.dx + (size_t)s * a.ld); *D = L; }
    }
    if (st > 0 && (int)threadIdx.x < D->ncam) {
        const size_t c = (size_t)s * a.cs + threadIdx.x;
        dev_inject_cam(a.cam_q + 4 * c, a.cam_p + 3 * c, a.dx + (size_t)s * a.ld + IMU_DIM + 6 * threadIdx.x);
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// dk_state: batch_imu_processing + predict_new_state (msckf.py:251-273, 341-388) and the state half of state_augmentation (:390-410) --
// a serial chain per stream that needs no covariance.  The covariance half (process_model :275-339, the new camera's rows and
// columns :411-423) runs in dk_cov, a one-wavefront kernel, from the records this leaves: until round 5 it ran here, on 256 threads
// with 27 KB of LDS and nine barriers per IMU sample -- two thirds of this workgroup's life, at 4 x 128 registers and 39 KB of LDS
// per stream the fattest thing the filter put beside the front-end's kernels (profiles/r05/README.md).
// ------------------------------------------------------------------------------------------------
// (a LANE per stream: the chain is serial per stream and independent between streams -- as thread 0 of a 256-thread workgroup it kept
//  four wavefronts of every stream resident for its ~50 us)
__global__ __launch_bounds__(64) void dk_state(DevArgs a)
{
    AV_FILTER_PRIO();
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 16) a.cnt_next[threadIdx.x] = 0;      // the NEXT step's list counters (this step's were zeroed a step ago)
    if (s >= a.S) return;
    DState* Dg = a.st + s;
    const DCtl C = a.ctl[s];
    {
        DState L = *Dg;                                     // a private copy of the state, written back at the end
        DState* D = &L;
        DCov cv; cv.act = 0; cv.cnt = 0; cv.first = C.imu_first; cv.pad = 0;
        if (C.has_init) {                                   // initialize_gravity_and_bias ran on the host when the 200th IMU sample arrived (msckf.py:230-249)
            for (int i = 0; i < 4; ++i) D->q[i] = C.q0[i];
            for (int i = 0; i < 3; ++i) { D->bg[i] = C.bg0[i]; D->gravity[i] = C.g0[i]; }
        }
        int act = C.active && !D->failed;
        if (act && D->ncam + 1 > a.cs) { D->failed = DFAIL_CAMS; act = 0; }
        if (act && D->first_img) { D->first_img = 0; D->ts = C.t_frame; }
        D->active = act; D->prune = 0;
        if (act) {
            double* P = a.P + (size_t)s * a.pstride;
            const int n = D->n, ld = a.ld;
            for (int k = 0; k < C.imu_cnt; ++k) {
                PropArgs pa;
                const DImu m = a.imu[C.imu_first + k];
                pa.P = P; pa.n = n; pa.ld = ld; pa.dt = m.t - D->ts;
                for (int i = 0; i < 3; ++i) { pa.gyro[i] = m.w[i] - D->bg[i]; pa.acc[i] = m.a[i] - D->ba[i]; pa.gravity[i] = D->gravity[i]; }
                for (int i = 0; i < 4; ++i) { pa.q_old[i] = D->q[i]; pa.noise[i] = a.noise[i]; }
                dev_predict_new_state(*D, pa.dt, pa.gyro, pa.acc);
                for (int i = 0; i < 4; ++i) { pa.q_new[i] = D->q[i]; pa.q_null[i] = D->qn[i]; }
                for (int i = 0; i < 3; ++i) { pa.v_null[i] = D->vn[i]; pa.p_null[i] = D->pn[i]; pa.v_new[i] = D->v[i]; pa.p_new[i] = D->p[i]; }
                for (int i = 0; i < 4; ++i) D->qn[i] = D->q[i];
                for (int i = 0; i < 3; ++i) { D->pn[i] = D->p[i]; D->vn[i] = D->v[i]; }
                D->null_aliased = 1;
                D->ts = m.t;
                a.prop[C.imu_first + k] = pa;
            }
            // ---- state_augmentation (msckf.py:390-410): the new camera state; its covariance rows are dk_cov's
            double Rwi[9], Rwc[9], tw[3], cq[4];
            h_to_rotation(D->q, Rwi);
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rwc[r * 3 + c] = D->R_ic[r * 3] * Rwi[c] + D->R_ic[r * 3 + 1] * Rwi[3 + c] + D->R_ic[r * 3 + 2] * Rwi[6 + c];
            h_mtv(Rwi, D->t_ci, tw);
            h_to_quaternion(Rwc, cq);
            const size_t c = (size_t)s * a.cs + D->ncam;
            a.cam_id[c] = D->next_imu_id++;
            for (int i = 0; i < 4; ++i) { a.cam_q[4 * c + i] = cq[i]; a.cam_qn[4 * c + i] = cq[i]; }
            for (int i = 0; i < 3; ++i) a.cam_p[3 * c + i] = D->p[i] + tw[i];
            cv.act = 1; cv.cnt = C.imu_cnt;
            cv.aa.P = P; cv.aa.n = n; cv.aa.ld = ld;
            for (int i = 0; i < 9; ++i) cv.aa.R_ic[i] = D->R_ic[i];
            const double sk[9] = {0, -tw[2], tw[1], tw[2], 0, -tw[0], -tw[1], tw[0], 0};
            for (int i = 0; i < 9; ++i) cv.aa.sk[i] = sk[i];
            D->n = n + 6; D->ncam += 1;
            a.ncam[s] = D->ncam; a.nstate[s] = D->n;
            for (int i = 0; i < 3; ++i) a.grav[3 * s + i] = D->gravity[i];
        }
        a.cov[s] = cv;
        *Dg = L;
    }
}

// ------------------------------------------------------------------------------------------------
// dk_imu_rate: IMU-rate odometry (include/airvision.h, "IMU-rate odometry"; launched behind dk_state only when av_msckf_batch_set_imu_rate
// is on).  dk_state leaves, per IMU sample it integrated, the state after dev_predict_new_state and the bias-corrected gyro in the
// sample's record a.prop[] (q_new, p_new, v_new, gyro: the doubles dk_cov reads), and its final word on the stream's part in the step in
// a.cov[] (act, first, cnt).  This kernel gathers them into records of 112 bytes, the sample's stamp from a.imu[] in front: ONE wavefront
// per stream, whatever shape the step's other kernels take, a lane per double of the stream's rows, so the stores are contiguous (a lane
// per stream inside dk_state would write 112-byte pieces cap x 112 bytes apart).  On overflow the LAST cap samples are kept: record j is
// sample cnt - min(cnt, cap) + j.  A stream dk_state left alone reads (0, 0).  Plain vector stores: no atomics, no LDS.
// (As a second instance of dk_state, the body a template over a bool, the records cost no launch -- but the instance with the bool off
//  no longer compiled to dk_state's code: 2,086 instructions against 2,083, 106 scalar registers with two spilled against 96 and none;
//  profiles/imu_rate/README.md.)
// ------------------------------------------------------------------------------------------------
struct DImuState { double t, p[3], q[4], v[3], w[3]; };
static_assert(sizeof(DImuState) == 112, "av_imu_state is 112 bytes");
struct IrOut { DImuState* rec; int* n; int cap; };      // [S][cap] records, [S][2] counts (had, written)
__global__ __launch_bounds__(64) void dk_imu_rate(DevArgs a, IrOut R)
{
    AV_FILTER_PRIO();
    const int s = blockIdx.x, lane = threadIdx.x;
    const DCov cv = a.cov[s];
    const int had = cv.act ? cv.cnt : 0, wr = had < R.cap ? had : R.cap, k0 = had - wr;
    if (lane == 0) { R.n[2 * (size_t)s] = had; R.n[2 * (size_t)s + 1] = wr; }
    constexpr int W = (int)(sizeof(DImuState) / 8);
    double* out = reinterpret_cast<double*>(R.rec + (size_t)s * R.cap);
    for (int e = lane; e < wr * W; e += 64) {
        const int j = e / W, f = e - j * W;
        const size_t i = (size_t)cv.first + k0 + j;
        const PropArgs& pa = a.prop[i];
        out[e] = f == 0 ? a.imu[i].t : (f < 4 ? pa.p_new[f - 1] : (f < 8 ? pa.q_new[f - 4] : (f < 11 ? pa.v_new[f - 8] : pa.gyro[f - 11])));
    }
}

// ------------------------------------------------------------------------------------------------
// dk_cov: process_model's covariance steps for all the frame's IMU samples (msckf.py:275-339), the cross block with the frame's
// accumulated transition, and the new camera state's rows and columns (:411-423) -- ONE wavefront per stream.  The 21 x 21 products
// are the block-sparse sums of propagate_body; its barriers are wavefront-local here.
// ------------------------------------------------------------------------------------------------
// NT = 64: one wavefront per stream (large batches: what counts beside the front-end is the footprint; that instance is the explicit
// specialisation below, this text is its bit reference); NT = 256: four (small batches: the GPU is not full and what counts is the time
// one stream takes)
template <int NT>
__global__ __launch_bounds__(NT) void dk_cov(DevArgs a)
{
    AV_FILTER_PRIO();
    __shared__ double P11s[IMU_DIM * IMU_DIM], PhiT[IMU_DIM * IMU_DIM], work[PROP_LDS_DOUBLES];
    const int s = blockIdx.x, tid = threadIdx.x, N = IMU_DIM;
    const DCov cv = a.cov[s];
    if (!cv.act) return;                                    // (workgroup-uniform)
    double* P = cv.aa.P;
    const int n = cv.aa.n, ld = cv.aa.ld;
    auto stamp = [&](int i) { if (a.prof && s == 0 && tid == 0) a.prof[i] = __builtin_amdgcn_s_memrealtime(); };
    stamp(0);
    if (cv.cnt > 0) {
        for (int i = tid; i < N * N; i += NT) { const int r = i / N, c = i - r * N; P11s[i] = P[(size_t)r * ld + c]; PhiT[i] = r == c ? 1.0 : 0.0; }
        __syncthreads();
        for (int k = 0; k < cv.cnt; ++k) propagate_body<true, NT>(a.prop[cv.first + k], P11s, PhiT, work);        // each ends on a barrier
        stamp(1);
        // cross block with the frame's accumulated transition: a lane per column of P12, its 21 old entries parked in LDS (the work
        // matrices are free again; a lane reads back only what it wrote), every new entry a dense 21-term sum -- the zeros of the
        // transition multiply to exact zeros -- mirrored into P21
        const int nc = n - N;
        constexpr int CW = 64, NRQ = NT / CW;                // 64 columns at a time; with four wavefronts each takes every fourth row
        const int cl = tid % CW, rq = tid / CW;
        for (int c0 = 0; c0 < nc; c0 += CW) {
            const int c = c0 + cl;
            const bool in = c < nc;
            __syncthreads();                                 // (the previous chunk's readers are done)
            for (int k = rq; k < IMU_DIM; k += NRQ) work[k * CW + cl] = in ? P[(size_t)k * ld + N + c] : 0.0;
            __syncthreads();
#pragma unroll 1
            for (int r = rq; r < IMU_DIM; r += NRQ) {
                double sum = 0;
#pragma unroll 7
                for (int k = 0; k < IMU_DIM; ++k) sum += PhiT[r * N + k] * work[k * CW + cl];
                if (in) { P[(size_t)r * ld + N + c] = sum; P[(size_t)(N + c) * ld + r] = sum; }
            }
        }
        for (int i = tid; i < N * N; i += NT) { const int r = i / N, c = i - r * N; P[(size_t)r * ld + c] = P11s[i]; }
        __syncthreads();
    }
    stamp(2);
    augment_body<NT>(cv.aa);
}
// The one-wavefront instance has a body of its own (msckf.hip, "dk_cov<64>'s body"): the same sums bit for bit -- the instance above is
// what it is tested against -- as independent chains, in 96 registers without scratch and 19,120 B of LDS, so that the four wavefronts
// a 1,024-stream group puts on a CU leave LK all twenty of its own (4 x 19,120 + 20 x 3,840 B <= 160 KiB) and a wavefront fits the
// hole ONE retiring LK wavefront leaves on a SIMD.  Per sample: preparation | Fdt, patterns | Fdt^2 | Fdt^3, Phi | patches, pattern |
// Phi G, Phi P11, Phi PhiT | P11 | symmetrise; then the cross block out of registers and the augmentation, a lane per column.
// Parent body at NT = 64: 157 registers, 184 B of scratch per lane, 28,680 B of LDS, 0.58 ms per 2,048 streams alone and 1.1 ms beside the
// front-end; this one 0.23 and 0.36 ms (profiles/dk_cov_chains/README.md).
// (__launch_bounds__(256, 5) on a kernel launched with 64 threads: with a bound of 64 the compiler works out from the LDS size that no more
//  than two such workgroups share a SIMD, drops the request for five, and allocates 248 registers.)
template <>
__global__ __launch_bounds__(256, 5) void dk_cov<64>(DevArgs a)
{
    AV_FILTER_PRIO();
    __shared__ CovChainsLds L;
    const int s = blockIdx.x, tid = threadIdx.x, N = IMU_DIM;
    const DCov& cv = a.cov[s];                              // (read in place: a private copy, indexed by lane in the augmentation, is 184 B of scratch)
    if (!cv.act) return;                                    // (workgroup-uniform)
    const cvc_gptr P = (cvc_gptr)cv.aa.P;
    const int n = cv.aa.n, ld = cv.aa.ld, cnt = cv.cnt, first = cv.first;
    auto stamp = [&](int i) { if (a.prof && s == 0 && tid == 0) a.prof[i] = __builtin_amdgcn_s_memrealtime(); };
    stamp(0);
    if (cnt > 0) {
        double* PhiT = L.m + CVC_PHIA, * PhiTn = L.m + CVC_PHIB, * const P11s = L.m + CVC_P11;
        for (int i = tid; i < N * N; i += 64) { const int r = i / N, c = i - r * N; P11s[i] = P[(size_t)r * ld + c]; PhiT[i] = r == c ? 1.0 : 0.0; }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {                     // (each ends on a barrier)
            propagate_chains(a.prop[first + k], L, PhiT, PhiTn);
            double* const t = PhiT; PhiT = PhiTn; PhiTn = t;
        }
        stamp(1);
        cross_chains(P, n, ld, PhiT);
        for (int i = tid; i < N * N; i += 64) { const int r = i / N, c = i - r * N; P[(size_t)r * ld + c] = P11s[i]; }
        __syncthreads();
    }
    stamp(2);
    augment_chains(cv.aa, L.m + CVC_PP, L.m + CVC_PP + 6 * N, L.m + CVC_PP + 12 * N);
}

// observation CSR + per-feature records of the candidates cand[0 .. nc) of stream s (dict order), launch buckets and the
// triangulation list of phase `ph`.  full = true: all observations of every candidate (lost features); false: the two
// observations e0 / e1 (camera pruning), the features without a position get their complete track in the t_* CSR.
__device__ void dev_build_candidates(const DevArgs& a, const AvsTeam& T, const AvsStore& V, int s, int nc, const int* cand, bool full,
                                     int i0, int i1, const int* e0, const int* e1, int ph, int* lb /* LDS [8] */)
{
    const int tid = threadIdx.x;
    const size_t f0 = (size_t)s * a.FS, ob = (size_t)s * a.obs_stride;
    if (tid < 8) lb[tid] = 0;
    __syncthreads();
    int obs_run = 0, row_run = 0, tobs_run = 0;
    for (int base = 0; base < nc; base += (int)blockDim.x) {
        const int k = base + tid;
        const bool in = k < nc;
        const int fs = in ? cand[k] : 0;
        const int nall = in ? V.m_nobs[fs] : 0;
        const int nobs = full ? nall : (in ? 2 : 0);
        const int init = in ? V.m_init[fs] : 1;
        int to, tr, tt;
        const int o = obs_run + T.excl_scan(nobs, &to);
        const int r = row_run + T.excl_scan(in ? 4 * nobs - 3 : 0, &tr);
        const int t = tobs_run + T.excl_scan((!full && !init) ? nall : 0, &tt);
        if (in) {
            const size_t f = f0 + k;
            a.f_off[f] = (int)(ob + o); a.f_rowoff[f] = r; a.f_dof[f] = full ? nobs - 1 : 2; a.f_mslot[f] = fs;
            if (!full) a.t_off[f] = (int)(ob + t);          // CSR over ALL candidates: a feature that has its position owns an empty slice
            if (full) (void)avs_collect(V, fs, a.obs_cam + ob + o, a.obs_z + 4 * (ob + o));
            else {
                a.obs_cam[ob + o] = i0; a.obs_cam[ob + o + 1] = i1;
                const double* z0 = V.fr_z + ((size_t)avs_lslot(e0[k]) * V.cap + avs_lidx(e0[k])) * 4;
                const double* z1 = V.fr_z + ((size_t)avs_lslot(e1[k]) * V.cap + avs_lidx(e1[k])) * 4;
                for (int e = 0; e < 4; ++e) { a.obs_z[4 * (ob + o) + e] = z0[e]; a.obs_z[4 * (ob + o + 1) + e] = z1[e]; }
            }
            int valid = 1, tri = 0;
            if (init) { for (int e = 0; e < 3; ++e) a.f_pos[3 * f + e] = V.m_pos[(size_t)3 * fs + e]; }
            else {
                valid = 0; tri = 1;
                int* tc = full ? a.obs_cam + ob + o : a.t_obs_cam + ob + t;
                double* tz = full ? a.obs_z + 4 * (ob + o) : a.t_obs_z + 4 * (ob + t);
                if (!full) (void)avs_collect(V, fs, tc, tz);
                if (a.trans_thr >= 0) {                     // check_motion (feature_motion_checker.py:6-39); always true at the reference's -1
                    const size_t ca = (size_t)s * a.cs + tc[0], cb = (size_t)s * a.cs + tc[nall - 1];
                    double Ra[9], d[3] = {tz[0], tz[1], 1.0}, dw[3];
                    const double nd = h_norm3(d); d[0] /= nd; d[1] /= nd; d[2] /= nd;
                    h_to_rotation(a.cam_q + 4 * ca, Ra); h_mtv(Ra, d, dw);
                    const double tv[3] = {a.cam_p[3 * cb] - a.cam_p[3 * ca], a.cam_p[3 * cb + 1] - a.cam_p[3 * ca + 1], a.cam_p[3 * cb + 2] - a.cam_p[3 * ca + 2]};
                    const double par = tv[0] * dw[0] + tv[1] * dw[1] + tv[2] * dw[2];
                    const double o3[3] = {tv[0] - par * dw[0], tv[1] - par * dw[1], tv[2] - par * dw[2]};
                    if (!(h_norm3(o3) > a.trans_thr)) tri = 0;      // not triangulated, not evaluated (valid stays 0)
                }
            }
            a.f_valid[f] = valid;
            // launch bucket by track length, triangulation list: ranks inside the workgroup first, one global atomic per list below
            const int bk = (full && nobs > 8) ? 1 : 0;      // launch buckets: lost features by track length (<= 8 observations / longer), pruning candidates all in one
            V.tmp_a[k] = (bk << 24) | atomicAdd(&lb[bk], 1);
            V.tmp_b[k] = tri ? atomicAdd(&lb[5], 1) : -1;
        }
        obs_run += to; row_run += tr; tobs_run += tt;
    }
    __syncthreads();
    if (tid == 0) {
        a.f_off[f0 + nc] = (int)(ob + obs_run);
        if (!full) a.t_off[f0 + nc] = (int)(ob + tobs_run);
        a.n_cand[s] = nc;
        // More rows than the stream's own region of the block buffers holds (a blank frame loses every track at once): the candidates take
        // their rows from the pool all streams share, one bump of its counter per stream.  (Round 3 gated such a stream first and stored
        // in a second pass over the stacked features -- a launch per step whether or not any stream needed it.)
        int shift = 0;
        if (row_run > a.rows_cap) {
            // (lost-feature phase only: the pruning phase's rows are 12 doubles wide and always fit -- 5 rows per message slot, sub_reserve)
            const int base = ph == 0 ? atomicAdd(&a.cnt[8 * ph + 4], row_run) : -1;
            if (base >= 0 && base + row_run <= a.pool_rows) shift = (a.S - s) * a.rows_cap + base;      // pool row `base`, counted from this stream's first row
            else shift = -1;
        }
        lb[6] = shift;
        a.over[s] = 0;
        // pool exhausted: the stream stops (DFAIL_ROWS) and hands nothing to the launches of this phase -- no candidates, no list entries
        if (shift < 0) { DState* D = a.st + s; D->failed = DFAIL_ROWS; D->active = 0; a.n_cand[s] = 0; }
    }
    __syncthreads();
    const int shift = lb[6];
    if (shift < 0) {                                        // (workgroup-uniform)
        for (int k = tid; k < nc; k += (int)blockDim.x) { a.f_rowoff[f0 + k] = -1; a.f_valid[f0 + k] = 0; V.tmp_b[k] = -1; }
        __syncthreads();
        return;
    }
    if (tid < 6) { const int c = lb[tid]; lb[tid] = c > 0 ? atomicAdd(&a.cnt[8 * ph + tid], c) : 0; }       // -> base of this stream's share of the list
    __syncthreads();
    const size_t lstride = (size_t)a.S * a.cap;
    for (int k = tid; k < nc; k += (int)blockDim.x) {
        const size_t f = f0 + k;
        const int v = V.tmp_a[k], bk = v >> 24;
        a.blist[bk * lstride + lb[bk] + (v & 0xFFFFFF)] = (int)f;
        if (V.tmp_b[k] >= 0) a.tlist[lb[5] + V.tmp_b[k]] = (int)f;
        if (shift > 0) a.f_rowoff[f] += shift;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// dk_append: add_feature_observations (msckf.py:425-441) + the selection half of remove_lost_features (:614-640, 675-676)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dk_append_body(const DevArgs& a, unsigned long long* lds_keys)
{
    __shared__ int red[8], lb[8];
    const int s = blockIdx.x, tid = threadIdx.x;
    DState* D = a.st + s;
    if (!D->active) { if (tid == 0) { a.n_cand[s] = 0; a.over[s] = 0; a.f_off[(size_t)s * a.FS] = 0; } return; }       // block-uniform
    AvsTeam T; T.red = red;
    AvsStore V = dev_store(a, s);
    if (a.cap <= DEV_LDS_KEYS) V.keys = lds_keys;           // the sort's keys: n broadcast reads per item out of LDS instead of L2
    const int before = V.hdr[AVS_LIVE];
    __syncthreads();
    auto stamp = [&](int i) { if (a.prof && s == 0 && tid == 0) a.prof[i] = __builtin_amdgcn_s_memrealtime(); };
    stamp(3);
    int tracked = 0;
    const int nk = a.msg_n[s] < a.msg_cap ? a.msg_n[s] : a.msg_cap;
    const int slot = avs_add_frame(T, V, a.msg_ids + (size_t)s * a.msg_cap, a.msg_uv + (size_t)s * a.msg_cap * 4, nk, &tracked);
    if (slot < 0) {
        if (tid == 0) { D->failed = slot == -1 ? DFAIL_FRAMES : DFAIL_TABLE; D->active = 0; a.n_cand[s] = 0; a.over[s] = 0; }
        return;
    }
    if (tid == 0) D->tracking_rate = tracked / ((double)before + 1e-5);
    int* cand = a.cand + (size_t)s * a.cap; int* inval = a.e0 + (size_t)s * a.cap;
    int nc = 0, ni = 0;
    stamp(4);
    avs_select_lost(T, V, cand, &nc, inval, &ni);
    stamp(5);
    dev_build_candidates(a, T, V, s, nc, cand, true, 0, 0, nullptr, nullptr, 0, lb);
    stamp(6);
    dev_triangulate_own(a, V, s, nc, false);
    stamp(7);
    if (tid == 0 && lb[6] > 0) D->n_two_pass += 1;       // (counts the steps that took rows from the pool)
    // every feature that is not observed in this frame leaves the map now: processed or invalid (msckf.py:646-656, 675-676);
    // what the update needs of them is in the CSR
    avs_erase(T, V, cand, nc);
    avs_erase(T, V, inval, ni);
    stamp(8);
}

// ------------------------------------------------------------------------------------------------
// dk_begin: the first kernel of a step = dk_predict_body + dk_append_body (one launch: under contention with the front-end every
// launch of the chain waits ~0.3 ms for its workgroups to be placed, whatever it does)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dk_begin_body(const DevArgs& a)
{
    AV_FILTER_PRIO();
    __shared__ unsigned long long keys8[DEV_LDS_KEYS];      // the keys of the observation store's sorts
    dk_append_body(a, keys8);
}
// (Rounds 4-5: this kernel also ran the covariance steps -- 39 KB of LDS, 128 registers with 380 B of scratch, four workgroups per CU;
//  a 168-register build at three per CU took 874 us per 2,048-stream launch against 740: profiles/r04/README.md.)
__global__ __launch_bounds__(256, 5) void dk_begin4(DevArgs a) { dk_begin_body(a); }

// find_redundant_cam_states (msckf.py:678-709): window positions of the two camera states to drop, ascending
__device__ void dev_find_redundant(const DevArgs& a, int s, const DState& D, int* r0, int* r1)
{
    const int nc = D.ncam, key = nc - 4;
    const size_t c0 = (size_t)s * a.cs;
    int idx = key + 1, firstc = 0;
    double Rk[9];
    h_to_rotation(a.cam_q + 4 * (c0 + key), Rk);
    int sel[2];
    for (int k = 0; k < 2; ++k) {
        double Rc[9], RR[9], qq[4];
        h_to_rotation(a.cam_q + 4 * (c0 + idx), Rc);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) RR[r * 3 + c] = Rc[r * 3] * Rk[c * 3] + Rc[r * 3 + 1] * Rk[c * 3 + 1] + Rc[r * 3 + 2] * Rk[c * 3 + 2];
        h_to_quaternion(RR, qq);
        const double d[3] = {a.cam_p[3 * (c0 + idx)] - a.cam_p[3 * (c0 + key)], a.cam_p[3 * (c0 + idx) + 1] - a.cam_p[3 * (c0 + key) + 1], a.cam_p[3 * (c0 + idx) + 2] - a.cam_p[3 * (c0 + key) + 2]};
        const double ang = 2 * acos(qq[3]);
        if (ang < 0.2618 && h_norm3(d) < 0.4 && D.tracking_rate > 0.5) sel[k] = idx;
        else { sel[k] = firstc; ++firstc; }
        ++idx;
    }
    if (sel[0] > sel[1]) { const int t = sel[0]; sel[0] = sel[1]; sel[1] = t; }      // (camera ids ascend with the window position)
    *r0 = sel[0]; *r1 = sel[1];
}

// ------------------------------------------------------------------------------------------------
// Landmark map (include/airvision.h, "Landmark map"): the triangulated features of the step's two updates, per stream, as records of
// 40 bytes.  The per-phase feature arrays hold one update at a time, so the lost-feature records are written by dk_mid_lm before it
// rebuilds them and the pruning records by the dk_finish_*lm instances before the two frames leave the store.  ONE wavefront of the
// stream's workgroup writes, 64 candidates per trip, in candidate (= dict) order: a ballot and a prefix count of "publishes" give the
// slot, a prefix sum of 4 n_obs - 3 over the gated-in candidates, carried across trips, re-applies the 1,500-row cut of
// msckf.py:667-668 (the device evaluates every candidate; the feature whose rows take the sum over 1,500 is still used), plain vector
// stores write the record.  No atomics: the order is the same at both launch shapes.
// ------------------------------------------------------------------------------------------------
enum { LM_USED = 1, LM_REJECTED = 2, LM_TRACKED = 4, LM_NEW = 8 };
struct DLandmark { long long id; double p[3]; int flags; int n_obs; };
static_assert(sizeof(DLandmark) == 40, "av_landmark is 40 bytes");
struct LmOut { DLandmark* rec; int* n; int cap; };      // [S][cap] records, [S][2] counts (had, written)

// call with threadIdx.x < 64 (the first wavefront, all of its lanes).  prune = false: the lost-feature candidates, counts start at 0;
// true: the pruning candidates that got their position in this step (dev_build_candidates left tmp_b >= 0 for them, the triangulation
// f_valid), appended behind the lost-feature records
__device__ __forceinline__ void dev_landmarks(const DevArgs& a, int s, const LmOut& L, bool prune)
{
    const int lane = threadIdx.x;
    int* n = L.n + 2 * (size_t)s;
    const DState* D = a.st + s;
    if (!D->active) { if (lane == 0) { n[0] = 0; n[1] = 0; } return; }      // (wavefront-uniform)
    const size_t f0 = (size_t)s * a.FS, mo = (size_t)s * a.mcap;
    const int* tmp_b = a.tmp_b + (size_t)s * a.cap;
    DLandmark* rec = L.rec + (size_t)s * L.cap;
    const int nc = a.n_cand[s];
    int total = prune ? n[0] : 0, rows = 0;
    for (int base = 0; base < nc; base += 64) {
        const int k = base + lane;
        const size_t f = f0 + k;
        int pub = 0, fs = 0, nobs = 0, flags = 0, gated = 0;
        if (k < nc) {
            fs = a.f_mslot[f];
            const int pass = a.pass[f];
            if (prune) {
                pub = tmp_b[k] >= 0 && a.f_valid[f] != 0;
                nobs = a.m_nobs[mo + fs];
                flags = LM_TRACKED | LM_NEW | (pass ? LM_USED : LM_REJECTED);
            } else {
                pub = a.f_valid[f] != 0;
                nobs = a.f_off[f + 1] - a.f_off[f];         // (the feature has left the store: its observations are the CSR's)
                gated = pub && pass;
                flags = a.m_init[mo + fs] ? 0 : LM_NEW;     // (the lost features' triangulation does not touch the table's flag)
            }
        }
        const unsigned long long m = __ballot(pub);
        const int slot = total + __popcll(m & ((1ull << lane) - 1ull));
        if (!prune) {
            const int v = gated ? 4 * nobs - 3 : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            if (rows + incl - v <= 1500) flags |= gated ? LM_USED : LM_REJECTED;
            rows += __shfl(incl, 63);
        }
        if (pub && slot < L.cap) {
            DLandmark r;
            r.id = a.m_id[mo + fs]; r.p[0] = a.f_pos[3 * f]; r.p[1] = a.f_pos[3 * f + 1]; r.p[2] = a.f_pos[3 * f + 2]; r.flags = flags; r.n_obs = nobs;
            rec[slot] = r;
        }
        total += __popcll(m);
    }
    if (lane == 0) { n[0] = total; n[1] = total < L.cap ? total : L.cap; }
}

// ------------------------------------------------------------------------------------------------
// Innovation statistics (include/airvision.h, "Innovation statistics"): what the gates of the step's two updates decided, per stream, as
// two blocks of 64 bytes.  Like the landmark records they are taken while the per-phase arrays of the update stand: block 0 by the
// dk_mid_*st instances before dk_mid rebuilds them, block 1 by the dk_finish_*st instances.  ONE wavefront of the stream's workgroup
// works, 64 candidates per trip in candidate (= dict) order.  Counts: ballots.  The 1,500-row cut: dev_landmarks' prefix sum of 4 n_obs - 3
// over the gated-in candidates, carried across trips.  Sums of dof and gamma: lane l adds the candidates k = l, l + 64, l + 128, ... in
// ascending k into its own accumulators (a candidate that does not count adds nothing, not a zero), then ONE butterfly over the
// wavefront, x += shfl_xor(x, d) for d = 32, 16, 8, 4, 2, 1 in this order, leaves the same bits in every lane.  Only the first 64
// threads of the workgroup take part, so the 64- and the 256-thread launch add in the same order and write the same bytes.  No atomics,
// no LDS; lane 0 writes the block with plain vector stores.
// ------------------------------------------------------------------------------------------------
enum { FS_RAN = 1, FS_CUT = 2 };
struct DUpdStats { int n_cand, n_pos, n_eval, n_pass, dof_eval, dof_pass, rows, flags; double gamma_eval, gamma_pass, dx_pos, dx_rot; };
static_assert(sizeof(DUpdStats) == 64, "av_update_stats is 64 bytes");

// call with threadIdx.x < 64: `blocks` blocks of stream s, from block `first` on, become zero bytes (8 lanes x 8 bytes per block)
__device__ __forceinline__ void dev_stats_zero(DUpdStats* out, int s, int first, int blocks)
{
    unsigned long long* w = reinterpret_cast<unsigned long long*>(out + 2 * (size_t)s + first);
    if ((int)threadIdx.x < 8 * blocks) w[threadIdx.x] = 0ull;
}
// call with threadIdx.x < 64 (the first wavefront, all of its lanes) for an active stream, with a.stacked / a.dx those of the update the
// candidates belong to.  prune = false: block 0, the lost-feature update; true: block 1, the pruning update (no row cut)
__device__ __forceinline__ void dev_stats(const DevArgs& a, int s, DUpdStats* out, bool prune)
{
    const int lane = threadIdx.x;
    const size_t f0 = (size_t)s * a.FS;
    const int nc = a.n_cand[s];
    int n_pos = 0, n_eval = 0, n_pass = 0, rows = 0;
    int dof_e = 0, dof_p = 0;
    double g_e = 0.0, g_p = 0.0;
    for (int base = 0; base < nc; base += 64) {
        const int k = base + lane;
        const size_t f = f0 + k;
        int valid = 0, gated = 0, nobs = 0, dof = 0;
        double g = 0.0;
        if (k < nc) {
            valid = a.f_valid[f] != 0;
            if (valid) { gated = a.pass[f] != 0; nobs = a.f_off[f + 1] - a.f_off[f]; dof = a.f_dof[f]; g = a.gamma[f]; }
        }
        int ev = valid;
        if (!prune) {
            const int v = gated ? 4 * nobs - 3 : 0;
            int incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            ev = valid && rows + incl - v <= 1500;            // (the reference reaches this candidate: msckf.py:667-668)
            rows += __shfl(incl, 63);
        }
        const int ps = ev && gated;
        n_pos += __popcll(__ballot(valid)); n_eval += __popcll(__ballot(ev)); n_pass += __popcll(__ballot(ps));
        if (ev) { dof_e += dof; g_e += g; }
        if (ps) { dof_p += dof; g_p += g; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        dof_e += __shfl_xor(dof_e, d); dof_p += __shfl_xor(dof_p, d);
        g_e += __shfl_xor(g_e, d); g_p += __shfl_xor(g_p, d);
    }
    if (lane == 0) {
        const int st = a.stacked[s];
        DUpdStats r;
        r.n_cand = nc; r.n_pos = n_pos; r.n_eval = n_eval; r.n_pass = n_pass; r.dof_eval = dof_e; r.dof_pass = dof_p;
        r.rows = st > 0 ? st : 0;
        r.flags = (st > 0 ? FS_RAN : 0) | (n_eval < n_pos ? FS_CUT : 0);
        r.gamma_eval = g_e; r.gamma_pass = g_p; r.dx_pos = 0.0; r.dx_rot = 0.0;
        if (st > 0) {                                         // (the delta_x dev_apply_update injects)
            const double* dx = a.dx + (size_t)s * a.ld;
            r.dx_rot = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
            r.dx_pos = sqrt(dx[12] * dx[12] + dx[13] * dx[13] + dx[14] * dx[14]);
        }
        out[2 * (size_t)s + (prune ? 1 : 0)] = r;
    }
}

// ------------------------------------------------------------------------------------------------
// dk_mid: the lost-feature update lands in the state (msckf.py:568-595); then the selection half of prune_cam_state_buffer (:712-757)
// ------------------------------------------------------------------------------------------------
// returns (to every thread) the number of pruning candidates of stream s, -1 if the stream does not prune in this step; the
// candidates' records and CSR are written, V.tmp_b flags the ones that still need a position
__device__ __forceinline__ int dk_mid_body(const DevArgs& a, int s, AvsStore* Vout)
{
    __shared__ int red[8], lb[8], s_go, s_r0, s_r1, s_nc;
    __shared__ unsigned long long lds_keys[DEV_LDS_KEYS];
    const int tid = threadIdx.x;
    DState* D = a.st + s;
    if (!D->active) { if (tid == 0) { a.n_cand[s] = 0; a.over[s] = 0; } return -1; }
    dev_apply_update(a, s, D);
    if (tid == 0) {
        int go = !D->failed && D->ncam >= a.max_cam;
        if (D->failed) D->active = 0;
        if (go) { int r0, r1; dev_find_redundant(a, s, *D, &r0, &r1); D->prune = 1; D->rm0 = r0; D->rm1 = r1; D->n_prune_steps += 1; s_r0 = r0; s_r1 = r1; }
        s_go = go;
    }
    __syncthreads();
    if (!s_go) { if (tid == 0) { a.n_cand[s] = 0; a.over[s] = 0; } return -1; }
    AvsTeam T; T.red = red;
    AvsStore V = dev_store(a, s);
    if (a.cap <= DEV_LDS_KEYS) V.keys = lds_keys;
    int* cand = a.cand + (size_t)s * a.cap; int* e0 = a.e0 + (size_t)s * a.cap; int* e1 = a.e1 + (size_t)s * a.cap;
    int nc = 0;
    avs_select_prune(T, V, s_r0, s_r1, cand, e0, e1, &nc);
    dev_build_candidates(a, T, V, s, nc, cand, false, s_r0, s_r1, e0, e1, 1, lb);
    if (tid == 0) s_nc = nc;
    __syncthreads();
    *Vout = V;
    return s_nc;
}
__global__ __launch_bounds__(256, 5) void dk_mid(DevArgs a)
{
    AV_FILTER_PRIO();
    AvsStore V;
    (void)dk_mid_body(a, blockIdx.x, &V);
}
// dk_mid + the landmark records of the lost-feature update (av_msckf_batch_set_landmarks), written while its feature arrays stand
__global__ __launch_bounds__(256, 5) void dk_mid_lm(DevArgs a, LmOut L)
{
    AV_FILTER_PRIO();
    if (threadIdx.x < 64) dev_landmarks(a, blockIdx.x, L, false);
    __syncthreads();                                          // (the other wavefronts rebuild the arrays the writer reads)
    AvsStore V;
    (void)dk_mid_body(a, blockIdx.x, &V);
}
// dk_mid / dk_mid_lm + block 0 of the innovation statistics (av_msckf_batch_set_stats): the lost-feature update's gates, read while its
// feature arrays stand; a stream that takes no part in the step gets zeros
template <bool LM>
__device__ __forceinline__ void dk_mid_st_body(const DevArgs& a, const LmOut& L, DUpdStats* st)
{
    AV_FILTER_PRIO();
    const int s = blockIdx.x;
    if (threadIdx.x < 64) {
        if constexpr (LM) dev_landmarks(a, s, L, false);
        if (a.st[s].active) dev_stats(a, s, st, false);       // (wavefront-uniform)
        else dev_stats_zero(st, s, 0, 1);
    }
    __syncthreads();                                          // (the other wavefronts rebuild the arrays the first one reads)
    AvsStore V;
    (void)dk_mid_body(a, s, &V);
}
__global__ __launch_bounds__(256, 5) void dk_mid_st(DevArgs a, DUpdStats* st) { dk_mid_st_body<false>(a, LmOut{}, st); }
__global__ __launch_bounds__(256, 5) void dk_mid_lm_st(DevArgs a, LmOut L, DUpdStats* st) { dk_mid_st_body<true>(a, L, st); }

// ------------------------------------------------------------------------------------------------
// dk_finish: the pruning update lands in the state, the two camera states leave (msckf.py:774-786), online_reset (:821-843),
// publish (:845-867)
// ------------------------------------------------------------------------------------------------
// Odometry covariance (include/airvision.h, "Odometry covariance"): C = J P[0:21, 0:21] J^T of the stream as it is PUBLISHED -- the
// pruning update and the camera removal are in, online_reset has not run -- in the error coordinates p, theta, v, p_c, theta_c.  The upper
// triangle, row-major, 120 doubles; NaN where the step does not publish.  The first wavefront of the workgroup does the work: the 21 x 21
// block and the six rows of J that are not selections (record rows 9:15) are staged in LDS, every entry of the triangle is computed once.
// Entries of rows 0:9 x columns 0:9 are copies of the entries of P they select; rows 0:9 x columns 9:15 are one 21-term sum (the zeros of J
// multiply to exact zeros), the 6 x 6 corner is two nested ones.
constexpr int ODOM_COV_DOUBLES = 120;
// (The forecast, dk_forecast_cov, takes its record through this very function: it reads a.P, a.pstride, a.ld and of *D the flags, q, R_ic and
//  t_ci, nothing else, so a caller may hand it any 21 x 21 block and state by way of copies of the two records.)
__device__ __forceinline__ void dev_odom_cov(const DevArgs& a, int s, const DState* D, double* rec)
{
    __shared__ double Ps[IMU_DIM * IMU_DIM], Jl[6 * IMU_DIM];
    const int tid = threadIdx.x, N = IMU_DIM;
    if (!(D->active && !D->failed)) {                        // (workgroup-uniform: nobody writes the state between the removal's barrier and the reset's)
        if (tid < 64) for (int e = tid; e < ODOM_COV_DOUBLES; e += 64) rec[e] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double* P = a.P + (size_t)s * a.pstride;
    for (int i = tid; i < N * N; i += (int)blockDim.x) { const int r = i / N, c = i - r * N; Ps[i] = P[(size_t)r * a.ld + c]; }
    for (int i = tid; i < 6 * N; i += (int)blockDim.x) Jl[i] = 0.0;
    __syncthreads();
    if (tid == 0) {
        double Rbw[9];                                        // to_rotation(q): world -> body; R_wb is its transpose
        h_to_rotation(D->q, Rbw);
        const double tx = D->t_ci[0], ty = D->t_ci[1], tz = D->t_ci[2];
        for (int r = 0; r < 3; ++r) {
            const double r0 = Rbw[r], r1 = Rbw[3 + r], r2 = Rbw[6 + r];      // row r of R_wb
            // p_c = p + R_wb t_ci:  d p  -  R_wb [t_ci]x d theta  +  R_wb d t_ci
            Jl[r * N + 0] = -(r1 * tz - r2 * ty); Jl[r * N + 1] = -(r2 * tx - r0 * tz); Jl[r * N + 2] = -(r0 * ty - r1 * tx);
            Jl[r * N + 12 + r] = 1.0;
            Jl[r * N + 18] = r0; Jl[r * N + 19] = r1; Jl[r * N + 20] = r2;
            // theta_c = R_ic d theta + d theta_ext
            for (int c = 0; c < 3; ++c) Jl[(3 + r) * N + c] = D->R_ic[r * 3 + c];
            Jl[(3 + r) * N + 15 + r] = 1.0;
        }
    }
    __syncthreads();
    if (tid < 64) {
        for (int e = tid; e < ODOM_COV_DOUBLES; e += 64) {
            int i = 0, j = e;
            while (j >= 15 - i) { j -= 15 - i; ++i; }
            j += i;                                           // entry (i, j), i <= j, of the 15 x 15 record
            const int si = i < 3 ? 12 + i : (i < 6 ? i - 3 : i);      // state index that record row i selects (i < 9)
            double v;
            if (j < 9) {
                const int sj = j < 3 ? 12 + j : (j < 6 ? j - 3 : j);
                v = Ps[si * N + sj];
            } else if (i < 9) {
                v = 0.0;
                for (int l = 0; l < N; ++l) v += Ps[si * N + l] * Jl[(j - 9) * N + l];
            } else {
                v = 0.0;
                for (int k = 0; k < N; ++k) {
                    double m = 0.0;
                    for (int l = 0; l < N; ++l) m += Ps[k * N + l] * Jl[(j - 9) * N + l];
                    v += Jl[(i - 9) * N + k] * m;
                }
            }
            rec[e] = v;
        }
    }
}

// COV: the instance that also writes the stream's odometry-covariance record (dk_finish_cov); LM: the one that also appends the pruning
// update's landmark records (dk_finish_lm); STATS: the one that also writes block 1 of the innovation statistics (dk_finish_st); all
// false: dk_finish as it always was
template <bool COV, bool LM, bool STATS = false>
__device__ __forceinline__ void dk_finish_body(const DevArgs& a, int s, double* odom, const LmOut& L, DUpdStats* stats = nullptr)
{
    __shared__ int red[8], s_reset;
    const int tid = threadIdx.x;
    DState* D = a.st + s;
    double* o = a.out + (size_t)s * 12;
    if (D->active && D->prune) {
        dev_apply_update(a, s, D);                            // (a.stacked = the pruning phase's stacked rows here)
        if (tid == 0 && D->failed) D->active = 0;
        __syncthreads();
    }
    if constexpr (LM) {
        // the pruning candidates' records, while tmp_b, m_nobs and the feature arrays stand (the removal below changes them); a stream that
        // has stopped publishes nothing, its lost-feature records of this step included
        if (tid < 64) {
            if (!D->active) { if (tid == 0) { L.n[2 * (size_t)s] = 0; L.n[2 * (size_t)s + 1] = 0; } }
            else if (D->prune) dev_landmarks(a, s, L, true);
        }
        __syncthreads();
    }
    if constexpr (STATS) {
        // the pruning update's gates, while its feature arrays stand; no pruning in this step: a zero block; a stream that has stopped or
        // takes no part: both blocks zero, the lost-feature block of this step included
        if (tid < 64) {
            if (!D->active) dev_stats_zero(stats, s, 0, 2);
            else if (D->prune) dev_stats(a, s, stats, true);
            else dev_stats_zero(stats, s, 1, 1);
        }
        __syncthreads();
    }
    if (D->active && D->prune) {
        AvsTeam T; T.red = red;
        const AvsStore V = dev_store(a, s);
        double* P = a.P + (size_t)s * a.pstride; double* scr = a.scratch + (size_t)s * a.pstride;
        const int i0 = D->rm0, i1 = D->rm1, n = D->n;
        remove_two_cams_body(P, scr, n, a.ld, IMU_DIM + 6 * i0, IMU_DIM + 6 * i1);       // (i0 < i1: window positions ascending)
        avs_remove_frame(T, V, i1);
        avs_remove_frame(T, V, i0);
        if (tid == 0) {                                       // the two camera states leave the window (ascending positions stay ascending)
            const size_t c0 = (size_t)s * a.cs;
            int w = 0;
            for (int k = 0; k < D->ncam; ++k) {
                if (k == i0 || k == i1) continue;
                if (w != k) {
                    a.cam_id[c0 + w] = a.cam_id[c0 + k];
                    for (int e = 0; e < 4; ++e) { a.cam_q[4 * (c0 + w) + e] = a.cam_q[4 * (c0 + k) + e]; a.cam_qn[4 * (c0 + w) + e] = a.cam_qn[4 * (c0 + k) + e]; }
                    for (int e = 0; e < 3; ++e) a.cam_p[3 * (c0 + w) + e] = a.cam_p[3 * (c0 + k) + e];
                }
                ++w;
            }
            D->ncam -= 2; D->n -= 12;
            a.ncam[s] = D->ncam; a.nstate[s] = D->n;
        }
        __syncthreads();
    }
    // publish + online_reset
    if (tid == 0) {
        o[0] = D->failed ? -1.0 : (D->active ? 1.0 : 0.0); o[1] = D->ts;
        for (int i = 0; i < 3; ++i) { o[2 + i] = D->p[i]; o[9 + i] = D->v[i]; }
        for (int i = 0; i < 4; ++i) o[5 + i] = D->q[i];
        int reset = 0;
        if (D->active && a.pos_std_thr > 0) {
            const double* P = a.P + (size_t)s * a.pstride;
            const double m = fmax(sqrt(P[(size_t)12 * a.ld + 12]), fmax(sqrt(P[(size_t)13 * a.ld + 13]), sqrt(P[(size_t)14 * a.ld + 14])));
            reset = m >= a.pos_std_thr;                       // (a NaN deviation does not reset, as in the reference's comparison)
        }
        s_reset = reset;
    }
    if constexpr (COV) dev_odom_cov(a, s, D, odom + (size_t)s * ODOM_COV_DOUBLES);      // reads P and the state: before the reset's barrier
    __syncthreads();
    if (s_reset) {
        AvsTeam T; T.red = red;
        const AvsStore V = dev_store(a, s);
        avs_clear(T, V);
        double* P = a.P + (size_t)s * a.pstride;
        for (int i = tid; i < IMU_DIM * IMU_DIM; i += (int)blockDim.x) {     // reset_state_cov (msckf.py:788-798)
            const int r = i / IMU_DIM, c = i - r * IMU_DIM;
            double v = 0.0;
            if (r == c) { const int blk[5] = {3, 6, 9, 15, 18}; for (int k = 0; k < 5; ++k) if (r >= blk[k] && r < blk[k] + 3) v = a.cov0[k]; }
            P[(size_t)r * a.ld + c] = v;
        }
        if (tid == 0) { D->ncam = 0; D->n = IMU_DIM; D->resets += 1; a.ncam[s] = 0; a.nstate[s] = IMU_DIM; }
    }
}
__global__ __launch_bounds__(256, 5) void dk_finish(DevArgs a)
{
    AV_FILTER_PRIO();
    dk_finish_body<false, false>(a, blockIdx.x, nullptr, LmOut{});
}
// dk_finish + the odometry-covariance record of every stream (av_msckf_batch_set_odom_cov), odom = [S][ODOM_COV_DOUBLES]
__global__ __launch_bounds__(256, 5) void dk_finish_cov(DevArgs a, double* odom)
{
    AV_FILTER_PRIO();
    dk_finish_body<true, false>(a, blockIdx.x, odom, LmOut{});
}
// dk_finish / dk_finish_cov + the landmark records of the pruning update (av_msckf_batch_set_landmarks)
__global__ __launch_bounds__(256, 5) void dk_finish_lm(DevArgs a, LmOut L)
{
    AV_FILTER_PRIO();
    dk_finish_body<false, true>(a, blockIdx.x, nullptr, L);
}
__global__ __launch_bounds__(256, 5) void dk_finish_cov_lm(DevArgs a, double* odom, LmOut L)
{
    AV_FILTER_PRIO();
    dk_finish_body<true, true>(a, blockIdx.x, odom, L);
}
// the four above + block 1 of the innovation statistics (av_msckf_batch_set_stats)
__global__ __launch_bounds__(256, 5) void dk_finish_st(DevArgs a, DUpdStats* st)
{
    AV_FILTER_PRIO();
    dk_finish_body<false, false, true>(a, blockIdx.x, nullptr, LmOut{}, st);
}
__global__ __launch_bounds__(256, 5) void dk_finish_cov_st(DevArgs a, double* odom, DUpdStats* st)
{
    AV_FILTER_PRIO();
    dk_finish_body<true, false, true>(a, blockIdx.x, odom, LmOut{}, st);
}
__global__ __launch_bounds__(256, 5) void dk_finish_lm_st(DevArgs a, LmOut L, DUpdStats* st)
{
    AV_FILTER_PRIO();
    dk_finish_body<false, true, true>(a, blockIdx.x, nullptr, L, st);
}
__global__ __launch_bounds__(256, 5) void dk_finish_cov_lm_st(DevArgs a, double* odom, LmOut L, DUpdStats* st)
{
    AV_FILTER_PRIO();
    dk_finish_body<true, true, true>(a, blockIdx.x, odom, L, st);
}

// ------------------------------------------------------------------------------------------------
// Forecast (include/airvision.h, "Forecast"; launched behind the step's last per-stream kernel only when av_msckf_batch_set_forecast is
// on): the state and the covariance of the IMU block as the step LEAVES them -- both updates, the camera removal and online_reset are in --
// carried through the IMU samples the stream's buffer held beyond the frame time when the step was submitted.  The host stages those
// pending samples behind the stream's own in a.imu[] and addresses them by pend[s] = (first, had, staged): had were pending, the first
// staged = min(had, cap) of them lie at a.imu[first ..] and are integrated.  Both kernels only READ what the filter reads: DState, P, the step's own a.prop[] / a.cov[] records stay as they are.
//   dk_forecast_state  a LANE per stream, like dk_state: the serial chain on a private copy of DState, sample by sample exactly what
//                      dk_state does with a sample (dev_predict_new_state, the null states advanced as process_model does), one PropArgs
//                      per sample into a.prop[first + k], the region behind the step's own records.  Nothing goes back to a.st.
//   dk_forecast_cov    ONE wavefront per stream at every launch shape: the 21 x 21 block of P staged in LDS, propagate_body<true, 64> per
//                      sample on that copy (the camera blocks are not needed: the IMU block depends on nothing else), the 15 x 15 record
//                      by dev_odom_cov from the LDS copy with J at the last written record's orientation, the 112-byte records gathered
//                      a lane per double as dk_imu_rate does, the count pair; (0, 0) and a NaN row for a stream that does not publish.
// Plain vector stores: no atomics.
// ------------------------------------------------------------------------------------------------
struct FcOut { DImuState* rec; int* n; double* cov; int cap; const int* pend; };      // [S][cap] records, [S][2] counts (had, written), [S][120]; [S][3] (first, had, staged) of the slot
__device__ __forceinline__ bool dev_forecast_publishes(const DState* D) { return D->active && !D->failed; }
__global__ __launch_bounds__(64) void dk_forecast_state(DevArgs a, FcOut F)
{
    AV_FILTER_PRIO();
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.S) return;
    if (!dev_forecast_publishes(a.st + s)) return;
    DState L = a.st[s];                                       // a private copy of the state: never written back
    DState* D = &L;
    const int first = F.pend[3 * (size_t)s], st = F.pend[3 * (size_t)s + 2], wr = st < F.cap ? st : F.cap;
    for (int k = 0; k < wr; ++k) {                            // (dk_state's loop over the frame's samples, on the copy)
        PropArgs pa;
        const DImu m = a.imu[first + k];
        pa.P = nullptr; pa.n = D->n; pa.ld = a.ld; pa.dt = m.t - D->ts;
        for (int i = 0; i < 3; ++i) { pa.gyro[i] = m.w[i] - D->bg[i]; pa.acc[i] = m.a[i] - D->ba[i]; pa.gravity[i] = D->gravity[i]; }
        for (int i = 0; i < 4; ++i) { pa.q_old[i] = D->q[i]; pa.noise[i] = a.noise[i]; }
        dev_predict_new_state(*D, pa.dt, pa.gyro, pa.acc);
        for (int i = 0; i < 4; ++i) { pa.q_new[i] = D->q[i]; pa.q_null[i] = D->qn[i]; }
        for (int i = 0; i < 3; ++i) { pa.v_null[i] = D->vn[i]; pa.p_null[i] = D->pn[i]; pa.v_new[i] = D->v[i]; pa.p_new[i] = D->p[i]; }
        for (int i = 0; i < 4; ++i) D->qn[i] = D->q[i];
        for (int i = 0; i < 3; ++i) { D->pn[i] = D->p[i]; D->vn[i] = D->v[i]; }
        D->ts = m.t;
        a.prop[first + k] = pa;
    }
}
__global__ __launch_bounds__(64) void dk_forecast_cov(DevArgs a, FcOut F)
{
    AV_FILTER_PRIO();
    __shared__ double P11s[IMU_DIM * IMU_DIM], PhiT[IMU_DIM * IMU_DIM], work[PROP_LDS_DOUBLES];
    const int s = blockIdx.x, lane = threadIdx.x, N = IMU_DIM;
    const DState* D = a.st + s;
    double* cov = F.cov + (size_t)s * ODOM_COV_DOUBLES;
    if (!dev_forecast_publishes(D)) {                         // (wavefront-uniform)
        if (lane == 0) { F.n[2 * (size_t)s] = 0; F.n[2 * (size_t)s + 1] = 0; }
        for (int e = lane; e < ODOM_COV_DOUBLES; e += 64) cov[e] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const int first = F.pend[3 * (size_t)s], had = F.pend[3 * (size_t)s + 1], st = F.pend[3 * (size_t)s + 2], wr = st < F.cap ? st : F.cap;
    if (lane == 0) { F.n[2 * (size_t)s] = had; F.n[2 * (size_t)s + 1] = wr; }
    const double* P = a.P + (size_t)s * a.pstride;
    for (int i = lane; i < N * N; i += 64) { const int r = i / N, c = i - r * N; P11s[i] = P[(size_t)r * a.ld + c]; PhiT[i] = r == c ? 1.0 : 0.0; }
    __syncthreads();
    for (int k = 0; k < wr; ++k) propagate_body<true, 64, 1>(a.prop[first + k], P11s, PhiT, work);        // each ends on a barrier
    // the 15 x 15 record by the map dk_finish_cov uses, dev_odom_cov, from the propagated block in LDS: copies of the two records it reads,
    // P = the LDS block as stream 0 with leading dimension 21, q = the last written record's
    DevArgs al = a; al.P = P11s; al.pstride = 0; al.ld = N;
    DState Dl = *D;
    if (wr > 0) for (int i = 0; i < 4; ++i) Dl.q[i] = a.prop[first + wr - 1].q_new[i];
    dev_odom_cov(al, 0, &Dl, cov);
    constexpr int W = (int)(sizeof(DImuState) / 8);
    double* out = reinterpret_cast<double*>(F.rec + (size_t)s * F.cap);
    for (int e = lane; e < wr * W; e += 64) {
        const int j = e / W, f = e - j * W;
        const size_t i = (size_t)first + j;
        const PropArgs& pa = a.prop[i];
        out[e] = f == 0 ? a.imu[i].t : (f < 4 ? pa.p_new[f - 1] : (f < 8 ? pa.q_new[f - 4] : (f < 11 ? pa.v_new[f - 8] : pa.gyro[f - 11])));
    }
}

// ------------------------------------------------------------------------------------------------
// Zero-velocity update (include/airvision.h, "Zero-velocity update"; both kernels launched only when av_msckf_batch_set_zupt is on).  ONE
// wavefront per stream at every launch shape, plain vector stores, no atomics, no allocation; their arguments travel in ZuArgs, so DCtl
// and DevArgs are what they were and the step's other kernels compile to the code they had.
//   dk_zupt_detect  behind the prediction's launches (dk_state .. dk_begin4 .. dk_cov), ahead of the lost-feature phase: is the stream at
//                   rest in this step?  Read-only for the filter; writes the stream's record z.rec[s] and nothing else.
//                   IMU test: over the bias-corrected samples the step consumed, a.prop[first .. first + cnt) of a.cov[s], a lane per
//                   sample, strided: |gyro| <= gyro_max and | |acc| - |gravity| | <= acc_dev_max for every one of them (a NaN fails), and
//                   cnt >= 1; the two maxima go into the record.
//                   Vision test: over the entries of the frame dk_begin4 has just appended, order[hdr[AVS_N_ORDER] - 1], a lane per entry,
//                   strided: tracked = the entry has a previous observation (fr_prev >= 0), still = tracked and its cam0 point moved at
//                   most disparity_max (normalised units) against that observation.  Counts by ballot and popcount: integers, the same
//                   at every launch shape.  vis_ok = n_tracked >= min_tracks and 100 n_still >= still_percent n_tracked.
//                   A stream that takes no part in the step (a.cov[s].act == 0) or that the append has stopped reads a zero record; its
//                   two totals stay.
//   dk_zupt_update  behind the step's dk_finish* instance, ahead of the forecast: for a stream that is active, not failed and DETECTED,
//                   measurement_update (msckf.py:548-602) with H = the selection of state columns 6..8, r = -v and velocity_sigma^2 in
//                   place of observation_noise, on the state the step LEAVES (both updates, the camera removal and online_reset are in;
//                   the 12 published doubles are not rewritten).  S = P[6:9, 6:9] + sigma^2 I is 3 x 3: its Cholesky factor L in
//                   registers, every lane the same; S^-1 = L^-T L^-1 is applied as such, explicitly, no QR and no general solver.
//                   gamma = |L^-1 r|^2.  gate > 0 and gamma > gate: AV_ZU_GATED, nothing touched.  A pivot that is not positive and
//                   finite: AV_ZU_BAD, nothing touched, the stream is not failed.  Otherwise Y = C L^-T with C = P[:, 6:9] (n x 3) and
//                   delta_x = Y (L^-1 r) are staged in LDS (4 n doubles: 5,280 B at n = 165), one barrier, then P[i][j] -= y_i . y_j
//                   for i <= j only, the value stored at [i][j] and [j][i]: P stays bit-symmetric and nothing outside the n x n block of
//                   the ld-wide region is read or written.  delta_x lands through dev_inject_imu / dev_inject_cam, null-state aliasing
//                   included: lane 0 the IMU state, a lane per camera state.
// ------------------------------------------------------------------------------------------------
enum { ZU_IMU_OK = 1, ZU_VIS_OK = 2, ZU_DETECTED = 4, ZU_APPLIED = 8, ZU_GATED = 16, ZU_BAD = 32 };
struct DZupt { int flags, n_imu, n_tracked, n_still, detected_total, applied_total; double w_max, a_dev_max, v_norm, gamma, dx_pos; };
static_assert(sizeof(DZupt) == 64, "av_zupt is 64 bytes");
struct ZuArgs { DZupt* rec; double gyro_max, acc_dev_max, disparity_max, velocity_sigma, gate; int min_tracks, still_percent; };      // rec: [S]

__global__ __launch_bounds__(64) void dk_zupt_detect(DevArgs a, ZuArgs z)
{
    AV_FILTER_PRIO();
    const int s = blockIdx.x, lane = threadIdx.x;
    const DCov& cv = a.cov[s];
    const DState* D = a.st + s;
    DZupt* R = z.rec + s;
    if (!(cv.act && D->active && !D->failed)) {               // (wavefront-uniform)
        if (lane == 0) { R->flags = 0; R->n_imu = 0; R->n_tracked = 0; R->n_still = 0; R->w_max = 0.0; R->a_dev_max = 0.0; R->v_norm = 0.0; R->gamma = 0.0; R->dx_pos = 0.0; }
        return;
    }
    const int cnt = cv.cnt, first = cv.first;
    double w_max = 0.0, a_max = 0.0;
    int imu_fail = 0;
    for (int k = lane; k < cnt; k += 64) {
        const PropArgs& pa = a.prop[first + k];
        const double w = h_norm3(pa.gyro), ad = fabs(h_norm3(pa.acc) - h_norm3(pa.gravity));
        if (!(w <= z.gyro_max && ad <= z.acc_dev_max)) imu_fail = 1;
        w_max = fmax(w_max, w); a_max = fmax(a_max, ad);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { w_max = fmax(w_max, __shfl_xor(w_max, d)); a_max = fmax(a_max, __shfl_xor(a_max, d)); }
    const int imu_ok = cnt >= 1 && __ballot(imu_fail) == 0ull;
    const AvsStore V = dev_store(a, s);
    const int n_order = V.hdr[AVS_N_ORDER];
    const int slot = n_order > 0 ? V.order[n_order - 1] : -1;
    const int ne = slot >= 0 ? V.fr_n[slot] : 0;
    const double dm2 = z.disparity_max * z.disparity_max;
    int n_tracked = 0, n_still = 0;
    for (int base = 0; base < ne; base += 64) {
        const int i = base + lane;
        int tracked = 0, still = 0;
        if (i < ne) {
            const size_t e = (size_t)slot * V.cap + i;
            const int pl = V.fr_prev[e];
            if (pl >= 0) {
                tracked = 1;
                const double* z1 = V.fr_z + 4 * e;
                const double* z0 = V.fr_z + 4 * ((size_t)avs_lslot(pl) * V.cap + avs_lidx(pl));
                const double du = z1[0] - z0[0], dv = z1[1] - z0[1];
                still = du * du + dv * dv <= dm2;
            }
        }
        n_tracked += __popcll(__ballot(tracked)); n_still += __popcll(__ballot(still));
    }
    if (lane == 0) {
        const int vis_ok = n_tracked >= z.min_tracks && 100ll * n_still >= (long long)z.still_percent * n_tracked;
        const int det = imu_ok && vis_ok;
        R->flags = (imu_ok ? ZU_IMU_OK : 0) | (vis_ok ? ZU_VIS_OK : 0) | (det ? ZU_DETECTED : 0);
        R->n_imu = cnt; R->n_tracked = n_tracked; R->n_still = n_still;
        R->detected_total += det;
        R->w_max = w_max; R->a_dev_max = a_max; R->v_norm = 0.0; R->gamma = 0.0; R->dx_pos = 0.0;
    }
}

__global__ __launch_bounds__(64) void dk_zupt_update(DevArgs a, ZuArgs z)
{
    AV_FILTER_PRIO();
    extern __shared__ double zu_lds[];                        // Y [n][3], delta_x [n]; the launch gives 4 ld doubles
    const int s = blockIdx.x, lane = threadIdx.x;
    DState* D = a.st + s;
    DZupt* R = z.rec + s;
    if (!(D->active && !D->failed && (R->flags & ZU_DETECTED))) return;      // (wavefront-uniform)
    const int n = D->n, ld = a.ld, ncam = D->ncam;
    double* P = a.P + (size_t)s * a.pstride;
    double* Y = zu_lds; double* dxl = zu_lds + 3 * (size_t)n;
    const double s2 = z.velocity_sigma * z.velocity_sigma;
    const double s00 = P[(size_t)6 * ld + 6] + s2, s01 = P[(size_t)6 * ld + 7], s02 = P[(size_t)6 * ld + 8];
    const double s11 = P[(size_t)7 * ld + 7] + s2, s12 = P[(size_t)7 * ld + 8], s22 = P[(size_t)8 * ld + 8] + s2;
    // S = L L^T; a pivot that is not positive and finite makes everything behind it NaN
    const double l00 = sqrt(s00), l10 = s01 / l00, l20 = s02 / l00;
    const double d1 = s11 - l10 * l10, l11 = sqrt(d1), l21 = (s12 - l20 * l10) / l11;
    const double d2 = s22 - l20 * l20 - l21 * l21, l22 = sqrt(d2);
    const double v0 = D->v[0], v1 = D->v[1], v2 = D->v[2];
    const double r0 = (-v0) / l00, r1 = (-v1 - l10 * r0) / l11, r2 = (-v2 - l20 * r0 - l21 * r1) / l22;      // L^-1 r
    const double gamma = r0 * r0 + r1 * r1 + r2 * r2;
    const double v_norm = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    const bool gated = z.gate > 0.0 && gamma > z.gate;
    const bool bad = !(s00 > 0.0 && d1 > 0.0 && d2 > 0.0 && isfinite(s00) && isfinite(d1) && isfinite(d2) && isfinite(s01) && isfinite(s02) && isfinite(s12));
    if (gated || bad) {                                       // (wavefront-uniform: every lane holds the same numbers)
        if (lane == 0) { R->flags |= gated ? ZU_GATED : ZU_BAD; R->v_norm = v_norm; R->gamma = gamma; }
        return;
    }
    for (int i = lane; i < n; i += 64) {
        const double* c = P + (size_t)i * ld + 6;
        const double y0 = c[0] / l00, y1 = (c[1] - l10 * y0) / l11, y2 = (c[2] - l20 * y0 - l21 * y1) / l22;
        Y[3 * i] = y0; Y[3 * i + 1] = y1; Y[3 * i + 2] = y2;
        dxl[i] = y0 * r0 + y1 * r1 + y2 * r2;
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const double y0 = Y[3 * i], y1 = Y[3 * i + 1], y2 = Y[3 * i + 2];
        for (int j = i + lane; j < n; j += 64) {
            const double v = P[(size_t)i * ld + j] - (y0 * Y[3 * j] + y1 * Y[3 * j + 1] + y2 * Y[3 * j + 2]);
            P[(size_t)i * ld + j] = v; P[(size_t)j * ld + i] = v;
        }
    }
    if (lane == 0) {
        dev_inject_imu(*D, dxl);
        R->flags |= ZU_APPLIED; R->applied_total += 1;
        R->v_norm = v_norm; R->gamma = gamma;
        R->dx_pos = sqrt(dxl[12] * dxl[12] + dxl[13] * dxl[13] + dxl[14] * dxl[14]);
    }
    if (lane < ncam) {
        const size_t c = (size_t)s * a.cs + lane;
        dev_inject_cam(a.cam_q + 4 * c, a.cam_p + 3 * c, dxl + IMU_DIM + 6 * lane);
    }
}

// ------------------------------------------------------------------------------------------------
// dk_restart: stream restart (include/airvision.h, "Stream restart"; host side: dev_restart).  No step launches it.  One workgroup per
// LISTED stream, s = list[blockIdx.x] (the host has checked every index against S and removed repeats), on the group's own stream, so a
// step enqueued behind it finds the stream as dev_reserve first made it:
//   DState      zero, q = qn = identity, n = 21, first_img = 1, v / t_ci / R_ic / gravity of the batch's create call; its two run counters
//               (n_prune_steps, n_two_pass) are handed to the host first (carry), which keeps av_msckf_batch_counters accumulating
//   nstate, ncam, grav  21, 0, 0
//   P           the stream's WHOLE pstride region: zero, the create-time diagonal in the 21 x 21 block.  A new batch holds zeros outside
//               the live block, a used one the rows and columns of camera states that have left; the augmentation and the updates write
//               what they read there, but the region is cleared rather than that argued for every kernel.
//   store       avs_restart: empty window and map, births and the whole header zero (avs_clear alone leaves births and the sticky
//               hdr[AVS_OVERFLOW]), every persistent array as allocated
//   outputs     the stream's rows of out, of the odometry-covariance, landmark (records and counts) and statistics buffers: zero, as
//               allocated; likewise the IMU-rate and the forecast records and counts and the forecast covariance.  Every step rewrites them for every stream; they are cleared so that a
//               read of the buffers finds no old life.  The stream's zero-velocity record, its two run-wide totals included: zero.
// Not touched: Pn, T, Kt, scratch, the block buffers, the per-phase feature arrays and lists, the store's scratch -- every step writes
// what it reads of them; `work` (av_msckf_batch_work accumulates).  Overflow pool: a stream holds NO pool rows between steps.  The pool
// is a bump counter, cnt[4] of the step's counter set, zeroed for every step by the step before it (dk_state: cnt_next); a stream's
// share is the offset dev_build_candidates adds to its f_rowoff for that phase only.  There is nothing to hand back.
// Plain vector stores: no atomics, no LDS (the team's scan is not used: red stays null).
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(DState) % 8 == 0, "dk_restart clears DState by 8-byte words");
struct DRestart {
    const int* list; int* carry;                              // [n] streams; [n][2] the counters they held
    double v0[3], t_ci[3], gravity[3], R_ic[9];               // create-time values of the batch
    double* odom; LmOut lm; DUpdStats* stats; IrOut ir; FcOut fc;      // the optional outputs (null: off)
    DZupt* zupt;                                               // the zero-velocity records [S] (null: off)
};
__global__ __launch_bounds__(256) void dk_restart(DevArgs a, DRestart r)
{
    const int s = r.list[blockIdx.x], tid = threadIdx.x, nt = blockDim.x;
    if (s < 0 || s >= a.S) return;                            // (never: the host checks; keeps a bad list inside the buffers)
    if (tid == 0) {
        DState* Dg = a.st + s;
        r.carry[2 * blockIdx.x] = Dg->n_prune_steps; r.carry[2 * blockIdx.x + 1] = Dg->n_two_pass;
        DState D;
        unsigned long long* w = reinterpret_cast<unsigned long long*>(&D);
        for (int i = 0; i < (int)(sizeof(DState) / 8); ++i) w[i] = 0ull;
        D.q[3] = 1.0; D.qn[3] = 1.0; D.n = IMU_DIM; D.first_img = 1;
        for (int i = 0; i < 3; ++i) { D.v[i] = r.v0[i]; D.t_ci[i] = r.t_ci[i]; D.gravity[i] = r.gravity[i]; }
        for (int i = 0; i < 9; ++i) D.R_ic[i] = r.R_ic[i];
        *Dg = D;
        a.nstate[s] = IMU_DIM; a.ncam[s] = 0;
        for (int i = 0; i < 3; ++i) a.grav[3 * s + i] = 0.0;
        for (int i = 0; i < 12; ++i) a.out[(size_t)s * 12 + i] = 0.0;
        if (r.lm.rec) { r.lm.n[2 * (size_t)s] = 0; r.lm.n[2 * (size_t)s + 1] = 0; }
        if (r.ir.rec) { r.ir.n[2 * (size_t)s] = 0; r.ir.n[2 * (size_t)s + 1] = 0; }
        if (r.fc.rec) { r.fc.n[2 * (size_t)s] = 0; r.fc.n[2 * (size_t)s + 1] = 0; }
    }
    if (r.zupt && tid < (int)(sizeof(DZupt) / 8)) reinterpret_cast<unsigned long long*>(r.zupt + s)[tid] = 0ull;      // the record and both totals
    double* P = a.P + (size_t)s * a.pstride;
    for (size_t i = tid; i < a.pstride; i += nt) {            // reset_state_cov (msckf.py:788-798) in a cleared region
        const int rr = (int)(i / a.ld), c = (int)(i - (size_t)rr * a.ld);
        double v = 0.0;
        if (rr == c && rr < IMU_DIM) { const int blk[5] = {3, 6, 9, 15, 18}; for (int k = 0; k < 5; ++k) if (rr >= blk[k] && rr < blk[k] + 3) v = a.cov0[k]; }
        P[i] = v;
    }
    if (r.odom) for (int i = tid; i < ODOM_COV_DOUBLES; i += nt) r.odom[(size_t)s * ODOM_COV_DOUBLES + i] = 0.0;
    if (r.lm.rec) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(r.lm.rec + (size_t)s * r.lm.cap);
        for (int i = tid; i < r.lm.cap * (int)(sizeof(DLandmark) / 8); i += nt) w[i] = 0ull;
    }
    if (r.stats) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(r.stats + 2 * (size_t)s);
        for (int i = tid; i < 2 * (int)(sizeof(DUpdStats) / 8); i += nt) w[i] = 0ull;
    }
    if (r.ir.rec) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(r.ir.rec + (size_t)s * r.ir.cap);
        for (int i = tid; i < r.ir.cap * (int)(sizeof(DImuState) / 8); i += nt) w[i] = 0ull;
    }
    if (r.fc.rec) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(r.fc.rec + (size_t)s * r.fc.cap);
        for (int i = tid; i < r.fc.cap * (int)(sizeof(DImuState) / 8); i += nt) w[i] = 0ull;
        for (int i = tid; i < ODOM_COV_DOUBLES; i += nt) r.fc.cov[(size_t)s * ODOM_COV_DOUBLES + i] = 0.0;
    }
    AvsTeam T; T.red = nullptr;
    avs_restart(T, dev_store(a, s));
}

// ------------------------------------------------------------------------------------------------
// dk_prune_probe: parity tests only (av_msckf_predict_ops_dev; no step launches it).  Per stream, on the window as it stands:
// ops bit 0: dev_find_redundant -> red[2 s], red[2 s + 1]; bit 1: remove_two_cams_body for the window positions rm[2 s] < rm[2 s + 1],
// with the workgroup's threads as dk_finish has them.  The entry has checked every position against the window.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dk_prune_probe(DevArgs a, const int* ops, const int* rm, int* red)
{
    const int s = blockIdx.x;
    const DState* D = a.st + s;
    if ((ops[s] & 1) && threadIdx.x == 0) { int r0, r1; dev_find_redundant(a, s, *D, &r0, &r1); red[2 * s] = r0; red[2 * s + 1] = r1; }
    if (ops[s] & 2)                                            // (workgroup-uniform)
        remove_two_cams_body(a.P + (size_t)s * a.pstride, a.scratch + (size_t)s * a.pstride, D->n, a.ld, IMU_DIM + 6 * rm[2 * s], IMU_DIM + 6 * rm[2 * s + 1]);
}

}  // namespace

// ---- host-side handles of the device-resident path (functions: msckf_dev_host.inc) ---------------------------------------------
// The optional per-step outputs: ONE entry per array a step may carry beside its poses, in the order of their read-back on the stream.
// A feature is what a caller switches (av_msckf_batch_set_*) and hands a destination for (av_msckf_batch_next_*); its setting is
// 0 = off, else 1 (the landmark map, the IMU-rate odometry and the forecast: records per stream and step).  Their records and counts are
// two arrays of one feature; the forecast has a third, its covariance record.
// Everything else about them -- the batch's settings and next destinations, StepOuts, the device and pinned buffers, their allocation,
// read-back, hand-over and restart -- is an array indexed by this table or a loop over it.  A sixth output: an entry here (and in
// KOuts), its two exported wrappers, and the kernel instances that write it (dk_mid_kernels / dk_finish_kernels, msckf_dev_host.inc) -- or,
// for the IMU-rate odometry, the one kernel dev_launch_predict adds behind dk_state; for the forecast, the two kernels dev_launch_forecast
// adds behind dk_finish*.
enum OutFeat { F_COV, F_LM, F_STATS, F_IR, F_FC, N_FEAT };
enum OutArr { O_COV, O_LM, O_LMN, O_STATS, O_IR, O_IRN, O_FC, O_FCN, O_FCC, N_OUT };
struct OutWords { const char* fn; const char* noun; const char* needs; const char* is; };      // "av_msckf_batch_set_<fn>: <noun> <needs> ...", "<noun> <is> off"
constexpr OutWords W_COV = {"odom_cov", "the odometry covariance", "needs", "is"}, W_LM = {"landmarks", "the landmark map", "needs", "is"},
                   W_STATS = {"stats", "the innovation statistics", "need", "are"}, W_IR = {"imu_rate", "the IMU-rate odometry", "needs", "is"},
                   W_FC = {"forecast", "the forecast", "needs", "is"};
struct OutDesc {
    OutFeat feat; size_t fixed, per_setting; OutWords w;
    size_t bytes(const int* setting) const { return fixed + per_setting * (size_t)setting[feat]; }      // per stream
};
constexpr OutDesc OUTS[N_OUT] = {
    {F_COV, ODOM_COV_DOUBLES * 8, 0, W_COV},         // covariance records
    {F_LM, 0, AV_LANDMARK_BYTES, W_LM},              // landmark records
    {F_LM, 2 * 4, 0, W_LM},                          // landmark counts (had, written)
    {F_STATS, AV_FILTER_STATS_BYTES, 0, W_STATS},    // statistics records (two update blocks)
    {F_IR, 0, AV_IMU_STATE_BYTES, W_IR},             // IMU-rate records
    {F_IR, 2 * 4, 0, W_IR},                          // IMU-rate counts (had, written)
    {F_FC, 0, AV_IMU_STATE_BYTES, W_FC},             // forecast records
    {F_FC, 2 * 4, 0, W_FC},                          // forecast counts (had, written)
    {F_FC, ODOM_COV_DOUBLES * 8, 0, W_FC},           // forecast covariance record
};
constexpr const OutWords& out_words(OutFeat f) { for (int i = 0; i < N_OUT; ++i) if (OUTS[i].feat == f) return OUTS[i].w; return OUTS[0].w; }
// a step's destinations in the caller's memory (NULL: the step has none and the array is dropped)
struct StepOuts {
    void* p[N_OUT] = {};
    StepOuts at(const int* setting, size_t s0) const      // the slice of a group whose first stream is s0
    {
        StepOuts g;
        for (int i = 0; i < N_OUT; ++i) g.p[i] = p[i] ? (char*)p[i] + s0 * OUTS[i].bytes(setting) : nullptr;
        return g;
    }
};
struct KOuts { double* odom; LmOut lm; DUpdStats* stats; IrOut ir; FcOut fc; };      // the device arrays as the kernels' parameter lists and DRestart take them (dev_kouts)
constexpr int DEV_RING = 3;          // steps of a stream group that may be queued at once (inputs / outputs are ring-buffered)
struct DevSlot {
    DCtl* ctl_h = nullptr; DCtl* ctl_d = nullptr;
    DImu* imu_h = nullptr; DImu* imu_d = nullptr; size_t imu_cap = 0;
    PropArgs* prop_d = nullptr;      // [imu_cap] dk_begin -> dk_cov, one record per IMU sample
    int* pend_h = nullptr; int* pend_d = nullptr;      // [S][3] (first, had, staged) of every stream's pending samples in imu_h / imu_d (forecast on; NULL: off)
    long long* ids_h = nullptr; double* uv_h = nullptr; int* n_h = nullptr;      // pinned staging of a feature message that arrives in host arrays
    long long* ids_d = nullptr; double* uv_d = nullptr; int* n_d = nullptr;      // the message on the device (copied from the host arrays or from the front-end's buffers)
    double* out_h = nullptr; int* cnt_h = nullptr;                                // pinned landing zones of the step's only read-back
    char* outs_h[N_OUT] = {};                                                     // pinned landing zones of the step's optional outputs, [S] x the entry's bytes per stream (NULL: the feature is off)
    hipEvent_t done = nullptr;
    hipEvent_t t0[2] = {nullptr, nullptr}, t1[2] = {nullptr, nullptr}; bool t_used[2] = {false, false};      // av_msckf_batch_work: device time of the two phase chains
    bool in_flight = false;
    // the step's launch sequence captured as a HIP graph (small batches: the host's ~50 API calls per step are the bound there)
};
struct DevPath {
    int cap = 0;                     // message capacity the store and the per-feature arrays are built for
    DevArgs A;                       // base pointers and constants (per launch: a copy with the slot's inputs and the phase's results)
    DevSlot slot[DEV_RING];
    double* out_d = nullptr; int* stacked0 = nullptr; int* stacked1 = nullptr; UpdArgs* updbase = nullptr; UpdArgs* upd = nullptr;
    DCov* cov_d = nullptr;           // [S] dk_begin -> dk_cov
    char* outs_d[N_OUT] = {};        // what the dk_mid* / dk_finish* instances write of the optional outputs, [S] x the entry's bytes per stream (NULL: the feature is off)
    int dk_wg = 0;                   // AV_DK_WG read when the path is prepared: 64 / 256 = workgroup size of the per-stream kernels, 0 = by the group's stream count
    int launched_wg = 0;             // workgroup size dev_enqueue launched them with in the last enqueued step (0: no step yet); av_msckf_batch_launch_shape
    int* cols = nullptr; int* blk_row = nullptr; int* blk_len = nullptr; int* clist = nullptr; int* again = nullptr;
    double* work = nullptr; double* gamma = nullptr; int* pass = nullptr;
    int hint[16] = {0};              // list lengths of the last finished step (grids of the next one are sized from them; the kernels stride anyway)
    bool have_hint = false;
    long long growths = 0, steps = 0;
    // stream restart (dk_restart): the index list [S] and the counters the listed streams held [S][2], on the device and pinned; taken
    // with the rest at dev_reserve, so a restart allocates nothing
    int* rs_list_d = nullptr; int* rs_list_h = nullptr; int* rs_carry_d = nullptr; int* rs_carry_h = nullptr;
    DZupt* zupt_d = nullptr;         // [S] zero-velocity records, overwritten every step and read on demand (av_msckf_batch_read_zupt); NULL: the update is off
};
