
// msckf_batch.inc -- S independent MSCKF filters stepped together (included at the end of msckf.hip).
//
// The algorithm of MSCKF.feature_callback (reference: src/msckf.py:177-228 and everything it calls) for all streams at once, with
// the state, the observation map, the selections and the state injection of every stream on the device:
//   msckf_store.h       the observation store (device functions; the same text runs on the host against a dict model in the tests)
//   msckf_dev.inc       the records and the dk_* kernels of a step
//   msckf_dev_host.inc  the host side of a step: dev_launch enqueues the fixed launch sequence, dev_finish collects the published poses
// This file holds what is around them: the batch and its streams' host records (the IMU queue and the gravity / bias initialisation,
// which are the only per-stream work the host does), the work buffers of the update kernels, the stream groups with their worker
// threads, and the exported entry points.
#include <stdlib.h>
#include <deque>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace {

// ---- small fp64 helpers mirroring src/utils.py ----------------------------------------------------
__host__ __device__ inline void h_to_rotation(const double* qin, double* R)
{
    double n = sqrt(qin[0] * qin[0] + qin[1] * qin[1] + qin[2] * qin[2] + qin[3] * qin[3]);
    double x = qin[0] / n, y = qin[1] / n, z = qin[2] / n, w = qin[3] / n, c = 2 * w * w - 1;
    R[0] = c + 2 * x * x;          R[1] = 2 * w * z + 2 * x * y;   R[2] = -2 * w * y + 2 * x * z;
    R[3] = -2 * w * z + 2 * y * x; R[4] = c + 2 * y * y;           R[5] = 2 * w * x + 2 * y * z;
    R[6] = 2 * w * y + 2 * z * x;  R[7] = -2 * w * x + 2 * z * y;  R[8] = c + 2 * z * z;
}
__host__ __device__ inline void h_normalize4(double* q) { double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); for (int i = 0; i < 4; ++i) q[i] /= n; }
__host__ __device__ inline void h_to_quaternion(const double* R, double* q)
{   // utils.py:25-47
    if (R[8] < 0) {
        if (R[0] > R[4]) { q[0] = 1 + R[0] - R[4] - R[8]; q[1] = R[1] + R[3]; q[2] = R[6] + R[2]; q[3] = R[5] - R[7]; }
        else             { q[0] = R[1] + R[3]; q[1] = 1 - R[0] + R[4] - R[8]; q[2] = R[7] + R[5]; q[3] = R[6] - R[2]; }
    } else {
        if (R[0] < -R[4]) { q[0] = R[2] + R[6]; q[1] = R[7] + R[5]; q[2] = 1 - R[0] - R[4] + R[8]; q[3] = R[1] - R[3]; }
        else              { q[0] = R[5] - R[7]; q[1] = R[6] - R[2]; q[2] = R[1] - R[3]; q[3] = 1 + R[0] + R[4] + R[8]; }
    }
    h_normalize4(q);
}
__host__ __device__ inline void h_quat_mul(const double* a_in, const double* b_in, double* o)
{   // utils.py:61-76
    double a[4] = {a_in[0], a_in[1], a_in[2], a_in[3]}, b[4] = {b_in[0], b_in[1], b_in[2], b_in[3]};
    h_normalize4(a); h_normalize4(b);
    o[0] = a[3] * b[0] + a[2] * b[1] - a[1] * b[2] + a[0] * b[3];
    o[1] = -a[2] * b[0] + a[3] * b[1] + a[0] * b[2] + a[1] * b[3];
    o[2] = a[1] * b[0] - a[0] * b[1] + a[3] * b[2] + a[2] * b[3];
    o[3] = -a[0] * b[0] - a[1] * b[1] - a[2] * b[2] + a[3] * b[3];
    h_normalize4(o);
}
__host__ __device__ inline void h_small_angle(const double* dth, double* q)
{   // utils.py:79-93
    double d[3] = {dth[0] / 2., dth[1] / 2., dth[2] / 2.};
    double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (n2 <= 1) { q[0] = d[0]; q[1] = d[1]; q[2] = d[2]; q[3] = sqrt(1 - n2); }
    else { double s = sqrt(1 + n2); q[0] = d[0] / s; q[1] = d[1] / s; q[2] = d[2] / s; q[3] = 1. / s; }
}
__host__ __device__ inline void h_cross(const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
__host__ __device__ inline double h_norm3(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
__host__ __device__ inline void h_from_two_vectors(const double* v0_in, const double* v1_in, double* q)
{   // utils.py:96-120
    double n0 = h_norm3(v0_in), n1 = h_norm3(v1_in);
    double v0[3] = {v0_in[0] / n0, v0_in[1] / n0, v0_in[2] / n0}, v1[3] = {v1_in[0] / n1, v1_in[1] / n1, v1_in[2] / n1};
    double d = v0[0] * v1[0] + v0[1] * v1[1] + v0[2] * v1[2];
    double h[4];
    if (d < -0.999999) {
        double ex[3] = {1, 0, 0}, ax[3];
        h_cross(ex, v0, ax);
        if (h_norm3(ax) < 0.000001) { double ey[3] = {0, 1, 0}; h_cross(ey, v0, ax); }
        h[0] = ax[0]; h[1] = ax[1]; h[2] = ax[2]; h[3] = 0;
    } else if (d > 0.999999) {
        h[0] = h[1] = h[2] = 0; h[3] = 1;
    } else {
        double s = sqrt((1 + d) * 2), ax[3];
        h_cross(v0, v1, ax);
        h[0] = ax[0] / s; h[1] = ax[1] / s; h[2] = ax[2] / s; h[3] = 0.5 * s;
    }
    h_normalize4(h);
    q[0] = -h[0]; q[1] = -h[1]; q[2] = -h[2]; q[3] = h[3];
}
__host__ __device__ inline void h_mtv(const double* R, const double* v, double* o) { for (int i = 0; i < 3; ++i) o[i] = R[0 * 3 + i] * v[0] + R[1 * 3 + i] * v[1] + R[2 * 3 + i] * v[2]; }   // R^T v
__host__ __device__ inline void h_mv(const double* R, const double* v, double* o) { for (int i = 0; i < 3; ++i) o[i] = R[i * 3] * v[0] + R[i * 3 + 1] * v[1] + R[i * 3 + 2] * v[2]; }

struct BImu { double t, w[3], a[3]; };

// The host's record of one stream: its IMU queue, what initialize_gravity_and_bias computed until the device has taken it, and the
// initial state the accessors report before the first step.  From the first step on the state is the device's (DState).
struct BStream {
    std::deque<BImu> imu; std::mutex mu;
    bool gravity_set = false, first_img = true, active = false;
    double gravity_time = 0;                    // timestamp of the IMU sample that completed initialize_gravity_and_bias
    double ts = 0, q[4] = {0, 0, 0, 1}, v[3] = {0, 0, 0}, bg[3] = {0, 0, 0};
    double R_ic[9], t_ci[3], gravity[3];
    int n = IMU_DIM;
    bool dev_init_sent = false;                 // the gravity / bias initialisation has been handed to the device
    // A failure that concerns this stream alone stops THIS stream: it idles from then on (out[s*12] = -1,
    // av_msckf_batch_stream_status tells why) while the other streams of the batch keep running -- the reference's sequences never
    // stop one another.  The device stops a stream in its DState (dev_fail_message); this is the host's own mark.
    int failed = 0; char fail_msg[160] = "";
    // parity-test tap (av_msckf_batch_debug_*): per phase of the last step (0 = remove_lost_features, 1 = prune_cam_state_buffer)
    // the gating values in the reference's evaluation order, delta_x, the stacked rows and the covariance right after the update
    std::vector<double> dbg_gamma[2], dbg_dx[2], dbg_P[2]; int dbg_rows[2] = {0, 0}, dbg_n[2] = {0, 0};
};

}  // namespace

#include "msckf_store.h"
#include "msckf_dev.inc"

struct av_msckf_batch {
    int device = 0, S = 0, max_cam = 0, cam_slots = 0, ld = 0, rows_cap = 0;
    double gravity0[3], T01[16], R_ic0[9], t_ci0[3], cov0[5], noise[4], obs_noise, pos_std_thr, vel0[3];
    double opt5[5]; double trans_thr;
    std::vector<BStream> st;
    size_t pstride = 0, hstride = 0, rstride = 0, wstride = 0;
    double *P = nullptr, *Pn = nullptr, *T = nullptr, *Kt = nullptr, *W = nullptr, *Hblk = nullptr, *rblk = nullptr, *dx = nullptr, *scratch = nullptr, *chi2_dev = nullptr;
    // Owns every device and pinned block, event and stream of this batch or group, the DevPath's included.  Outgrown blocks stay
    // with it until destroy: nothing frees inside a run.
    AvResources res;
    int reserved_cap = 0;                       // message capacity (features per stream) the block buffers are sized for
    // counters of av_msckf_batch_counters (sub-batch; the parent sums its groups): what restarted streams held is added here
    long long n_steps = 0, n_prune_stream_steps = 0, n_two_pass_streams = 0;
    // av_msckf_batch_work: the time the phase chains spent on the device (HIP events of the ring slots around the launches of a phase)
    double w_chain_ms = 0; long long w_chain_dropped = 0;
    bool work_timing = false;
    bool debug_capture = false;
    bool rows_cap_auto = false;                 // rows_cap was sized from a message capacity (create passed 0): it may grow with a wider message
    hipEvent_t ev_wait = nullptr;                // blocking-sync event: a waiting thread sleeps instead of spinning on a core
    // ---- stream groups -----------------------------------------------------------------------------------
    // A batch of many streams is split into G independent sub-batches (disjoint stream ranges, own device buffers,
    // own HIP stream, own worker thread).  One step runs all groups concurrently: two latency chains share the device.
    // Streams never interact, so the results are those of the ungrouped batch.
    std::vector<av_msckf_batch*> subs;          // non-empty on the parent only
    int per_sub = 0;                            // streams per group (the last one may hold fewer)
    hipStream_t own = nullptr;                  // sub: its stream
    std::thread worker; std::mutex wmu; std::condition_variable wcv;
    struct Job { std::function<int()> launch, finish; };
    std::deque<Job> jobs; long long n_submitted = 0, n_done = 0; bool quit = false; int job_rc = 0; char job_err[512] = "";
    DevPath dev{};                              // device-resident state + observation store (msckf_dev.inc); dev.cap == 0 until the first step
    long long dev_seq = 0;                      // steps submitted (ring slot = dev_seq % DEV_RING)
    hipEvent_t ev_msg[4] = {nullptr, nullptr, nullptr, nullptr};      // submit_dev: the message copy of ring slot k has been enqueued
    struct Pending { int slot; double* out; StepOuts outs; };
    std::deque<Pending> direct_pending;         // one group, no worker: steps launched and not yet finished (slot, caller's out, caller's arrays for the optional outputs)
    // the optional outputs (OUTS, msckf_dev.inc).  out_set: every feature's setting (av_msckf_batch_set_*), on the batch and on every
    // group; next_outs: the destinations av_msckf_batch_next_* handed over for the next step (batch only), taken by that step
    int out_set[N_FEAT] = {}; StepOuts next_outs;
    // the zero-velocity update (airvision.h, "Zero-velocity update"; av_msckf_batch_set_zupt): on the batch and on every group
    bool zupt_on = false; av_zupt_params zupt{};
    explicit av_msckf_batch(int n) : st(n) {}
};

namespace {

// the optional outputs' destinations handed over for the next step: taken, and cleared, by the step that is being submitted
inline StepOuts take_outs(av_msckf_batch* b) { const StepOuts o = b->next_outs; b->next_outs = StepOuts(); return o; }

// ---- the kernels' argument records, the part that comes from the batch; the caller (msckf_dev_host.inc) adds what is its own.
//      TriArgs: tri_args_base (msckf.hip).

// A zeroed FeatArgs with the camera states, the covariance, the block buffers, their strides and the constants of the batch.  The caller
// adds the observation CSR, the per-feature arrays (pos, dof, row_off, gamma, pass), and how a feature finds its stream and its gravity.
inline FeatArgs b_feat_args(const av_msckf_batch* b, bool cut1500, const double* cam_q, const double* cam_p, const double* cam_qn)
{
    FeatArgs a; memset(&a, 0, sizeof(a));
    a.cam_q = cam_q; a.cam_p = cam_p; a.cam_qn = cam_qn; a.cam_pn = cam_p;      // position_null aliases position (msckf.py:403-404)
    a.ld = b->ld; a.P = b->P; a.chi2 = b->chi2_dev;
    unpack_T01(b->T01, a.R01, a.t01);                       // (gravity stays zero: every stream has its own, stream_gravity)
    a.obs_noise = b->obs_noise; a.Hout = b->Hblk; a.rout = b->rblk;
    a.cam_stride = b->cam_slots; a.p_stride = b->pstride; a.h_stride = b->hstride; a.r_stride = b->rstride;
    // camera pruning stacks only features seen from BOTH removed cameras and factorises exactly those 12 columns, so every
    // column the update gathers is written by the feature itself: no need to clear 141-wide rows (5.6 KB per feature)
    a.zero_fill = cut1500 ? 1 : 0;
    return a;
}

// The work buffers of the batched update and how they are sized: per stream one p_stride (>= ld * ld doubles) each of T, Kt, Pn and
// Sbuf, upd_w_doubles of W (the transposed copy of [H | r]: ld + 1 columns of ldt = rows_cap entries) and ld doubles of dx.  One place
// for the batch (sub_create, sub_reserve, b_upd_args) and for the parity-test entry av_msckf_update_ops_dev.
inline size_t upd_w_doubles(int rows_cap, int ld) { return (size_t)rows_cap * (ld + 1); }
struct UpdBufs {
    double *P, *Pn, *T, *Kt, *Sbuf, *W, *dx; const double *Hblk, *rblk;
    size_t pstride, hstride, rstride, wstride; int ld, rows_cap; double obs_noise;
};
// A zeroed UpdArgs with the work buffers of stream s and their strides.  The caller adds n, m, nc, mode, its block lists and prof.
inline UpdArgs upd_args_of(const UpdBufs& B, int s)
{
    UpdArgs u; memset(&u, 0, sizeof(u));
    u.P = B.P + (size_t)s * B.pstride; u.ld = B.ld;
    u.Hsrc = B.Hblk + (size_t)s * B.hstride; u.rsrc = B.rblk + (size_t)s * B.rstride;
    u.W = B.W + (size_t)s * B.wstride; u.ldt = B.rows_cap; u.T = B.T + (size_t)s * B.pstride; u.Kt = B.Kt + (size_t)s * B.pstride;
    u.Pn = B.Pn + (size_t)s * B.pstride; u.dx = B.dx + (size_t)s * B.ld; u.obs_noise = B.obs_noise;
    u.Sbuf = B.Sbuf + (size_t)s * B.pstride;
    return u;
}
inline UpdArgs b_upd_args(const av_msckf_batch* b, int s)
{
    // (Sbuf: the removal scratch, free between the camera removals that use it)
    const UpdBufs B{b->P, b->Pn, b->T, b->Kt, b->scratch, b->W, b->dx, b->Hblk, b->rblk, b->pstride, b->hstride, b->rstride, b->wstride, b->ld, b->rows_cap, b->obs_noise};
    return upd_args_of(B, s);
}

// wait for the group's stream: spinning (hipStreamSynchronize) or sleeping on a blocking event (AV_MSCKF_WAIT=block)
int b_wait(av_msckf_batch* b, hipStream_t stm)
{
    static const bool block = [] { const char* e = getenv("AV_MSCKF_WAIT"); return e && !strcmp(e, "block"); }();
    if (block && b->ev_wait) { AV_HIP(hipEventRecord(b->ev_wait, stm)); AV_HIP(hipEventSynchronize(b->ev_wait)); return AV_OK; }
    AV_HIP(hipStreamSynchronize(stm));
    return AV_OK;
}

int b_reset_cov(av_msckf_batch* b, int s, hipStream_t stm)
{   // reset_state_cov (msckf.py:788-798)
    std::vector<double> P0((size_t)IMU_DIM * IMU_DIM, 0.0);
    const int blk[5] = {3, 6, 9, 15, 18};
    for (int k = 0; k < 5; ++k) for (int i = 0; i < 3; ++i) P0[(size_t)(blk[k] + i) * IMU_DIM + blk[k] + i] = b->cov0[k];
    AV_HIP(hipMemcpy2DAsync(b->P + (size_t)s * b->pstride, sizeof(double) * b->ld, P0.data(), sizeof(double) * IMU_DIM,
                            sizeof(double) * IMU_DIM, IMU_DIM, hipMemcpyHostToDevice, stm));
    { int rcw = b_wait(b, stm); if (rcw) return rcw; }
    b->st[s].n = IMU_DIM;
    return AV_OK;
}

}  // namespace

static void sub_destroy(av_msckf_batch* b);
namespace { int dev_launch(av_msckf_batch* b, int k, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap, const double* timestamps, bool dev_msg, hipEvent_t ready, hipStream_t stm); int dev_finish(av_msckf_batch* b, int k, double* out, const StepOuts& outs); int dev_read_state(av_msckf_batch* b, int s, DState* D); const char* dev_fail_message(int code, int* av_code); int dev_reserve(av_msckf_batch* b, int cap); int dev_upload_updbase(av_msckf_batch* b); int dev_restart(av_msckf_batch* b, const int* list, int n, hipStream_t stm); }

// Stream for the filter's kernels.  AV_MSCKF_CUS="first:count" confines them to `count` compute units starting at CU `first`
// (hipExtStreamCreateWithCUMask) -- together with a complementary mask on the caller's front-end stream this partitions the
// chip, so that the filter's latency-bound kernels never queue behind the front-end's resident workgroups.  Without the
// variable: an ordinary stream at the default priority.
static int make_filter_stream(AvResources& res, hipStream_t* out)
{
    const char* e = getenv("AV_MSCKF_CUS");
    int first = 0, count = 0;
    if (e && sscanf(e, "%d:%d", &first, &count) == 2 && count > 0) {
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = first; c < first + count && c < 256; ++c) mask[c >> 5] |= 1u << (c & 31);
        return res.stream_on_cus(out, 8, mask);
    }
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    // The filter's chain never waits for the host, so it runs at the DEFAULT stream priority, not the highest -- the
    // front-end's kernels keep their speed (11.5 instead of 16 ms of spans per 2,048-stream step) and the complete path gains
    // (DESIGN.md section 7: 131 k vs 114 k frames/s).
    return res.stream(out, hipStreamNonBlocking, (lo + hi) / 2);
}

// Rows of the overflow pool behind the last stream's block-buffer region.  A stream whose lost-feature
// candidates reserve more rows than its own region holds (a blank frame drops every track at once: ~4,500 rows) takes the rows
// from here -- one atomic bump per stream and step -- instead of gating first and storing in a second pass: that second pass had to
// be LAUNCHED every step (its list is only known on the device) and, idle as it normally was, waited ~1.1 ms per step for a CU
// with 69 KB of LDS and 4 x 176 registers free beside the front-end (profiles/r04/README.md).  Exhausting the pool stops the stream
// with AV_E_CAPACITY (DFAIL_ROWS).  AV_MSCKF_POOL_ROWS overrides the size.
static size_t b_pool_rows(const av_msckf_batch* b, int rows_cap)
{
    if (rows_cap <= 0) return 0;
    if (const char* e = getenv("AV_MSCKF_POOL_ROWS")) { const long v = atol(e); if (v > 0) return (size_t)v; }
    // Sized for a burst, not for the worst case of every stream at once: one stream in eight losing all its tracks in the same step
    // (each then needs about one region's worth of rows on top of its own), never less than 131,072 rows.  Footprint: rows x ld
    // doubles -- at 1,024 streams per group, rows_cap 4,096 and ld 152 that is 0.64 GB per group (the block buffers themselves:
    // 5.1 GB; the pool was as large again when it held S x rows_cap rows).
    const size_t per = ((size_t)b->S + 7) / 8 * (size_t)rows_cap;
    return per > 131072 ? per : 131072;
}

static int sub_create(int n_streams, int max_cam_states, int rows_cap, const double* chi2_table_100, const double gravity[3],
                                    const double* T_cam0_cam1_rowmajor44, const double* R_imu_cam0_t_cam0_imu12, const double cov_init5[5],
                                    const double noise4[4], double obs_noise, double position_std_threshold, const double velocity0[3],
                                    const double* opt6, int device, av_msckf_batch** out)
{
    if (!out || n_streams <= 0 || max_cam_states < 4 || max_cam_states > 30 || (rows_cap != 0 && rows_cap < 1664) || !chi2_table_100 || !gravity || !T_cam0_cam1_rowmajor44 ||
        !R_imu_cam0_t_cam0_imu12 || !cov_init5 || !noise4 || !velocity0 || !opt6) { av_set_error("av_msckf_batch_create: bad arguments"); return AV_E_INVALID; }
    {   // configurations the LDS layouts cannot hold are rejected here, not at the first long track (160 KB per workgroup):
        // a feature can be observed from every camera state, and the update factorises up to 6 columns per state
        const size_t lf = feature_lds_bytes(max_cam_states), lb = update_back_lds(rows_cap ? rows_cap : 2048, 6 * (max_cam_states + 1));
        if (lf > 160 * 1024 || lb > 160 * 1024) {
            av_set_error("av_msckf_batch_create: max_cam_states %d needs %zu B (feature blocks) / %zu B (update) of LDS, 163840 available", max_cam_states, lf, lb);
            return AV_E_CAPACITY;
        }
    }
    // One back-end pass of the batched update keeps k = min(m, n_c) <= BATCH_KMAX rows (S / T^T tiles, the packed Cholesky triangle
    // in LDS, upd_compress); n_c can reach 6 columns per camera state, so the window must satisfy 6 * max_cam_states <= BATCH_KMAX.
    // (The reference default is 20 -> n_c <= 120; the single-filter API av_msckf_* has no such limit.)
    constexpr int BATCH_KMAX = 144;
    if (6 * max_cam_states > BATCH_KMAX) {
        av_set_error("av_msckf_batch_create: max_cam_states %d: the batched update holds at most %d rows / columns per pass (6 per camera state: max_cam_states <= %d)",
                     max_cam_states, BATCH_KMAX, BATCH_KMAX / 6);
        return AV_E_CAPACITY;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { av_set_error("av_msckf_batch_create: no HIP device visible"); return AV_E_NODEVICE; }
    AV_HIP(hipSetDevice(device));
    // Process-wide, for the OpenMP teams of the library's other translation units (the front-end's per-stream loops, the PNG reader):
    // their idle workers must not spin next to the HIP runtime threads and this batch's group workers.
    setenv("OMP_WAIT_POLICY", "passive", 0);
    setenv("KMP_BLOCKTIME", "0", 0);
    struct Guard { av_msckf_batch* b; ~Guard() { sub_destroy(b); } } guard{new (std::nothrow) av_msckf_batch(n_streams)};      // until *out = b: no return leaves a live batch behind
    av_msckf_batch* b = guard.b;
    if (!b) { av_set_error("out of host memory"); return AV_E_INVALID; }
    b->device = b->res.device = device; b->S = n_streams; b->max_cam = max_cam_states; b->cam_slots = max_cam_states + 1; b->rows_cap = rows_cap;
    b->ld = ((IMU_DIM + 6 * b->cam_slots) + 7) & ~7;
    for (int i = 0; i < 3; ++i) { b->gravity0[i] = gravity[i]; b->vel0[i] = velocity0[i]; }
    for (int i = 0; i < 16; ++i) b->T01[i] = T_cam0_cam1_rowmajor44[i];
    for (int i = 0; i < 9; ++i) b->R_ic0[i] = R_imu_cam0_t_cam0_imu12[i];
    for (int i = 0; i < 3; ++i) b->t_ci0[i] = R_imu_cam0_t_cam0_imu12[9 + i];
    for (int i = 0; i < 5; ++i) { b->cov0[i] = cov_init5[i]; b->opt5[i] = opt6[i]; }
    b->trans_thr = opt6[5];
    for (int i = 0; i < 4; ++i) b->noise[i] = noise4[i];
    b->obs_noise = obs_noise; b->pos_std_thr = position_std_threshold;
    const size_t S = n_streams;
    b->pstride = (size_t)b->ld * b->ld; b->hstride = (size_t)rows_cap * b->ld; b->rstride = rows_cap; b->wstride = upd_w_doubles(rows_cap, b->ld);
    int rc;
#define A(p, cnt) if ((rc = b->res.dev(&(p), (size_t)(cnt)))) return rc;
    A(b->P, S * b->pstride) A(b->Pn, S * b->pstride) A(b->T, S * b->pstride) A(b->Kt, S * b->pstride) A(b->scratch, S * b->pstride)
    if (rows_cap > 0) { const size_t pool = b_pool_rows(b, rows_cap); A(b->W, S * b->wstride) A(b->Hblk, S * b->hstride + pool * b->ld) A(b->rblk, S * b->rstride + pool) }
    A(b->dx, S * b->ld) A(b->chi2_dev, 100)
#undef A
    AV_HIP(hipMemcpy(b->chi2_dev, chi2_table_100, sizeof(double) * 100, hipMemcpyHostToDevice));
    if ((rc = b->res.event(&b->ev_wait, hipEventDisableTiming | hipEventBlockingSync))) return rc;
    for (int s = 0; s < n_streams; ++s) {
        BStream& T = b->st[s];
        for (int i = 0; i < 3; ++i) { T.gravity[i] = gravity[i]; T.v[i] = velocity0[i]; T.t_ci[i] = b->t_ci0[i]; }
        for (int i = 0; i < 9; ++i) T.R_ic[i] = b->R_ic0[i];
        if ((rc = b_reset_cov(b, s, nullptr))) return rc;
    }
    guard.b = nullptr;
    *out = b;
    return AV_OK;
}

static void sub_destroy(av_msckf_batch* b)
{
    if (!b) return;
    b->res.release();                 // (the group's worker has been joined by the caller)
    delete b;
}

static int sub_push_imu(av_msckf_batch* b, const int32_t* stream_idx, const double* timestamps, const double* gyro, const double* acc, int n)
{
    if (!b || !stream_idx || !timestamps || !gyro || !acc || n < 0) { av_set_error("av_msckf_batch_push_imu: bad arguments"); return AV_E_INVALID; }
    for (int i = 0; i < n; ++i) {
        const int s = stream_idx[i];
        if (s < 0 || s >= b->S) { av_set_error("av_msckf_batch_push_imu: stream %d out of range", s); return AV_E_INVALID; }
        BStream& T = b->st[s];
        std::lock_guard<std::mutex> g(T.mu);
        BImu m; m.t = timestamps[i];
        for (int k = 0; k < 3; ++k) { m.w[k] = gyro[3 * (size_t)i + k]; m.a[k] = acc[3 * (size_t)i + k]; }
        T.imu.push_back(m);
        if (!T.gravity_set && T.imu.size() >= 200) {
            // initialize_gravity_and_bias (msckf.py:230-249)
            double sw[3] = {0, 0, 0}, sa[3] = {0, 0, 0};
            for (const BImu& q : T.imu) for (int k = 0; k < 3; ++k) { sw[k] += q.w[k]; sa[k] += q.a[k]; }
            const double cnt = (double)T.imu.size();
            double gi[3];
            for (int k = 0; k < 3; ++k) { T.bg[k] = sw[k] / cnt; gi[k] = sa[k] / cnt; }
            const double gn = h_norm3(gi);
            T.gravity[0] = 0; T.gravity[1] = 0; T.gravity[2] = -gn;
            double mg[3] = {0, 0, gn};
            h_from_two_vectors(mg, gi, T.q);
            T.gravity_time = m.t;
            T.gravity_set = true;
        }
    }
    return AV_OK;
}

// Size the block buffers of the update kernels (rows_cap rows per stream and the overflow pool) for feature messages of `cap`
// features per stream, so that no step allocates, frees or synchronises for memory.  The arrays of the observation store and of
// the per-feature lists are dev_reserve's.  Bound: the camera pruning stacks at most 5 rows for each of the cap features of a message.
static int sub_reserve(av_msckf_batch* b, int cap)
{
    if (cap <= b->reserved_cap) return AV_OK;
    if (b->rows_cap == 0 || (b->rows_cap_auto && 5 * cap > b->rows_cap)) {
        // rows_cap 0 at create = size the block buffers from the message capacity; a later, wider message grows them (they hold
        // per-phase scratch only; the outgrown allocations stay with the owner until destroy: no free inside a run)
        if (b->rows_cap_auto) { int rcw = b_wait(b, nullptr); if (rcw) return rcw; AV_HIP(hipDeviceSynchronize()); }
        b->rows_cap_auto = true;
        {   // a regrow is geometric (x1.5 at least): a message that widens by 64 features at a time must not rebuild every time
            const int want = 5 * cap + 64 > 2048 ? 5 * cap + 64 : 2048, geo = b->rows_cap + b->rows_cap / 2;
            b->rows_cap = want > geo ? want : geo;
        }
        const size_t Sn = (size_t)b->S;
        b->hstride = (size_t)b->rows_cap * b->ld; b->rstride = b->rows_cap; b->wstride = upd_w_doubles(b->rows_cap, b->ld);
        int rc0;
        const size_t pool = b_pool_rows(b, b->rows_cap);
        if ((rc0 = b->res.dev(&b->W, Sn * b->wstride)) || (rc0 = b->res.dev(&b->Hblk, Sn * b->hstride + pool * b->ld)) || (rc0 = b->res.dev(&b->rblk, Sn * b->rstride + pool))) return rc0;
    }
    if (5 * cap > b->rows_cap) {
        av_set_error("batched MSCKF: rows_cap %d cannot hold the camera-pruning update of %d features per message (5 rows each: need >= %d)",
                     b->rows_cap, cap, 5 * cap);
        return AV_E_CAPACITY;
    }
    b->reserved_cap = cap;
    return AV_OK;
}

// feature_callback for every stream (msckf.py:177-228).  Features of stream s: ids[s*cap + k], uv[(s*cap+k)*4 ..], k < n_feat[s]
// (host arrays).  out[s*12 ..] = published, t, p(3), q(4), v(3) of the IMU state.
static int sub_step(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                                  const double* timestamps, double* out, void* stream)
{
    if (!b || !ids || !uv || !n_feat || !timestamps || !out || cap <= 0) { av_set_error("av_msckf_batch_step: bad arguments"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(b->device));
    const int k = (int)(b->dev_seq++ % DEV_RING);
    const StepOuts outs = take_outs(b);
    const int rc = dev_launch(b, k, ids, uv, n_feat, cap, timestamps, false, nullptr, (hipStream_t)stream);
    return rc ? rc : dev_finish(b, k, out, outs);
}

static int sub_get_cov(av_msckf_batch* b, int stream_idx, double* P_host, int n, void* stream)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !P_host) { av_set_error("av_msckf_batch_get_cov: bad arguments"); return AV_E_INVALID; }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(b->device));
    int n_now = b->st[stream_idx].n;
    if (b->dev.cap > 0) { DState D; int rcd = dev_read_state(b, stream_idx, &D); if (rcd) return rcd; n_now = D.n; }
    if (n != n_now) { av_set_error("av_msckf_batch_get_cov: n = %d, the stream's state has %d", n, n_now); return AV_E_INVALID; }
    AV_HIP(hipMemcpy2DAsync(P_host, sizeof(double) * n, b->P + (size_t)stream_idx * b->pstride, sizeof(double) * b->ld, sizeof(double) * n, n, hipMemcpyDeviceToHost, stm));
    { int rcw = b_wait(b, stm); if (rcw) return rcw; }
    return AV_OK;
}

// [n_state, n_cam, n_map] of one stream
static int sub_sizes(av_msckf_batch* b, int stream_idx, int32_t out3[3])
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !out3) { av_set_error("av_msckf_batch_sizes: bad arguments"); return AV_E_INVALID; }
    if (b->dev.cap > 0) {
        DState D; int rcd = dev_read_state(b, stream_idx, &D); if (rcd) return rcd;
        int live = 0;
        AV_HIP(hipMemcpy(&live, b->dev.A.hdr + (size_t)stream_idx * AVS_HDR_WORDS + AVS_LIVE, sizeof(int), hipMemcpyDeviceToHost));
        out3[0] = D.n; out3[1] = D.ncam; out3[2] = live;
        return AV_OK;
    }
    out3[0] = b->st[stream_idx].n; out3[1] = 0; out3[2] = 0;      // before the first step: no camera state, an empty map
    return AV_OK;
}

// Full state of one stream for parity tests (SURVEY 8b "get_state"): everything measurement_update injects into
// (msckf.py:576-595).  imu32 = [timestamp, q(4), p(3), v(3), gyro_bias(3), acc_bias(3), R_imu_cam0 (9, row-major), t_cam0_imu(3),
// gravity(3)]; camera states in window order: ids and [q(4), p(3)] each.  Call with no step in flight (after _wait(0)).
static int sub_get_state(av_msckf_batch* b, int stream_idx, double imu32[32], int64_t* cam_ids, double* cam_qp7, int cam_cap, int32_t* n_cam)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !imu32 || !n_cam || cam_cap < 0 || (cam_cap > 0 && (!cam_ids || !cam_qp7))) { av_set_error("av_msckf_batch_get_state: bad arguments"); return AV_E_INVALID; }
    if (b->dev.cap > 0) {
        DState D; int rcd = dev_read_state(b, stream_idx, &D); if (rcd) return rcd;
        double* o = imu32;
        *o++ = D.ts;
        for (int i = 0; i < 4; ++i) *o++ = D.q[i];
        for (int i = 0; i < 3; ++i) *o++ = D.p[i];
        for (int i = 0; i < 3; ++i) *o++ = D.v[i];
        for (int i = 0; i < 3; ++i) *o++ = D.bg[i];
        for (int i = 0; i < 3; ++i) *o++ = D.ba[i];
        for (int i = 0; i < 9; ++i) *o++ = D.R_ic[i];
        for (int i = 0; i < 3; ++i) *o++ = D.t_ci[i];
        for (int i = 0; i < 3; ++i) *o++ = D.gravity[i];
        *n_cam = D.ncam;
        if (D.ncam > cam_cap) { if (cam_cap == 0) return AV_OK; av_set_error("av_msckf_batch_get_state: %d camera states > cam_cap %d", D.ncam, cam_cap); return AV_E_CAPACITY; }
        const DevArgs& A = b->dev.A;
        std::vector<long long> cid(D.ncam); std::vector<double> cq((size_t)4 * D.ncam), cp((size_t)3 * D.ncam);
        const size_t c0 = (size_t)stream_idx * A.cs;
        if (D.ncam > 0) {
            AV_HIP(hipMemcpy(cid.data(), A.cam_id + c0, sizeof(long long) * D.ncam, hipMemcpyDeviceToHost));
            AV_HIP(hipMemcpy(cq.data(), A.cam_q + 4 * c0, sizeof(double) * 4 * D.ncam, hipMemcpyDeviceToHost));
            AV_HIP(hipMemcpy(cp.data(), A.cam_p + 3 * c0, sizeof(double) * 3 * D.ncam, hipMemcpyDeviceToHost));
        }
        for (int k = 0; k < D.ncam; ++k) {
            cam_ids[k] = cid[k];
            for (int i = 0; i < 4; ++i) cam_qp7[7 * k + i] = cq[(size_t)4 * k + i];
            for (int i = 0; i < 3; ++i) cam_qp7[7 * k + 4 + i] = cp[(size_t)3 * k + i];
        }
        return AV_OK;
    }
    // before the first step: the initial host record (no camera state, position and accelerometer bias at their zero)
    const BStream& T = b->st[stream_idx];
    double* o = imu32;
    *o++ = T.ts;
    for (int i = 0; i < 4; ++i) *o++ = T.q[i];
    for (int i = 0; i < 3; ++i) *o++ = 0.0;
    for (int i = 0; i < 3; ++i) *o++ = T.v[i];
    for (int i = 0; i < 3; ++i) *o++ = T.bg[i];
    for (int i = 0; i < 3; ++i) *o++ = 0.0;
    for (int i = 0; i < 9; ++i) *o++ = T.R_ic[i];
    for (int i = 0; i < 3; ++i) *o++ = T.t_ci[i];
    for (int i = 0; i < 3; ++i) *o++ = T.gravity[i];
    *n_cam = 0;
    return AV_OK;
}

// 0 while the stream runs; the error code that stopped it otherwise (message copied to msg, NUL-terminated)
static int sub_stream_status(av_msckf_batch* b, int stream_idx, int32_t* status, char* msg, int msg_cap)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !status) { av_set_error("av_msckf_batch_stream_status: bad arguments"); return AV_E_INVALID; }
    const BStream& T = b->st[stream_idx];
    if (b->dev.cap > 0 && !T.failed) {
        DState D; int rcd = dev_read_state(b, stream_idx, &D); if (rcd) return rcd;
        int code = 0;
        const char* why = D.failed ? dev_fail_message(D.failed, &code) : "";
        *status = code;
        if (msg && msg_cap > 0) { strncpy(msg, why, (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        return AV_OK;
    }
    *status = T.failed;
    if (msg && msg_cap > 0) { strncpy(msg, T.fail_msg, (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
    return AV_OK;
}


#include "msckf_dev_host.inc"

// ---- exported entry points: one sub-batch, or a parent over stream groups --------------------------------------
namespace {

void group_worker(av_msckf_batch* g)
{
    (void)hipSetDevice(g->device);
    std::deque<av_msckf_batch::Job> launched;                    // steps enqueued on the device whose results have not been collected
    const size_t depth = DEV_RING - 1;
    std::unique_lock<std::mutex> lk(g->wmu);
    auto note = [&](int rc) { if (rc && !g->job_rc) { g->job_rc = rc; strncpy(g->job_err, av_last_error(), sizeof(g->job_err) - 1); g->job_err[sizeof(g->job_err) - 1] = 0; } };
    for (;;) {
        g->wcv.wait(lk, [&] { return !g->jobs.empty() || !launched.empty() || g->quit; });
        if (!g->jobs.empty() && launched.size() < depth) {
            av_msckf_batch::Job job = std::move(g->jobs.front());
            g->jobs.pop_front();
            const bool skip = g->job_rc != 0;                     // an earlier step of this group failed: drain without running
            lk.unlock();
            const int rc = skip ? 0 : job.launch();
            lk.lock();
            note(rc);
            if (skip || rc) { ++g->n_done; g->wcv.notify_all(); }
            else launched.push_back(std::move(job));
            continue;
        }
        if (!launched.empty()) {
            av_msckf_batch::Job job = std::move(launched.front());
            launched.pop_front();
            lk.unlock();
            const int rc = job.finish ? job.finish() : 0;
            lk.lock();
            note(rc);
            ++g->n_done;
            g->wcv.notify_all();
            continue;
        }
        if (g->quit) return;
    }
}

int default_groups(int n_streams)
{
    const char* e = getenv("AV_MSCKF_GROUPS");
    // the groups only add concurrency between two latency chains; more of them just compete (2,048 streams: 1 / 2 / 3 / 4 / 8 groups =
    // 132 / 128-134 / 121 / 101 / 80 k frames/s)
    int g = e ? atoi(e) : (n_streams >= 1024 ? 2 : 1);
    if (g > 8) g = 8;
    if (g > n_streams) g = n_streams;
    return g < 1 ? 1 : g;
}

}  // namespace

AV_EXPORT int av_msckf_batch_create(int n_streams, int max_cam_states, int rows_cap, const double* chi2_table_100, const double gravity[3],
                                    const double* T_cam0_cam1_rowmajor44, const double* R_imu_cam0_t_cam0_imu12, const double cov_init5[5],
                                    const double noise4[4], double obs_noise, double position_std_threshold, const double velocity0[3],
                                    const double* opt6, int device, av_msckf_batch** out)
{
    if (!out || n_streams <= 0) { av_set_error("av_msckf_batch_create: bad arguments"); return AV_E_INVALID; }
    const int G = default_groups(n_streams);
    if (G == 1)
        return sub_create(n_streams, max_cam_states, rows_cap, chi2_table_100, gravity, T_cam0_cam1_rowmajor44, R_imu_cam0_t_cam0_imu12, cov_init5, noise4,
                          obs_noise, position_std_threshold, velocity0, opt6, device, out);
    av_msckf_batch* p = new (std::nothrow) av_msckf_batch(0);
    if (!p) { av_set_error("out of host memory"); return AV_E_INVALID; }
    p->device = p->res.device = device; p->S = n_streams; p->per_sub = (n_streams + G - 1) / G;
    for (int s0 = 0; s0 < n_streams; s0 += p->per_sub) {
        const int cnt = n_streams - s0 < p->per_sub ? n_streams - s0 : p->per_sub;
        av_msckf_batch* g = nullptr;
        int rc = sub_create(cnt, max_cam_states, rows_cap, chi2_table_100, gravity, T_cam0_cam1_rowmajor44, R_imu_cam0_t_cam0_imu12, cov_init5, noise4,
                            obs_noise, position_std_threshold, velocity0, opt6, device, &g);
        if (rc == AV_OK) rc = make_filter_stream(g->res, &g->own);
        if (rc) { if (g) sub_destroy(g); av_msckf_batch_destroy(p); return rc; }
        p->subs.push_back(g);
        g->worker = std::thread(group_worker, g);
    }
    *out = p;
    return AV_OK;
}

AV_EXPORT void av_msckf_batch_destroy(av_msckf_batch* b)
{
    if (!b) return;
    if (b->subs.empty() && !b->per_sub) { sub_destroy(b); return; }
    for (av_msckf_batch* g : b->subs) {
        if (g->worker.joinable()) {
            { std::lock_guard<std::mutex> lk(g->wmu); g->quit = true; }
            g->wcv.notify_all();
            g->worker.join();
        }
        sub_destroy(g);
    }
    delete b;
}

AV_EXPORT int av_msckf_batch_push_imu(av_msckf_batch* b, const int32_t* stream_idx, const double* timestamps, const double* gyro, const double* acc, int n)
{
    if (!b || !stream_idx || !timestamps || !gyro || !acc || n < 0) { av_set_error("av_msckf_batch_push_imu: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) return sub_push_imu(b, stream_idx, timestamps, gyro, acc, n);
    for (int i = 0; i < n; ++i) {
        const int s = stream_idx[i];
        if (s < 0 || s >= b->S) { av_set_error("av_msckf_batch_push_imu: stream %d out of range", s); return AV_E_INVALID; }
        const int32_t local = s % b->per_sub;
        const int rc = sub_push_imu(b->subs[s / b->per_sub], &local, timestamps + i, gyro + 3 * (size_t)i, acc + 3 * (size_t)i, 1);
        if (rc) return rc;
    }
    return AV_OK;
}

namespace {

// one group, no worker thread: collect launched steps until at most max_pending are outstanding
int direct_drain(av_msckf_batch* b, size_t max_pending)
{
    int rc = AV_OK;
    while (b->direct_pending.size() > max_pending) {
        const av_msckf_batch::Pending pr = b->direct_pending.front();
        b->direct_pending.pop_front();
        const int r = dev_finish(b, pr.slot, pr.out, pr.outs);
        if (r && !rc) rc = r;
    }
    return rc;
}

// the group's buffers for messages of `cap` features (first step, or a wider message: drains the group first)
int dev_prepare(av_msckf_batch* g, int cap)
{
    if (g->dev.cap >= cap && g->reserved_cap >= cap) return AV_OK;
    AV_HIP(hipSetDevice(g->device));
    int rc;
    const bool first = g->dev.cap == 0;
    const int rows_before = g->rows_cap;
    if ((rc = sub_reserve(g, cap)) || (rc = dev_reserve(g, cap))) return rc;
    if (first || rows_before != g->rows_cap) rc = dev_upload_updbase(g);
    return rc;
}

}  // namespace

AV_EXPORT int av_msckf_batch_wait(av_msckf_batch* b, int max_pending)
{
    if (!b || max_pending < 0) { av_set_error("av_msckf_batch_wait: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) {
        if (b->direct_pending.empty()) return AV_OK;
        AV_HIP(hipSetDevice(b->device));
        return direct_drain(b, (size_t)max_pending);
    }
    int rc = AV_OK;
    for (av_msckf_batch* g : b->subs) {
        std::unique_lock<std::mutex> lk(g->wmu);
        g->wcv.wait(lk, [&] { return g->n_submitted - g->n_done <= (long long)max_pending; });
        if (g->job_rc && !rc) { rc = g->job_rc; av_set_error("%s", g->job_err); }
    }
    return rc;
}

AV_EXPORT int av_msckf_batch_submit(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                                    const double* timestamps, double* out, void* stream)
{
    if (!b || !ids || !uv || !n_feat || !timestamps || !out || cap <= 0) { av_set_error("av_msckf_batch_submit: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) {
        // one group: the step is enqueued here and collected by av_msckf_batch_wait (the arrays are consumed before this returns)
        AV_HIP(hipSetDevice(b->device));
        int rc = direct_drain(b, DEV_RING - 2);
        if (rc) return rc;
        const int k = (int)(b->dev_seq++ % DEV_RING);
        const StepOuts outs = take_outs(b);
        if ((rc = dev_launch(b, k, ids, uv, n_feat, cap, timestamps, false, nullptr, (hipStream_t)stream))) return rc;
        b->direct_pending.push_back({k, out, outs});
        return AV_OK;
    }
    const int k = (int)(b->dev_seq++ % DEV_RING);
    const StepOuts outs = take_outs(b);
    for (size_t gi = 0; gi < b->subs.size(); ++gi) {
        av_msckf_batch* g = b->subs[gi];
        const size_t s0 = gi * (size_t)b->per_sub;
        av_msckf_batch::Job job;
        const StepOuts go = outs.at(b->out_set, s0);
        job.launch = [=] { return dev_launch(g, k, ids + s0 * cap, uv + s0 * cap * 4, n_feat + s0, cap, timestamps + s0, false, nullptr, g->own); };
        job.finish = [=] { return dev_finish(g, k, out + s0 * 12, go); };
        std::lock_guard<std::mutex> lk(g->wmu);
        g->jobs.push_back(std::move(job));
        ++g->n_submitted;
        g->wcv.notify_all();
    }
    return AV_OK;
}

// The feature message straight from the front-end's device buffers (av_frontend_features_dev): no host round trip.  The three
// arrays are read by copies enqueued on `msg_stream` -- the stream that produced them, i.e. the one the front-end's step ran on --
// before this call returns, so the producer may overwrite them with its next step at once; the filter's kernels run on the groups'
// own streams (one group: on `stream`) behind an event.  timestamps / out: host arrays, valid until the step has been waited for.
AV_EXPORT int av_msckf_batch_submit_dev(av_msckf_batch* b, const int64_t* ids_dev, const double* uv_dev, const int32_t* n_feat_dev, int cap,
                                        const double* timestamps, double* out, void* msg_stream, void* stream)
{
    if (!b || !ids_dev || !uv_dev || !n_feat_dev || !timestamps || !out || cap <= 0) { av_set_error("av_msckf_batch_submit_dev: bad arguments"); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    AV_HIP(hipSetDevice(b->device));
    int rc;
    bool need = false;
    for (av_msckf_batch* g : parts) if (g->dev.cap < cap) need = true;
    if (need) {
        if ((rc = av_msckf_batch_wait(b, 0))) return rc;
        for (av_msckf_batch* g : parts) if ((rc = dev_prepare(g, cap))) return rc;
    }
    // slot k of every group is free once the step submitted DEV_RING steps ago has been collected
    if ((rc = av_msckf_batch_wait(b, b->subs.empty() ? DEV_RING - 2 : DEV_RING - 1))) return rc;
    const int k = (int)(b->dev_seq++ % DEV_RING);
    hipStream_t ms = (hipStream_t)msg_stream;
    if (!b->ev_msg[k] && (rc = b->res.event(&b->ev_msg[k], hipEventDisableTiming))) return rc;
    size_t s0 = 0;
    for (av_msckf_batch* g : parts) {
        DevSlot& sl = g->dev.slot[k];
        const size_t Sg = (size_t)g->S, dc = (size_t)g->dev.cap;
        AV_HIP(hipMemcpyAsync(sl.n_d, n_feat_dev + s0, sizeof(int) * Sg, hipMemcpyDeviceToDevice, ms));
        if (dc == (size_t)cap) {
            AV_HIP(hipMemcpyAsync(sl.ids_d, ids_dev + s0 * cap, sizeof(long long) * Sg * cap, hipMemcpyDeviceToDevice, ms));
            AV_HIP(hipMemcpyAsync(sl.uv_d, uv_dev + s0 * cap * 4, sizeof(double) * 4 * Sg * cap, hipMemcpyDeviceToDevice, ms));
        } else {
            AV_HIP(hipMemcpy2DAsync(sl.ids_d, sizeof(long long) * dc, ids_dev + s0 * cap, sizeof(long long) * cap, sizeof(long long) * cap, Sg, hipMemcpyDeviceToDevice, ms));
            AV_HIP(hipMemcpy2DAsync(sl.uv_d, sizeof(double) * 4 * dc, uv_dev + s0 * cap * 4, sizeof(double) * 4 * cap, sizeof(double) * 4 * cap, Sg, hipMemcpyDeviceToDevice, ms));
        }
        s0 += Sg;
    }
    AV_HIP(hipEventRecord(b->ev_msg[k], ms));
    hipEvent_t ready = b->ev_msg[k];
    const StepOuts outs = take_outs(b);
    if (b->subs.empty()) {
        if ((rc = dev_launch(b, k, nullptr, nullptr, nullptr, cap, timestamps, true, ready, (hipStream_t)stream))) return rc;
        b->direct_pending.push_back({k, out, outs});
        return AV_OK;
    }
    s0 = 0;
    for (av_msckf_batch* g : b->subs) {
        const size_t o = s0;
        const StepOuts go = outs.at(b->out_set, o);
        av_msckf_batch::Job job;
        job.launch = [=] { return dev_launch(g, k, nullptr, nullptr, nullptr, cap, timestamps + o, true, ready, g->own); };
        job.finish = [=] { return dev_finish(g, k, out + o * 12, go); };
        s0 += (size_t)g->S;
        std::lock_guard<std::mutex> lk(g->wmu);
        g->jobs.push_back(std::move(job));
        ++g->n_submitted;
        g->wcv.notify_all();
    }
    return AV_OK;
}

// Always 1: the filter state and the observation map of a batch live on the device (msckf_dev.inc; av_msckf_batch_submit_dev is
// available).  Kept for callers written when a host-bookkeeping form existed beside it.
AV_EXPORT int av_msckf_batch_device_resident(const av_msckf_batch* b)
{
    if (!b) { av_set_error("av_msckf_batch_device_resident: bad arguments"); return AV_E_INVALID; }
    return 1;
}

AV_EXPORT int av_msckf_batch_step(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                                  const double* timestamps, double* out, void* stream)
{
    if (!b || !ids || !uv || !n_feat || !timestamps || !out || cap <= 0) { av_set_error("av_msckf_batch_step: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) {
        AV_HIP(hipSetDevice(b->device));
        const int rc0 = direct_drain(b, 0);
        if (rc0) return rc0;
        return sub_step(b, ids, uv, n_feat, cap, timestamps, out, stream);
    }
    // the caller's stream orders this step after whatever it enqueued before; the groups then run on their own streams
    AV_HIP(hipSetDevice(b->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    int rc = av_msckf_batch_submit(b, ids, uv, n_feat, cap, timestamps, out, stream);
    if (rc) return rc;
    return av_msckf_batch_wait(b, 0);
}

// The optional per-step outputs (OUTS, msckf_dev.inc; airvision.h: "Odometry covariance", "Landmark map", "Innovation statistics",
// "IMU-rate odometry", "Forecast").
// set: before the batch's first step -- the groups size their buffers when they prepare the device-resident path.  next: the
// destination of the next step's arrays, taken by that step.
static_assert(sizeof(av_landmark) == AV_LANDMARK_BYTES && sizeof(DLandmark) == AV_LANDMARK_BYTES, "av_landmark layout");
static_assert(LM_USED == AV_LM_USED && LM_REJECTED == AV_LM_REJECTED && LM_TRACKED == AV_LM_TRACKED && LM_NEW == AV_LM_NEW, "AV_LM_* bits");
static_assert(sizeof(av_update_stats) == 64 && sizeof(av_filter_stats) == AV_FILTER_STATS_BYTES && sizeof(DUpdStats) == sizeof(av_update_stats), "av_filter_stats layout");
static_assert(offsetof(av_update_stats, gamma_eval) == offsetof(DUpdStats, gamma_eval) && offsetof(av_update_stats, dx_rot) == offsetof(DUpdStats, dx_rot) && offsetof(av_update_stats, flags) == offsetof(DUpdStats, flags), "av_update_stats fields");
static_assert(FS_RAN == AV_FS_RAN && FS_CUT == AV_FS_CUT, "AV_FS_* bits");
static_assert(sizeof(av_imu_state) == AV_IMU_STATE_BYTES && sizeof(DImuState) == AV_IMU_STATE_BYTES, "av_imu_state layout");
static_assert(offsetof(av_imu_state, p) == offsetof(DImuState, p) && offsetof(av_imu_state, q) == offsetof(DImuState, q) && offsetof(av_imu_state, v) == offsetof(DImuState, v) && offsetof(av_imu_state, w) == offsetof(DImuState, w), "av_imu_state fields");
constexpr int IMU_RATE_CAP_MAX = 4096;
constexpr int FORECAST_CAP_MAX = 4096;
static_assert(ODOM_COV_DOUBLES == AV_ODOM_COV_DOUBLES, "the forecast's covariance record is an odometry-covariance record");

namespace {

// the body of av_msckf_batch_set_*: feature f gets `setting` on the batch and on every group (args_ok: the wrapper's own argument check)
int batch_set_out(av_msckf_batch* b, OutFeat f, int setting, bool args_ok = true)
{
    const OutWords& w = out_words(f);
    if (!b || !args_ok) { av_set_error("av_msckf_batch_set_%s: bad arguments", w.fn); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    bool stepped = b->dev_seq > 0;
    for (av_msckf_batch* g : parts) if (g->n_steps > 0 || g->dev.cap > 0) stepped = true;
    if (stepped) { av_set_error("av_msckf_batch_set_%s: the batch has stepped; %s %s switched before the first step", w.fn, w.noun, w.is); return AV_E_INVALID; }
    b->out_set[f] = setting;
    for (int i = 0; i < N_OUT; ++i) if (OUTS[i].feat == f) b->next_outs.p[i] = nullptr;
    for (av_msckf_batch* g : parts) g->out_set[f] = setting;
    return AV_OK;
}

// the body of av_msckf_batch_next_*: dst = the caller's arrays for the feature's entries of OUTS, in the table's order
int batch_next_out(av_msckf_batch* b, OutFeat f, std::initializer_list<void*> dst)
{
    const OutWords& w = out_words(f);
    bool ok = b != nullptr;
    for (void* p : dst) ok = ok && p;
    if (!ok) { av_set_error("av_msckf_batch_next_%s: bad arguments", w.fn); return AV_E_INVALID; }
    if (!b->out_set[f]) { av_set_error("av_msckf_batch_next_%s: %s %s off (av_msckf_batch_set_%s)", w.fn, w.noun, w.is, w.fn); return AV_E_INVALID; }
    const void* const* p = dst.begin();
    for (int i = 0; i < N_OUT; ++i) if (OUTS[i].feat == f) b->next_outs.p[i] = const_cast<void*>(*p++);
    return AV_OK;
}

}  // namespace

AV_EXPORT int av_msckf_batch_set_odom_cov(av_msckf_batch* b, int enable) { return batch_set_out(b, F_COV, enable != 0); }
AV_EXPORT int av_msckf_batch_next_odom_cov(av_msckf_batch* b, double* cov_host) { return batch_next_out(b, F_COV, {cov_host}); }
AV_EXPORT int av_msckf_batch_set_landmarks(av_msckf_batch* b, int cap) { return batch_set_out(b, F_LM, cap, cap >= 0 && cap <= (1 << 20)); }
AV_EXPORT int av_msckf_batch_next_landmarks(av_msckf_batch* b, av_landmark* rec, int32_t* n) { return batch_next_out(b, F_LM, {rec, n}); }
AV_EXPORT int av_msckf_batch_set_stats(av_msckf_batch* b, int enable) { return batch_set_out(b, F_STATS, enable != 0); }
AV_EXPORT int av_msckf_batch_next_stats(av_msckf_batch* b, av_filter_stats* rec_host) { return batch_next_out(b, F_STATS, {rec_host}); }
AV_EXPORT int av_msckf_batch_set_imu_rate(av_msckf_batch* b, int cap) { return batch_set_out(b, F_IR, cap, cap >= 0 && cap <= IMU_RATE_CAP_MAX); }
AV_EXPORT int av_msckf_batch_next_imu_rate(av_msckf_batch* b, av_imu_state* rec, int32_t* n) { return batch_next_out(b, F_IR, {rec, n}); }
AV_EXPORT int av_msckf_batch_set_forecast(av_msckf_batch* b, int cap) { return batch_set_out(b, F_FC, cap, cap >= 0 && cap <= FORECAST_CAP_MAX); }
AV_EXPORT int av_msckf_batch_next_forecast(av_msckf_batch* b, av_imu_state* rec, int32_t* n, double* cov) { return batch_next_out(b, F_FC, {rec, n, cov}); }

// The zero-velocity update (airvision.h, "Zero-velocity update").  Not an entry of OUTS: its record is not delivered with a step's
// read-back, it lives in one device array per group (DevPath::zupt_d, taken at dev_reserve when the update is on) and is read on demand.
static_assert(sizeof(av_zupt) == AV_ZUPT_BYTES && sizeof(DZupt) == AV_ZUPT_BYTES, "av_zupt layout");
static_assert(offsetof(av_zupt, applied_total) == offsetof(DZupt, applied_total) && offsetof(av_zupt, w_max) == offsetof(DZupt, w_max) && offsetof(av_zupt, dx_pos) == offsetof(DZupt, dx_pos), "av_zupt fields");
static_assert(ZU_IMU_OK == AV_ZU_IMU_OK && ZU_VIS_OK == AV_ZU_VIS_OK && ZU_DETECTED == AV_ZU_DETECTED && ZU_APPLIED == AV_ZU_APPLIED && ZU_GATED == AV_ZU_GATED && ZU_BAD == AV_ZU_BAD, "AV_ZU_* bits");
static bool zupt_params_ok(const av_zupt_params* p)
{
    return std::isfinite(p->gyro_max) && p->gyro_max >= 0 && std::isfinite(p->acc_dev_max) && p->acc_dev_max >= 0 && std::isfinite(p->disparity_max) && p->disparity_max >= 0 &&
           std::isfinite(p->velocity_sigma) && p->velocity_sigma > 0 && std::isfinite(p->gate) && p->gate >= 0 && p->min_tracks >= 0 && p->still_percent >= 0 && p->still_percent <= 100;
}
AV_EXPORT int av_msckf_batch_set_zupt(av_msckf_batch* b, const av_zupt_params* p)
{
    if (!b) { av_set_error("av_msckf_batch_set_zupt: bad arguments"); return AV_E_INVALID; }
    if (p && !zupt_params_ok(p)) {
        av_set_error("av_msckf_batch_set_zupt: parameters out of range (thresholds >= 0, velocity_sigma > 0, gate >= 0, all finite, min_tracks >= 0, still_percent 0 .. 100)");
        return AV_E_INVALID;
    }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    bool stepped = b->dev_seq > 0;
    for (av_msckf_batch* g : parts) if (g->n_steps > 0 || g->dev.cap > 0) stepped = true;
    if (stepped) { av_set_error("av_msckf_batch_set_zupt: the batch has stepped; the zero-velocity update is switched before the first step"); return AV_E_INVALID; }
    b->zupt_on = p != nullptr;
    if (p) b->zupt = *p;
    for (av_msckf_batch* g : parts) { g->zupt_on = b->zupt_on; g->zupt = b->zupt; }
    return AV_OK;
}
AV_EXPORT int av_msckf_batch_read_zupt(av_msckf_batch* b, av_zupt* out)
{
    if (!b || !out) { av_set_error("av_msckf_batch_read_zupt: bad arguments"); return AV_E_INVALID; }
    const int rc = av_msckf_batch_wait(b, 0);
    if (rc) return rc;
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    memset(out, 0, sizeof(av_zupt) * (size_t)b->S);
    size_t s0 = 0;
    for (av_msckf_batch* g : parts) {
        if (g->dev.zupt_d) {
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(out + s0, g->dev.zupt_d, sizeof(av_zupt) * (size_t)g->S, hipMemcpyDeviceToHost));
        }
        s0 += (size_t)g->S;
    }
    return AV_OK;
}

AV_EXPORT int av_msckf_batch_get_cov(av_msckf_batch* b, int stream_idx, double* P_host, int n, void* stream)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S) { av_set_error("av_msckf_batch_get_cov: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) return sub_get_cov(b, stream_idx, P_host, n, stream);
    return sub_get_cov(b->subs[stream_idx / b->per_sub], stream_idx % b->per_sub, P_host, n, stream);
}

// [n_state, n_cam, n_map] of one stream
AV_EXPORT int av_msckf_batch_sizes(av_msckf_batch* b, int stream_idx, int32_t out3[3])
{
    if (!b || stream_idx < 0 || stream_idx >= b->S) { av_set_error("av_msckf_batch_sizes: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) return sub_sizes(b, stream_idx, out3);
    return sub_sizes(b->subs[stream_idx / b->per_sub], stream_idx % b->per_sub, out3);
}

AV_EXPORT int av_msckf_batch_get_state(av_msckf_batch* b, int stream_idx, double imu32[32], int64_t* cam_ids, double* cam_qp7, int cam_cap, int32_t* n_cam)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S) { av_set_error("av_msckf_batch_get_state: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) return sub_get_state(b, stream_idx, imu32, cam_ids, cam_qp7, cam_cap, n_cam);
    return sub_get_state(b->subs[stream_idx / b->per_sub], stream_idx % b->per_sub, imu32, cam_ids, cam_qp7, cam_cap, n_cam);
}

AV_EXPORT int av_msckf_batch_stream_status(av_msckf_batch* b, int stream_idx, int32_t* status, char* msg, int msg_cap)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S) { av_set_error("av_msckf_batch_stream_status: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) return sub_stream_status(b, stream_idx, status, msg, msg_cap);
    return sub_stream_status(b->subs[stream_idx / b->per_sub], stream_idx % b->per_sub, status, msg, msg_cap);
}

// Stream restart (airvision.h, "Stream restart").  One group: its listed streams (local indices, distinct, in range; the group is
// drained) go back to what sub_create and dev_reserve made of them -- the host record here, the device state by dk_restart.
static int sub_restart(av_msckf_batch* g, const std::vector<int>& list)
{
    for (const int s : list) {
        BStream& T = g->st[s];
        std::lock_guard<std::mutex> lk(T.mu);
        T.imu.clear();                                       // samples pushed before the call belong to the old life
        T.gravity_set = false; T.first_img = true; T.active = false;
        T.gravity_time = 0; T.dev_init_sent = false;
        T.ts = 0; T.n = IMU_DIM;
        for (int i = 0; i < 4; ++i) T.q[i] = i == 3 ? 1.0 : 0.0;
        for (int i = 0; i < 3; ++i) { T.bg[i] = 0; T.v[i] = g->vel0[i]; T.gravity[i] = g->gravity0[i]; T.t_ci[i] = g->t_ci0[i]; }
        for (int i = 0; i < 9; ++i) T.R_ic[i] = g->R_ic0[i];
        T.failed = 0; T.fail_msg[0] = 0;
        for (int ph = 0; ph < 2; ++ph) { T.dbg_gamma[ph].clear(); T.dbg_dx[ph].clear(); T.dbg_P[ph].clear(); T.dbg_rows[ph] = 0; T.dbg_n[ph] = 0; }
    }
    return dev_restart(g, list.data(), (int)list.size(), g->own);
}

AV_EXPORT int av_msckf_batch_restart(av_msckf_batch* b, const int32_t* stream_idx, int n)
{
    if (!b || n < 0 || (n > 0 && !stream_idx)) { av_set_error("av_msckf_batch_restart: bad arguments"); return AV_E_INVALID; }
    for (int i = 0; i < n; ++i) if (stream_idx[i] < 0 || stream_idx[i] >= b->S) { av_set_error("av_msckf_batch_restart: stream %d out of range", stream_idx[i]); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    if (n == 0) return AV_OK;
    int rc = av_msckf_batch_wait(b, 0);                      // queued steps belong to the old life: they retire, their outputs are delivered
    if (rc) return rc;
    // every index to its group and local index; a repeated index counts once
    std::vector<std::vector<int>> lists(parts.size());
    std::vector<char> seen((size_t)b->S, 0);
    for (int i = 0; i < n; ++i) {
        const int s = stream_idx[i];
        if (seen[s]) continue;
        seen[s] = 1;
        if (b->subs.empty()) lists[0].push_back(s); else lists[(size_t)(s / b->per_sub)].push_back(s % b->per_sub);
    }
    for (size_t gi = 0; gi < parts.size(); ++gi) if (!lists[gi].empty() && (rc = sub_restart(parts[gi], lists[gi]))) return rc;
    return AV_OK;
}

// Parity-test tap.  capture(1): from the next step on every stream keeps, for the two update phases of its LAST step, what the
// reference computes inside gating_test / measurement_update (msckf.py:604-612, 548-602) but never returns.  read: phase 0 =
// remove_lost_features, 1 = prune_cam_state_buffer; gamma[] in the reference's evaluation order, delta_x (n doubles), the
// covariance right after the update (n x n, before the camera states of the pruning phase are removed), rows stacked (0 = the
// phase ran no update: dx / P are then not written).  Drain first.  Capturing costs synchronous copies: tests only.
AV_EXPORT int av_msckf_batch_debug_capture(av_msckf_batch* b, int enable)
{
    if (!b) { av_set_error("av_msckf_batch_debug_capture: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) b->debug_capture = enable != 0;
    for (av_msckf_batch* g : b->subs) g->debug_capture = enable != 0;
    return AV_OK;
}
AV_EXPORT int av_msckf_batch_debug_read(av_msckf_batch* b, int stream_idx, int phase, double* gamma, int gamma_cap, int32_t* n_gamma,
                                        double* dx, double* P_after, int n_cap, int32_t* n_state, int32_t* rows)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || phase < 0 || phase > 1 || !n_gamma || !n_state || !rows || gamma_cap < 0 || n_cap < 0) { av_set_error("av_msckf_batch_debug_read: bad arguments"); return AV_E_INVALID; }
    av_msckf_batch* g = b->subs.empty() ? b : b->subs[stream_idx / b->per_sub];
    const BStream& T = g->st[b->subs.empty() ? stream_idx : stream_idx % b->per_sub];
    *n_gamma = (int32_t)T.dbg_gamma[phase].size(); *rows = T.dbg_rows[phase]; *n_state = T.dbg_n[phase];
    if (gamma && (int)T.dbg_gamma[phase].size() <= gamma_cap) memcpy(gamma, T.dbg_gamma[phase].data(), sizeof(double) * T.dbg_gamma[phase].size());
    else if (gamma) { av_set_error("av_msckf_batch_debug_read: %zu gating values > gamma_cap %d", T.dbg_gamma[phase].size(), gamma_cap); return AV_E_CAPACITY; }
    if (T.dbg_rows[phase] > 0) {
        const int n = T.dbg_n[phase];
        if (n > n_cap) { av_set_error("av_msckf_batch_debug_read: state dimension %d > n_cap %d", n, n_cap); return AV_E_CAPACITY; }
        if (dx) memcpy(dx, T.dbg_dx[phase].data(), sizeof(double) * n);
        if (P_after && T.dbg_P[phase].size() == (size_t)n * n) memcpy(P_after, T.dbg_P[phase].data(), sizeof(double) * n * n);
    }
    return AV_OK;
}

// Parity-test entry for the per-feature launch shapes of the device-resident filter (tests only; no step of the filter calls it): on the
// caller's device arrays, triangulate_kernel in its list form with one wavefront per workgroup, then launch_feature_dev, both exactly as
// dev_phase launches them -- device-side counts, valid[] written by the triangulation and read by the gate, stream of feature f =
// f / fs_stride, `teams` as dev_grid_hint would give it (the kernels stride over their lists whatever the grid).  No kernel of its own.
// tri_list_dev = NULL skips the triangulation: pos_dev / valid_dev are then the caller's.  `ctx` lends its chi^2 table and its device.
AV_EXPORT int av_msckf_feature_ops_dev(av_msckf* c, int n_streams, int fs_stride, int cam_stride, int max_obs, int compact, int zero_fill, int teams,
                                       const int32_t* tri_list_dev, const int32_t* n_tri_dev, const int32_t* feat_list_dev, const int32_t* n_feat_dev,
                                       const int32_t* obs_off_dev, const int32_t* obs_cam_dev, const double* obs_z_dev, const int32_t* dof_dev, const int32_t* row_off_dev,
                                       const double* cam_q_dev, const double* cam_p_dev, const double* cam_qn_dev, const double* cam_pn_dev,
                                       const double* P_dev, int ld, int64_t p_stride, const double* gravity_dev,
                                       const double* T_cam0_cam1_rowmajor44, const double* opt5, double obs_noise,
                                       double* pos_dev, int32_t* valid_dev, double* H_dev, int64_t h_stride, double* r_dev, int64_t r_stride,
                                       double* gamma_dev, int32_t* pass_dev, void* stream)
{
    if (!c || n_streams < 1 || fs_stride < 1 || cam_stride < 1 || max_obs < 1 || teams < 1 || teams > 262144 || (tri_list_dev && !n_tri_dev) ||
        !obs_off_dev || !obs_cam_dev || !obs_z_dev || !cam_q_dev || !cam_p_dev || !T_cam0_cam1_rowmajor44 || !opt5 || !pos_dev || !valid_dev ||
        (feat_list_dev && (!n_feat_dev || !dof_dev || !row_off_dev || !cam_qn_dev || !cam_pn_dev || !P_dev || !gravity_dev || !H_dev || !r_dev || !gamma_dev || !pass_dev)) ||
        ld < IMU_DIM + 6 * cam_stride || p_stride < 0 || h_stride < 0 || r_stride < 0 ||
        compact < 0 || (compact > 0 && (compact < 6 * max_obs || zero_fill))) {         // (the zero fill clears full-width rows: compact rows have no room for it)
        av_set_error("av_msckf_feature_ops_dev: bad arguments");
        return AV_E_INVALID;
    }
    if (2 * max_obs > 64) { av_set_error("av_msckf_feature_ops_dev: %d observations per feature exceed one wavefront (32)", max_obs); return AV_E_CAPACITY; }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(c->device));
    if (tri_list_dev) {
        TriArgs t = tri_args_base(cam_q_dev, cam_p_dev, cam_stride, T_cam0_cam1_rowmajor44, opt5);
        t.obs_off = obs_off_dev; t.obs_cam = obs_cam_dev; t.obs_z = obs_z_dev;
        t.out_pos = pos_dev; t.out_valid = valid_dev;
        t.list = tri_list_dev; t.n_list_dev = n_tri_dev; t.fs_stride = fs_stride;
        hipLaunchKernelGGL(triangulate_kernel, dim3(teams), dim3(64), 0, stm, t);
        AV_LAUNCH_CHECK();
    }
    if (!feat_list_dev) return AV_OK;
    FeatArgs f; memset(&f, 0, sizeof(f));
    f.cam_q = cam_q_dev; f.cam_p = cam_p_dev; f.cam_qn = cam_qn_dev; f.cam_pn = cam_pn_dev;
    f.ld = ld; f.P = P_dev; f.chi2 = c->chi2;
    unpack_T01(T_cam0_cam1_rowmajor44, f.R01, f.t01);
    f.obs_noise = obs_noise; f.Hout = H_dev; f.rout = r_dev;
    f.cam_stride = cam_stride; f.p_stride = (size_t)p_stride; f.h_stride = (size_t)h_stride; f.r_stride = (size_t)r_stride;
    f.zero_fill = zero_fill ? 1 : 0; f.compact = compact;
    f.fs_stride = fs_stride; f.stream_gravity = gravity_dev;
    f.obs_off = obs_off_dev; f.obs_cam = obs_cam_dev; f.obs_z = obs_z_dev; f.pos = pos_dev; f.dof = dof_dev; f.row_off = row_off_dev;
    f.gamma = gamma_dev; f.pass = pass_dev; f.valid = valid_dev;
    f.feat_list = feat_list_dev; f.n_list_dev = n_feat_dev;
    return launch_feature_dev(f, teams, max_obs, stm);
}

// Parity-test entry for the prediction of the device-resident filter (tests only; no step of the filter calls it): for n_streams
// streams described by flat host arrays, what a step launches before any feature is looked at -- dk_state, then dk_cov<wg>, through
// dev_launch_predict, the helper dev_enqueue itself calls -- on the caller's device arrays of camera states and covariances; then, for
// the streams that ask for it, dev_find_redundant and remove_two_cams_body through dk_prune_probe (the one kernel only this entry
// launches).  Layouts (doubles / ints per stream):
//   state_io[43]    ts, q[4], p[3], v[3], bg[3], ba[3], R_ic[9], t_ci[3], qn[4], pn[3], vn[3], gravity[3], tracking_rate   (in / out)
//   state_int_io[6] n, ncam, failed, null_aliased, first_img (in / out), active (out)
//   ctl[6]          active, imu_first, imu_cnt, ops (bit 0: redundancy rule, bit 1: removal), rm0, rm1 (window positions, after the prediction)
//   imu[7]          t, w[3], a[3] per sample
//   redundant_out[2] the two positions of the redundancy rule, -1 where it was not asked for
// Every argument is checked before anything is launched: no input can send a kernel out of bounds.  Synchronises.
// cap > 0 (av_msckf_predict_ops_dev_rate): dev_launch_predict also launches the IMU-rate record kernel; rec_out [S][cap] and n_out [S][2]
// go to the device as the caller filled them and come back as the kernel left them.
static int predict_ops_dev_body(av_msckf* c, int n_streams, int wg, int cam_stride, int ld, int64_t p_stride,
                                double* state_io, int32_t* state_int_io, const double* t_frame, const int32_t* ctl,
                                const double* imu, int n_imu, const double* noise4,
                                double* cam_q_dev, double* cam_p_dev, double* cam_qn_dev, double* P_dev,
                                int32_t* redundant_out, void* stream, int cap, av_imu_state* rec_out, int32_t* n_out)
{
    constexpr int SD = 43, SI = 6, CI = 6;
    if (cap < 0 || cap > IMU_RATE_CAP_MAX || (cap > 0 && (!rec_out || !n_out)) ||
        !c || n_streams < 1 || n_streams > 65536 || (wg != 64 && wg != 256) || cam_stride < 1 || cam_stride > 64 || n_imu < 0 || (n_imu > 0 && !imu) ||
        !state_io || !state_int_io || !t_frame || !ctl || !noise4 || !cam_q_dev || !cam_p_dev || !cam_qn_dev || !P_dev || !redundant_out ||
        ld < IMU_DIM + 6 * cam_stride || p_stride < (int64_t)ld * ld) {
        av_set_error("av_msckf_predict_ops_dev: bad arguments");
        return AV_E_INVALID;
    }
    const int S = n_streams;
    bool any_ops = false;
    for (int s = 0; s < S; ++s) {
        const int32_t* I = state_int_io + (size_t)s * SI; const int32_t* C = ctl + (size_t)s * CI;
        const int n = I[0], ncam = I[1];
        if (ncam < 0 || n != IMU_DIM + 6 * ncam || C[1] < 0 || C[2] < 0 || (int64_t)C[1] + C[2] > n_imu || (C[3] & ~3)) {
            av_set_error("av_msckf_predict_ops_dev: stream %d: inconsistent sizes, samples outside their array or unknown ops", s);
            return AV_E_INVALID;
        }
        // a full window (ncam == cam_stride) is the kernel's own refusal to test (DFAIL_CAMS: nothing of the stream is touched); more is not representable
        if (ncam > cam_stride) { av_set_error("av_msckf_predict_ops_dev: stream %d holds %d camera states, cam_stride is %d", s, ncam, cam_stride); return AV_E_CAPACITY; }
        const bool grows = C[0] && !I[2] && ncam + 1 <= cam_stride;          // what dk_state decides
        const int after = ncam + (grows ? 1 : 0);
        if ((C[3] & 1) && after < 4) { av_set_error("av_msckf_predict_ops_dev: stream %d: the redundancy rule needs four camera states", s); return AV_E_INVALID; }
        if ((C[3] & 2) && !(C[4] >= 0 && C[4] < C[5] && C[5] < after)) {
            av_set_error("av_msckf_predict_ops_dev: stream %d: removal positions %d, %d are not ascending inside a window of %d", s, C[4], C[5], after);
            return AV_E_INVALID;
        }
        any_ops = any_ops || C[3];
    }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(c->device));
    // one device allocation for everything the kernels need besides the caller's arrays, released on every way out
    struct Arena { AvScratch mem; char* p = nullptr; size_t used = 0;
                   size_t take(size_t bytes) { const size_t o = used; used += (bytes + 255) / 256 * 256; return o; } } ar;
    const size_t nimu = (size_t)(n_imu > 0 ? n_imu : 1), ncs = (size_t)S * cam_stride;
    const size_t o_st = ar.take(sizeof(DState) * S), o_ctl = ar.take(sizeof(DCtl) * S), o_imu = ar.take(sizeof(DImu) * nimu), o_prop = ar.take(sizeof(PropArgs) * nimu),
                 o_cov = ar.take(sizeof(DCov) * S), o_cnt = ar.take(sizeof(int) * 16), o_id = ar.take(sizeof(long long) * ncs), o_nc = ar.take(sizeof(int) * S),
                 o_ns = ar.take(sizeof(int) * S), o_gr = ar.take(sizeof(double) * 3 * S), o_ops = ar.take(sizeof(int) * S), o_rm = ar.take(sizeof(int) * 2 * S),
                 o_red = ar.take(sizeof(int) * 2 * S), o_scr = ar.take(any_ops ? sizeof(double) * (size_t)p_stride * S : 8),
                 o_ir = ar.take(sizeof(DImuState) * S * (size_t)(cap > 0 ? cap : 1)), o_irn = ar.take(sizeof(int) * 2 * S);
    { const int rca = ar.mem.alloc(ar.used); if (rca) return rca; }
    ar.p = static_cast<char*>(ar.mem.p);
    std::vector<DState> st((size_t)S); std::vector<DCtl> ct((size_t)S); std::vector<DImu> im(nimu);
    std::vector<int> ops((size_t)S), rm((size_t)2 * S), red((size_t)2 * S, -1);
    memset(st.data(), 0, sizeof(DState) * S); memset(ct.data(), 0, sizeof(DCtl) * S); memset(im.data(), 0, sizeof(DImu) * nimu);
    for (int s = 0; s < S; ++s) {
        const double* d = state_io + (size_t)s * SD; const int32_t* I = state_int_io + (size_t)s * SI; const int32_t* C = ctl + (size_t)s * CI;
        DState& D = st[s];
        D.ts = d[0];
        memcpy(D.q, d + 1, 32); memcpy(D.p, d + 5, 24); memcpy(D.v, d + 8, 24); memcpy(D.bg, d + 11, 24); memcpy(D.ba, d + 14, 24);
        memcpy(D.R_ic, d + 17, 72); memcpy(D.t_ci, d + 26, 24); memcpy(D.qn, d + 29, 32); memcpy(D.pn, d + 33, 24); memcpy(D.vn, d + 36, 24);
        memcpy(D.gravity, d + 39, 24); D.tracking_rate = d[42];
        D.n = I[0]; D.ncam = I[1]; D.failed = I[2]; D.null_aliased = I[3]; D.first_img = I[4];
        DCtl& K = ct[s];
        K.t_frame = t_frame[s]; K.active = C[0]; K.has_init = 0; K.imu_first = C[1]; K.imu_cnt = C[2];
        ops[s] = C[3]; rm[2 * s] = C[4]; rm[2 * s + 1] = C[5];
    }
    for (int i = 0; i < n_imu; ++i) { im[i].t = imu[7 * i]; for (int e = 0; e < 3; ++e) { im[i].w[e] = imu[7 * i + 1 + e]; im[i].a[e] = imu[7 * i + 4 + e]; } }
    DevArgs a; memset(&a, 0, sizeof(a));
    a.S = S; a.cs = cam_stride; a.max_cam = cam_stride - 1; a.ld = ld; a.pstride = (size_t)p_stride;
    a.P = P_dev; a.scratch = (double*)(ar.p + o_scr);
    a.st = (DState*)(ar.p + o_st); a.cam_id = (long long*)(ar.p + o_id); a.cam_q = cam_q_dev; a.cam_p = cam_p_dev; a.cam_qn = cam_qn_dev;
    a.ncam = (int*)(ar.p + o_nc); a.nstate = (int*)(ar.p + o_ns); a.grav = (double*)(ar.p + o_gr);
    a.cnt = a.cnt_next = (int*)(ar.p + o_cnt);
    a.ctl = (const DCtl*)(ar.p + o_ctl); a.imu = (const DImu*)(ar.p + o_imu); a.prop = (PropArgs*)(ar.p + o_prop); a.cov = (DCov*)(ar.p + o_cov);
    for (int i = 0; i < 4; ++i) a.noise[i] = noise4[i];
    AV_HIP(hipMemcpyAsync(a.st, st.data(), sizeof(DState) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_ctl, ct.data(), sizeof(DCtl) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_imu, im.data(), sizeof(DImu) * nimu, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_ops, ops.data(), sizeof(int) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_rm, rm.data(), sizeof(int) * 2 * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_red, red.data(), sizeof(int) * 2 * S, hipMemcpyHostToDevice, stm));
    IrOut ir{};
    if (cap > 0) {
        ir = IrOut{(DImuState*)(ar.p + o_ir), (int*)(ar.p + o_irn), cap};
        AV_HIP(hipMemcpyAsync(ir.rec, rec_out, sizeof(DImuState) * S * (size_t)cap, hipMemcpyHostToDevice, stm));
        AV_HIP(hipMemcpyAsync(ir.n, n_out, sizeof(int) * 2 * S, hipMemcpyHostToDevice, stm));
    }
    dev_launch_predict(a, S, wg, false, stm, ir);
    AV_LAUNCH_CHECK();
    if (cap > 0) {
        AV_HIP(hipMemcpyAsync(rec_out, ir.rec, sizeof(DImuState) * S * (size_t)cap, hipMemcpyDeviceToHost, stm));
        AV_HIP(hipMemcpyAsync(n_out, ir.n, sizeof(int) * 2 * S, hipMemcpyDeviceToHost, stm));
    }
    if (any_ops) {
        hipLaunchKernelGGL(dk_prune_probe, dim3(S), dim3(wg), 0, stm, a, (const int*)(ar.p + o_ops), (const int*)(ar.p + o_rm), (int*)(ar.p + o_red));
        AV_LAUNCH_CHECK();
    }
    AV_HIP(hipMemcpyAsync(st.data(), a.st, sizeof(DState) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(red.data(), ar.p + o_red, sizeof(int) * 2 * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipStreamSynchronize(stm));
    for (int s = 0; s < S; ++s) {
        double* d = state_io + (size_t)s * SD; int32_t* I = state_int_io + (size_t)s * SI;
        const DState& D = st[s];
        d[0] = D.ts;
        memcpy(d + 1, D.q, 32); memcpy(d + 5, D.p, 24); memcpy(d + 8, D.v, 24); memcpy(d + 11, D.bg, 24); memcpy(d + 14, D.ba, 24);
        memcpy(d + 17, D.R_ic, 72); memcpy(d + 26, D.t_ci, 24); memcpy(d + 29, D.qn, 32); memcpy(d + 33, D.pn, 24); memcpy(d + 36, D.vn, 24);
        memcpy(d + 39, D.gravity, 24); d[42] = D.tracking_rate;
        I[0] = D.n; I[1] = D.ncam; I[2] = D.failed; I[3] = D.null_aliased; I[4] = D.first_img; I[5] = D.active;
        redundant_out[2 * s] = red[2 * s]; redundant_out[2 * s + 1] = red[2 * s + 1];
    }
    return AV_OK;
}
AV_EXPORT int av_msckf_predict_ops_dev(av_msckf* c, int n_streams, int wg, int cam_stride, int ld, int64_t p_stride,
                                       double* state_io, int32_t* state_int_io, const double* t_frame, const int32_t* ctl,
                                       const double* imu, int n_imu, const double* noise4,
                                       double* cam_q_dev, double* cam_p_dev, double* cam_qn_dev, double* P_dev,
                                       int32_t* redundant_out, void* stream)
{
    return predict_ops_dev_body(c, n_streams, wg, cam_stride, ld, p_stride, state_io, state_int_io, t_frame, ctl, imu, n_imu, noise4,
                                cam_q_dev, cam_p_dev, cam_qn_dev, P_dev, redundant_out, stream, 0, nullptr, nullptr);
}
// The same with the IMU-rate odometry on (airvision.h, "IMU-rate odometry"): cap >= 1 records per stream, rec_out [n_streams][cap] and
// n_out [n_streams][2] HOST arrays, uploaded as the caller filled them (a pre-fill shows what the kernel did not write) and read back.
AV_EXPORT int av_msckf_predict_ops_dev_rate(av_msckf* c, int n_streams, int wg, int cam_stride, int ld, int64_t p_stride,
                                            double* state_io, int32_t* state_int_io, const double* t_frame, const int32_t* ctl,
                                            const double* imu, int n_imu, const double* noise4,
                                            double* cam_q_dev, double* cam_p_dev, double* cam_qn_dev, double* P_dev,
                                            int32_t* redundant_out, void* stream, int cap, av_imu_state* rec_out, int32_t* n_out)
{
    if (cap < 1) { av_set_error("av_msckf_predict_ops_dev_rate: cap must be 1 .. %d", IMU_RATE_CAP_MAX); return AV_E_INVALID; }
    return predict_ops_dev_body(c, n_streams, wg, cam_stride, ld, p_stride, state_io, state_int_io, t_frame, ctl, imu, n_imu, noise4,
                                cam_q_dev, cam_p_dev, cam_qn_dev, P_dev, redundant_out, stream, cap, rec_out, n_out);
}

// Parity-test entry for the batched measurement update (tests only; no step of the filter calls it): for n_streams streams, what a phase
// of a step launches from the stacking decisions to the covariance update -- dev_launch_update, the helper dev_phase itself calls -- on
// the caller's candidate features, block buffers and covariances.  phase 0: the lost-feature phase's configuration (the `> 1500 rows`
// cut, no information form, dense rows, streams with more than kch rows compressed; kch = 0: the step's own, min(136, ld)); phase 1: the pruning phase's (no cut, information
// form for the streams that qualify; hld > 0: compact rows and NO Cholesky back end, as a step launches it).  Candidates of stream s are
// the slots [s * fs_stride, s * fs_stride + n_cand[s]) of obs_off [n_streams * fs_stride + 1] / pass / row_off (HOST arrays; obs_cam
// [n_obs] holds the camera slot of every observation); their rows lie in the stream's region of the DEVICE block buffers (H_dev +
// s * h_stride, rows of hld > 0 ? hld : ld doubles; r_dev + s * r_stride; rows_cap rows each).  The work buffers are the batch's
// (upd_args_of: ldt = rows_cap, one p_stride each), taken here and released before the entry returns.  Returns per stream delta_x
// (dx_io [ld], uploaded as the caller filled it), stacked, the touched columns (cols_out [6 cam_stride], -1 behind them) and the record
// upd_stack_kernel wrote (rec_out [5]: m, nc, mode, kdir, n_blk).  Every argument is checked before anything is launched -- the
// stacking rule is repeated on the host for it --, so that no input can send a kernel out of bounds.  Synchronises.
AV_EXPORT int av_msckf_update_ops_dev(av_msckf* c, int n_streams, int phase, int kch, int fs_stride, int cam_stride, int hld,
                                      const int32_t* stream_n, const int32_t* stream_mode, const int32_t* n_cand,
                                      const int32_t* obs_off, const int32_t* obs_cam, int n_obs, const int32_t* pass, const int32_t* row_off,
                                      const double* H_dev, int64_t h_stride, const double* r_dev, int64_t r_stride, int rows_cap,
                                      double* P_dev, int ld, int64_t p_stride, double obs_noise,
                                      double* dx_io, int32_t* stacked_out, int32_t* cols_out, int32_t* rec_out, void* stream)
{
    constexpr int KMAX = 144;                    // rows one back-end pass keeps at most (BATCH_KMAX; upd_gather_kernel's row map holds 256)
    if (!c || n_streams < 1 || n_streams > 4096 || (phase != 0 && phase != 1) || kch < 0 || kch > DEV_KCH || fs_stride < 1 || fs_stride > (1 << 20) ||
        cam_stride < 1 || cam_stride > 64 || hld < 0 || n_obs < 0 || rows_cap < 1 || rows_cap > (1 << 20) || ld < IMU_DIM || ld > IMU_DIM + 6 * 64 ||
        p_stride < (int64_t)ld * ld || !stream_n || !stream_mode || !n_cand || !obs_off || (n_obs > 0 && !obs_cam) || !pass || !row_off ||
        !H_dev || !r_dev || !P_dev || !dx_io || !stacked_out || !cols_out || !rec_out || !(obs_noise > 0.0)) {
        av_set_error("av_msckf_update_ops_dev: bad arguments");
        return AV_E_INVALID;
    }
    if (phase == 0 && hld != 0) { av_set_error("av_msckf_update_ops_dev: compact rows (hld = %d) are the pruning phase's: phase 0 reads full-width rows", hld); return AV_E_INVALID; }
    const int S = n_streams, kc = kch ? kch : dev_kch(ld), width = hld > 0 ? hld : ld;
    const bool rounds = hld == 0, info = phase == 1;
    if (h_stride < (int64_t)rows_cap * width || r_stride < rows_cap) { av_set_error("av_msckf_update_ops_dev: the block-buffer strides do not hold rows_cap = %d rows", rows_cap); return AV_E_INVALID; }
    const int kmax = kc > 6 * cam_stride ? kc : 6 * cam_stride;
    size_t lds_i = 0;
    // the stacking rule (upd_stack_kernel) on the host: every index and size a kernel will use is known, and checked, before the launch
    for (int s = 0; s < S; ++s) {
        const int n = stream_n[s], nk = n_cand[s];
        if (n > ld) { av_set_error("av_msckf_update_ops_dev: stream %d: n = %d exceeds ld = %d", s, n, ld); return AV_E_CAPACITY; }
        if (n < IMU_DIM || (n - IMU_DIM) % 6 || (stream_mode[s] != 1 && stream_mode[s] != 2)) { av_set_error("av_msckf_update_ops_dev: stream %d: n = %d is not 21 + 6 ncam, or mode %d is not 1 or 2", s, n, stream_mode[s]); return AV_E_INVALID; }
        const int ncam = (n - IMU_DIM) / 6;
        if (ncam > cam_stride) { av_set_error("av_msckf_update_ops_dev: stream %d holds %d camera states, cam_stride is %d", s, ncam, cam_stride); return AV_E_CAPACITY; }
        if (nk < 0) { av_set_error("av_msckf_update_ops_dev: stream %d: negative candidate count", s); return AV_E_INVALID; }
        if (nk > fs_stride) { av_set_error("av_msckf_update_ops_dev: stream %d: %d candidates, fs_stride is %d", s, nk, fs_stride); return AV_E_CAPACITY; }
        long long m = 0; int nb = 0; unsigned long long used = 0ull;
        for (int k = 0; k < nk; ++k) {
            const size_t i = (size_t)s * fs_stride + k;
            const int o0 = obs_off[i], o1 = obs_off[i + 1];
            if (o0 < 0 || o1 < o0 || o1 > n_obs || o1 - o0 > 64) { av_set_error("av_msckf_update_ops_dev: stream %d, candidate %d: observations outside their array", s, k); return AV_E_INVALID; }
            for (int q = o0; q < o1; ++q) if (obs_cam[q] < 0 || obs_cam[q] >= ncam) { av_set_error("av_msckf_update_ops_dev: stream %d, candidate %d: camera slot %d outside the window of %d (cam_stride %d)", s, k, obs_cam[q], ncam, cam_stride); return AV_E_INVALID; }
            const int rows = 4 * (o1 - o0) - 3;
            if (pass[i] && rows < 1) { av_set_error("av_msckf_update_ops_dev: stream %d, candidate %d passes the gate without an observation", s, k); return AV_E_INVALID; }
            if (!pass[i] || (phase == 0 && m > 1500)) continue;      // (behind the cut nothing is stacked; the kernel still reads the flags)
            if (row_off[i] < 0 || (long long)row_off[i] + rows > rows_cap) { av_set_error("av_msckf_update_ops_dev: stream %d, candidate %d: rows %d .. %d outside the block buffer of %d rows", s, k, row_off[i], row_off[i] + rows, rows_cap); return AV_E_CAPACITY; }
            m += rows; ++nb;
            for (int q = o0; q < o1; ++q) used |= 1ull << obs_cam[q];
        }
        if (nb > STACK_LDS_BLOCKS || stream_mode[s] == 2 || m == 0) continue;      // the kernel's own refusals: nothing of the stream is touched
        const int nc = 6 * __builtin_popcountll(used);
        if (nc > MFMA_MAXCOLS) { av_set_error("av_msckf_update_ops_dev: stream %d touches %d columns, the back end holds %d", s, nc, MFMA_MAXCOLS); return AV_E_CAPACITY; }
        if (m > rows_cap) { av_set_error("av_msckf_update_ops_dev: stream %d stacks %lld rows, ldt = rows_cap is %d", s, m, rows_cap); return AV_E_CAPACITY; }
        const bool inf = info && nc <= INFO_NC && m <= INFO_MAXROWS;
        if (hld > 0 && (!inf || hld < nc)) { av_set_error("av_msckf_update_ops_dev: stream %d: compact rows of %d doubles, but the stream touches %d columns or does not take the information form", s, hld, nc); return AV_E_INVALID; }
        if (inf) { const size_t l = upd_info_lds(nc, n, (int)m); lds_i = l > lds_i ? l : lds_i; continue; }
        const bool comp = m > kc && upd_compress((int)m, nc);
        const long long k = m <= kc ? m : upd_k((int)m, nc);
        if (k > KMAX || k > ld || k > kmax || (size_t)((k + 15) / 16) * 256 > (size_t)p_stride) { av_set_error("av_msckf_update_ops_dev: stream %d keeps %lld rows in one pass (at most %d, ld = %d)", s, k, KMAX, ld); return AV_E_CAPACITY; }
        if (comp && (m > 2 * (long long)p_stride || nc + 1 > ld)) { av_set_error("av_msckf_update_ops_dev: stream %d: the row map of %lld rows does not fit its work buffer", s, m); return AV_E_CAPACITY; }
    }
    if (lds_i > 160 * 1024) { av_set_error("av_msckf_update_ops_dev: the information form needs %zu B of LDS, 163840 available", lds_i); return AV_E_CAPACITY; }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(c->device));
    // one device allocation for everything the kernels need besides the caller's arrays, released on every way out
    struct Arena { AvScratch mem; char* p = nullptr; size_t used = 0;
                   size_t take(size_t bytes) { const size_t o = used; used += (bytes + 255) / 256 * 256; return o; } } ar;
    const size_t nf = (size_t)S * fs_stride + 1, ps = (size_t)p_stride, ws = upd_w_doubles(rows_cap, ld), ncols = (size_t)S * 6 * cam_stride;
    const size_t o_W = ar.take(sizeof(double) * S * ws), o_T = ar.take(sizeof(double) * S * ps), o_Kt = ar.take(sizeof(double) * S * ps),
                 o_Pn = ar.take(sizeof(double) * S * ps), o_Sb = ar.take(sizeof(double) * S * ps), o_dx = ar.take(sizeof(double) * S * ld),
                 o_base = ar.take(sizeof(UpdArgs) * S), o_upd = ar.take(sizeof(UpdArgs) * S), o_br = ar.take(sizeof(int) * nf), o_bl = ar.take(sizeof(int) * nf),
                 o_cols = ar.take(sizeof(int) * ncols), o_clist = ar.take(sizeof(int) * ((size_t)S + 8)), o_cnt = ar.take(sizeof(int) * 16),
                 o_stk = ar.take(sizeof(int) * S), o_n = ar.take(sizeof(int) * S), o_nc = ar.take(sizeof(int) * S), o_off = ar.take(sizeof(int) * nf),
                 o_cam = ar.take(sizeof(int) * (size_t)(n_obs > 0 ? n_obs : 1)), o_pass = ar.take(sizeof(int) * nf), o_ro = ar.take(sizeof(int) * nf);
    { const int rca = ar.mem.alloc(ar.used); if (rca) return rca; }
    ar.p = static_cast<char*>(ar.mem.p);
    AV_HIP(hipMemsetAsync(ar.p, 0, ar.used, stm));
    AV_HIP(hipMemsetAsync(ar.p + o_cols, 0xFF, sizeof(int) * ncols, stm));          // -1 behind a stream's touched columns
    const UpdBufs B{P_dev, (double*)(ar.p + o_Pn), (double*)(ar.p + o_T), (double*)(ar.p + o_Kt), (double*)(ar.p + o_Sb), (double*)(ar.p + o_W), (double*)(ar.p + o_dx),
                    H_dev, r_dev, ps, (size_t)h_stride, (size_t)r_stride, ws, ld, rows_cap, obs_noise};
    std::vector<UpdArgs> base((size_t)S);
    for (int s = 0; s < S; ++s) { UpdArgs& u = base[s] = upd_args_of(B, s); u.n = stream_n[s]; u.mode = stream_mode[s]; }
    AV_HIP(hipMemcpyAsync(ar.p + o_base, base.data(), sizeof(UpdArgs) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_dx, dx_io, sizeof(double) * S * ld, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_n, stream_n, sizeof(int) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_nc, n_cand, sizeof(int) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_off, obs_off, sizeof(int) * nf, hipMemcpyHostToDevice, stm));
    if (n_obs > 0) AV_HIP(hipMemcpyAsync(ar.p + o_cam, obs_cam, sizeof(int) * n_obs, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_pass, pass, sizeof(int) * (nf - 1), hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_ro, row_off, sizeof(int) * (nf - 1), hipMemcpyHostToDevice, stm));
    int* cnt = (int*)(ar.p + o_cnt);
    StackArgs sa; memset(&sa, 0, sizeof(sa));
    sa.n_cand = (const int*)(ar.p + o_nc); sa.fs_stride = fs_stride; sa.stream_n = (const int*)(ar.p + o_n);
    sa.pass = (const int*)(ar.p + o_pass); sa.obs_off = (const int*)(ar.p + o_off); sa.obs_cam = (const int*)(ar.p + o_cam); sa.row_off = (const int*)(ar.p + o_ro);
    sa.blk_row = (int*)(ar.p + o_br); sa.blk_len = (int*)(ar.p + o_bl); sa.cols = (int*)(ar.p + o_cols); sa.cols_stride = 6 * cam_stride;
    sa.base = (const UpdArgs*)(ar.p + o_base); sa.out = (UpdArgs*)(ar.p + o_upd); sa.S = S; sa.rounds = 1; sa.cut1500 = phase == 0 ? 1 : 0; sa.kch = kc;
    sa.stacked = (int*)(ar.p + o_stk); sa.clist = (int*)(ar.p + o_clist); sa.clist_count = cnt + 6;
    sa.hld = hld; sa.no_info = phase == 0 ? 1 : 0;
    UpdLaunch ul;
    ul.info = info; ul.lds_info = lds_i ? lds_i : upd_info_lds(12, IMU_DIM, 1);
    ul.rounds = rounds; ul.n_list = (unsigned)S; ul.k1max = 6 * cam_stride + 1; ul.kmax = kmax; ul.nmax = ld;
    { const int rcl = dev_launch_update(sa, ul, stm); if (rcl) return rcl; }
    std::vector<UpdArgs> upd((size_t)S);
    std::vector<int> cols(ncols);
    AV_HIP(hipMemcpyAsync(upd.data(), ar.p + o_upd, sizeof(UpdArgs) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(dx_io, ar.p + o_dx, sizeof(double) * S * ld, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(stacked_out, ar.p + o_stk, sizeof(int) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(cols_out, ar.p + o_cols, sizeof(int) * ncols, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipStreamSynchronize(stm));
    for (int s = 0; s < S; ++s) {
        const UpdArgs& u = upd[s];
        int32_t* r = rec_out + (size_t)5 * s;
        r[0] = u.m; r[1] = u.nc; r[2] = u.mode; r[3] = u.kdir; r[4] = u.n_blk;
    }
    return AV_OK;
}

// Parity-test entry for the forecast (airvision.h, "Forecast"; tests only; no step of the filter calls it): for n_streams streams
// described by the flat host arrays of av_msckf_predict_ops_dev -- state_io[43], state_int_io[6], of which `active` is an INPUT here: the
// state a step leaves -- the forecast's two kernels through dev_launch_forecast, the helper dev_enqueue itself calls, on the caller's
// device covariances.  pend[2] per stream = (first, count): its pending samples are imu[first .. first + count), of which the first
// min(count, cap) are integrated.  rec_out [n_streams][cap], n_out [n_streams][2] and cov_out [n_streams][120] are HOST arrays, uploaded
// as the caller filled them (a pre-fill shows what the kernels did not write) and read back.  state_io and state_int_io come back as the
// kernels left them on the device: unchanged.  Every argument is checked before anything is launched.  Synchronises.
AV_EXPORT int av_msckf_forecast_ops_dev(av_msckf* c, int n_streams, int ld, int64_t p_stride, double* state_io, int32_t* state_int_io,
                                        const double* imu, int n_imu, const int32_t* pend, const double* noise4, double* P_dev, void* stream,
                                        int cap, av_imu_state* rec_out, int32_t* n_out, double* cov_out)
{
    constexpr int SD = 43, SI = 6;
    if (!c || n_streams < 1 || n_streams > 65536 || cap < 1 || cap > FORECAST_CAP_MAX || n_imu < 0 || (n_imu > 0 && !imu) || !state_io || !state_int_io ||
        !pend || !noise4 || !P_dev || !rec_out || !n_out || !cov_out || ld < IMU_DIM || p_stride < (int64_t)ld * ld) {
        av_set_error("av_msckf_forecast_ops_dev: bad arguments");
        return AV_E_INVALID;
    }
    const int S = n_streams;
    for (int s = 0; s < S; ++s) {
        const int32_t* I = state_int_io + (size_t)s * SI;
        if (I[1] < 0 || I[0] != IMU_DIM + 6 * I[1] || I[0] > ld || pend[2 * s] < 0 || pend[2 * s + 1] < 0 || (int64_t)pend[2 * s] + pend[2 * s + 1] > n_imu) {
            av_set_error("av_msckf_forecast_ops_dev: stream %d: inconsistent sizes or samples outside their array", s);
            return AV_E_INVALID;
        }
    }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(c->device));
    struct Arena { AvScratch mem; char* p = nullptr; size_t used = 0;
                   size_t take(size_t bytes) { const size_t o = used; used += (bytes + 255) / 256 * 256; return o; } } ar;
    const size_t nimu = (size_t)(n_imu > 0 ? n_imu : 1);
    const size_t o_st = ar.take(sizeof(DState) * S), o_imu = ar.take(sizeof(DImu) * nimu), o_prop = ar.take(sizeof(PropArgs) * nimu), o_pend = ar.take(sizeof(int) * 3 * S),
                 o_rec = ar.take(sizeof(DImuState) * S * (size_t)cap), o_n = ar.take(sizeof(int) * 2 * S), o_cov = ar.take(sizeof(double) * ODOM_COV_DOUBLES * S);
    { const int rca = ar.mem.alloc(ar.used); if (rca) return rca; }
    ar.p = static_cast<char*>(ar.mem.p);
    std::vector<DState> st((size_t)S); std::vector<DImu> im(nimu); std::vector<int> pd((size_t)3 * S);
    memset(st.data(), 0, sizeof(DState) * S); memset(im.data(), 0, sizeof(DImu) * nimu);
    for (int s = 0; s < S; ++s) {
        const double* d = state_io + (size_t)s * SD; const int32_t* I = state_int_io + (size_t)s * SI;
        DState& D = st[s];
        D.ts = d[0];
        memcpy(D.q, d + 1, 32); memcpy(D.p, d + 5, 24); memcpy(D.v, d + 8, 24); memcpy(D.bg, d + 11, 24); memcpy(D.ba, d + 14, 24);
        memcpy(D.R_ic, d + 17, 72); memcpy(D.t_ci, d + 26, 24); memcpy(D.qn, d + 29, 32); memcpy(D.pn, d + 33, 24); memcpy(D.vn, d + 36, 24);
        memcpy(D.gravity, d + 39, 24); D.tracking_rate = d[42];
        D.n = I[0]; D.ncam = I[1]; D.failed = I[2]; D.null_aliased = I[3]; D.first_img = I[4]; D.active = I[5];
        pd[3 * s] = pend[2 * s]; pd[3 * s + 1] = pend[2 * s + 1]; pd[3 * s + 2] = pend[2 * s + 1] < cap ? pend[2 * s + 1] : cap;
    }
    for (int i = 0; i < n_imu; ++i) { im[i].t = imu[7 * i]; for (int e = 0; e < 3; ++e) { im[i].w[e] = imu[7 * i + 1 + e]; im[i].a[e] = imu[7 * i + 4 + e]; } }
    DevArgs a; memset(&a, 0, sizeof(a));
    a.S = S; a.ld = ld; a.pstride = (size_t)p_stride; a.P = P_dev;
    a.st = (DState*)(ar.p + o_st); a.imu = (const DImu*)(ar.p + o_imu); a.prop = (PropArgs*)(ar.p + o_prop);
    for (int i = 0; i < 4; ++i) a.noise[i] = noise4[i];
    const FcOut fc{(DImuState*)(ar.p + o_rec), (int*)(ar.p + o_n), (double*)(ar.p + o_cov), cap, (const int*)(ar.p + o_pend)};
    AV_HIP(hipMemcpyAsync(a.st, st.data(), sizeof(DState) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_imu, im.data(), sizeof(DImu) * nimu, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(ar.p + o_pend, pd.data(), sizeof(int) * 3 * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(fc.rec, rec_out, sizeof(DImuState) * S * (size_t)cap, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(fc.n, n_out, sizeof(int) * 2 * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(fc.cov, cov_out, sizeof(double) * ODOM_COV_DOUBLES * S, hipMemcpyHostToDevice, stm));
    dev_launch_forecast(a, S, fc, stm);
    AV_LAUNCH_CHECK();
    AV_HIP(hipMemcpyAsync(rec_out, fc.rec, sizeof(DImuState) * S * (size_t)cap, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(n_out, fc.n, sizeof(int) * 2 * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(cov_out, fc.cov, sizeof(double) * ODOM_COV_DOUBLES * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(st.data(), a.st, sizeof(DState) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipStreamSynchronize(stm));
    for (int s = 0; s < S; ++s) {
        double* d = state_io + (size_t)s * SD; int32_t* I = state_int_io + (size_t)s * SI;
        const DState& D = st[s];
        d[0] = D.ts;
        memcpy(d + 1, D.q, 32); memcpy(d + 5, D.p, 24); memcpy(d + 8, D.v, 24); memcpy(d + 11, D.bg, 24); memcpy(d + 14, D.ba, 24);
        memcpy(d + 17, D.R_ic, 72); memcpy(d + 26, D.t_ci, 24); memcpy(d + 29, D.qn, 32); memcpy(d + 33, D.pn, 24); memcpy(d + 36, D.vn, 24);
        memcpy(d + 39, D.gravity, 24); d[42] = D.tracking_rate;
        I[0] = D.n; I[1] = D.ncam; I[2] = D.failed; I[3] = D.null_aliased; I[4] = D.first_img; I[5] = D.active;
    }
    return AV_OK;
}

// Parity-test entry for the zero-velocity update (airvision.h, "Zero-velocity update"; tests only; no step of the filter calls it): for
// n_streams streams described by the flat host arrays of av_msckf_predict_ops_dev -- `active` an INPUT, as in av_msckf_forecast_ops_dev --
// dk_zupt_update through dev_launch_zupt_update, the helper dev_enqueue itself calls, on the caller's device camera states and
// covariances.  rec_io: HOST records, uploaded as the caller filled them (flags: the detector's verdict per stream) and read back.
// Every argument is checked before anything is launched.  Synchronises.
AV_EXPORT int av_msckf_zupt_ops_dev(av_msckf* c, int n_streams, int cam_stride, int ld, int64_t p_stride, double* state_io, int32_t* state_int_io,
                                    double* cam_q_dev, double* cam_p_dev, double* P_dev, const av_zupt_params* params, av_zupt* rec_io, void* stream)
{
    constexpr int SD = 43, SI = 6;
    if (!c || n_streams < 1 || n_streams > 65536 || cam_stride < 1 || cam_stride > 64 || !state_io || !state_int_io || !cam_q_dev || !cam_p_dev || !P_dev ||
        !params || !rec_io || ld < IMU_DIM || ld > IMU_DIM + 6 * 64 || p_stride < (int64_t)ld * ld || !zupt_params_ok(params)) {
        av_set_error("av_msckf_zupt_ops_dev: bad arguments");
        return AV_E_INVALID;
    }
    const int S = n_streams;
    for (int s = 0; s < S; ++s) {
        const int32_t* I = state_int_io + (size_t)s * SI;
        if (I[1] < 0 || I[1] > cam_stride || I[0] != IMU_DIM + 6 * I[1] || I[0] > ld) {
            av_set_error("av_msckf_zupt_ops_dev: stream %d: n = %d, %d camera states, cam_stride %d, ld %d do not fit", s, I[0], I[1], cam_stride, ld);
            return AV_E_INVALID;
        }
    }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(c->device));
    struct Arena { AvScratch mem; char* p = nullptr; size_t used = 0;
                   size_t take(size_t bytes) { const size_t o = used; used += (bytes + 255) / 256 * 256; return o; } } ar;
    const size_t o_st = ar.take(sizeof(DState) * S), o_rec = ar.take(sizeof(DZupt) * S);
    { const int rca = ar.mem.alloc(ar.used); if (rca) return rca; }
    ar.p = static_cast<char*>(ar.mem.p);
    std::vector<DState> st((size_t)S);
    memset(st.data(), 0, sizeof(DState) * S);
    for (int s = 0; s < S; ++s) {
        const double* d = state_io + (size_t)s * SD; const int32_t* I = state_int_io + (size_t)s * SI;
        DState& D = st[s];
        D.ts = d[0];
        memcpy(D.q, d + 1, 32); memcpy(D.p, d + 5, 24); memcpy(D.v, d + 8, 24); memcpy(D.bg, d + 11, 24); memcpy(D.ba, d + 14, 24);
        memcpy(D.R_ic, d + 17, 72); memcpy(D.t_ci, d + 26, 24); memcpy(D.qn, d + 29, 32); memcpy(D.pn, d + 33, 24); memcpy(D.vn, d + 36, 24);
        memcpy(D.gravity, d + 39, 24); D.tracking_rate = d[42];
        D.n = I[0]; D.ncam = I[1]; D.failed = I[2]; D.null_aliased = I[3]; D.first_img = I[4]; D.active = I[5];
    }
    DevArgs a; memset(&a, 0, sizeof(a));
    a.S = S; a.cs = cam_stride; a.ld = ld; a.pstride = (size_t)p_stride; a.P = P_dev;
    a.st = (DState*)(ar.p + o_st); a.cam_q = cam_q_dev; a.cam_p = cam_p_dev;
    const ZuArgs z = dev_zu_args(*params, (DZupt*)(ar.p + o_rec));
    AV_HIP(hipMemcpyAsync(a.st, st.data(), sizeof(DState) * S, hipMemcpyHostToDevice, stm));
    AV_HIP(hipMemcpyAsync(z.rec, rec_io, sizeof(DZupt) * S, hipMemcpyHostToDevice, stm));
    dev_launch_zupt_update(a, S, z, stm);
    AV_LAUNCH_CHECK();
    AV_HIP(hipMemcpyAsync(rec_io, z.rec, sizeof(DZupt) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(st.data(), a.st, sizeof(DState) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipStreamSynchronize(stm));
    for (int s = 0; s < S; ++s) {
        double* d = state_io + (size_t)s * SD; int32_t* I = state_int_io + (size_t)s * SI;
        const DState& D = st[s];
        d[0] = D.ts;
        memcpy(d + 1, D.q, 32); memcpy(d + 5, D.p, 24); memcpy(d + 8, D.v, 24); memcpy(d + 11, D.bg, 24); memcpy(d + 14, D.ba, 24);
        memcpy(d + 17, D.R_ic, 72); memcpy(d + 26, D.t_ci, 24); memcpy(d + 29, D.qn, 32); memcpy(d + 33, D.pn, 24); memcpy(d + 36, D.vn, 24);
        memcpy(d + 39, D.gravity, 24); d[42] = D.tracking_rate;
        I[0] = D.n; I[1] = D.ncam; I[2] = D.failed; I[3] = D.null_aliased; I[4] = D.first_img; I[5] = D.active;
    }
    return AV_OK;
}

// Work done so far, for the filter's roofline (drain first): [algorithmic fp64 flops of the gates, of the updates without the
// reference's QR, of that QR by the survey's formula, features gated, updates run, rows stacked, device time of the phase chains
// in ms (sum over stream groups; 0 unless timing was switched on with enable != 0 -- two HIP events per phase and group), phase
// timings that could not be read (counted, not silently dropped)].
// enable < 0 only reads.
AV_EXPORT int av_msckf_batch_work(av_msckf_batch* b, int enable, double out8[8])
{
    double* out6 = out8;
    if (!b || !out6) { av_set_error("av_msckf_batch_work: bad arguments"); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    for (int i = 0; i < 8; ++i) out6[i] = 0;
    for (av_msckf_batch* g : parts) {
        out6[6] += g->w_chain_ms; out6[7] += (double)g->w_chain_dropped;
        if (g->dev.cap > 0) {          // the counters are accumulated per stream by upd_stack_kernel
            std::vector<double> w((size_t)g->S * 8);
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(w.data(), g->dev.work, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
            for (int s = 0; s < g->S; ++s) { out6[0] += w[8 * s]; out6[1] += w[8 * s + 1]; out6[2] += w[8 * s + 2]; out6[3] += w[8 * s + 3]; out6[4] += w[8 * s + 4]; out6[5] += w[8 * s + 5]; }
        }
        if (enable >= 0) g->work_timing = enable != 0;
    }
    return AV_OK;
}

AV_EXPORT int av_msckf_batch_work_executed(av_msckf_batch* b, double* out2)
{
    if (!b || !out2) { av_set_error("av_msckf_batch_work_executed: bad arguments"); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    out2[0] = out2[1] = 0;
    for (av_msckf_batch* g : parts)
        if (g->dev.cap > 0) {
            std::vector<double> w((size_t)g->S * 8);
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(w.data(), g->dev.work, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
            for (int s = 0; s < g->S; ++s) { out2[0] += w[8 * s + 6]; out2[1] += w[8 * s + 7]; }
        }
    return AV_OK;
}

// [steps, stream-steps that ran the camera pruning, stream-steps whose lost-feature candidates outgrew rows_cap (rows from the
//  overflow pool), rebuilds of the device arrays after the first step (a wider message, more IMU samples in a frame), min / max
//  camera states, min / max map features] over all streams
AV_EXPORT int av_msckf_batch_counters(av_msckf_batch* b, int64_t out8[8])
{
    if (!b || !out8) { av_set_error("av_msckf_batch_counters: bad arguments"); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    long long steps = 0, prunes = 0, two = 0, grow = 0, cmin = 1 << 30, cmax = 0, mmin = 1 << 30, mmax = 0;
    for (av_msckf_batch* g : parts) {
        if (g->n_steps > steps) steps = g->n_steps;
        prunes += g->n_prune_stream_steps; two += g->n_two_pass_streams;
        if (g->dev.cap > 0) {
            std::vector<DState> st((size_t)g->S); std::vector<int> hdr((size_t)g->S * AVS_HDR_WORDS);
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(st.data(), g->dev.A.st, sizeof(DState) * st.size(), hipMemcpyDeviceToHost));
            AV_HIP(hipMemcpy(hdr.data(), g->dev.A.hdr, sizeof(int) * hdr.size(), hipMemcpyDeviceToHost));
            grow += g->dev.growths;
            for (int s = 0; s < g->S; ++s) {
                prunes += st[s].n_prune_steps; two += st[s].n_two_pass;
                const long long c = st[s].ncam, m = hdr[(size_t)s * AVS_HDR_WORDS + AVS_LIVE];
                if (c < cmin) cmin = c;
                if (c > cmax) cmax = c;
                if (m < mmin) mmin = m;
                if (m > mmax) mmax = m;
            }
            continue;
        }
        cmin = mmin = 0;          // a group before its first step: no camera state, empty maps
    }
    out8[0] = steps; out8[1] = prunes; out8[2] = two; out8[3] = grow; out8[4] = cmin; out8[5] = cmax; out8[6] = mmin; out8[7] = mmax;
    return AV_OK;
}

// What the batch launched: out17[0] = stream groups (1 without sub-batches), then per group its stream count and the workgroup size
// dev_enqueue gave the per-stream kernels (dk_begin4 / dk_cov / dk_mid / dk_finish) in the group's last enqueued step: 64 or 256, 0
// before its first step.  Reported as recorded at the launch, never recomputed.  Drains the queue
// first (the groups' workers write the record).
AV_EXPORT int av_msckf_batch_launch_shape(av_msckf_batch* b, int32_t out17[17])
{
    if (!b || !out17) { av_set_error("av_msckf_batch_launch_shape: bad arguments"); return AV_E_INVALID; }
    const int rc = av_msckf_batch_wait(b, 0);
    if (rc) return rc;
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    for (int i = 0; i < 17; ++i) out17[i] = 0;
    out17[0] = (int32_t)parts.size();          // (default_groups caps the groups at 8)
    for (size_t g = 0; g < parts.size() && g < 8; ++g) {
        out17[1 + 2 * g] = parts[g]->S;
        out17[2 + 2 * g] = parts[g]->dev.launched_wg;
    }
    return AV_OK;
}

// ---- the filter's quaternion / rotation helpers for host callers (src/utils.py:12-120; JPL convention [x, y, z, w]) --------
// The drop-in Python classes (dropin/utils.py) call these instead of restating the formulas: one implementation, the one the
// batched filter itself uses.  Pure host functions: no device, no context.
AV_EXPORT int av_quat_to_rotation(const double q[4], double R_rowmajor9[9])
{
    if (!q || !R_rowmajor9) { av_set_error("av_quat_to_rotation: bad arguments"); return AV_E_INVALID; }
    h_to_rotation(q, R_rowmajor9);
    return AV_OK;
}
AV_EXPORT int av_rotation_to_quat(const double R_rowmajor9[9], double q[4])
{
    if (!q || !R_rowmajor9) { av_set_error("av_rotation_to_quat: bad arguments"); return AV_E_INVALID; }
    h_to_quaternion(R_rowmajor9, q);
    return AV_OK;
}
AV_EXPORT int av_quat_multiply(const double q1[4], const double q2[4], double out[4])
{
    if (!q1 || !q2 || !out) { av_set_error("av_quat_multiply: bad arguments"); return AV_E_INVALID; }
    h_quat_mul(q1, q2, out);
    return AV_OK;
}
AV_EXPORT int av_quat_small_angle(const double dtheta[3], double q[4])
{
    if (!dtheta || !q) { av_set_error("av_quat_small_angle: bad arguments"); return AV_E_INVALID; }
    h_small_angle(dtheta, q);
    return AV_OK;
}
AV_EXPORT int av_quat_from_two_vectors(const double v0[3], const double v1[3], double q[4])
{
    if (!v0 || !v1 || !q) { av_set_error("av_quat_from_two_vectors: bad arguments"); return AV_E_INVALID; }
    h_from_two_vectors(v0, v1, q);
    return AV_OK;
}
