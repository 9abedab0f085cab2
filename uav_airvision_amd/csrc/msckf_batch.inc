// msckf_batch.inc -- S independent MSCKF filters stepped together (included at the end of msckf.hip).
//
// Same algorithm and the same kernels as the single-filter API above, but the bookkeeping of
// MSCKF.feature_callback (reference: src/msckf.py:177-228 and everything it calls) is done here in C++
// for all streams, and every numeric phase is ONE batched launch over all streams:
//   propagate (block per stream, its IMU samples in order) -> augment -> [lost features]
//   triangulate (wave per feature, all streams) -> Jacobian/null-space/gate (block per feature, all
//   streams) -> stacked update (block per stream) -> [camera pruning] triangulate -> blocks -> update ->
//   row/column removal -> position variances for the online reset.
// The host only moves CSR index lists down and gate flags / delta_x / 3 variances per stream up.
#include <stdarg.h>
#include <stdlib.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <deque>
#include <list>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>

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
struct BCam { long long id; double t, q[4], p[3], qn[4]; };     // position_null aliases position (msckf.py:403-404)

// map_server (msckf.py:120, a dict id -> Feature whose observations are a dict camera id -> measurement), stored FRAME-MAJOR:
// one array set per camera state of the window holding that frame's message as it arrived (ids, measurements) plus, per
// entry, links to the same feature's entry in the previous / next frame it was seen in, and the feature's slot in a small
// per-stream table (birth number = insertion order of the dict, position, initialised flag, observation count, newest entry).
// Appending a frame is a sequential copy plus one probe per feature into a hash of ONLY the previous message (12 KB, cache
// resident) -- not 300 read-modify-writes of per-feature observation vectors scattered over 600 MB of tables; a feature's
// observations are gathered by walking its links (only for the ~40 lost / ~300 pruning candidates of a frame); removing a
// camera state removes its frame (the links of its neighbours are joined).  This is also the layout a device-resident table
// needs (DESIGN.md section 7).
struct FMeta {
    long long id = 0, birth = 0;
    double pos[3] = {0, 0, 0};
    bool init = false, alive = false;
    int nobs = 0;
    int tail = -1;                 // link to the newest entry of the feature
};
struct FeatStore {
    static constexpr int NSLOT = 32;                    // frames (= camera states) held at once; links pack (slot << 24 | index)
    struct Frame { long long cam = -1; int n = 0; std::vector<long long> id; std::vector<double> z; std::vector<int> fslot, prev, next; };
    Frame fr[NSLOT];
    std::vector<int> order;                             // frame slots in camera-state order (parallel to BStream::cams)
    int pos_of[NSLOT];                                  // frame slot -> index in `order` (camera index), -1 = free
    std::vector<FMeta> meta; std::vector<int> free_meta;
    std::vector<long long> hkey; std::vector<int> hval;  // id -> entry index of the NEWEST frame (-1 = empty)
    int live = 0;
    long long births = 0;
    FeatStore() { for (int i = 0; i < NSLOT; ++i) pos_of[i] = -1; }
    static int link(int slot, int idx) { return (slot << 24) | idx; }
    static int lslot(int l) { return l >> 24; }
    static int lidx(int l) { return l & 0xFFFFFF; }
    static size_t mix(long long id) { unsigned long long x = (unsigned long long)id * 0x9E3779B97F4A7C15ull; return (size_t)(x ^ (x >> 29)); }
    int hfind(long long id) const
    {
        if (hkey.empty()) return -1;
        const size_t m = hkey.size() - 1;
        for (size_t h = mix(id) & m;; h = (h + 1) & m) {
            if (hval[h] < 0) return -1;
            if (hkey[h] == id) return hval[h];
        }
    }
    void hput(std::vector<long long>& k, std::vector<int>& v, long long id, int idx) const
    {
        const size_t m = k.size() - 1;
        size_t h = mix(id) & m;
        while (v[h] >= 0) h = (h + 1) & m;
        k[h] = id; v[h] = idx;
    }
    int newest() const { return order.empty() ? -1 : order.back(); }
    // add_feature_observations for one message (msckf.py:425-441); returns the number of tracked features
    int add_frame(long long cam_id, const long long* ids, const double* uv, int nk)
    {
        int slot = -1;
        for (int i = 0; i < NSLOT; ++i) if (pos_of[i] < 0) { slot = i; break; }
        if (slot < 0) return -1;
        const int pslot = newest();
        Frame& F = fr[slot];
        F.cam = cam_id; F.n = 0;
        F.id.resize(nk); F.z.resize((size_t)4 * nk); F.fslot.resize(nk); F.prev.resize(nk); F.next.resize(nk);
        // hash of THIS message, built while it is added (a duplicate id inside one message re-assigns the same dict key)
        size_t cells = 64;
        while (cells < (size_t)nk * 2 + 16) cells *= 2;
        std::vector<long long>& nk_key = hkey2; std::vector<int>& nk_val = hval2;
        nk_key.assign(cells, 0); nk_val.assign(cells, -1);
        Frame* P = pslot >= 0 ? &fr[pslot] : nullptr;
        int tracked = 0;
        for (int k = 0; k < nk; ++k) {
            const long long id = ids[k];
            {   // duplicate inside this message?
                const size_t m = cells - 1;
                size_t h = mix(id) & m;
                int dup = -1;
                for (;; h = (h + 1) & m) { if (nk_val[h] < 0) break; if (nk_key[h] == id) { dup = nk_val[h]; break; } }
                if (dup >= 0) { for (int e = 0; e < 4; ++e) F.z[(size_t)4 * dup + e] = uv[(size_t)4 * k + e]; ++tracked; continue; }
                nk_key[h] = id; nk_val[h] = F.n;
            }
            const int i = F.n++;
            F.id[i] = id;
            for (int e = 0; e < 4; ++e) F.z[(size_t)4 * i + e] = uv[(size_t)4 * k + e];
            F.next[i] = -1;
            const int pi = P ? hfind(id) : -1;
            if (pi >= 0 && P->fslot[pi] >= 0) {
                const int fs = P->fslot[pi];
                F.fslot[i] = fs; F.prev[i] = link(pslot, pi); P->next[pi] = link(slot, i);
                FMeta& m = meta[fs]; ++m.nobs; m.tail = link(slot, i);
                ++tracked;
            } else {
                int fs;
                if (!free_meta.empty()) { fs = free_meta.back(); free_meta.pop_back(); } else { fs = (int)meta.size(); meta.emplace_back(); }
                FMeta& m = meta[fs];
                m = FMeta(); m.id = id; m.birth = births++; m.alive = true; m.nobs = 1; m.tail = link(slot, i);
                F.fslot[i] = fs; F.prev[i] = -1;
                ++live;
            }
        }
        hkey.swap(nk_key); hval.swap(nk_val);
        pos_of[slot] = (int)order.size();
        order.push_back(slot);
        return tracked;
    }
    // observations of a feature in ascending camera order: camera index (position in `order`) and measurement pointer
    int collect(const FMeta& m, int* cam_idx, const double** z, int cap) const
    {
        int n = 0;
        for (int l = m.tail; l >= 0 && n < cap; ) {
            const Frame& F = fr[lslot(l)];
            const int i = lidx(l);
            cam_idx[n] = pos_of[lslot(l)]; z[n] = &F.z[(size_t)4 * i]; ++n;
            l = F.prev[i];
        }
        for (int a = 0, b = n - 1; a < b; ++a, --b) { std::swap(cam_idx[a], cam_idx[b]); std::swap(z[a], z[b]); }
        return n;
    }
    // delete a feature: its entries stay in their frames as dead entries until the frames go
    void erase(int fs)
    {
        FMeta& m = meta[fs];
        for (int l = m.tail; l >= 0; ) { Frame& F = fr[lslot(l)]; const int i = lidx(l); F.fslot[i] = -1; l = F.prev[i]; }
        m.alive = false; m.tail = -1;
        free_meta.push_back(fs); --live;
    }
    // remove the frame of camera index `ci` (its camera state leaves the window): neighbours are linked past it
    void remove_frame(int ci)
    {
        const int slot = order[ci];
        Frame& F = fr[slot];
        for (int i = 0; i < F.n; ++i) {
            const int fs = F.fslot[i];
            if (fs < 0) continue;
            const int pl = F.prev[i], nl = F.next[i];
            if (pl >= 0) fr[lslot(pl)].next[lidx(pl)] = nl;
            if (nl >= 0) fr[lslot(nl)].prev[lidx(nl)] = pl;
            FMeta& m = meta[fs];
            --m.nobs;
            if (nl < 0) m.tail = pl;                    // (the newest frame is never removed while its features live; kept for safety)
        }
        F.n = 0; F.cam = -1;
        pos_of[slot] = -1;
        order.erase(order.begin() + ci);
        for (size_t k = ci; k < order.size(); ++k) pos_of[order[k]] = (int)k;
    }
    void clear()
    {
        for (int i = 0; i < NSLOT; ++i) { fr[i].n = 0; fr[i].cam = -1; pos_of[i] = -1; }
        order.clear(); meta.clear(); free_meta.clear(); hkey.clear(); hval.clear(); live = 0;
    }
    std::vector<long long> hkey2; std::vector<int> hval2;     // scratch of add_frame
};

struct BStream {
    std::deque<BImu> imu; std::mutex mu;
    bool gravity_set = false, first_img = true, null_aliased = false, active = false;
    double gravity_time = 0;                    // timestamp of the IMU sample that completed initialize_gravity_and_bias
    long long next_imu_id = 0, imu_id = 0;
    double ts = 0, q[4] = {0, 0, 0, 1}, p[3] = {0, 0, 0}, v[3] = {0, 0, 0}, bg[3] = {0, 0, 0}, ba[3] = {0, 0, 0};
    double R_ic[9], t_ci[3], qn[4] = {0, 0, 0, 1}, pn[3] = {0, 0, 0}, vn[3] = {0, 0, 0}, gravity[3];
    std::vector<BCam> cams;
    FeatStore map;
    double tracking_rate = 0;
    int n = IMU_DIM;
    bool has_imu_id = false;
    bool dev_init_sent = false;                 // device-resident path: the gravity / bias initialisation has been handed to the device
    // A failure that concerns this stream alone (its window or its block list outgrew a fixed capacity) stops THIS stream: it
    // idles from then on (out[s*12] = -1, av_msckf_batch_stream_status tells why) while the other streams of the batch keep
    // running -- the reference's sequences never stop one another.
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
    double chi2[100];
    std::vector<BStream> st;
    size_t pstride = 0, hstride = 0, rstride = 0, wstride = 0;
    double *P = nullptr, *Pn = nullptr, *T = nullptr, *Kt = nullptr, *W = nullptr, *Hblk = nullptr, *rblk = nullptr, *dx = nullptr, *scratch = nullptr, *chi2_dev = nullptr, *pvar = nullptr;
    // Owns every device and pinned block, event and stream of this batch or group, the DevPath's and the DevBufs' included (declared
    // ahead of them: they register with it).  Outgrown blocks stay with it until destroy: nothing frees inside a run.
    AvResources res;
    DevBuf<PropArgs> d_prop{res}; DevBuf<int> d_first{res}; DevBuf<AugArgs> d_aug{res}; DevBuf<RemArgs> d_rem{res}; DevBuf<UpdArgs> d_upd{res};
    DevBuf<int> d_clist{res}, d_flist{res}, d_obs_off{res}, d_obs_cam{res}, d_fstream{res}, d_dof{res}, d_rowoff{res}, d_pass{res}, d_valid{res}, d_blk_row{res},
                d_blk_len{res}, d_ncam{res}, d_cols{res};
    DevBuf<double> d_obs_z{res}, d_pos{res}, d_gamma{res}, d_cam_q{res}, d_cam_p{res}, d_cam_qn{res}, d_grav{res};
    // triangulation launch (own buffers: its results stay on the device for the feature kernels queued right behind it)
    DevBuf<int> d_tobs_off{res}, d_tobs_cam{res}, d_tfs{res}, d_tvalid{res}, d_tri_idx{res}, d_rbeg{res}, d_stacked{res};
    DevBuf<double> d_tobs_z{res}, d_tpos{res};
    DevBuf<UpdArgs> d_updbase{res};
    double *h_dx = nullptr, *h_pv = nullptr;    // pinned landing zones of the per-step read-backs
    int reserved_cap = 0;                       // message capacity (features per stream) the buffers below are sized for
    // counters of av_msckf_batch_counters (sub-batch; the parent sums its groups)
    long long n_steps = 0, n_prune_stream_steps = 0, n_update_stream_steps = 0, n_two_pass_streams = 0;
    // work counters of av_msckf_batch_work: algorithmic fp64 flops (SURVEY 8d) of the gates and updates this group ran, and the
    // time its phase chains spent on the device (HIP events on the group's stream around the launches of a phase)
    double w_gate_flops = 0, w_update_flops = 0, w_qr_flops = 0, w_chain_ms = 0; long long w_gated = 0, w_rows = 0, w_updates = 0, w_chain_dropped = 0;
    hipEvent_t ev_t0[2] = {nullptr, nullptr}, ev_t1[2] = {nullptr, nullptr}; bool ev_used[2] = {false, false};
    bool work_timing = false;
    bool debug_capture = false;
    bool pool_on = false;                       // device-resident path: the block buffers end in a row pool shared by all streams (b_pool_rows)
    bool rows_cap_auto = false;                 // rows_cap was sized from a message capacity (create passed 0): it may grow with a wider message
    hipStream_t aux[4] = {nullptr, nullptr, nullptr, nullptr};      // the track-length buckets of feature_kernel run concurrently
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_wait = nullptr;                // blocking-sync event: a waiting worker sleeps instead of spinning on a core
    // ---- stream groups -----------------------------------------------------------------------------------
    // A batch of many streams is split into G independent sub-batches (disjoint stream ranges, own device buffers,
    // own HIP stream, own worker thread with a share of the host cores).  One step runs all groups concurrently:
    // the bookkeeping of one group overlaps the kernels of the others, which a single lock-step chain
    // (host phase -> launch -> wait for gate flags -> host phase ...) cannot do.  Streams never interact, so
    // the results are those of the ungrouped batch.
    std::vector<av_msckf_batch*> subs;          // non-empty on the parent only
    int per_sub = 0;                            // streams per group (the last one may hold fewer)
    hipStream_t own = nullptr;                  // sub: its stream
    int host_cap = 0;                           // sub: OpenMP threads of its worker
    std::thread worker; std::mutex wmu; std::condition_variable wcv;
    struct Job { std::function<int()> launch, finish; };
    std::deque<Job> jobs; long long n_submitted = 0, n_done = 0; bool quit = false; int job_rc = 0; char job_err[512] = "";
    DevPath* dev = nullptr;                     // device-resident state + observation store (msckf_dev.inc); NULL: the host-bookkeeping path (AV_MSCKF_STORE=host)
    long long dev_seq = 0;                      // steps submitted (ring slot = dev_seq % DEV_RING)
    hipEvent_t ev_msg[4] = {nullptr, nullptr, nullptr, nullptr};      // submit_dev: the message copy of ring slot k has been enqueued
    struct Pending { int slot; double* out; StepOuts outs; };
    std::deque<Pending> direct_pending;         // one group, no worker: steps launched and not yet finished (slot, caller's out, caller's arrays for the optional outputs)
    // the optional outputs (OUTS, msckf_dev.inc).  out_set: every feature's setting (av_msckf_batch_set_*), on the batch and on every
    // group; next_outs: the destinations av_msckf_batch_next_* handed over for the next step (batch only), taken by that step
    int out_set[N_FEAT] = {}; StepOuts next_outs;
    explicit av_msckf_batch(int n) : st(n) {}
};

namespace {

// the optional outputs' destinations handed over for the next step: taken, and cleared, by the step that is being submitted
inline StepOuts take_outs(av_msckf_batch* b) { const StepOuts o = b->next_outs; b->next_outs = StepOuts(); return o; }

// ---- the kernels' argument records, the part every caller of a batch shares (the device-resident filter, the host-bookkeeping chain
//      and its synchronous fallback); each caller adds what is its own.  TriArgs: tri_args_base (msckf.hip).

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

// A zeroed UpdArgs with the work buffers of stream s and their strides.  The caller adds n, m, nc, mode, its block lists and prof.
inline UpdArgs b_upd_args(const av_msckf_batch* b, int s)
{
    UpdArgs u; memset(&u, 0, sizeof(u));
    u.P = b->P + (size_t)s * b->pstride; u.ld = b->ld;
    u.Hsrc = b->Hblk + (size_t)s * b->hstride; u.rsrc = b->rblk + (size_t)s * b->rstride;
    u.W = b->W + (size_t)s * b->wstride; u.ldt = b->rows_cap; u.T = b->T + (size_t)s * b->pstride; u.Kt = b->Kt + (size_t)s * b->pstride;
    u.Pn = b->Pn + (size_t)s * b->pstride; u.dx = b->dx + (size_t)s * b->ld; u.obs_noise = b->obs_noise;
    u.Sbuf = b->scratch + (size_t)s * b->pstride;          // free between the camera removals that use it
    return u;
}

// A feature selected for a batched kernel: its observations are a slice [first, first+n) of the pools
// (no per-feature heap allocation; the prune path builds ~300 of these per stream and frame).
struct ObsPool { std::vector<int> cam; std::vector<const double*> z; };

// streams are independent on the host too: per-stream loops run on all cores (OpenMP), each writing only
// its own PerStream scratch; the pieces are concatenated afterwards in stream order (deterministic).
// Team size: a GPU box gives one process a share of ~16 cores however many the node reports.
inline int host_thread_budget()
{
    static const int cap = [] { const char* e = getenv("AV_HOST_THREADS"); int v = e ? atoi(e) : 16; return v < 1 ? 1 : (v > 64 ? 64 : v); }();
    return cap;
}
thread_local int tl_host_cap = 0;        // set by a stream group's worker thread: its share of the budget
inline int host_threads(int work)
{
    const int cap = tl_host_cap > 0 ? tl_host_cap : host_thread_budget();
    return work < cap ? (work < 1 ? 1 : work) : cap;
}
template <typename F>
inline void par_streams(int S, F&& fn)
{
    const int nt = host_threads(S / 4);
    if (nt <= 1) { for (int s = 0; s < S; ++s) fn(s); return; }
#pragma omp parallel for schedule(dynamic, 4) num_threads(nt)
    for (int s = 0; s < S; ++s) fn(s);
}
struct FeatRef {
    int s; FMeta* f; int fs = -1; int dof; int n = 0; int first = 0;      // fs: the feature's slot in its stream's FeatStore::meta
    void add(ObsPool& p, int ci, const double* zz) { if (n == 0) first = (int)p.cam.size(); p.cam.push_back(ci); p.z.push_back(zz); ++n; }
};

void b_fail_stream(av_msckf_batch* b, int s, int rc, const char* fmt, ...)
{
    BStream& T = b->st[s];
    if (T.failed) return;
    T.failed = rc; T.active = false;
    va_list ap; va_start(ap, fmt); vsnprintf(T.fail_msg, sizeof(T.fail_msg), fmt, ap); va_end(ap);
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

void b_predict_new_state(BStream& S, double dt, const double* gyro, const double* acc)
{   // msckf.py:341-388
    double gn = h_norm3(gyro);
    double Om[16] = {0, gyro[2], -gyro[1], gyro[0], -gyro[2], 0, gyro[0], gyro[1], gyro[1], -gyro[0], 0, gyro[2], -gyro[0], -gyro[1], -gyro[2], 0};
    auto apply = [&](double c, double s_over, double lin, double* out) {
        // out = (c * I + s_over * Om) q   or   c * (I + Om * lin) q
        for (int i = 0; i < 4; ++i) {
            double acc_ = 0;
            for (int j = 0; j < 4; ++j) {
                double m = (gn > 1e-5) ? ((i == j ? c : 0.0) + s_over * Om[i * 4 + j]) : (c * ((i == j ? 1.0 : 0.0) + Om[i * 4 + j] * lin));
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
    const double* k3v = k2v;                       // k2 and k3 share the half-step rotation (A.13)
    double vnew[3], pnew[3];
    for (int i = 0; i < 3; ++i) {
        double k1p = S.v[i], k2p = S.v[i] + k1v[i] * dt / 2., k3p = S.v[i] + k2v[i] * dt / 2, k4p = S.v[i] + k3v[i] * dt;
        vnew[i] = S.v[i] + (k1v[i] + 2 * k2v[i] + 2 * k3v[i] + k4v[i]) * dt / 6.;
        pnew[i] = S.p[i] + (k1p + 2 * k2p + 2 * k3p + k4p) * dt / 6.;
    }
    double nq = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int i = 0; i < 4; ++i) S.q[i] = dq[i] / nq;
    for (int i = 0; i < 3; ++i) { S.v[i] = vnew[i]; S.p[i] = pnew[i]; }
}

void b_inject(BStream& S, const double* dx)
{   // state injection of measurement_update (msckf.py:576-595) with the reference's in-place aliasing
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
    for (size_t k = 0; k < S.cams.size(); ++k) {
        const double* d = dx + 21 + 6 * k;
        double cq[4], co[4];
        h_small_angle(d, cq); h_quat_mul(cq, S.cams[k].q, co);
        for (int i = 0; i < 4; ++i) S.cams[k].q[i] = co[i];
        for (int i = 0; i < 3; ++i) S.cams[k].p[i] += d[3 + i];
    }
}

// camera states are kept in ascending id order (ids only grow, erase keeps the order): binary search
int b_cam_index(const BStream& S, long long id)
{
    int lo = 0, hi = (int)S.cams.size() - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const long long v = S.cams[mid].id;
        if (v == id) return mid;
        if (v < id) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// upload camera arrays of all streams (slot-major) + per-stream gravity / counts
int b_upload_cams(av_msckf_batch* b, hipStream_t stm)
{
    const int S = b->S, cs = b->cam_slots;
    std::vector<double> q((size_t)S * cs * 4, 0.0), p((size_t)S * cs * 3, 0.0), qn((size_t)S * cs * 4, 0.0), g((size_t)S * 3);
    std::vector<int> nc(S);
    for (int s = 0; s < S; ++s) {
        const BStream& T = b->st[s];
        nc[s] = (int)T.cams.size();
        for (size_t k = 0; k < T.cams.size(); ++k) {
            for (int i = 0; i < 4; ++i) { q[((size_t)s * cs + k) * 4 + i] = T.cams[k].q[i]; qn[((size_t)s * cs + k) * 4 + i] = T.cams[k].qn[i]; }
            for (int i = 0; i < 3; ++i) p[((size_t)s * cs + k) * 3 + i] = T.cams[k].p[i];
        }
        for (int i = 0; i < 3; ++i) g[(size_t)s * 3 + i] = T.gravity[i];
    }
    int rc;
    if ((rc = b->d_cam_q.upload(q, stm)) || (rc = b->d_cam_p.upload(p, stm)) || (rc = b->d_cam_qn.upload(qn, stm)) ||
        (rc = b->d_grav.upload(g, stm)) || (rc = b->d_ncam.upload(nc, stm))) return rc;
    return AV_OK;
}

// Triangulation of every not-yet-initialised feature of `refs` (batched), in two halves so that the results can stay on
// the device for the kernels queued behind the launch: b_tri_launch builds the observation CSR and enqueues the kernel
// (todo[k] = index into refs of the k-th triangulated feature; ok[i] = 0 for a feature that fails check_motion),
// b_tri_collect copies positions / validity (read back into the pinned stages of d_tpos / d_tvalid) into the features.
int b_tri_launch(av_msckf_batch* b, std::vector<FeatRef>& refs, std::vector<char>& ok, std::vector<int>& todo, hipStream_t stm)
{
    ok.assign(refs.size(), 1);
    todo.clear();
    std::vector<char> need(refs.size(), 0);
    {
        const int nr = (int)refs.size();
#pragma omp parallel for schedule(static) num_threads(host_threads(nr / 2048))
        for (int i = 0; i < nr; ++i) need[i] = refs[i].f->init ? 0 : 1;          // pointer chasing: worth spreading over cores
    }
    for (size_t i = 0; i < refs.size(); ++i) {
        if (!need[i]) continue;
        // check_motion is always true at translation_threshold < 0 (config.py:12); the general test is evaluated on demand
        if (b->trans_thr >= 0) {
            const BStream& T = b->st[refs[i].s];
            int oc[FeatStore::NSLOT]; const double* oz[FeatStore::NSLOT];
            const int no = T.map.collect(*refs[i].f, oc, oz, FeatStore::NSLOT);
            const int ia = oc[0], ib = oc[no - 1];
            double Ra[9], d[3] = {oz[0][0], oz[0][1], 1.0}, dw[3];
            double nd = h_norm3(d); d[0] /= nd; d[1] /= nd; d[2] /= nd;
            h_to_rotation(T.cams[ia].q, Ra); h_mtv(Ra, d, dw);
            double t[3] = {T.cams[ib].p[0] - T.cams[ia].p[0], T.cams[ib].p[1] - T.cams[ia].p[1], T.cams[ib].p[2] - T.cams[ia].p[2]};
            double par = t[0] * dw[0] + t[1] * dw[1] + t[2] * dw[2];
            double o[3] = {t[0] - par * dw[0], t[1] - par * dw[1], t[2] - par * dw[2]};
            if (!(h_norm3(o) > b->trans_thr)) { ok[i] = 0; continue; }
        }
        todo.push_back((int)i);
    }
    if (todo.empty()) return AV_OK;
    // CSR of the observations that still have a camera state: count, prefix, fill (pinned staging, all cores)
    const int nf = (int)todo.size();
    std::vector<int> off(nf + 1, 0), fs(nf);
#pragma omp parallel for schedule(static) num_threads(host_threads(nf / 1024))
    for (int k = 0; k < nf; ++k) {
        const FeatRef& r = refs[todo[k]];
        const BStream& T = b->st[r.s];
        (void)T;
        off[k + 1] = r.f->nobs; fs[k] = r.s;                 // every frame of the window has its camera state
    }
    int maxobs = 0;
    for (int k = 0; k < nf; ++k) { if (off[k + 1] > maxobs) maxobs = off[k + 1]; off[k + 1] += off[k]; }
    if (2 * maxobs > 64) { av_set_error("batched triangulation: %d observations exceed one wavefront", maxobs); return AV_E_CAPACITY; }
    int rc;
    int* cam = nullptr; double* z = nullptr;
    if ((rc = b->d_tobs_cam.stage_for((size_t)off[nf], stm, &cam)) || (rc = b->d_tobs_z.stage_for((size_t)off[nf] * 4, stm, &z))) return rc;
#pragma omp parallel for schedule(static) num_threads(host_threads(nf / 1024))
    for (int k = 0; k < nf; ++k) {
        const FeatRef& r = refs[todo[k]];
        const BStream& T = b->st[r.s];
        int oc[FeatStore::NSLOT]; const double* oz[FeatStore::NSLOT];
        const int no = T.map.collect(*r.f, oc, oz, FeatStore::NSLOT);
        for (int q = 0, w = off[k]; q < no; ++q, ++w) {
            cam[w] = oc[q];
            for (int e = 0; e < 4; ++e) z[(size_t)w * 4 + e] = oz[q][e];
        }
    }
    if ((rc = b->d_tobs_off.upload(off, stm)) || (rc = b->d_tobs_cam.commit((size_t)off[nf], stm)) || (rc = b->d_tobs_z.commit((size_t)off[nf] * 4, stm)) ||
        (rc = b->d_tfs.upload(fs, stm)) || (rc = b->d_tpos.reserve((size_t)nf * 3, true)) || (rc = b->d_tvalid.reserve(nf, true))) return rc;
    TriArgs a = tri_args_base(b->d_cam_q.p, b->d_cam_p.p, b->cam_slots, b->T01, b->opt5);
    a.n_feat = nf; a.obs_off = b->d_tobs_off.p; a.obs_cam = b->d_tobs_cam.p; a.obs_z = b->d_tobs_z.p;
    a.feat_stream = b->d_tfs.p;
    a.out_pos = b->d_tpos.p; a.out_valid = b->d_tvalid.p;
    hipLaunchKernelGGL(triangulate_kernel, dim3((nf + 3) / 4), dim3(256), 0, stm, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
int b_tri_readback(av_msckf_batch* b, int nf, hipStream_t stm)
{
    if (nf <= 0) return AV_OK;
    AV_HIP(hipMemcpyAsync(b->d_tpos.stage, b->d_tpos.p, sizeof(double) * 3 * nf, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(b->d_tvalid.stage, b->d_tvalid.p, sizeof(int) * nf, hipMemcpyDeviceToHost, stm));
    return AV_OK;
}
void b_tri_collect(av_msckf_batch* b, std::vector<FeatRef>& refs, const std::vector<int>& todo, std::vector<char>& ok)
{
    const int nf = (int)todo.size();
    const double* pos = b->d_tpos.stage; const int* valid = b->d_tvalid.stage;
#pragma omp parallel for schedule(static) num_threads(host_threads(nf / 1024))
    for (int k = 0; k < nf; ++k) {
        FMeta* f = refs[todo[k]].f;
        for (int i = 0; i < 3; ++i) f->pos[i] = pos[(size_t)k * 3 + i];
        f->init = valid[k] != 0;
        ok[todo[k]] = valid[k] != 0;
    }
}
// synchronous form (the fallback path of b_process below)
int b_initialize(av_msckf_batch* b, std::vector<FeatRef>& refs, std::vector<char>& ok, hipStream_t stm)
{
    std::vector<int> todo;
    int rc;
    if ((rc = b_tri_launch(b, refs, ok, todo, stm))) return rc;
    if (todo.empty()) return AV_OK;
    if ((rc = b_tri_readback(b, (int)todo.size(), stm))) return rc;
    if ((rc = b_wait(b, stm))) return rc;
    b_tri_collect(b, refs, todo, ok);
    return AV_OK;
}

// feature_kernel launches in buckets of track length: the LDS footprint grows with M^2 (150 KB at M = 21, 8 KB at M = 4), so
// short tracks must not inherit the occupancy of the longest one.  sel: feature indices in launch order.
int b_launch_buckets(av_msckf_batch* b, FeatArgs a, const std::vector<FeatRef>& refs, const std::vector<int>& sel, int maxobs, hipStream_t stm)
{
    const int edges[5] = {4, 8, 12, 16, 1 << 30};
    // counting sort of the features by bucket (stable: launch order inside a bucket = feature order)
    auto bucket_of = [&](int n) { return n <= edges[0] ? 0 : (n <= edges[1] ? 1 : (n <= edges[2] ? 2 : (n <= edges[3] ? 3 : 4))); };
    const int ns = (int)sel.size();
    std::vector<int> order(ns);
    std::vector<int> bstart(6, 0);
    for (int i = 0; i < ns; ++i) ++bstart[bucket_of(refs[sel[i]].n) + 1];
    for (int bk = 0; bk < 5; ++bk) bstart[bk + 1] += bstart[bk];
    {
        int fill[5] = {bstart[0], bstart[1], bstart[2], bstart[3], bstart[4]};
        for (int i = 0; i < ns; ++i) order[fill[bucket_of(refs[sel[i]].n)]++] = sel[i];
    }
    int rc2;
    if ((rc2 = b->d_flist.upload(order, stm))) return rc2;
    // fork: bucket 0 stays on the caller's stream, buckets 1..4 run on auxiliary streams behind an event
    AV_HIP(hipEventRecord(b->ev_fork, stm));
    bool used_aux[4] = {false, false, false, false};
    for (int bk = 0; bk < 5; ++bk) {
        const int cnt = bstart[bk + 1] - bstart[bk];
        if (cnt == 0) continue;
        hipStream_t ls = stm;
        if (bk > 0) { ls = b->aux[bk - 1]; used_aux[bk - 1] = true; AV_HIP(hipStreamWaitEvent(ls, b->ev_fork, 0)); }
        const int Mx = edges[bk] < maxobs ? edges[bk] : maxobs;
        a.feat_list = b->d_flist.p + bstart[bk];
        if ((rc2 = launch_feature_kernel(a, cnt, Mx, ls))) return rc2;
    }
    for (int i = 0; i < 4; ++i) if (used_aux[i]) { AV_HIP(hipEventRecord(b->ev_join[i], b->aux[i])); AV_HIP(hipStreamWaitEvent(stm, b->ev_join[i], 0)); }
    return AV_OK;
}

// Jacobian + null space + gate for `refs` (cam_idx / z / dof filled), then the stacked update per stream.
// cut1500: apply the `> 1500 rows` break of remove_lost_features (msckf.py:667-668).
int b_blocks_and_update(av_msckf_batch* b, std::vector<FeatRef>& refs, const ObsPool& pool, bool cut1500, hipStream_t stm)
{
    const int S = b->S;
    if (refs.empty()) return AV_OK;
    const int nf = (int)refs.size();
    std::vector<int> off(nf + 1, 0), fs(nf), dof(nf), rowoff(nf), rows(nf);
    std::vector<int> stream_rows(S, 0);
    int maxobs = 0;
    for (int i = 0; i < nf; ++i) {                      // cheap sequential pass: offsets
        const FeatRef& r = refs[i];
        off[i + 1] = off[i] + r.n;
        fs[i] = r.s; dof[i] = r.dof; rows[i] = 4 * r.n - 3;
        rowoff[i] = stream_rows[r.s]; stream_rows[r.s] += rows[i];
        if (r.n > maxobs) maxobs = r.n;
    }
    // A stream whose candidates would reserve more rows than the block buffer holds (a blank or blurred frame drops every
    // track at once: ~cap features x up to 4*21-3 rows) is gated FIRST and written SECOND: its features run with row
    // offset -1 (gate only, nothing stored), the stacking decision below keeps the gated ones up to the reference's
    // `> 1500 rows` cut (msckf.py:667-668), and only those are run again with compact offsets.  The reference itself never
    // evaluates a feature behind the cut, so the result is the same; rows_cap >= 1500 + one block always suffices.
    std::vector<char> over(S, 0);
    bool any_over = false;
    for (int s = 0; s < S; ++s) if (stream_rows[s] > b->rows_cap) { over[s] = 1; any_over = true; ++b->n_two_pass_streams; }
    if (any_over) for (int i = 0; i < nf; ++i) if (over[refs[i].s]) rowoff[i] = -1;
    int rc;
    // observation CSR, written straight into the pinned staging buffers by all cores
    int* cam = nullptr; double* z = nullptr; double* pos = nullptr;
    if ((rc = b->d_obs_cam.stage_for((size_t)off[nf], stm, &cam)) || (rc = b->d_obs_z.stage_for((size_t)off[nf] * 4, stm, &z)) ||
        (rc = b->d_pos.stage_for((size_t)nf * 3, stm, &pos))) return rc;
#pragma omp parallel for schedule(static) num_threads(host_threads(nf / 512))
    for (int i = 0; i < nf; ++i) {
        const FeatRef& r = refs[i];
        for (int k = 0; k < r.n; ++k) {
            cam[off[i] + k] = pool.cam[r.first + k];
            const double* zz = pool.z[r.first + k];
            for (int e = 0; e < 4; ++e) z[(size_t)(off[i] + k) * 4 + e] = zz[e];
        }
        for (int e = 0; e < 3; ++e) pos[(size_t)i * 3 + e] = r.f->pos[e];
    }
    if ((rc = b->d_obs_off.upload(off, stm)) || (rc = b->d_obs_cam.commit((size_t)off[nf], stm)) || (rc = b->d_obs_z.commit((size_t)off[nf] * 4, stm)) ||
        (rc = b->d_fstream.upload(fs, stm)) || (rc = b->d_dof.upload(dof, stm)) || (rc = b->d_rowoff.upload(rowoff, stm)) ||
        (rc = b->d_pos.commit((size_t)nf * 3, stm)) || (rc = b->d_gamma.ensure(nf)) || (rc = b->d_pass.ensure(nf))) return rc;
    FeatArgs a = b_feat_args(b, cut1500, b->d_cam_q.p, b->d_cam_p.p, b->d_cam_qn.p);
    a.n_feat = nf; a.Mmax = maxobs; a.feat_stream = b->d_fstream.p; a.stream_ncam = b->d_ncam.p; a.stream_gravity = b->d_grav.p;
    a.obs_off = b->d_obs_off.p; a.obs_cam = b->d_obs_cam.p; a.obs_z = b->d_obs_z.p; a.pos = b->d_pos.p; a.dof = b->d_dof.p; a.row_off = b->d_rowoff.p;
    a.gamma = b->d_gamma.p; a.pass = b->d_pass.p;
    auto launch_buckets = [&](const std::vector<int>& sel) -> int { return b_launch_buckets(b, a, refs, sel, maxobs, stm); };
    {
        std::vector<int> all(nf);
        for (int i = 0; i < nf; ++i) all[i] = i;
        if ((rc = launch_buckets(all))) return rc;
    }
    std::vector<int> pass(nf);
    AV_HIP(hipMemcpyAsync(pass.data(), b->d_pass.p, sizeof(int) * nf, hipMemcpyDeviceToHost, stm));
    { int rcw = b_wait(b, stm); if (rcw) return rcw; }
    // stacking decisions per stream, in feature order (refs are stream-major, map order inside a stream):
    // every stream scans only its own contiguous range of refs, streams in parallel
    std::vector<int> rbeg(S + 1, 0);
    for (int i = 0; i < nf; ++i) rbeg[refs[i].s + 1] = i + 1;
    for (int s = 0; s < S; ++s) if (rbeg[s + 1] < rbeg[s]) rbeg[s + 1] = rbeg[s];
    std::vector<std::vector<int>> br(S), bl(S);
    std::vector<int> stacked(S, 0);
    std::vector<std::vector<char>> used(S);
    std::vector<std::vector<int>> again(S);                 // two-pass streams: the features to run again, now with storage
    par_streams(S, [&](int s) {
        used[s].assign(b->st[s].cams.size(), 0);
        for (int i = rbeg[s]; i < rbeg[s + 1]; ++i) {
            if (pass[i]) {
                if (over[s]) {
                    if (stacked[s] + rows[i] > b->rows_cap) break;      // cannot happen with rows_cap >= max(1500 + 81, 5 * cap) (checked at create / reserve)
                    rowoff[i] = stacked[s]; again[s].push_back(i);
                }
                br[s].push_back(rowoff[i]); bl[s].push_back(rows[i]); stacked[s] += rows[i];
                for (int q = 0; q < refs[i].n; ++q) used[s][pool.cam[refs[i].first + q]] = 1;
            }
            if (cut1500 && stacked[s] > 1500) break;
        }
    });
    if (any_over) {
        std::vector<int> sel;
        for (int s = 0; s < S; ++s) sel.insert(sel.end(), again[s].begin(), again[s].end());
        if (!sel.empty()) {
            if ((rc = b->d_rowoff.upload(rowoff, stm))) return rc;        // the first pass has retired (its flags are here)
            if ((rc = launch_buckets(sel))) return rc;
        }
    }
    std::vector<int> all_r, all_l, all_cols;
    std::vector<size_t> col_off(S, 0);
    std::vector<UpdArgs> ua(S);
    int nmax = 0, ncinfo = 0, ninfo = 0, minfo = 0; bool any = false, any_info = false, any_qr = false;
    for (int s = 0; s < S; ++s) {
        UpdArgs& u = ua[s];
        memset(&u, 0, sizeof(u));                           // a stream without an update: m = 0, nothing else is read
        if (stacked[s] == 0) continue;
        any = true;
        const BStream& T = b->st[s];
        const int n_blk = (int)br[s].size();
        if (n_blk > 4 * UT) { b_fail_stream(b, s, AV_E_CAPACITY, "stream stacks %d blocks > %d in one update", n_blk, 4 * UT); stacked[s] = 0; continue; }
        u = b_upd_args(b, s);
        u.m = stacked[s]; u.n = T.n; u.n_blk = n_blk;
        u.blk_row = reinterpret_cast<const int*>((size_t)all_r.size());       // patched to device addresses below
        all_r.insert(all_r.end(), br[s].begin(), br[s].end()); all_l.insert(all_l.end(), bl[s].begin(), bl[s].end());
        col_off[s] = all_cols.size();
        for (size_t ci = 0; ci < used[s].size(); ++ci) if (used[s][ci]) for (int e = 0; e < 6; ++e) all_cols.push_back(IMU_DIM + 6 * (int)ci + e);
        u.nc = (int)(all_cols.size() - col_off[s]);
        u.mode = upd_info_form(u.m, u.nc) ? 1 : 0;
        if (u.mode) { any_info = true; if (u.nc > ncinfo) ncinfo = u.nc; if (T.n > ninfo) ninfo = T.n; if (u.m > minfo) minfo = u.m; continue; }
        any_qr = true;
        if (T.n > nmax) nmax = T.n;
    }
    if (!any) return AV_OK;
    if ((rc = b->d_blk_row.upload(all_r, stm)) || (rc = b->d_blk_len.upload(all_l, stm)) || (rc = b->d_cols.upload(all_cols, stm))) return rc;
    for (int s = 0; s < S; ++s) if (ua[s].m > 0) {
        size_t o = reinterpret_cast<size_t>(ua[s].blk_row);
        ua[s].blk_row = b->d_blk_row.p + o; ua[s].blk_len = b->d_blk_len.p + o;
        ua[s].cols = b->d_cols.p + col_off[s];
    }
    if ((rc = msckf_lds_opt_in())) return rc;
    // ---- sequential chunks instead of a QR.  A stream that stacks more rows than the back end keeps (KCH) is updated in
    //      several rounds of at most KCH rows each: the EKF update with [H0; H1] equals the update with H0 followed by the
    //      update with H1 on the updated covariance and the residual r1 - H1 dx (independent noise), so no stream needs the
    //      1024-thread QR workgroup any more -- it waited ~1 ms per launch for a whole CU to drain and was the largest item of
    //      the step's chain.  Round r of all streams runs as one set of launches; most streams have one round.
    constexpr int KCH = 144;
    std::vector<std::vector<int>> cstart(S);                 // first block of every chunk of stream s (+ end)
    int R = 1;
    for (int s = 0; s < S; ++s) {
        if (ua[s].m <= 0 || ua[s].mode != 0) continue;
        int acc = 0;
        cstart[s].push_back(0);
        for (int k = 0; k < (int)bl[s].size(); ++k) {
            if (acc + bl[s][k] > KCH) { cstart[s].push_back(k); acc = 0; }
            acc += bl[s][k];
        }
        cstart[s].push_back((int)bl[s].size());
        if ((int)cstart[s].size() - 1 > R) R = (int)cstart[s].size() - 1;
    }
    std::vector<UpdArgs> uar((size_t)R * S);
    std::vector<int> kmax_r(R, 0);
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < S; ++s) {
            UpdArgs& u = uar[(size_t)r * S + s];
            u = ua[s];
            u.round = r; u.kdir = 0;
            if (ua[s].m <= 0) continue;
            if (ua[s].mode != 0) { if (r > 0) u.m = 0; continue; }
            const int nch = (int)cstart[s].size() - 1;
            if (r >= nch) { u.m = 0; continue; }
            const int b0 = cstart[s][r], b1 = cstart[s][r + 1];
            int rows_ = 0;
            for (int k = b0; k < b1; ++k) rows_ += bl[s][k];
            u.blk_row = ua[s].blk_row + b0; u.blk_len = ua[s].blk_len + b0; u.n_blk = b1 - b0;
            u.m = rows_; u.kdir = rows_;
            if (rows_ > kmax_r[r]) kmax_r[r] = rows_;
        }
    if ((rc = b->d_upd.upload(uar, stm))) return rc;
    if (any_info) {                                          // few-column streams (camera pruning): information form, one light kernel
        const size_t lds_i = upd_info_lds(ncinfo, ninfo, minfo);
        if (lds_i > 160 * 1024) { av_set_error("batched MSCKF: information-form update needs %zu B of LDS", lds_i); return AV_E_CAPACITY; }
        hipLaunchKernelGGL(upd_info_kernel, dim3(S), dim3(256), lds_i, stm, b->d_upd.p);
    }
    if (any_qr) for (int r = 0; r < R; ++r) {
        const UpdArgs* arr = b->d_upd.p + (size_t)r * S;
        if (kmax_r[r] <= 0) continue;
        hipLaunchKernelGGL(upd_gather_kernel, dim3(S), dim3(256), 0, stm, arr);
        // back end: the products around the per-stream factor kernel (msckf.hip: launch_upd_back)
        launch_upd_back(arr, S, kmax_r[r], nmax, stm);
    }
    AV_LAUNCH_CHECK();
    std::vector<double> dx((size_t)S * b->ld);
    AV_HIP(hipMemcpyAsync(dx.data(), b->dx, sizeof(double) * S * b->ld, hipMemcpyDeviceToHost, stm));
    { int rcw = b_wait(b, stm); if (rcw) return rcw; }
    if (b->debug_capture) {          // the same tap as b_chain_finish, for the phases that took this synchronous path
        const int ph = cut1500 ? 0 : 1;
        std::vector<double> g(nf);
        (void)hipMemcpy(g.data(), b->d_gamma.p, sizeof(double) * nf, hipMemcpyDeviceToHost);
        std::vector<int> acc(S, 0); std::vector<char> cutf(S, 0);
        for (int i = 0; i < nf; ++i) {
            const int s = refs[i].s;
            if (cutf[s]) continue;
            b->st[s].dbg_gamma[ph].push_back(g[i]);
            if (pass[i]) acc[s] += rows[i];
            if (cut1500 && acc[s] > 1500) cutf[s] = 1;
        }
        for (int s = 0; s < S; ++s) if (ua[s].m > 0) {
            BStream& T = b->st[s];
            T.dbg_rows[ph] = ua[s].m; T.dbg_n[ph] = T.n;
            T.dbg_dx[ph].assign(dx.data() + (size_t)s * b->ld, dx.data() + (size_t)s * b->ld + T.n);
            T.dbg_P[ph].resize((size_t)T.n * T.n);
            (void)hipMemcpy2D(T.dbg_P[ph].data(), sizeof(double) * T.n, b->P + (size_t)s * b->pstride, sizeof(double) * b->ld, sizeof(double) * T.n, T.n, hipMemcpyDeviceToHost);
        }
    }
    for (int s = 0; s < S; ++s) if (ua[s].m > 0) b_inject(b->st[s], dx.data() + (size_t)s * b->ld);
    return AV_OK;
}

// ------------------------------------------------------------------------------------------------
// Chained form of "triangulate -> Jacobian/gate -> stack -> update" for one phase of the step (lost features or camera
// pruning): every kernel is queued behind the previous one and the decisions in between are taken on the device
// (feature_kernel reads the triangulation results in place, upd_stack_kernel turns the gate flags into the block lists,
// column lists and chunk rounds of the back end), so the host waits ONCE per phase -- for delta_x, the stacked-row counts
// and the new feature positions together -- instead of three times (positions, gate flags, delta_x).
//
// `refs` holds ALL candidates of the phase (initialised or not), observations in `pool`.  b_chain_launch enqueues
// everything including the read-backs; the caller may queue more work on the stream (camera removal, position
// variances), waits, and calls b_chain_finish, which applies the results to the host-side bookkeeping.  ok[i] = 0 marks a
// feature whose triangulation failed.  Cases the chain does not cover run the synchronous path inside b_chain_launch
// (ctx.done): a stream whose candidates exceed rows_cap (two-pass gating), more than 60 rounds.
// ------------------------------------------------------------------------------------------------
struct ChainCtx {
    std::vector<int> todo;          // refs triangulated by this phase
    std::vector<char> ok;
    bool cut1500 = false;           // phase: remove_lost_features (true) / prune_cam_state_buffer
    std::vector<int> n_at_launch;   // debug capture: state dimension of every stream when the phase was launched
    bool launched = false;          // read-backs are queued: wait, then b_chain_finish
    bool done = false;              // handled synchronously
    int nf = 0;
};
constexpr int CHAIN_KCH = 144;      // rows of one sequential chunk (= the back end's limit)

int b_chain_launch(av_msckf_batch* b, std::vector<FeatRef>& refs, const ObsPool& pool, bool cut1500, hipStream_t stm, ChainCtx& ctx)
{
    ctx = ChainCtx();
    const int S = b->S, nf = (int)refs.size();
    ctx.nf = nf; ctx.cut1500 = cut1500;
    if (b->debug_capture) { ctx.n_at_launch.resize(S); for (int s = 0; s < S; ++s) ctx.n_at_launch[s] = b->st[s].n; }
    if (nf == 0) { ctx.done = true; return AV_OK; }
    // One round for every stream: a stream that stacks more rows than one back-end pass holds is first compressed to its n_c
    // non-zero columns' worth of rows (the Gram compression below -- a few per cent of the streams of a frame).  Sequential chunk
    // rounds cost every stream of the group the latency of the LONGEST stream's rounds: at 512 streams per group the longest
    // stacks 300-500 rows when the mean stacks 130, i.e. 3-5 rounds of six launches where one would do.
    int rc;
    // per-feature offsets, per-stream row reservations, cameras touched, all-pass chunk count (upper bound of the rounds)
    std::vector<int> off(nf + 1, 0), fs(nf), dof(nf), rowoff(nf), rbeg(S + 1, 0);
    std::vector<int> stream_rows(S, 0), rounds_s(S, 0), chunk_acc(S, 0);
    std::vector<unsigned long long> touched(S, 0ull);
    int maxobs = 0;
    bool any_over = false;
    for (int i = 0; i < nf; ++i) {
        const FeatRef& r = refs[i];
        const int rows = 4 * r.n - 3, s = r.s;
        off[i + 1] = off[i] + r.n; fs[i] = s; dof[i] = r.dof;
        rowoff[i] = stream_rows[s]; stream_rows[s] += rows;
        rbeg[s + 1] = i + 1;
        if (r.n > maxobs) maxobs = r.n;
        for (int k = 0; k < r.n; ++k) touched[s] |= 1ull << pool.cam[r.first + k];
        // next-fit chunks if every candidate passed the gate: next-fit is monotone (a subsequence never needs more chunks), so this
        // bounds the rounds of whatever subset the gate lets through
        if (rounds_s[s] == 0) rounds_s[s] = 1;
        if (chunk_acc[s] + rows > CHAIN_KCH) { ++rounds_s[s]; chunk_acc[s] = 0; }
        chunk_acc[s] += rows;
    }
    if (cut1500) for (int s = 0; s < S; ++s) {
        // behind the `> 1500 rows` cut at most 1500 + one block are stacked, and two consecutive chunks always hold more than
        // CHAIN_KCH rows together: c <= 2 ceil(rows / KCH) - 1
        const int rows = stream_rows[s] < 1500 + 81 ? stream_rows[s] : 1500 + 81;
        const int bound = 2 * ((rows + CHAIN_KCH - 1) / CHAIN_KCH) - 1;
        if (rounds_s[s] > bound) rounds_s[s] = bound < 1 ? 1 : bound;
    }
    for (int s = 0; s < S; ++s) { if (rbeg[s + 1] < rbeg[s]) rbeg[s + 1] = rbeg[s]; if (stream_rows[s] > b->rows_cap) any_over = true; }
    int R = 0, nmax = 0; bool any_info = false; int ncinfo = 0, ninfo = 0, minfo = 0;
    std::vector<int> clist;                              // streams that may need the compression
    std::vector<char> info_ok(S, 0), dead(S, 0);
    for (int s = 0; s < S; ++s) {
        if (stream_rows[s] == 0) continue;
        const int nct = 6 * __builtin_popcountll(touched[s]);
        if (nct <= INFO_NC) {                    // the stacked Jacobian cannot touch more than INFO_NC columns: information form
            info_ok[s] = 1; any_info = true;                 // (or, with m <= nc rows, one ordinary round)
            if (nct > ncinfo) ncinfo = nct;
            if (b->st[s].n > ninfo) ninfo = b->st[s].n;
            const int mm = stream_rows[s] < INFO_MAXROWS ? stream_rows[s] : INFO_MAXROWS;
            if (mm > minfo) minfo = mm;
            rounds_s[s] = stream_rows[s] > INFO_MAXROWS ? rounds_s[s] : 0;      // information form whatever the gate leaves: no round
        }
        if (rounds_s[s] > 1) {
            // rows the compression may be handed: behind the `> 1500 rows` cut at most 1500 + one block; its row map must fit the stream's Kt buffer
            const int fr = cut1500 && stream_rows[s] > 1500 + 81 ? 1500 + 81 : stream_rows[s];
            rounds_s[s] = 1;
            const bool fits = (size_t)fr <= 2 * b->pstride;
            if (!fits) { dead[s] = 1; b_fail_stream(b, s, AV_E_CAPACITY, "a %d-row update over more than %d columns exceeds the compression stage", fr, INFO_NC); }
            else clist.push_back(s);
        }
        if (rounds_s[s] > R) R = rounds_s[s];
        if (b->st[s].n > nmax) nmax = b->st[s].n;
    }
    if (any_over || R > 60) {
        // synchronous path: positions first, then the features that have one
        ctx.done = true;
        std::vector<char> ok;
        if ((rc = b_initialize(b, refs, ok, stm)) || (rc = b_wait(b, stm))) return rc;
        std::vector<FeatRef> proc;
        proc.reserve(refs.size());
        for (size_t i = 0; i < refs.size(); ++i) if (ok[i]) proc.push_back(refs[i]);
        ctx.ok.swap(ok);
        return b_blocks_and_update(b, proc, pool, cut1500, stm);
    }
    // ---- triangulation of the candidates without a position (results stay on the device)
    const int ph = cut1500 ? 0 : 1;
    if (b->work_timing) { AV_HIP(hipEventRecord(b->ev_t0[ph], stm)); b->ev_used[ph] = true; }
    if ((rc = b_tri_launch(b, refs, ctx.ok, ctx.todo, stm))) return rc;
    std::vector<int> tri_idx(nf, -1);
    for (size_t k = 0; k < ctx.todo.size(); ++k) tri_idx[ctx.todo[k]] = (int)k;
    for (int i = 0; i < nf; ++i) if (!ctx.ok[i]) tri_idx[i] = -2;          // failed check_motion: never evaluated
    // ---- observation CSR of the feature kernels, written straight into the pinned staging buffers by all cores
    int* cam = nullptr; double* z = nullptr; double* pos = nullptr;
    if ((rc = b->d_obs_cam.stage_for((size_t)off[nf], stm, &cam)) || (rc = b->d_obs_z.stage_for((size_t)off[nf] * 4, stm, &z)) ||
        (rc = b->d_pos.stage_for((size_t)nf * 3, stm, &pos))) return rc;
#pragma omp parallel for schedule(static) num_threads(host_threads(nf / 512))
    for (int i = 0; i < nf; ++i) {
        const FeatRef& r = refs[i];
        for (int k = 0; k < r.n; ++k) {
            cam[off[i] + k] = pool.cam[r.first + k];
            const double* zz = pool.z[r.first + k];
            for (int e = 0; e < 4; ++e) z[(size_t)(off[i] + k) * 4 + e] = zz[e];
        }
        for (int e = 0; e < 3; ++e) pos[(size_t)i * 3 + e] = r.f->pos[e];
    }
    if ((rc = b->d_obs_off.upload(off, stm)) || (rc = b->d_obs_cam.commit((size_t)off[nf], stm)) || (rc = b->d_obs_z.commit((size_t)off[nf] * 4, stm)) ||
        (rc = b->d_fstream.upload(fs, stm)) || (rc = b->d_dof.upload(dof, stm)) || (rc = b->d_rowoff.upload(rowoff, stm)) ||
        (rc = b->d_pos.commit((size_t)nf * 3, stm)) || (rc = b->d_gamma.ensure(nf)) || (rc = b->d_pass.ensure(nf)) ||
        (rc = b->d_tri_idx.upload(tri_idx, stm)) || (rc = b->d_rbeg.upload(rbeg, stm))) return rc;
    FeatArgs a = b_feat_args(b, cut1500, b->d_cam_q.p, b->d_cam_p.p, b->d_cam_qn.p);
    a.n_feat = nf; a.Mmax = maxobs; a.feat_stream = b->d_fstream.p; a.stream_ncam = b->d_ncam.p; a.stream_gravity = b->d_grav.p;
    a.obs_off = b->d_obs_off.p; a.obs_cam = b->d_obs_cam.p; a.obs_z = b->d_obs_z.p; a.pos = b->d_pos.p; a.dof = b->d_dof.p; a.row_off = b->d_rowoff.p;
    a.gamma = b->d_gamma.p; a.pass = b->d_pass.p;
    a.tri_idx = b->d_tri_idx.p; a.tri_pos = b->d_tpos.p; a.tri_valid = b->d_tvalid.p;
    {
        std::vector<int> all(nf);
        for (int i = 0; i < nf; ++i) all[i] = i;
        if ((rc = b_launch_buckets(b, a, refs, all, maxobs, stm))) return rc;
    }
    // ---- stacking on the device, then the back end for R rounds (streams that need fewer see m = 0)
    std::vector<UpdArgs> base(S);
    for (int s = 0; s < S; ++s) {
        UpdArgs& u = base[s] = b_upd_args(b, s);
        u.n = b->st[s].n;
        u.mode = dead[s] ? 2 : info_ok[s];      // 2: the stream takes no update in this phase (it was stopped above)
    }
    if ((rc = b->d_clist.upload(clist, stm)) || (rc = b->d_updbase.upload(base, stm)) || (rc = b->d_upd.ensure((size_t)(R > 0 ? R : 1) * S)) || (rc = b->d_blk_row.ensure(nf)) || (rc = b->d_blk_len.ensure(nf)) ||
        (rc = b->d_cols.ensure((size_t)S * 6 * b->cam_slots)) || (rc = b->d_stacked.reserve(S, true))) return rc;
    StackArgs sa; memset(&sa, 0, sizeof(sa));
    sa.rbeg = b->d_rbeg.p; sa.pass = b->d_pass.p; sa.obs_off = b->d_obs_off.p; sa.obs_cam = b->d_obs_cam.p; sa.row_off = b->d_rowoff.p;
    sa.blk_row = b->d_blk_row.p; sa.blk_len = b->d_blk_len.p; sa.cols = b->d_cols.p; sa.cols_stride = 6 * b->cam_slots;
    sa.base = b->d_updbase.p; sa.out = b->d_upd.p; sa.S = S; sa.rounds = R > 0 ? R : 1; sa.cut1500 = cut1500 ? 1 : 0; sa.kch = CHAIN_KCH; sa.stacked = b->d_stacked.p;
    hipLaunchKernelGGL(upd_stack_kernel, dim3(S), dim3(64), 0, stm, sa);
    if ((rc = msckf_lds_opt_in())) return rc;
    if (any_info) {
        const size_t lds_i = upd_info_lds(ncinfo, ninfo, minfo);
        if (lds_i > 160 * 1024) { av_set_error("batched MSCKF: information-form update needs %zu B of LDS", lds_i); return AV_E_CAPACITY; }
        hipLaunchKernelGGL(upd_info_kernel, dim3(S), dim3(256), lds_i, stm, b->d_upd.p);
    }
    // (rounds are empty launches for the streams that do not need them; R = 0: every stream with candidates takes the
    //  information form)
    if (R > 0) {
        for (int r = 0; r < R; ++r) {
            const UpdArgs* arr = b->d_upd.p + (size_t)r * S;
            if (r == 0 && !clist.empty()) {
                // streams that exceed a pass: Gram compression (msckf.hip "Row compression WITHOUT a QR"): row map, partial Gram slabs
                // per 256-row chunk and lower tile, bordered Cholesky -> the k = n_c rows [F | f] of W
                const unsigned nl = (unsigned)clist.size();
                hipLaunchKernelGGL(upd_rowmap_kernel, dim3(nl), dim3(64), 0, stm, arr, b->d_clist.p, (const int*)nullptr);
                const int k1max = 6 * b->max_cam + 1;                                  // a lost feature is not seen from the newest camera state: n_c <= 6 max_cam
                launch_upd_compress(arr, b->d_clist.p, nullptr, nl, k1max, stm);
            }
            hipLaunchKernelGGL(upd_gather_kernel, dim3(S), dim3(256), 0, stm, arr);
            launch_upd_back(arr, S, CHAIN_KCH, nmax, stm);
        }
    }
    AV_LAUNCH_CHECK();
    if (b->debug_capture)
        for (int s = 0; s < S; ++s) if (stream_rows[s] > 0) {
            BStream& T = b->st[s];
            T.dbg_P[ph].resize((size_t)T.n * T.n);
            AV_HIP(hipMemcpy2DAsync(T.dbg_P[ph].data(), sizeof(double) * T.n, b->P + (size_t)s * b->pstride, sizeof(double) * b->ld, sizeof(double) * T.n, T.n, hipMemcpyDeviceToHost, stm));
        }
    if (b->work_timing) AV_HIP(hipEventRecord(b->ev_t1[ph], stm));
    AV_HIP(hipMemcpyAsync(b->h_dx, b->dx, sizeof(double) * S * b->ld, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(b->d_stacked.stage, b->d_stacked.p, sizeof(int) * S, hipMemcpyDeviceToHost, stm));
    if ((rc = b_tri_readback(b, (int)ctx.todo.size(), stm))) return rc;
    ctx.launched = true;
    return AV_OK;
}

// after the wait: positions of the triangulated features, state injection of the streams that were updated
int b_chain_finish(av_msckf_batch* b, std::vector<FeatRef>& refs, ChainCtx& ctx)
{
    if (!ctx.launched) return AV_OK;
    const int S = b->S;
    b_tri_collect(b, refs, ctx.todo, ctx.ok);
    const int* stacked = b->d_stacked.stage;
    // stacked < 0: the stream's block list or its chunk rounds outgrew what the back end was launched for.  upd_stack_kernel gave
    // that stream m = 0 in every round, so its covariance is untouched and no delta_x exists: the stream stops here, consistent;
    // every other stream of the group has been updated and is injected below.
    for (int s = 0; s < S; ++s)
        if (stacked[s] == UPD_BAD_PIVOT) b_fail_stream(b, s, AV_E_NUMERIC, "a Cholesky factorisation of the stacked update met a non-positive or non-finite pivot (rank-deficient Gram matrix or corrupt covariance); update skipped, stream stopped");
        else if (stacked[s] < 0) b_fail_stream(b, s, AV_E_CAPACITY, "stream stacks more than %d blocks or more chunk rounds than the back end was launched for", STACK_LDS_BLOCKS);
    par_streams(S, [&](int s) { if (stacked[s] > 0) b_inject(b->st[s], b->h_dx + (size_t)s * b->ld); });
    if (b->debug_capture) {
        // gating values of the candidates the reference would have evaluated: in map order, features whose triangulation failed
        // are deleted before the gate (msckf.py:634-637), and the loop stops once more than 1500 rows are stacked (:667-668)
        const int ph = ctx.cut1500 ? 0 : 1;
        std::vector<double> g(ctx.nf); std::vector<int> pass(ctx.nf);
        if (ctx.nf > 0) {
            (void)hipMemcpy(g.data(), b->d_gamma.p, sizeof(double) * ctx.nf, hipMemcpyDeviceToHost);
            (void)hipMemcpy(pass.data(), b->d_pass.p, sizeof(int) * ctx.nf, hipMemcpyDeviceToHost);
        }
        std::vector<int> acc(S, 0); std::vector<char> cut(S, 0);
        for (int i = 0; i < ctx.nf; ++i) {
            const int s = refs[i].s;
            if (cut[s] || (!ctx.ok.empty() && !ctx.ok[i])) continue;
            b->st[s].dbg_gamma[ph].push_back(g[i]);
            if (pass[i]) acc[s] += 4 * refs[i].n - 3;
            if (ctx.cut1500 && acc[s] > 1500) cut[s] = 1;
        }
        for (int s = 0; s < S; ++s) if (stacked[s] > 0) {
            BStream& T = b->st[s];
            const int n = ctx.n_at_launch.empty() ? T.n : ctx.n_at_launch[s];
            T.dbg_rows[ph] = stacked[s]; T.dbg_n[ph] = n;
            T.dbg_dx[ph].assign(b->h_dx + (size_t)s * b->ld, b->h_dx + (size_t)s * b->ld + n);
        }
    }
    {   // work counters (SURVEY 8d): per gated feature with r = 4M-3 rows against n columns  2 r n^2 + 2 r^2 n + r^3/3;
        // per update of m stacked rows with k = min(m, n) rows kept:  S = (H P) H^T  2 k n^2 + 2 k^2 n,  Cholesky k^3/3,  solve 2 k^2 n,
        // covariance update 4 k n^2  (= the survey's 4 n^3 + n^3/3 + 2 n^3 + 4 n^3 at k = n), and -- counted apart, because the
        // column-compressed update here never runs it at that size -- the reference's thin QR 2 m n^2 - 2/3 n^3 when m > n
        for (int i = 0; i < ctx.nf; ++i) {
            if (!ctx.ok.empty() && !ctx.ok[i]) continue;
            const double r = 4.0 * refs[i].n - 3.0, n = (double)b->st[refs[i].s].n;
            b->w_gate_flops += 2 * r * n * n + 2 * r * r * n + r * r * r / 3.0; ++b->w_gated;
        }
        for (int s = 0; s < S; ++s) if (stacked[s] > 0) {
            const double m = stacked[s], n = (double)b->st[s].n, k = m < n ? m : n;
            b->w_update_flops += 2 * k * n * n + 2 * k * k * n + k * k * k / 3.0 + 2 * k * k * n + 4 * k * n * n;
            if (m > n) b->w_qr_flops += 2 * m * n * n - 2.0 / 3.0 * n * n * n;
            b->w_rows += stacked[s]; ++b->w_updates;
        }
        {   // only the pair of the phase that has just been waited for (the other phase's chain may still be in flight)
            const int ph = ctx.cut1500 ? 0 : 1;
            if (b->ev_used[ph]) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, b->ev_t0[ph], b->ev_t1[ph]) == hipSuccess) b->w_chain_ms += ms; else ++b->w_chain_dropped;
                b->ev_used[ph] = false;
            }
        }
    }
    return AV_OK;
}

}  // namespace

static void sub_destroy(av_msckf_batch* b);
namespace { int dev_launch(av_msckf_batch* b, int k, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap, const double* timestamps, bool dev_msg, hipEvent_t ready, hipStream_t stm); int dev_finish(av_msckf_batch* b, int k, double* out, const StepOuts& outs); int dev_read_state(av_msckf_batch* b, int s, DState* D); const char* dev_fail_message(int code, int* av_code); int dev_reserve(av_msckf_batch* b, int cap); int dev_upload_updbase(av_msckf_batch* b); int dev_restart(av_msckf_batch* b, const int* list, int n, hipStream_t stm); }

// Stream for the filter's kernels.  AV_MSCKF_CUS="first:count" confines them to `count` compute units starting at CU `first`
// (hipExtStreamCreateWithCUMask) -- together with a complementary mask on the caller's front-end stream this partitions the
// chip, so that the filter's latency-bound kernels never queue behind the front-end's resident workgroups.  Without the
// variable: an ordinary stream, at the highest priority for the host-bookkeeping path, at the default priority otherwise.
static int make_filter_stream(AvResources& res, hipStream_t* out, bool host_store)
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
    // Device-resident filter (the default): its chain never waits for the host, so it runs at the DEFAULT stream priority -- the
    // front-end's kernels keep their speed (11.5 instead of 16 ms of spans per 2,048-stream step) and the complete path gains
    // (DESIGN.md section 7: 131 k vs 114 k frames/s).  The host-bookkeeping path (AV_MSCKF_STORE=host) keeps the highest priority:
    // its launches are interleaved with host phases and must be scheduled at once.
    return res.stream(out, hipStreamNonBlocking, host_store ? hi : (lo + hi) / 2);
}

// Rows of the overflow pool behind the last stream's block-buffer region (device-resident path).  A stream whose lost-feature
// candidates reserve more rows than its own region holds (a blank frame drops every track at once: ~4,500 rows) takes the rows
// from here -- one atomic bump per stream and step -- instead of gating first and storing in a second pass: that second pass had to
// be LAUNCHED every step (its list is only known on the device) and, idle as it normally was, waited ~1.1 ms per step for a CU
// with 69 KB of LDS and 4 x 176 registers free beside the front-end (profiles/r04/README.md).  Exhausting the pool stops the stream
// with AV_E_CAPACITY (DFAIL_ROWS).  AV_MSCKF_POOL_ROWS overrides the size.
static size_t b_pool_rows(const av_msckf_batch* b, int rows_cap)
{
    if (!b->pool_on || rows_cap <= 0) return 0;
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
                                    const double* opt6, int device, bool host_store, av_msckf_batch** out)
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
    // One back-end pass of the chained update keeps k = min(m, n_c) <= CHAIN_KCH rows (S / T^T tiles, the packed Cholesky triangle
    // in LDS, upd_compress); n_c can reach 6 columns per camera state, so the window must satisfy 6 * max_cam_states <= CHAIN_KCH.
    // (The reference default is 20 -> n_c <= 120; the single-filter API av_msckf_* has no such limit.)
    if (6 * max_cam_states > CHAIN_KCH) {
        av_set_error("av_msckf_batch_create: max_cam_states %d: the batched update holds at most %d rows / columns per pass (6 per camera state: max_cam_states <= %d)",
                     max_cam_states, CHAIN_KCH, CHAIN_KCH / 6);
        return AV_E_CAPACITY;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { av_set_error("av_msckf_batch_create: no HIP device visible"); return AV_E_NODEVICE; }
    AV_HIP(hipSetDevice(device));
    setenv("OMP_WAIT_POLICY", "passive", 0);      // idle OpenMP workers must not spin next to the HIP runtime threads
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
    for (int i = 0; i < 100; ++i) b->chi2[i] = chi2_table_100[i];
    b->obs_noise = obs_noise; b->pos_std_thr = position_std_threshold;
    // The filter's state and observation map live on the device (msckf_dev.inc) unless AV_MSCKF_STORE=host asks for the
    // host-bookkeeping path (A/B runs).
    b->pool_on = !host_store;
    const size_t S = n_streams;
    b->pstride = (size_t)b->ld * b->ld; b->hstride = (size_t)rows_cap * b->ld; b->rstride = rows_cap; b->wstride = (size_t)rows_cap * (b->ld + 1);
    int rc;
#define A(p, cnt) if ((rc = b->res.dev(&(p), (size_t)(cnt)))) return rc;
    A(b->P, S * b->pstride) A(b->Pn, S * b->pstride) A(b->T, S * b->pstride) A(b->Kt, S * b->pstride) A(b->scratch, S * b->pstride)
    if (rows_cap > 0) { const size_t pool = b_pool_rows(b, rows_cap); A(b->W, S * b->wstride) A(b->Hblk, S * b->hstride + pool * b->ld) A(b->rblk, S * b->rstride + pool) }
    A(b->dx, S * b->ld) A(b->chi2_dev, 100) A(b->pvar, 3 * S)
#undef A
    AV_HIP(hipMemcpy(b->chi2_dev, chi2_table_100, sizeof(double) * 100, hipMemcpyHostToDevice));
    if ((rc = b->res.pinned(&b->h_dx, S * b->ld)) || (rc = b->res.pinned(&b->h_pv, 3 * S))) return rc;
    for (int i = 0; i < 4; ++i) if ((rc = make_filter_stream(b->res, &b->aux[i], host_store)) || (rc = b->res.event(&b->ev_join[i], hipEventDisableTiming))) return rc;
    if ((rc = b->res.event(&b->ev_fork, hipEventDisableTiming)) || (rc = b->res.event(&b->ev_wait, hipEventDisableTiming | hipEventBlockingSync))) return rc;
    for (int i = 0; i < 2; ++i) if ((rc = b->res.event(&b->ev_t0[i], hipEventDefault)) || (rc = b->res.event(&b->ev_t1[i], hipEventDefault))) return rc;
    for (int s = 0; s < n_streams; ++s) {
        BStream& T = b->st[s];
        for (int i = 0; i < 3; ++i) { T.gravity[i] = gravity[i]; T.v[i] = velocity0[i]; T.t_ci[i] = b->t_ci0[i]; }
        for (int i = 0; i < 9; ++i) T.R_ic[i] = b->R_ic0[i];
        if ((rc = b_reset_cov(b, s, nullptr))) return rc;
    }
    if (b->pool_on) { b->dev = new (std::nothrow) DevPath(); if (!b->dev) { av_set_error("out of host memory"); return AV_E_INVALID; } }
    guard.b = nullptr;
    *out = b;
    return AV_OK;
}

static void sub_destroy(av_msckf_batch* b)
{
    if (!b) return;
    b->res.release();                 // (the group's worker has been joined by the caller)
    delete b->dev;
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

// Size every per-step device buffer and its pinned staging for the worst case of a feature message of `cap` features per
// stream, so that no step allocates, frees or synchronises for memory (DevBuf growth stays as a counted fallback).
// Bounds: every feature that is not observed in the current frame leaves the map in that same frame (processed or
// invalid, msckf.py:614-676), so a stream holds at most cap features after a step and at most 2*cap inside one; the
// lost-feature candidates are at most the cap features of the previous frame, the prune candidates at most the cap of
// this one; a feature holds at most one observation per camera state.
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
        b->hstride = (size_t)b->rows_cap * b->ld; b->rstride = b->rows_cap; b->wstride = (size_t)b->rows_cap * (b->ld + 1);
        int rc0;
        const size_t pool = b_pool_rows(b, b->rows_cap);
        if ((rc0 = b->res.dev(&b->W, Sn * b->wstride)) || (rc0 = b->res.dev(&b->Hblk, Sn * b->hstride + pool * b->ld)) || (rc0 = b->res.dev(&b->rblk, Sn * b->rstride + pool))) return rc0;
    }
    if (5 * cap > b->rows_cap) {
        av_set_error("batched MSCKF: rows_cap %d cannot hold the camera-pruning update of %d features per message (5 rows each: need >= %d)",
                     b->rows_cap, cap, 5 * cap);
        return AV_E_CAPACITY;
    }
    if (b->dev) { b->reserved_cap = cap; return AV_OK; }       // device-resident path: its own arrays (dev_reserve), none of the CSR staging below
    const size_t S = (size_t)b->S, cs = (size_t)b->cam_slots, nf = S * (size_t)cap + 64;
    int rc;
    if ((rc = b->d_clist.reserve(S, true)) || (rc = b->d_flist.reserve(nf, true)) || (rc = b->d_obs_off.reserve(nf + 1, true)) || (rc = b->d_obs_cam.reserve(nf * cs, true)) ||
        (rc = b->d_obs_z.reserve(nf * cs * 4, true)) || (rc = b->d_fstream.reserve(nf, true)) || (rc = b->d_dof.reserve(nf, true)) ||
        (rc = b->d_rowoff.reserve(nf, true)) || (rc = b->d_pass.reserve(nf, false)) || (rc = b->d_valid.reserve(nf, false)) ||
        (rc = b->d_gamma.reserve(nf, false)) || (rc = b->d_pos.reserve(nf * 3, true)) || (rc = b->d_blk_row.reserve(nf, true)) ||
        (rc = b->d_blk_len.reserve(nf, true)) || (rc = b->d_cols.reserve(S * 6 * cs, true)) || (rc = b->d_ncam.reserve(S, true)) ||
        (rc = b->d_cam_q.reserve(S * cs * 4, true)) || (rc = b->d_cam_p.reserve(S * cs * 3, true)) || (rc = b->d_cam_qn.reserve(S * cs * 4, true)) ||
        (rc = b->d_grav.reserve(S * 3, true)) || (rc = b->d_prop.reserve(S * 24, true)) || (rc = b->d_first.reserve(S + 1, true)) ||
        (rc = b->d_aug.reserve(S, true)) || (rc = b->d_rem.reserve(S, true)) || (rc = b->d_upd.reserve(S * 24, true)) ||
        (rc = b->d_tobs_off.reserve(nf + 1, true)) || (rc = b->d_tobs_cam.reserve(nf * cs, true)) || (rc = b->d_tobs_z.reserve(nf * cs * 4, true)) ||
        (rc = b->d_tfs.reserve(nf, true)) || (rc = b->d_tvalid.reserve(nf, true)) || (rc = b->d_tpos.reserve(nf * 3, true)) ||
        (rc = b->d_tri_idx.reserve(nf, true)) || (rc = b->d_rbeg.reserve(S + 1, true)) || (rc = b->d_stacked.reserve(S, true)) ||
        (rc = b->d_updbase.reserve(S, true))) return rc;
    b->reserved_cap = cap;
    return AV_OK;
}

static long long sub_growths(const av_msckf_batch* b) { return b->res.growths(); }

// feature_callback for every stream (msckf.py:177-228).  Features of stream s: ids[s*cap + k], uv[(s*cap+k)*4 ..], k < n_feat[s]
// (host arrays).  out[s*12 ..] = published, t, p(3), q(4), v(3) of the IMU state.
static int sub_step(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                                  const double* timestamps, double* out, void* stream)
{
    if (!b || !ids || !uv || !n_feat || !timestamps || !out || cap <= 0) { av_set_error("av_msckf_batch_step: bad arguments"); return AV_E_INVALID; }
    hipStream_t stm = (hipStream_t)stream;
    const int S = b->S;
    AV_HIP(hipSetDevice(b->device));
    int rc;
    if (b->dev) {
        const int k = (int)(b->dev_seq++ % DEV_RING);
        const StepOuts outs = take_outs(b);
        if ((rc = dev_launch(b, k, ids, uv, n_feat, cap, timestamps, false, nullptr, stm))) return rc;
        return dev_finish(b, k, out, outs);
    }
    if ((rc = sub_reserve(b, cap))) return rc;
    ++b->n_steps;
    if (b->debug_capture) for (BStream& T : b->st) for (int ph = 0; ph < 2; ++ph) { T.dbg_gamma[ph].clear(); T.dbg_dx[ph].clear(); T.dbg_P[ph].clear(); T.dbg_rows[ph] = 0; T.dbg_n[ph] = 0; }
    // ---- batch_imu_processing + process_model (msckf.py:251-339) ---------------------------------
    // two passes: count the IMU samples of this frame per stream, then every stream writes its PropArgs at its offset of
    // the pinned staging buffer (no per-stream vectors, no serial concatenation)
    std::vector<int> first(S + 1, 0);
    par_streams(S, [&](int s) {
        BStream& T = b->st[s];
        std::lock_guard<std::mutex> g(T.mu);
        // msckf.py:182-183 under the deterministic replay of SURVEY 3.5 (IMU messages with timestamp <= t are delivered
        // before the frame at t): the filter is live for this frame iff the sample that completed the gravity
        // initialisation is not newer than the frame -- a function of the data, not of when push_imu happened to run.
        // Read under the stream's mutex: push_imu may be initialising q / bg / gravity on another thread right now.
        // timestamps[s] < 0 (or NaN): the caller has no frame for this stream in this step (ragged sequence lengths in a
        // sweep): the stream idles, its state is untouched and out[s*12] reads 0.
        T.active = !T.failed && T.gravity_set && timestamps[s] >= 0 && T.gravity_time <= timestamps[s];
        if (T.active && (int)T.cams.size() + 1 > b->cam_slots) b_fail_stream(b, s, AV_E_CAPACITY, "stream exceeds %d camera states", b->cam_slots);
        if (!T.active) return;
        const double t0 = T.first_img ? timestamps[s] : T.ts;
        int cnt = 0;
        for (const BImu& m : T.imu) {
            if (m.t < t0) continue;
            if (m.t > timestamps[s]) break;
            ++cnt;
        }
        first[s + 1] = cnt;
    });
    for (int s = 0; s < S; ++s) first[s + 1] += first[s];
    PropArgs* props = nullptr;
    if ((rc = b->d_prop.stage_for((size_t)first[S], stm, &props))) return rc;
    // The per-stream host phases up to the first device round trip (IMU integration, state augmentation, observation
    // bookkeeping, lost-feature selection) run in TWO parallel regions below (the second one overlaps the propagate and
    // augment kernels): a fork/join per phase costs more than the phases themselves once stream groups share the cores.
    auto ph_imu = [&](int s) {
        BStream& T = b->st[s];
        if (!T.active) return;
        if (T.first_img) { T.first_img = false; T.ts = timestamps[s]; }
        std::lock_guard<std::mutex> g(T.mu);
        size_t used = 0;
        int w = first[s];
        for (const BImu& m : T.imu) {
            if (m.t < T.ts) { ++used; continue; }
            if (m.t > timestamps[s] || w >= first[s + 1]) break;      // samples pushed since the count wait for the next frame
            PropArgs& a = props[w++];
            a.P = b->P + (size_t)s * b->pstride; a.n = T.n; a.ld = b->ld; a.dt = m.t - T.ts;
            for (int i = 0; i < 3; ++i) { a.gyro[i] = m.w[i] - T.bg[i]; a.acc[i] = m.a[i] - T.ba[i]; a.gravity[i] = T.gravity[i]; }
            for (int i = 0; i < 4; ++i) { a.q_old[i] = T.q[i]; a.noise[i] = b->noise[i]; }
            b_predict_new_state(T, a.dt, a.gyro, a.acc);
            for (int i = 0; i < 4; ++i) { a.q_new[i] = T.q[i]; a.q_null[i] = T.qn[i]; }
            for (int i = 0; i < 3; ++i) { a.v_null[i] = T.vn[i]; a.p_null[i] = T.pn[i]; a.v_new[i] = T.v[i]; a.p_new[i] = T.p[i]; }
            for (int i = 0; i < 4; ++i) T.qn[i] = T.q[i];
            for (int i = 0; i < 3; ++i) { T.pn[i] = T.p[i]; T.vn[i] = T.v[i]; }
            T.null_aliased = true;
            ++used;
            T.ts = m.t;
        }
        T.imu_id = T.next_imu_id++;
        T.imu.erase(T.imu.begin(), T.imu.begin() + used);
    };
    // ---- state_augmentation (msckf.py:390-423) ---------------------------------------------------
    std::vector<AugArgs> aug_s(S);
    auto ph_aug = [&](int s) {
        BStream& T = b->st[s];
        if (!T.active) return;
        double Rwi[9], Rwc[9], tw[3];
        h_to_rotation(T.q, Rwi);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rwc[r * 3 + c] = T.R_ic[r * 3] * Rwi[c] + T.R_ic[r * 3 + 1] * Rwi[3 + c] + T.R_ic[r * 3 + 2] * Rwi[6 + c];
        h_mtv(Rwi, T.t_ci, tw);
        BCam cs; cs.id = T.imu_id; cs.t = timestamps[s];
        h_to_quaternion(Rwc, cs.q);
        for (int i = 0; i < 4; ++i) cs.qn[i] = cs.q[i];
        for (int i = 0; i < 3; ++i) cs.p[i] = T.p[i] + tw[i];
        T.cams.push_back(cs);
        AugArgs& a = aug_s[s]; a.P = b->P + (size_t)s * b->pstride; a.n = T.n; a.ld = b->ld;
        for (int i = 0; i < 9; ++i) a.R_ic[i] = T.R_ic[i];
        const double sk[9] = {0, -tw[2], tw[1], tw[2], 0, -tw[0], -tw[1], tw[0], 0};
        for (int i = 0; i < 9; ++i) a.sk[i] = sk[i];
        T.n += 6;
    };
    // ---- add_feature_observations (msckf.py:425-441) -----------------------------------------------
    auto ph_addobs = [&](int s) {
        BStream& T = b->st[s];
        if (!T.active) return;
        const size_t before = (size_t)T.map.live;
        const int nk = n_feat[s];
        static_assert(sizeof(long long) == sizeof(int64_t), "feature ids");
        const int tracked = T.map.add_frame(T.imu_id, reinterpret_cast<const long long*>(ids) + (size_t)s * cap, uv + (size_t)s * cap * 4, nk);
        if (tracked < 0) { b_fail_stream(b, s, AV_E_CAPACITY, "more than %d frames in the stream's window", FeatStore::NSLOT); return; }
        T.tracking_rate = tracked / ((double)before + 1e-5);
    };
    // ---- remove_lost_features, selection (msckf.py:614-640) -------------------------------------------
    std::vector<std::vector<FeatRef>> cand_s(S);
    std::vector<std::vector<int>> invalid(S);               // feature slots to delete
    auto ph_lost_select = [&](int s) {
        BStream& T = b->st[s];
        if (!T.active) return;
        // every live feature was seen in the frame before this one (features that are not are deleted in the same step): the
        // lost ones are that frame's entries without a successor.  Dict order = birth order.
        FeatStore& M = T.map;
        if (M.order.size() < 2) return;
        const FeatStore::Frame& P = M.fr[M.order[M.order.size() - 2]];
        for (int i = 0; i < P.n; ++i) {
            const int fs = P.fslot[i];
            if (fs < 0 || P.next[i] >= 0) continue;
            FMeta& m = M.meta[fs];
            if (m.nobs < 3) { invalid[s].push_back(fs); continue; }
            FeatRef r; r.s = s; r.f = &m; r.fs = fs; r.dof = 0;
            cand_s[s].push_back(r);
        }
        std::sort(cand_s[s].begin(), cand_s[s].end(), [](const FeatRef& x, const FeatRef& y) { return x.f->birth < y.f->birth; });
    };
    par_streams(S, [&](int s) { ph_imu(s); ph_aug(s); });
    if (first[S] > 0) {
        if ((rc = b->d_prop.commit((size_t)first[S], stm)) || (rc = b->d_first.upload(first, stm))) return rc;
        hipLaunchKernelGGL(propagate_batch_kernel, dim3(S), dim3(256), 0, stm, b->d_prop.p, b->d_first.p);
        AV_LAUNCH_CHECK();
    }
    {
        std::vector<AugArgs> augs;
        for (int s = 0; s < S; ++s) if (b->st[s].active) augs.push_back(aug_s[s]);
        if (!augs.empty()) {
            if ((rc = b->d_aug.upload(augs, stm))) return rc;
            hipLaunchKernelGGL(augment_batch_kernel, dim3((unsigned)augs.size()), dim3(256), 0, stm, b->d_aug.p);
            AV_LAUNCH_CHECK();
        }
    }
    par_streams(S, [&](int s) { ph_addobs(s); ph_lost_select(s); });      // overlaps the two kernels above
    if ((rc = b_upload_cams(b, stm))) return rc;
    // concatenation of per-stream FeatRef lists + observation pools, in stream order
    auto concat = [&](std::vector<std::vector<FeatRef>>& rs, std::vector<ObsPool>& ps, std::vector<FeatRef>& out, ObsPool& pool) {
        std::vector<size_t> ro(S + 1, 0), po(S + 1, 0);
        for (int s = 0; s < S; ++s) { ro[s + 1] = ro[s] + rs[s].size(); po[s + 1] = po[s] + ps[s].cam.size(); }
        out.resize(ro[S]); pool.cam.resize(po[S]); pool.z.resize(po[S]);
        par_streams(S, [&](int s) {
            for (size_t k = 0; k < ps[s].cam.size(); ++k) { pool.cam[po[s] + k] = ps[s].cam[k]; pool.z[po[s] + k] = ps[s].z[k]; }
            for (size_t k = 0; k < rs[s].size(); ++k) { FeatRef r = rs[s][k]; r.first += (int)po[s]; out[ro[s] + k] = r; }
        });
    };
    auto concat_refs = [&](const std::vector<std::vector<FeatRef>>& rs, std::vector<FeatRef>& out, std::vector<size_t>& beg) {
        beg.assign(S + 1, 0);
        for (int s = 0; s < S; ++s) beg[s + 1] = beg[s] + rs[s].size();
        out.resize(beg[S]);
        par_streams(S, [&](int s) { for (size_t k = 0; k < rs[s].size(); ++k) out[beg[s] + k] = rs[s][k]; });
    };
    // ---- remove_lost_features (msckf.py:614-676) ----------------------------------------------------
    bool synced = false;          // has the stream been waited for since the camera arrays were staged?
    {
        std::vector<FeatRef> cand;
        std::vector<size_t> cbeg;
        concat_refs(cand_s, cand, cbeg);
        // every candidate goes down the chain (triangulation results are consumed on the device; a feature that fails it is
        // not evaluated), and every candidate is deleted afterwards: processed or invalid (msckf.py:646-656, 675-676)
        std::vector<std::vector<FeatRef>> proc_s(S); std::vector<ObsPool> pool_s(S);
        par_streams(S, [&](int s) {
            const BStream& T = b->st[s];
            for (size_t i = cbeg[s]; i < cbeg[s + 1]; ++i) {
                FeatRef r = cand[i];
                int oc[FeatStore::NSLOT]; const double* oz[FeatStore::NSLOT];
                const int no = T.map.collect(*r.f, oc, oz, FeatStore::NSLOT);
                for (int q = 0; q < no; ++q) r.add(pool_s[s], oc[q], oz[q]);
                r.dof = r.n - 1;
                proc_s[s].push_back(r);
            }
        });
        std::vector<FeatRef> proc; ObsPool pool;
        concat(proc_s, pool_s, proc, pool);
        ChainCtx cx;
        if ((rc = b_chain_launch(b, proc, pool, true, stm, cx))) return rc;
        if (cx.launched) { if ((rc = b_wait(b, stm)) || (rc = b_chain_finish(b, proc, cx))) return rc; }
        if (!proc.empty()) synced = true;
        par_streams(S, [&](int s) {
            BStream& T = b->st[s];
            for (const FeatRef& r : proc_s[s]) invalid[s].push_back(r.fs);
            for (int fs : invalid[s]) T.map.erase(fs);
        });
    }
    // ---- prune_cam_state_buffer (msckf.py:678-786) ----------------------------------------------------
    bool have_pv = false;         // position variances already read back (with the pruning phase's results)
    {
        std::vector<std::array<long long, 2>> rm(S);
        std::vector<char> prune(S, 0);
        par_streams(S, [&](int s) {
            BStream& T = b->st[s];
            if (!T.active || (int)T.cams.size() < b->max_cam) return;
            prune[s] = 1;
            // find_redundant_cam_states
            const int nc = (int)T.cams.size(), key = nc - 4;
            int idx = key + 1, firstc = 0;
            double Rk[9]; h_to_rotation(T.cams[key].q, Rk);
            long long sel[2];
            for (int k = 0; k < 2; ++k) {
                double Rc[9], RR[9], qq[4];
                h_to_rotation(T.cams[idx].q, Rc);
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) RR[r * 3 + c] = Rc[r * 3] * Rk[c * 3] + Rc[r * 3 + 1] * Rk[c * 3 + 1] + Rc[r * 3 + 2] * Rk[c * 3 + 2];
                h_to_quaternion(RR, qq);
                const double d[3] = {T.cams[idx].p[0] - T.cams[key].p[0], T.cams[idx].p[1] - T.cams[key].p[1], T.cams[idx].p[2] - T.cams[key].p[2]};
                const double ang = 2 * acos(qq[3]);
                if (ang < 0.2618 && h_norm3(d) < 0.4 && T.tracking_rate > 0.5) sel[k] = T.cams[idx].id;
                else { sel[k] = T.cams[firstc].id; ++firstc; }
                ++idx;
            }
            if (sel[0] > sel[1]) std::swap(sel[0], sel[1]);
            rm[s] = {sel[0], sel[1]};
        });
        bool any = false;
        for (int s = 0; s < S; ++s) if (prune[s]) { any = true; ++b->n_prune_stream_steps; }
        if (any) {
            if (!synced) { if ((rc = b_wait(b, stm))) return rc; }     // the staging buffers of the camera arrays are about to be rewritten
            if ((rc = b_upload_cams(b, stm))) return rc;       // the lost-feature update moved the camera states
            std::vector<std::vector<FeatRef>> cand_s(S);
            std::vector<std::vector<FeatRef>> proc_s(S); std::vector<ObsPool> pool_s(S);
            par_streams(S, [&](int s) {
                if (!prune[s]) return;
                BStream& T = b->st[s];
                const long long r0 = rm[s][0], r1 = rm[s][1];
                const int i0 = b_cam_index(T, r0), i1 = b_cam_index(T, r1);
                // a candidate (msckf.py:736-757) was seen from BOTH removed cameras: follow the links of the entries of frame i0 to
                // frame i1.  (A feature seen from only one of them just loses that observation when the frames go, below.)
                // Triangulated inside the chain from ALL its observations if it has no position yet, evaluated on the two.
                FeatStore& M = T.map;
                const FeatStore::Frame& A = M.fr[M.order[i0]];
                for (int i = 0; i < A.n; ++i) {
                    const int fs = A.fslot[i];
                    if (fs < 0) continue;
                    int l = A.next[i];
                    while (l >= 0 && M.pos_of[FeatStore::lslot(l)] < i1) l = M.fr[FeatStore::lslot(l)].next[FeatStore::lidx(l)];
                    if (l < 0 || M.pos_of[FeatStore::lslot(l)] != i1) continue;
                    FeatRef r; r.s = s; r.f = &M.meta[fs]; r.fs = fs; r.dof = 2;
                    r.add(pool_s[s], i0, &A.z[(size_t)4 * i]);
                    r.add(pool_s[s], i1, &M.fr[FeatStore::lslot(l)].z[(size_t)4 * FeatStore::lidx(l)]);
                    proc_s[s].push_back(r);
                }
                // dict order (a reference keeps its own pool slice, so sorting the references is enough)
                std::sort(proc_s[s].begin(), proc_s[s].end(), [](const FeatRef& x, const FeatRef& y) { return x.f->birth < y.f->birth; });
            });
            std::vector<FeatRef> proc; ObsPool pool;
            concat(proc_s, pool_s, proc, pool);
            ChainCtx cx;
            if ((rc = b_chain_launch(b, proc, pool, false, stm, cx))) return rc;
            // the two camera states leave the covariance right behind the update (nothing here depends on the host's copy of the
            // state); the position variances of `publish` ride on the same wait
            std::vector<RemArgs> ra(S);
            par_streams(S, [&](int s) {
                RemArgs& a = ra[s];
                memset(&a, 0, sizeof(a)); a.start0 = a.start1 = -1;
                if (!prune[s]) return;
                const BStream& T = b->st[s];
                const int i0 = b_cam_index(T, rm[s][0]), i1 = b_cam_index(T, rm[s][1]);
                a.P = b->P + (size_t)s * b->pstride; a.scratch = b->scratch + (size_t)s * b->pstride; a.n = T.n; a.ld = b->ld;
                a.start0 = IMU_DIM + 6 * i0; a.start1 = IMU_DIM + 6 * (i1 - 1);
            });
            if ((rc = b->d_rem.upload(ra, stm))) return rc;
            hipLaunchKernelGGL(remove_cam_batch_kernel, dim3(S), dim3(256), 0, stm, b->d_rem.p);
            AV_LAUNCH_CHECK();
            hipLaunchKernelGGL(pos_var_kernel, dim3((3 * S + 255) / 256), dim3(256), 0, stm, b->P, b->pstride, b->ld, S, b->pvar);
            AV_LAUNCH_CHECK();
            AV_HIP(hipMemcpyAsync(b->h_pv, b->pvar, sizeof(double) * 3 * S, hipMemcpyDeviceToHost, stm));
            if ((rc = b_wait(b, stm)) || (rc = b_chain_finish(b, proc, cx))) return rc;
            have_pv = true;
            // the two frames go (with them both observations of every candidate and the single ones of the other features), then the cameras
            par_streams(S, [&](int s) {
                if (!prune[s]) return;
                BStream& T = b->st[s];
                const int i0 = b_cam_index(T, rm[s][0]), i1 = b_cam_index(T, rm[s][1]);
                T.map.remove_frame(i1); T.map.remove_frame(i0);         // every observation taken from the two cameras goes with them
                T.cams.erase(T.cams.begin() + i1); T.cams.erase(T.cams.begin() + i0);
                T.n -= 12;
            });
        }
    }
    // ---- publish + online_reset (msckf.py:821-867) -----------------------------------------------------
    if (!have_pv) {
        hipLaunchKernelGGL(pos_var_kernel, dim3((3 * S + 255) / 256), dim3(256), 0, stm, b->P, b->pstride, b->ld, S, b->pvar);
        AV_LAUNCH_CHECK();
        AV_HIP(hipMemcpyAsync(b->h_pv, b->pvar, sizeof(double) * 3 * S, hipMemcpyDeviceToHost, stm));
        if ((rc = b_wait(b, stm))) return rc;
    }
    const double* pv = b->h_pv;
    for (int s = 0; s < S; ++s) {
        BStream& T = b->st[s];
        double* o = out + (size_t)s * 12;
        o[0] = T.failed ? -1.0 : (T.active ? 1.0 : 0.0); o[1] = T.ts;
        for (int i = 0; i < 3; ++i) { o[2 + i] = T.p[i]; o[9 + i] = T.v[i]; }
        for (int i = 0; i < 4; ++i) o[5 + i] = T.q[i];
        if (!T.active || b->pos_std_thr <= 0) continue;
        const double m = fmax(sqrt(pv[3 * s]), fmax(sqrt(pv[3 * s + 1]), sqrt(pv[3 * s + 2])));
        if (m < b->pos_std_thr) continue;
        T.cams.clear(); T.map.clear();
        if ((rc = b_reset_cov(b, s, stm))) return rc;
    }
    return AV_OK;
}

static int sub_get_cov(av_msckf_batch* b, int stream_idx, double* P_host, int n, void* stream)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !P_host) { av_set_error("av_msckf_batch_get_cov: bad arguments"); return AV_E_INVALID; }
    hipStream_t stm = (hipStream_t)stream;
    AV_HIP(hipSetDevice(b->device));
    int n_now = b->st[stream_idx].n;
    if (b->dev && b->dev->cap > 0) { DState D; int rcd = dev_read_state(b, stream_idx, &D); if (rcd) return rcd; n_now = D.n; }
    if (n != n_now) { av_set_error("av_msckf_batch_get_cov: n = %d, the stream's state has %d", n, n_now); return AV_E_INVALID; }
    AV_HIP(hipMemcpy2DAsync(P_host, sizeof(double) * n, b->P + (size_t)stream_idx * b->pstride, sizeof(double) * b->ld, sizeof(double) * n, n, hipMemcpyDeviceToHost, stm));
    { int rcw = b_wait(b, stm); if (rcw) return rcw; }
    return AV_OK;
}

// [n_state, n_cam, n_map] of one stream
static int sub_sizes(av_msckf_batch* b, int stream_idx, int32_t out3[3])
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !out3) { av_set_error("av_msckf_batch_sizes: bad arguments"); return AV_E_INVALID; }
    if (b->dev && b->dev->cap > 0) {
        DState D; int rcd = dev_read_state(b, stream_idx, &D); if (rcd) return rcd;
        int live = 0;
        AV_HIP(hipMemcpy(&live, b->dev->A.hdr + (size_t)stream_idx * AVS_HDR_WORDS + AVS_LIVE, sizeof(int), hipMemcpyDeviceToHost));
        out3[0] = D.n; out3[1] = D.ncam; out3[2] = live;
        return AV_OK;
    }
    out3[0] = b->st[stream_idx].n; out3[1] = (int)b->st[stream_idx].cams.size(); out3[2] = b->st[stream_idx].map.live;
    return AV_OK;
}

// Full state of one stream for parity tests (SURVEY 8b "get_state"): everything measurement_update injects into
// (msckf.py:576-595).  imu32 = [timestamp, q(4), p(3), v(3), gyro_bias(3), acc_bias(3), R_imu_cam0 (9, row-major), t_cam0_imu(3),
// gravity(3)]; camera states in window order: ids and [q(4), p(3)] each.  Call with no step in flight (after _wait(0)).
static int sub_get_state(av_msckf_batch* b, int stream_idx, double imu32[32], int64_t* cam_ids, double* cam_qp7, int cam_cap, int32_t* n_cam)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !imu32 || !n_cam || cam_cap < 0 || (cam_cap > 0 && (!cam_ids || !cam_qp7))) { av_set_error("av_msckf_batch_get_state: bad arguments"); return AV_E_INVALID; }
    if (b->dev && b->dev->cap > 0) {
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
        const DevArgs& A = b->dev->A;
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
    const BStream& T = b->st[stream_idx];
    double* o = imu32;
    *o++ = T.ts;
    for (int i = 0; i < 4; ++i) *o++ = T.q[i];
    for (int i = 0; i < 3; ++i) *o++ = T.p[i];
    for (int i = 0; i < 3; ++i) *o++ = T.v[i];
    for (int i = 0; i < 3; ++i) *o++ = T.bg[i];
    for (int i = 0; i < 3; ++i) *o++ = T.ba[i];
    for (int i = 0; i < 9; ++i) *o++ = T.R_ic[i];
    for (int i = 0; i < 3; ++i) *o++ = T.t_ci[i];
    for (int i = 0; i < 3; ++i) *o++ = T.gravity[i];
    *n_cam = (int32_t)T.cams.size();
    if ((int)T.cams.size() > cam_cap) { if (cam_cap == 0) return AV_OK; av_set_error("av_msckf_batch_get_state: %zu camera states > cam_cap %d", T.cams.size(), cam_cap); return AV_E_CAPACITY; }
    for (size_t k = 0; k < T.cams.size(); ++k) {
        cam_ids[k] = T.cams[k].id;
        for (int i = 0; i < 4; ++i) cam_qp7[7 * k + i] = T.cams[k].q[i];
        for (int i = 0; i < 3; ++i) cam_qp7[7 * k + 4 + i] = T.cams[k].p[i];
    }
    return AV_OK;
}

// 0 while the stream runs; the error code that stopped it otherwise (message copied to msg, NUL-terminated)
static int sub_stream_status(av_msckf_batch* b, int stream_idx, int32_t* status, char* msg, int msg_cap)
{
    if (!b || stream_idx < 0 || stream_idx >= b->S || !status) { av_set_error("av_msckf_batch_stream_status: bad arguments"); return AV_E_INVALID; }
    const BStream& T = b->st[stream_idx];
    if (b->dev && b->dev->cap > 0 && !T.failed) {
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
    tl_host_cap = g->host_cap;
    (void)hipSetDevice(g->device);
    std::deque<av_msckf_batch::Job> launched;                    // steps enqueued on the device whose results have not been collected
    const size_t depth = g->dev ? DEV_RING - 1 : 1;
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

int default_groups(int n_streams, bool host_store)
{
    const char* e = getenv("AV_MSCKF_GROUPS");
    // host-bookkeeping path: 4 groups overlap one group's host phases with the others' kernels.  Device-resident path: the groups only
    // add concurrency between two latency chains; more of them just compete (2,048 streams: 1 / 2 / 3 / 4 / 8 groups = 132 / 128-134 /
    // 121 / 101 / 80 k frames/s at the default priority)
    int g = e ? atoi(e) : (host_store ? (n_streams >= 256 ? 4 : (n_streams >= 64 ? 2 : 1)) : (n_streams >= 1024 ? 2 : 1));
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
    const char* store = getenv("AV_MSCKF_STORE");           // read once: the groups, their streams' priority and the filter's path follow it
    const bool host_store = store && !strcmp(store, "host");
    const int G = default_groups(n_streams, host_store);
    if (G == 1)
        return sub_create(n_streams, max_cam_states, rows_cap, chi2_table_100, gravity, T_cam0_cam1_rowmajor44, R_imu_cam0_t_cam0_imu12, cov_init5, noise4,
                          obs_noise, position_std_threshold, velocity0, opt6, device, host_store, out);
    av_msckf_batch* p = new (std::nothrow) av_msckf_batch(0);
    if (!p) { av_set_error("out of host memory"); return AV_E_INVALID; }
    p->device = p->res.device = device; p->S = n_streams; p->per_sub = (n_streams + G - 1) / G;
    // a group's workers sleep while its kernels run, so the groups together may hold twice the core budget
    const int share = 2 * host_thread_budget() / G < 1 ? 1 : 2 * host_thread_budget() / G;
    for (int s0 = 0; s0 < n_streams; s0 += p->per_sub) {
        const int cnt = n_streams - s0 < p->per_sub ? n_streams - s0 : p->per_sub;
        av_msckf_batch* g = nullptr;
        int rc = sub_create(cnt, max_cam_states, rows_cap, chi2_table_100, gravity, T_cam0_cam1_rowmajor44, R_imu_cam0_t_cam0_imu12, cov_init5, noise4,
                            obs_noise, position_std_threshold, velocity0, opt6, device, host_store, &g);
        if (rc == AV_OK) {
            // highest priority: the filter's kernels are short, latency-bound and on the step's critical path; the
            // front-end's throughput kernels (other streams) fill whatever they leave free
            rc = make_filter_stream(g->res, &g->own, host_store);
        }
        if (rc) { if (g) sub_destroy(g); av_msckf_batch_destroy(p); return rc; }
        g->host_cap = share;
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

// one group, no worker thread (device-resident path): collect launched steps until at most max_pending are outstanding
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

// buffers of the device-resident path for messages of `cap` features (first step, or a wider message: drains the group first)
int dev_prepare(av_msckf_batch* g, int cap)
{
    if (g->dev->cap >= cap && g->reserved_cap >= cap) return AV_OK;
    AV_HIP(hipSetDevice(g->device));
    int rc;
    const bool first = g->dev->cap == 0;
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
        if (!b->dev || b->direct_pending.empty()) return AV_OK;
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
        if (!b->dev) return sub_step(b, ids, uv, n_feat, cap, timestamps, out, stream);      // host bookkeeping, one group: nothing to decouple
        // device-resident, one group: the step is enqueued here and collected by av_msckf_batch_wait (the arrays are consumed before this returns)
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
        if (g->dev) {
            const StepOuts go = outs.at(b->out_set, s0);
            job.launch = [=] { return dev_launch(g, k, ids + s0 * cap, uv + s0 * cap * 4, n_feat + s0, cap, timestamps + s0, false, nullptr, g->own); };
            job.finish = [=] { return dev_finish(g, k, out + s0 * 12, go); };
        } else {
            job.launch = [=] { return sub_step(g, ids + s0 * cap, uv + s0 * cap * 4, n_feat + s0, cap, timestamps + s0, out + s0 * 12, g->own); };
        }
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
    for (av_msckf_batch* g : parts) if (!g->dev) { av_set_error("av_msckf_batch_submit_dev: the device-resident path is switched off (AV_MSCKF_STORE=host or a diagnostic switch)"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(b->device));
    int rc;
    bool need = false;
    for (av_msckf_batch* g : parts) if (g->dev->cap < cap) need = true;
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
        DevSlot& sl = g->dev->slot[k];
        const size_t Sg = (size_t)g->S, dc = (size_t)g->dev->cap;
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

// 1: the filter state and the observation map of this batch live on the device (msckf_dev.inc; av_msckf_batch_submit_dev is
// available), 0: host bookkeeping (AV_MSCKF_STORE=host or a diagnostic switch of that path)
AV_EXPORT int av_msckf_batch_device_resident(const av_msckf_batch* b)
{
    if (!b) { av_set_error("av_msckf_batch_device_resident: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) return b->dev ? 1 : 0;
    for (const av_msckf_batch* g : b->subs) if (!g->dev) return 0;
    return 1;
}

AV_EXPORT int av_msckf_batch_step(av_msckf_batch* b, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap,
                                  const double* timestamps, double* out, void* stream)
{
    if (!b || !ids || !uv || !n_feat || !timestamps || !out || cap <= 0) { av_set_error("av_msckf_batch_step: bad arguments"); return AV_E_INVALID; }
    if (b->subs.empty()) {
        if (b->dev) { AV_HIP(hipSetDevice(b->device)); int rc0 = direct_drain(b, 0); if (rc0) return rc0; }
        return sub_step(b, ids, uv, n_feat, cap, timestamps, out, stream);
    }
    // the caller's stream orders this step after whatever it enqueued before; the groups then run on their own streams
    AV_HIP(hipSetDevice(b->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    int rc = av_msckf_batch_submit(b, ids, uv, n_feat, cap, timestamps, out, stream);
    if (rc) return rc;
    return av_msckf_batch_wait(b, 0);
}

// The optional per-step outputs (OUTS, msckf_dev.inc; airvision.h: "Odometry covariance", "Landmark map", "Innovation statistics").
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

namespace {

// the body of av_msckf_batch_set_*: feature f gets `setting` on the batch and on every group (args_ok: the wrapper's own argument check)
int batch_set_out(av_msckf_batch* b, OutFeat f, int setting, bool args_ok = true)
{
    const OutWords& w = out_words(f);
    if (!b || !args_ok) { av_set_error("av_msckf_batch_set_%s: bad arguments", w.fn); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    if (setting) for (av_msckf_batch* g : parts) if (!g->dev) {
        av_set_error("av_msckf_batch_set_%s: %s %s the device-resident filter; this batch runs the host-bookkeeping path (AV_MSCKF_STORE=host)", w.fn, w.noun, w.needs);
        return AV_E_INVALID;
    }
    bool stepped = b->dev_seq > 0;
    for (av_msckf_batch* g : parts) if (g->n_steps > 0 || (g->dev && g->dev->cap > 0)) stepped = true;
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
        T.gravity_set = false; T.first_img = true; T.null_aliased = false; T.active = false;
        T.gravity_time = 0; T.next_imu_id = 0; T.imu_id = 0; T.has_imu_id = false; T.dev_init_sent = false;
        T.ts = 0; T.tracking_rate = 0; T.n = IMU_DIM;
        for (int i = 0; i < 4; ++i) { T.q[i] = i == 3 ? 1.0 : 0.0; T.qn[i] = i == 3 ? 1.0 : 0.0; }
        for (int i = 0; i < 3; ++i) { T.p[i] = 0; T.bg[i] = 0; T.ba[i] = 0; T.pn[i] = 0; T.vn[i] = 0; T.v[i] = g->vel0[i]; T.gravity[i] = g->gravity0[i]; T.t_ci[i] = g->t_ci0[i]; }
        for (int i = 0; i < 9; ++i) T.R_ic[i] = g->R_ic0[i];
        T.cams.clear(); T.map.clear();
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
    for (av_msckf_batch* g : parts) if (!g->dev) {
        av_set_error("av_msckf_batch_restart: the stream restart needs the device-resident filter; this batch runs the host-bookkeeping path (AV_MSCKF_STORE=host)");
        return AV_E_INVALID;
    }
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
        out6[0] += g->w_gate_flops; out6[1] += g->w_update_flops; out6[2] += g->w_qr_flops; out6[3] += (double)g->w_gated; out6[4] += (double)g->w_updates;
        out6[5] += (double)g->w_rows; out6[6] += g->w_chain_ms; out6[7] += (double)g->w_chain_dropped;
        if (g->dev && g->dev->cap > 0) {          // device-resident path: the counters are accumulated per stream by upd_stack_kernel
            std::vector<double> w((size_t)g->S * 8);
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(w.data(), g->dev->work, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
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
        if (g->dev && g->dev->cap > 0) {
            std::vector<double> w((size_t)g->S * 8);
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(w.data(), g->dev->work, sizeof(double) * w.size(), hipMemcpyDeviceToHost));
            for (int s = 0; s < g->S; ++s) { out2[0] += w[8 * s + 6]; out2[1] += w[8 * s + 7]; }
        }
    return AV_OK;
}

// [steps, stream-steps that ran the camera pruning, streams gated in two passes (reserved rows > rows_cap), DevBuf
//  reallocations after the first reserve, min / max camera states, min / max map features] over all streams
AV_EXPORT int av_msckf_batch_counters(av_msckf_batch* b, int64_t out8[8])
{
    if (!b || !out8) { av_set_error("av_msckf_batch_counters: bad arguments"); return AV_E_INVALID; }
    std::vector<av_msckf_batch*> parts = b->subs;
    if (parts.empty()) parts.push_back(b);
    long long steps = 0, prunes = 0, two = 0, grow = 0, cmin = 1 << 30, cmax = 0, mmin = 1 << 30, mmax = 0;
    for (av_msckf_batch* g : parts) {
        if (g->n_steps > steps) steps = g->n_steps;
        prunes += g->n_prune_stream_steps; two += g->n_two_pass_streams; grow += sub_growths(g);
        if (g->dev && g->dev->cap > 0) {
            std::vector<DState> st((size_t)g->S); std::vector<int> hdr((size_t)g->S * AVS_HDR_WORDS);
            AV_HIP(hipSetDevice(g->device));
            AV_HIP(hipMemcpy(st.data(), g->dev->A.st, sizeof(DState) * st.size(), hipMemcpyDeviceToHost));
            AV_HIP(hipMemcpy(hdr.data(), g->dev->A.hdr, sizeof(int) * hdr.size(), hipMemcpyDeviceToHost));
            grow += g->dev->growths;
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
        for (const BStream& T : g->st) {
            const long long c = (long long)T.cams.size(), m = T.map.live;
            if (c < cmin) cmin = c;
            if (c > cmax) cmax = c;
            if (m < mmin) mmin = m;
            if (m > mmax) mmax = m;
        }
    }
    out8[0] = steps; out8[1] = prunes; out8[2] = two; out8[3] = grow; out8[4] = cmin; out8[5] = cmax; out8[6] = mmin; out8[7] = mmax;
    return AV_OK;
}

// What the batch launched: out17[0] = stream groups (1 without sub-batches), then per group its stream count and the workgroup size
// dev_enqueue gave the per-stream kernels (dk_begin4 / dk_cov / dk_mid / dk_finish) in the group's last enqueued step: 64 or 256, 0
// before its first step and on the host-bookkeeping path.  Reported as recorded at the launch, never recomputed.  Drains the queue
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
        out17[2 + 2 * g] = parts[g]->dev ? parts[g]->dev->launched_wg : 0;
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
