// msckf_dev_host.inc -- host side of the device-resident batched filter (kernels: msckf_dev.inc; included by msckf_batch.inc).
//
// A step of a stream group = dev_launch (fills the slot's control records and IMU samples, enqueues the fixed launch sequence and
// the read-back of the published poses; never waits for the device) + dev_finish (waits for that read-back, hands the poses to
// the caller).  The group's worker keeps up to DEV_RING - 1 steps launched ahead of the one it is waiting for.
namespace {

constexpr int DEV_KCH = 136;       // stacked rows one back-end pass takes directly (74.6 KB of LDS for the factor: two workgroups per CU)
// ... and never more than ld: a pass of k rows keeps S, T^T and Y in [k][ld] buffers of ld * ld doubles, so with a window below 17 camera
// states (ld < 136) a stream that stacks more than ld rows is compressed to its nc < ld columns' worth first.  (Not closed by this: such a
// window's stream with ld < m <= 136 rows over nc columns, 2 m <= 3 nc, which upd_compress leaves uncompressed.)
inline int dev_kch(int ld) { return DEV_KCH < ld ? DEV_KCH : ld; }

// copy of the store of every stream into arrays built for a larger message capacity (a wider feature message arrived)
__global__ __launch_bounds__(256) void dk_migrate(DevArgs o, DevArgs n)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const AvsStore A = dev_store(o, s), B = dev_store(n, s);
    for (int i = tid; i < A.ns; i += 256) { B.fr_n[i] = A.fr_n[i]; B.pos_of[i] = A.pos_of[i]; B.order[i] = A.order[i]; }
    for (int i = tid; i < AVS_HDR_WORDS; i += 256) B.hdr[i] = A.hdr[i];
    if (tid == 0) *B.births = *A.births;
    for (int sl = 0; sl < A.ns; ++sl) {
        const int cnt = A.fr_n[sl];
        for (int i = tid; i < cnt; i += 256) {
            const size_t a = (size_t)sl * A.cap + i, b = (size_t)sl * B.cap + i;
            B.fr_id[b] = A.fr_id[a]; B.fr_fslot[b] = A.fr_fslot[a]; B.fr_prev[b] = A.fr_prev[a]; B.fr_next[b] = A.fr_next[a];
            for (int e = 0; e < 4; ++e) B.fr_z[4 * b + e] = A.fr_z[4 * a + e];
        }
    }
    for (int i = tid; i < A.mcap; i += 256) {
        B.m_id[i] = A.m_id[i]; B.m_birth[i] = A.m_birth[i]; B.m_init[i] = A.m_init[i]; B.m_nobs[i] = A.m_nobs[i]; B.m_tail[i] = A.m_tail[i]; B.free_stack[i] = A.free_stack[i];
        for (int e = 0; e < 3; ++e) B.m_pos[(size_t)3 * i + e] = A.m_pos[(size_t)3 * i + e];
    }
}

// Build (or rebuild for a larger capacity) everything whose size depends on the capacity of a feature message.
int dev_reserve(av_msckf_batch* b, int cap)
{
    DevPath* d = &b->dev;
    if (cap <= d->cap) return AV_OK;
    if (cap >= (1 << 24)) { av_set_error("batched MSCKF: message capacity %d exceeds the store's link format", cap); return AV_E_CAPACITY; }
    const bool grow = d->cap > 0;
    // a wider message after the first step: drain, build the larger arrays, carry the stores over (rare; counted in `growths`).
    // Grows geometrically so that a message that widens a little at a time does not rebuild every time.
    if (grow) { AV_HIP(hipDeviceSynchronize()); cap = cap > d->cap + d->cap / 2 ? cap : d->cap + d->cap / 2; ++d->growths; }
    int rc;
    const size_t S = (size_t)b->S, cs = (size_t)b->cam_slots;
    DevArgs old = d->A;
    DevArgs& A = d->A;
    { const char* e = getenv("AV_DK_WG"); const int v = e ? atoi(e) : 0; d->dk_wg = (v == 256 || v == 64) ? v : 0; }
    A.S = b->S; A.cap = cap; A.FS = cap + 1; A.cs = b->cam_slots; A.max_cam = b->max_cam; A.ld = b->ld; A.rows_cap = b->rows_cap; A.pool_rows = (int)b_pool_rows(b, b->rows_cap);
    A.obs_stride = (int)((size_t)cap * cs); A.pstride = b->pstride; A.P = b->P; A.scratch = b->scratch;
    A.mcap = 2 * cap + 64; A.ns = b->cam_slots + 1;
    int hc = 64; while (hc < 2 * cap + 16) hc *= 2;
    A.hcells = hc;
    if ((size_t)S * A.FS >= (1u << 31) || S * (size_t)A.obs_stride >= (1u << 31)) { av_set_error("batched MSCKF: %zu streams x %d features exceed the 32-bit feature index", S, cap); return AV_E_CAPACITY; }
    const size_t nf = S * (size_t)A.FS + 8, no = S * (size_t)A.obs_stride + 8, ne = S * (size_t)A.ns * cap, nm = S * (size_t)A.mcap;
#define DA(ptr, cnt) if ((rc = b->res.dev(&(ptr), (size_t)(cnt)))) return rc;
#define DAF(ptr, cnt, fill) if ((rc = b->res.dev(&(ptr), (size_t)(cnt), fill))) return rc;
    if (!grow) {
        DA(A.st, S) DA(A.cam_id, S * cs) DA(A.cam_q, S * cs * 4) DA(A.cam_p, S * cs * 3) DA(A.cam_qn, S * cs * 4) DA(A.ncam, S) DA(A.nstate, S) DA(A.grav, S * 3)
        DA(A.n_cand, S) DA(A.over, S) DA(A.cnt, 32) DA(d->out_d, S * 12) DA(d->cov_d, S) DA(d->stacked0, S) DA(d->stacked1, S) DA(d->updbase, S) DA(d->upd, S * 2)
        DA(d->cols, S * 6 * cs) DA(d->clist, S + 8) DA(d->work, S * 8)
        for (int i = 0; i < N_OUT; ++i) if (b->out_set[OUTS[i].feat]) DA(d->outs_d[i], S * OUTS[i].bytes(b->out_set))
        DA(d->rs_list_d, S) DA(d->rs_carry_d, S * 2)
        if (b->zupt_on) DA(d->zupt_d, S)                     // the zero-velocity records: zero, like their totals
        if ((rc = b->res.pinned(&d->rs_list_h, S)) || (rc = b->res.pinned(&d->rs_carry_h, S * 2))) return rc;
        DAF(A.pos_of, S * A.ns, 0xFF) DAF(A.order, S * A.ns, 0xFF) DA(A.fr_n, S * A.ns) DA(A.hdr, S * AVS_HDR_WORDS) DA(A.births, S)
    }
    DA(A.fr_id, ne) DA(A.fr_z, ne * 4) DA(A.fr_fslot, ne) DA(A.fr_prev, ne) DA(A.fr_next, ne)
    DA(A.m_id, nm) DA(A.m_birth, nm) DA(A.m_pos, nm * 3) DA(A.m_init, nm) DA(A.m_nobs, nm) DA(A.m_tail, nm) DA(A.free_stack, nm)
    DA(A.hash_a, S * hc) DA(A.hash_b, S * hc) DA(A.hash_c, S * hc)
    DA(A.tmp_a, S * cap) DA(A.tmp_b, S * cap) DA(A.tmp_c, S * cap) DA(A.keys, S * cap) DA(A.cand, S * cap) DA(A.e0, S * cap) DA(A.e1, S * cap)
    DA(A.f_off, nf) DA(A.obs_cam, no) DA(A.obs_z, no * 4) DA(A.f_pos, nf * 3) DA(A.f_dof, nf) DA(A.f_rowoff, nf) DA(A.f_valid, nf) DA(A.f_mslot, nf)
    DA(A.t_off, nf) DA(A.t_obs_cam, no) DA(A.t_obs_z, no * 4)
    DA(A.blist, 5 * S * cap + 8) DA(A.tlist, S * cap + 8) DA(d->blk_row, nf) DA(d->blk_len, nf) DA(d->again, nf) DA(d->gamma, nf) DA(d->pass, nf)
    for (int k = 0; k < DEV_RING; ++k) {
        DevSlot& sl = d->slot[k];
        if (!grow) {
            if ((rc = b->res.pinned(&sl.ctl_h, S)) || (rc = b->res.pinned(&sl.out_h, S * 12)) || (rc = b->res.pinned(&sl.cnt_h, 16))) return rc;
            DA(sl.ctl_d, S) DA(sl.n_d, S)
            if ((rc = b->res.pinned(&sl.n_h, S))) return rc;
            for (int i = 0; i < N_OUT; ++i) if (b->out_set[OUTS[i].feat] && (rc = b->res.pinned(&sl.outs_h[i], S * OUTS[i].bytes(b->out_set)))) return rc;
            if (b->out_set[F_FC]) { DA(sl.pend_d, S * 3) if ((rc = b->res.pinned(&sl.pend_h, S * 3))) return rc; }      // the forecast's (first, had, staged) per stream
            if ((rc = b->res.event(&sl.done, hipEventDisableTiming | hipEventBlockingSync))) return rc;
            for (int ph = 0; ph < 2; ++ph) if ((rc = b->res.event(&sl.t0[ph], hipEventDefault)) || (rc = b->res.event(&sl.t1[ph], hipEventDefault))) return rc;
        }
        DA(sl.ids_d, S * cap) DA(sl.uv_d, S * cap * 4)
        if ((rc = b->res.pinned(&sl.ids_h, S * cap)) || (rc = b->res.pinned(&sl.uv_h, S * cap * 4))) return rc;
    }
#undef DA
#undef DAF
    unpack_T01(b->T01, A.R01, A.t01);
    for (int i = 0; i < 4; ++i) A.noise[i] = b->noise[i];
    for (int i = 0; i < 5; ++i) A.cov0[i] = b->cov0[i];
    A.trans_thr = b->trans_thr; A.pos_std_thr = b->pos_std_thr;
    unpack_opt5(b->opt5, A);
    A.Hblk = b->Hblk; A.rblk = b->rblk; A.hstride = b->hstride; A.rstride = b->rstride; A.chi2 = b->chi2_dev; A.obs_noise = b->obs_noise;
    A.gamma = d->gamma; A.pass = d->pass; A.updbase = d->updbase; A.upd = d->upd; A.cols = d->cols; A.cols_stride = 6 * b->cam_slots;
    A.blk_row = d->blk_row; A.blk_len = d->blk_len; A.stacked_out = d->stacked1; A.work = d->work;
    A.stacked = nullptr; A.dx = b->dx; A.ctl = nullptr; A.imu = nullptr; A.prop = nullptr; A.cov = d->cov_d; A.msg_ids = nullptr; A.msg_uv = nullptr; A.msg_n = nullptr; A.msg_cap = cap; A.out = d->out_d;
    if (!grow) {
        std::vector<DState> st(S);
        for (size_t s = 0; s < S; ++s) {
            DState& D = st[s]; const BStream& T = b->st[s];
            memset(&D, 0, sizeof(D));
            D.q[3] = 1.0; D.qn[3] = 1.0; D.n = IMU_DIM; D.first_img = 1;
            for (int i = 0; i < 3; ++i) { D.v[i] = T.v[i]; D.t_ci[i] = T.t_ci[i]; D.gravity[i] = T.gravity[i]; }
            for (int i = 0; i < 9; ++i) D.R_ic[i] = T.R_ic[i];
        }
        AV_HIP(hipMemcpy(A.st, st.data(), sizeof(DState) * S, hipMemcpyHostToDevice));
        std::vector<int> n21(S, IMU_DIM);
        AV_HIP(hipMemcpy(A.nstate, n21.data(), sizeof(int) * S, hipMemcpyHostToDevice));
    } else {
        hipLaunchKernelGGL(dk_migrate, dim3((unsigned)S), dim3(256), 0, nullptr, old, A);
        AV_LAUNCH_CHECK();
        AV_HIP(hipDeviceSynchronize());          // (the outgrown arrays stay allocated until destroy: nothing frees inside a run)
    }
    d->cap = cap;
    return AV_OK;
}

// Diagnostic phase stamps (AV_DEV_FPROF, AV_DEV_UPROF): the first team or workgroup of a kernel writes clock ticks into a small device
// buffer, the host reads them back after every 16th launch, which synchronises the stream (timing runs only).  One instance per
// switch, built where it is first used: with the switch unset nothing is allocated and nothing ever waits.
struct DevStamps {
    unsigned long long* dev = nullptr;       // [32] on the device; NULL: the switch is unset
    int calls = 0;
    explicit DevStamps(bool on)
    {
        if (on && hipMalloc((void**)&dev, 256) == hipSuccess) { (void)hipMemset(dev, 0, 256); (void)hipStreamSynchronize(nullptr); } else dev = nullptr;
    }
    // call once behind every stamped launch; true: the stamps are in t (a read that fails prints nothing, the step's own checks report the error)
    bool read(hipStream_t stm, unsigned long long t[32])
    {
        return dev && (++calls & 15) == 0 && hipStreamSynchronize(stm) == hipSuccess && hipMemcpy(t, dev, 256, hipMemcpyDeviceToHost) == hipSuccess;
    }
};
// "[label, 10 ns ticks] name t[1]-t[0]  name t[2]-t[1] ..." on stderr
void print_stamps(const char* label, const unsigned long long* t, std::initializer_list<const char*> names)
{
    char line[512];
    int w = snprintf(line, sizeof(line), "[%s, 10 ns ticks]", label);
    const char* sep = " ";
    for (const char* nm : names) { w += snprintf(line + w, sizeof(line) - w, "%s%s %llu", sep, nm, t[1] - t[0]); ++t; sep = "  "; }
    fprintf(stderr, "%s\n", line);
}
DevStamps& dev_uprof() { static DevStamps st(getenv("AV_DEV_UPROF") != nullptr); return st; }                                  // the dk_* and update kernels, stream 0
DevStamps& dev_fprof_team() { static DevStamps st(getenv("AV_DEV_FPROF") != nullptr); return st; }                             // the pruning phase's feature kernel, team 0
DevStamps& dev_fprof_long() { static DevStamps st(getenv("AV_DEV_FPROF") && atoi(getenv("AV_DEV_FPROF")) == 2); return st; }   // the long-track bucket, workgroup 0

// per-stream constants of the update kernels (pointers into the group's work buffers); rebuilt when rows_cap changes
int dev_upload_updbase(av_msckf_batch* b)
{
    DevPath* d = &b->dev;
    std::vector<UpdArgs> base((size_t)b->S);
    for (int s = 0; s < b->S; ++s) {
        UpdArgs& u = base[s] = b_upd_args(b, s);
        u.n = IMU_DIM; u.mode = 1;
        if (s == 0) u.prof = dev_uprof().dev;
    }
    AV_HIP(hipMemcpy(d->updbase, base.data(), sizeof(UpdArgs) * base.size(), hipMemcpyHostToDevice));
    d->A.rows_cap = b->rows_cap; d->A.pool_rows = (int)b_pool_rows(b, b->rows_cap); d->A.Hblk = b->Hblk; d->A.rblk = b->rblk; d->A.hstride = b->hstride; d->A.rstride = b->rstride;
    return AV_OK;
}

int launch_feature_dev(FeatArgs a, int teams, int Mx, hipStream_t st)
{
    int rc0 = msckf_lds_opt_in();
    if (rc0) return rc0;
    a.Mmax = Mx; a.n_list = 0;
    // lanes per feature: two-observation features (the pruning phase) by teams of 8 (360 us per 2,048-stream launch; 16 lanes: 564, 4 lanes: 398
    // -- profiles/r04/README.md), tracks of up to four observations by one wavefront, longer ones by a workgroup
    // (tracks of up to 8 / 12 observations by one wavefront instead of a workgroup: 172.4-173.3 / 173.6 k against 174.0 k frames/s, round 5)
    const int team = Mx <= 2 ? 8 : (Mx <= 4 ? 64 : 256);
    const size_t per = (feature_lds_bytes(Mx, team) + 7) / 8 * 8;
    a.team_doubles = (int)(per / 8);
    // teams of a wavefront or less: ONE wavefront per workgroup.  Beside the front-end a 256-thread workgroup needs a free slot on all
    // four SIMDs of a CU at once; a single wavefront takes the first hole a retiring wavefront leaves (profiles/r05/README.md: the
    // kernels of the chain that are launched as single wavefronts run at their exclusive speed in the shared run, the others 2-5x slower)
    const int wg = team == 256 ? 256 : 64;
    const int tpb = wg / team;
    const size_t lds = per * tpb;
    if (lds > 160 * 1024) { av_set_error("MSCKF feature blocks: %d observations per feature need %zu B of LDS", Mx, lds); return AV_E_CAPACITY; }
    int blocks = (teams + tpb - 1) / tpb;
    if (blocks < 1) blocks = 1;
    if (blocks > 262144) blocks = 262144;
    if (team == 8) hipLaunchKernelGGL(feature_kernel8, dim3(blocks), dim3(wg), lds, st, a);
    else if (team == 64) hipLaunchKernelGGL(feature_kernel<64>, dim3(blocks), dim3(wg), lds, st, a);
    else hipLaunchKernelGGL(feature_kernel<256>, dim3(blocks), dim3(256), lds, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// teams to launch for a list whose length the device decides: what the last finished step needed plus a margin (the kernels stride
// over the list whatever the grid), the worst case before any step has finished
int dev_grid_hint(const DevPath* d, int idx, int worst, int floor_teams = 256)
{
    if (!d->have_hint) return worst < 1 ? 1 : worst;
    // A little above the last step's count, never below a small floor.  Idle workgroups are NOT free: each one is dispatched,
    // allocates its LDS (up to 69 KB in the long-track bucket) and queues for a CU beside the front-end's workgroups -- with a floor
    // of 16 teams per stream the five lost-feature buckets launched 16,384 workgroups each for ~2,000 features per group-step and
    // took 0.84 ms with the GPU to themselves, 3.9 ms in the shared path.  A step whose load jumps (every stream prunes at once, a
    // blank frame drops every track) strides over its lists with the previous step's grid once; the next step's grid follows.
    long long g = (long long)d->hint[idx] * 112 / 100 + 64;
    if (g < floor_teams) g = floor_teams;
    if (g > worst) g = worst;
    return g < 1 ? 1 : (int)g;
}

// The update's launches of a phase, in a phase's order: upd_stack_kernel (the stacking decisions), [upd_info_kernel: the information
// form, in the pruning phase], then -- where the phase can need the Cholesky back end -- upd_rowmap_kernel and the compression of the
// long streams, upd_gather_kernel and the five back-end kernels.  One place for the step (dev_phase) and for the parity-test entry
// av_msckf_update_ops_dev, so that the entry launches what the step launches.
struct UpdLaunch {
    bool info = false; size_t lds_info = 0;      // launch upd_info_kernel with this much dynamic LDS
    bool rounds = false;                         // launch the compression and the Cholesky back end
    unsigned n_list = 1;                         // workgroups that stride over the device-written list of long streams
    int k1max = 1, kmax = 1, nmax = 1;           // what the grids have to cover: bordered Gram size, rows a pass keeps, state dimension
};
int dev_launch_update(const StackArgs& sa, const UpdLaunch& ul, hipStream_t stm)
{
    int rc;
    const int S = sa.S;
    hipLaunchKernelGGL(upd_stack_kernel, dim3(S), dim3(64), 0, stm, sa);
    AV_LAUNCH_CHECK();
    // (no second feature pass: a stream whose candidates outgrow its region of the block buffers takes rows from the shared pool,
    //  dev_build_candidates -- the pass had to be launched every step and waited ~1.1 ms for a CU beside the front-end to do nothing)
    if ((rc = msckf_lds_opt_in())) return rc;
    if (ul.info) {
        if (ul.lds_info > 160 * 1024) { av_set_error("batched MSCKF: information-form update needs %zu B of LDS", ul.lds_info); return AV_E_CAPACITY; }
        hipLaunchKernelGGL(upd_info_kernel, dim3(S), dim3(256), ul.lds_info, stm, sa.out);
        unsigned long long t[32];
        if (dev_uprof().read(stm, t)) {                     // diagnostic (AV_DEV_UPROF=1): phase stamps of stream 0's workgroups
            print_stamps("dk_begin stream 0", t + 16, {"imu steps", "cross block", "augment+gap", "add frame", "select lost", "candidates", "triangulate", "erase"});
            print_stamps("upd_info stream 0", t, {"row map", "gram", "Pc", "F,G", "gauss-jordan", "scale", "P update"});
        }
    }
    if (ul.rounds) {
        hipLaunchKernelGGL(upd_rowmap_kernel, dim3(ul.n_list), dim3(64), 0, stm, sa.out, sa.clist, (const int*)sa.clist_count);
        launch_upd_compress(sa.out, sa.clist, (const int*)sa.clist_count, ul.n_list, ul.k1max, stm);
        hipLaunchKernelGGL(upd_gather_kernel, dim3(S), dim3(256), 0, stm, sa.out);
        // (the factor kernel: one launch for every pass length.  Two launches -- passes of up to 96 rows with 37 KB of LDS, four
        //  workgroups per CU, then the longer ones -- took 180 + 601 us against 659: most passes of a steady stream keep more than 96 rows)
        launch_upd_back(sa.out, S, ul.kmax, ul.nmax, stm);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// One update phase on the device: triangulate -> Jacobian / null space / gate (length buckets) -> stacking decisions -> [second
// pass of the streams gated without storage] -> compression of the long streams -> back end / information form.
// ph = 0: remove_lost_features (msckf.py:614-676), 1: prune_cam_state_buffer (:712-786).
int dev_phase(av_msckf_batch* b, int ph, hipStream_t stm, DevSlot& slot, int* cnt_step)
{
    DevPath* d = &b->dev;
    const DevArgs& A = d->A;
    const int S = b->S, cap = d->cap;
    const bool cut1500 = ph == 0;
    int* cnt = cnt_step + 8 * ph;
    int rc;
    if (b->work_timing) { AV_HIP(hipEventRecord(slot.t0[ph], stm)); slot.t_used[ph] = true; }
    const int worst = S * cap;
    if (ph == 1) {   // pruning phase, unfused form: triangulation of the listed features from the t_* CSR (= all their observations); the lost
                     // features' triangulation runs inside dk_begin
        TriArgs t = tri_args_base(A.cam_q, A.cam_p, b->cam_slots, b->T01, b->opt5);
        t.obs_off = A.t_off; t.obs_cam = A.t_obs_cam; t.obs_z = A.t_obs_z;
        t.out_pos = A.f_pos; t.out_valid = A.f_valid;
        t.list = A.tlist; t.n_list_dev = cnt + 5; t.fs_stride = A.FS;      // (n_feat and feat_stream stay 0: the list is the device's, the stream is f / fs_stride)
        t.f_mslot = A.f_mslot; t.meta_pos = A.m_pos; t.meta_init = A.m_init; t.meta_stride = A.mcap;
        int blocks = dev_grid_hint(d, 8 * ph + 5, worst);       // a wavefront per workgroup (launch_feature_dev has the reason)
        if (blocks > 262144) blocks = 262144;
        hipLaunchKernelGGL(triangulate_kernel, dim3(blocks), dim3(64), 0, stm, t);
        AV_LAUNCH_CHECK();
    }
    FeatArgs f = b_feat_args(b, cut1500, A.cam_q, A.cam_p, A.cam_qn);
    f.fs_stride = A.FS; f.stream_ncam = A.ncam; f.stream_gravity = A.grav;      // (n_feat and feat_stream stay 0: device-written lists, stream = f / fs_stride)
    f.obs_off = A.f_off; f.obs_cam = A.obs_cam; f.obs_z = A.obs_z; f.pos = A.f_pos; f.dof = A.f_dof; f.row_off = A.f_rowoff;
    f.gamma = d->gamma; f.pass = d->pass; f.valid = A.f_valid;
    // does this phase ever need the Cholesky back end?  If not (the pruning phase as a rule) its only reader is upd_info_kernel, which gathers
    // the 12 columns of the two cameras that go -- the columns every candidate writes: the rows are then stored compact, 12 doubles
    // each (480 contiguous bytes per feature instead of ten 48-byte pieces 1.2 KB apart, for the writer and for the reader)
    const bool rounds = ph == 0 || 5 * cap > INFO_MAXROWS;
    const int hld = rounds ? 0 : 12;
    f.compact = hld;
    if (ph == 0) {
        // length buckets (the LDS footprint grows with the square of the track length), one launch after the other on the group's own
        // stream.  Round 3 forked them onto four auxiliary streams; with ~2 lost features per stream and step the kernels are short
        // and what they waited for was their turn in a hardware queue shared with the front-end's stream (the 10+ HIP streams of a
        // process map onto 4 hardware queues: a bucket launched at 2.07 ms started at 4.77 ms behind an LK kernel) -- sequential
        // launches finish the phase in 1.3 ms instead of 3.0 and save twelve event calls per step.
        // (round 3's five buckets are two here -- tracks of up to 8 observations: 14 KB of LDS per workgroup; longer ones: 69 KB -- because
        // a steady frame loses ~2 features per stream: the launches, not the workgroups, are what the phase costs)
        const int edges[DEV_BUCKETS] = {8, b->cam_slots};
        for (int bk = 0; bk < DEV_BUCKETS; ++bk) {
            if (bk > 0 && edges[bk - 1] >= b->cam_slots) break;
            f.feat_list = A.blist + (size_t)bk * S * cap; f.n_list_dev = cnt + bk;
            const int Mx = edges[bk] < b->cam_slots ? edges[bk] : b->cam_slots;
            // diagnostic (AV_DEV_FPROF=2): phase stamps of the long-track bucket's first workgroup
            const bool stamped = bk == DEV_BUCKETS - 1 && dev_fprof_long().dev;
            f.prof = stamped ? dev_fprof_long().dev : nullptr;
            if ((rc = launch_feature_dev(f, dev_grid_hint(d, bk, worst), Mx < 5 ? 5 : Mx, stm))) return rc;
            unsigned long long t[32];
            if (stamped && dev_fprof_long().read(stm, t)) print_stamps("feature<256> workgroup 0", t, {"jacobian", "G", "reflectors", "rows out", "gate"});
            f.prof = nullptr;
        }
    } else {
        f.feat_list = A.blist; f.n_list_dev = cnt;           // every pruning candidate has exactly two observations: one bucket, 16-lane teams
        f.prof = dev_fprof_team().dev;                       // diagnostic (AV_DEV_FPROF=1): phase stamps of the grid's first team
        if ((rc = launch_feature_dev(f, dev_grid_hint(d, 8, worst), 2, stm))) return rc;
        unsigned long long t[32];
        if (dev_fprof_team().read(stm, t)) print_stamps("feature<16> team 0", t, {"jacobian", "G", "reflectors", "rows out", "gate"});
    }
    // ---- stacking decisions, then the update itself (dev_launch_update)
    StackArgs sa; memset(&sa, 0, sizeof(sa));
    sa.rbeg = nullptr; sa.n_cand = A.n_cand; sa.fs_stride = A.FS; sa.stream_n = A.nstate; sa.valid = A.f_valid;
    sa.pass = d->pass; sa.obs_off = A.f_off; sa.obs_cam = A.obs_cam; sa.row_off = A.f_rowoff;
    sa.blk_row = d->blk_row; sa.blk_len = d->blk_len; sa.cols = d->cols; sa.cols_stride = 6 * b->cam_slots;
    sa.base = d->updbase; sa.out = d->upd; sa.S = S; sa.rounds = 1; sa.cut1500 = cut1500 ? 1 : 0; sa.kch = dev_kch(b->ld); sa.stacked = ph == 0 ? d->stacked0 : d->stacked1;
    sa.over = A.over; sa.row_off_w = A.f_rowoff; sa.again_list = d->again; sa.again_count = cnt + 7;
    sa.clist = d->clist; sa.clist_count = cnt + 6; sa.work = d->work;
    sa.hld = hld;
    sa.no_info = ph == 0 ? 1 : 0;           // lost features: seen from many cameras as a rule; the few-column streams of the first frames take the same back end
    UpdLaunch ul;
    ul.info = ph == 1;
    if (ul.info) {
        const int minfo = 5 * cap < INFO_MAXROWS ? 5 * cap : INFO_MAXROWS;
        ul.lds_info = upd_info_lds(12, b->ld, minfo);
    }
    ul.rounds = rounds;
    // workgroups stride over the device-written list of long streams, sized from the last step's list length
    ul.n_list = (unsigned)dev_grid_hint(d, 8 * ph + 6, S, 32);
    ul.k1max = 6 * b->cam_slots + 1;
    // rows a pass keeps: a direct stream its m <= DEV_KCH stacked rows, a compressed one its n_c <= 6 max_cam columns' worth
    ul.kmax = DEV_KCH > 6 * b->max_cam ? DEV_KCH : 6 * b->max_cam;
    ul.nmax = b->ld;
    if ((rc = dev_launch_update(sa, ul, stm))) return rc;
    AV_LAUNCH_CHECK();
    if (slot.t_used[ph]) AV_HIP(hipEventRecord(slot.t1[ph], stm));
    return AV_OK;
}

// parity-test tap (av_msckf_batch_debug_*): what the phase that has just run computed, read back synchronously
int dev_debug_capture(av_msckf_batch* b, int ph, hipStream_t stm)
{
    DevPath* d = &b->dev;
    const DevArgs& A = d->A;
    const int S = b->S;
    AV_HIP(hipStreamSynchronize(stm));
    const size_t nf = (size_t)S * A.FS + 1;
    std::vector<int> n_cand(S), off(nf), valid(nf), pass(nf), stacked(S), nstate(S);
    std::vector<double> gamma(nf), dx((size_t)S * b->ld);
    AV_HIP(hipMemcpy(n_cand.data(), A.n_cand, sizeof(int) * S, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(off.data(), A.f_off, sizeof(int) * nf, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(valid.data(), A.f_valid, sizeof(int) * nf, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(pass.data(), d->pass, sizeof(int) * nf, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(gamma.data(), d->gamma, sizeof(double) * nf, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(stacked.data(), ph == 0 ? d->stacked0 : d->stacked1, sizeof(int) * S, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(nstate.data(), A.nstate, sizeof(int) * S, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(dx.data(), b->dx, sizeof(double) * S * b->ld, hipMemcpyDeviceToHost));
    for (int s = 0; s < S; ++s) {
        BStream& T = b->st[s];
        // gating values of the candidates the reference would have evaluated: in map order, features whose triangulation failed are
        // deleted before the gate (msckf.py:634-637), and the loop stops once more than 1500 rows are stacked (:667-668)
        int acc = 0;
        for (int k = 0; k < n_cand[s]; ++k) {
            const size_t f = (size_t)s * A.FS + k;
            if (!valid[f]) continue;
            T.dbg_gamma[ph].push_back(gamma[f]);
            if (pass[f]) acc += 4 * (off[f + 1] - off[f]) - 3;
            if (ph == 0 && acc > 1500) break;
        }
        if (stacked[s] > 0) {
            const int n = nstate[s];
            T.dbg_rows[ph] = stacked[s]; T.dbg_n[ph] = n;
            T.dbg_dx[ph].assign(dx.data() + (size_t)s * b->ld, dx.data() + (size_t)s * b->ld + n);
            T.dbg_P[ph].resize((size_t)n * n);
            AV_HIP(hipMemcpy2D(T.dbg_P[ph].data(), sizeof(double) * n, b->P + (size_t)s * b->pstride, sizeof(double) * b->ld, sizeof(double) * n, n, hipMemcpyDeviceToHost));
        }
    }
    return AV_OK;
}

int dev_enqueue(av_msckf_batch* b, int k, bool dev_msg, size_t n_imu, hipStream_t stm);

// feature_callback for every stream of the group (msckf.py:177-228), device-resident form: enqueue only.
// ids / uv / n_feat: host arrays (dev_msg = false: copied through the slot's pinned staging) or the slot's device buffers already
// filled by the caller's stream (dev_msg = true; `ready` orders this step behind that copy).
int dev_launch(av_msckf_batch* b, int k, const int64_t* ids, const double* uv, const int32_t* n_feat, int cap, const double* timestamps,
               bool dev_msg, hipEvent_t ready, hipStream_t stm)
{
    DevPath* d = &b->dev;
    const int S = b->S;
    AV_HIP(hipSetDevice(b->device));
    int rc;
    if ((rc = sub_reserve(b, cap))) return rc;               // block buffers (rows_cap) of the update kernels
    const bool first = d->cap == 0;
    const int rows_cap_before = d->A.rows_cap;
    if ((rc = dev_reserve(b, cap))) return rc;
    if (first || rows_cap_before != b->rows_cap) { if ((rc = dev_upload_updbase(b))) return rc; }
    DevSlot& sl = d->slot[k];
    if (sl.in_flight) { av_set_error("batched MSCKF: ring slot %d is still in flight", k); return AV_E_INVALID; }
    ++b->n_steps;
    if (b->debug_capture) for (BStream& T : b->st) for (int ph = 0; ph < 2; ++ph) { T.dbg_gamma[ph].clear(); T.dbg_dx[ph].clear(); T.dbg_P[ph].clear(); T.dbg_rows[ph] = 0; T.dbg_n[ph] = 0; }
    // ---- control records + IMU samples of this frame (batch_imu_processing's selection, msckf.py:251-273; the arithmetic is on the device)
    size_t n_imu = 0;
    const size_t fc_cap = (size_t)b->out_set[F_FC];
    for (int s = 0; s < S; ++s) {
        BStream& T = b->st[s];
        std::lock_guard<std::mutex> g(T.mu);
        // msckf.py:182-183 under the deterministic replay of SURVEY 3.5: live for this frame iff the sample that completed the gravity
        // initialisation is not newer than the frame; timestamps[s] < 0 (or NaN): no frame for this stream in this step
        T.active = !T.failed && T.gravity_set && timestamps[s] >= 0 && T.gravity_time <= timestamps[s];
        if (!T.active) continue;
        const double t0 = T.first_img ? timestamps[s] : T.ts;
        size_t pending = 0;            // forecast: the samples beyond the frame time ride behind the stream's own, the first fc_cap of them
        for (const BImu& m : T.imu) { if (m.t < t0) continue; if (m.t > timestamps[s]) { if (!fc_cap || ++pending >= fc_cap) break; continue; } ++n_imu; }
        n_imu += pending;
    }
    if (n_imu > sl.imu_cap) {          // (sized generously at the first step; grows if a frame ever spans more IMU samples)
        // forecast on: room for every stream's full share of pending samples from the start, so that a caller who pushes further ahead later
        // does not make the staging grow
        const size_t ncap = n_imu + n_imu / 2 + (size_t)S * 16 + 64 + (size_t)S * fc_cap;
        if (sl.imu_cap) { AV_HIP(hipStreamSynchronize(stm)); ++d->growths; }
        if ((rc = b->res.pinned(&sl.imu_h, ncap)) || (rc = b->res.dev(&sl.imu_d, ncap)) || (rc = b->res.dev(&sl.prop_d, ncap))) return rc;
        sl.imu_cap = ncap;
    }
    size_t w = 0;
    for (int s = 0; s < S; ++s) {
        BStream& T = b->st[s];
        DCtl& C = sl.ctl_h[s];
        C.t_frame = timestamps[s]; C.active = T.active ? 1 : 0; C.has_init = 0; C.imu_first = (int)w; C.imu_cnt = 0;
        if (fc_cap) { sl.pend_h[3 * s] = (int)w; sl.pend_h[3 * s + 1] = 0; sl.pend_h[3 * s + 2] = 0; }
        if (!T.active) continue;
        std::lock_guard<std::mutex> g(T.mu);
        if (!T.dev_init_sent) {            // first live frame of the stream: hand the device what initialize_gravity_and_bias computed (msckf.py:230-249)
            T.dev_init_sent = true; C.has_init = 1;
            for (int i = 0; i < 4; ++i) C.q0[i] = T.q[i];
            for (int i = 0; i < 3; ++i) { C.bg0[i] = T.bg[i]; C.g0[i] = T.gravity[i]; }
        }
        if (T.first_img) { T.first_img = false; T.ts = timestamps[s]; }
        size_t used = 0;
        for (const BImu& m : T.imu) {
            if (m.t < T.ts) { ++used; continue; }
            if (m.t > timestamps[s] || w >= sl.imu_cap) break;
            DImu& o = sl.imu_h[w++];
            o.t = m.t;
            for (int i = 0; i < 3; ++i) { o.w[i] = m.w[i]; o.a[i] = m.a[i]; }
            ++C.imu_cnt; ++used;
            T.ts = m.t;
        }
        T.imu.erase(T.imu.begin(), T.imu.begin() + used);
        if (fc_cap) {
            // Forecast: what is left has t > the frame time -- the pending samples, in push order.  They STAY in the buffer (the next step
            // consumes them as it always would); the first min(had, cap) of them are staged behind the stream's own samples.
            sl.pend_h[3 * s] = (int)w;
            const size_t had = T.imu.size();
            size_t staged = 0;
            for (; staged < had && staged < fc_cap && w < sl.imu_cap; ++staged) {
                const BImu& m = T.imu[staged];
                DImu& o = sl.imu_h[w++];
                o.t = m.t;
                for (int i = 0; i < 3; ++i) { o.w[i] = m.w[i]; o.a[i] = m.a[i]; }
            }
            // (staged < min(had, cap) only if samples were pushed between the sizing pass above and this one, past the staging's slack: the
            //  device integrates what was staged and the count pair says so)
            sl.pend_h[3 * s + 1] = (int)(had < (size_t)INT32_MAX ? had : (size_t)INT32_MAX); sl.pend_h[3 * s + 2] = (int)staged;
        }
    }
    // ---- the feature message (host arrays: through the slot's pinned staging)
    if (!dev_msg) {
        for (int s = 0; s < S; ++s) {
            const int nk = n_feat[s] < 0 ? 0 : (n_feat[s] > cap ? cap : n_feat[s]);
            sl.n_h[s] = nk;
            memcpy(sl.ids_h + (size_t)s * d->cap, ids + (size_t)s * cap, sizeof(long long) * nk);
            memcpy(sl.uv_h + (size_t)s * d->cap * 4, uv + (size_t)s * cap * 4, sizeof(double) * 4 * nk);
        }
    }
    if (dev_msg && ready) AV_HIP(hipStreamWaitEvent(stm, ready, 0));
    // d->steps selects the list-counter set (dev_enqueue: the step being enqueued is number d->steps + 1); it moves on only once the
    // step is enqueued.  A step that failed half-way may have run dk_begin (which zeroes the OTHER set) or not: neither set can be
    // trusted then, both are cleared behind whatever was enqueued.
    if ((rc = dev_enqueue(b, k, dev_msg, w, stm))) { (void)hipMemsetAsync(d->A.cnt, 0, sizeof(int) * 32, stm); return rc; }
    ++d->steps;
    AV_HIP(hipEventRecord(sl.done, stm));
    sl.in_flight = true;
    return AV_OK;
}

// The prediction's launches of a step, in a step's order: dk_state, [dk_imu_rate: the IMU-rate odometry, when it is on], [dk_begin4: the
// frame's observations, independent of the covariance], dk_cov<dk_wg>.  One place for the step (dev_enqueue, append = true) and for the parity-test entry av_msckf_predict_ops_dev (append =
// false: it has no observation store), so that the entry launches what the step launches.
// ir.rec set (av_msckf_batch_set_imu_rate): dk_imu_rate behind dk_state, one wavefront per stream whatever dk_wg is.
void dev_launch_predict(const DevArgs& a, int S, int dk_wg, bool append, hipStream_t stm, const IrOut& ir = IrOut{})
{
    hipLaunchKernelGGL(dk_state, dim3((S + 63) / 64), dim3(64), 0, stm, a);     // state integration + the new camera state: a lane per stream
    if (ir.rec) hipLaunchKernelGGL(dk_imu_rate, dim3(S), dim3(64), 0, stm, a, ir);      // the IMU-rate records, from what dk_state left for dk_cov
    if (append) hipLaunchKernelGGL(dk_begin4, dim3(S), dim3(dk_wg), 0, stm, a);
    if (dk_wg == 64) hipLaunchKernelGGL(dk_cov<64>, dim3(S), dim3(64), 0, stm, a);          // the covariance half of the prediction and of the augmentation
    else hipLaunchKernelGGL(dk_cov<256>, dim3(S), dim3(256), 0, stm, a);
}

// The forecast's launches (av_msckf_batch_set_forecast), behind the step's last per-stream kernel: the state chain a lane per stream, then
// the covariance, the records and the counts one wavefront per stream whatever shape the step's other kernels take.  One place for the
// step (dev_enqueue) and for the parity-test entry av_msckf_forecast_ops_dev.  a.imu / a.prop hold the pending samples and the room for
// their records at fc.pend[s] = (first, had, staged): staged <= min(had, fc.cap) samples lie at a.imu[first ..].
void dev_launch_forecast(const DevArgs& a, int S, const FcOut& fc, hipStream_t stm)
{
    hipLaunchKernelGGL(dk_forecast_state, dim3((S + 63) / 64), dim3(64), 0, stm, a, fc);
    hipLaunchKernelGGL(dk_forecast_cov, dim3(S), dim3(64), 0, stm, a, fc);
}

// The zero-velocity update's two launches (av_msckf_batch_set_zupt), one wavefront per stream whatever shape the step's other kernels take:
// the detector behind the prediction's launches and ahead of the lost-feature phase, the update behind the step's last per-stream kernel
// and ahead of the forecast.  One place for the step (dev_enqueue) and, the update's, for the parity-test entry av_msckf_zupt_ops_dev.
// The update stages Y and delta_x in 4 ld doubles of dynamic LDS.
ZuArgs dev_zu_args(const av_zupt_params& p, DZupt* rec)
{
    return ZuArgs{rec, p.gyro_max, p.acc_dev_max, p.disparity_max, p.velocity_sigma, p.gate, p.min_tracks, p.still_percent};
}
void dev_launch_zupt_detect(const DevArgs& a, int S, const ZuArgs& z, hipStream_t stm)
{
    hipLaunchKernelGGL(dk_zupt_detect, dim3(S), dim3(64), 0, stm, a, z);
}
void dev_launch_zupt_update(const DevArgs& a, int S, const ZuArgs& z, hipStream_t stm)
{
    hipLaunchKernelGGL(dk_zupt_update, dim3(S), dim3(64), sizeof(double) * 4 * (size_t)a.ld, stm, a, z);
}

// The named instances of dk_mid and dk_finish (profiles/filter_stats/README.md has why they are named instances), by the outputs that
// are on: the same launches as with all off, the instance also writes those outputs' records and the step reads them back.  Every
// instance's parameter list is DevArgs, then the ordered subset of (double* odom, LmOut, DUpdStats*) of its set bits: the order
// dev_launch_outs pushes the arguments in.
const void* const dk_mid_kernels[2][2] = {        // [landmarks][statistics]
    {(const void*)dk_mid, (const void*)dk_mid_st}, {(const void*)dk_mid_lm, (const void*)dk_mid_lm_st}};
const void* const dk_finish_kernels[2][2][2] = {  // [covariance][landmarks][statistics]
    {{(const void*)dk_finish, (const void*)dk_finish_st}, {(const void*)dk_finish_lm, (const void*)dk_finish_lm_st}},
    {{(const void*)dk_finish_cov, (const void*)dk_finish_cov_st}, {(const void*)dk_finish_cov_lm, (const void*)dk_finish_cov_lm_st}}};
static_assert(std::is_same<decltype(&dk_mid_lm_st), void (*)(DevArgs, LmOut, DUpdStats*)>::value &&
              std::is_same<decltype(&dk_finish_cov_lm_st), void (*)(DevArgs, double*, LmOut, DUpdStats*)>::value, "dev_launch_outs: covariance, landmarks, statistics");
KOuts dev_kouts(const av_msckf_batch* b)          // the one place that gives the table's device arrays their types
{
    char* const* p = b->dev.outs_d;
    return {(double*)p[O_COV], LmOut{(DLandmark*)p[O_LM], (int*)p[O_LMN], b->out_set[F_LM]}, (DUpdStats*)p[O_STATS],
            IrOut{(DImuState*)p[O_IR], (int*)p[O_IRN], b->out_set[F_IR]},
            FcOut{(DImuState*)p[O_FC], (int*)p[O_FCN], (double*)p[O_FCC], b->out_set[F_FC], nullptr}};
}
int dev_launch_outs(bool finish, const av_msckf_batch* b, DevArgs& a, int wg, hipStream_t stm)
{
    KOuts o = dev_kouts(b);
    const bool cov = finish && o.odom, lm = o.lm.rec, stats = o.stats;      // (dk_mid writes no covariance record)
    const void* kernel = finish ? dk_finish_kernels[cov][lm][stats] : dk_mid_kernels[lm][stats];
    void* args[4] = {&a}; int n = 1;
    if (cov) args[n++] = &o.odom;
    if (lm) args[n++] = &o.lm;
    if (stats) args[n++] = &o.stats;
    AV_HIP(hipLaunchKernel(kernel, dim3(b->S), dim3(wg), args, 0, stm));
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// the device side of one step on slot k: uploads of the slot's staging, the kernels, the read-back of the poses (no waits, no
// host decisions: the sequence is the same every step, which is what lets it be captured as a graph)
int dev_enqueue(av_msckf_batch* b, int k, bool dev_msg, size_t n_imu, hipStream_t stm)
{
    DevPath* d = &b->dev;
    DevSlot& sl = d->slot[k];
    const int S = b->S;
    int rc;
    AV_HIP(hipMemcpyAsync(sl.ctl_d, sl.ctl_h, sizeof(DCtl) * S, hipMemcpyHostToDevice, stm));
    if (n_imu) AV_HIP(hipMemcpyAsync(sl.imu_d, sl.imu_h, sizeof(DImu) * n_imu, hipMemcpyHostToDevice, stm));      // (forecast on: the pending samples ride in the same upload)
    if (sl.pend_d) AV_HIP(hipMemcpyAsync(sl.pend_d, sl.pend_h, sizeof(int) * 3 * S, hipMemcpyHostToDevice, stm));
    if (!dev_msg) {
        AV_HIP(hipMemcpyAsync(sl.n_d, sl.n_h, sizeof(int) * S, hipMemcpyHostToDevice, stm));
        AV_HIP(hipMemcpyAsync(sl.ids_d, sl.ids_h, sizeof(long long) * S * d->cap, hipMemcpyHostToDevice, stm));
        AV_HIP(hipMemcpyAsync(sl.uv_d, sl.uv_h, sizeof(double) * 4 * S * d->cap, hipMemcpyHostToDevice, stm));
    }
    DevArgs a = d->A;
    a.ctl = sl.ctl_d; a.imu = sl.imu_d; a.prop = sl.prop_d; a.msg_ids = sl.ids_d; a.msg_uv = sl.uv_d; a.msg_n = sl.n_d; a.msg_cap = d->cap;
    // list counters: two sets, used by alternate steps (a step's first kernel zeroes the other set for the step after it)
    const int par = (int)((d->steps + 1) & 1);
    a.cnt = d->A.cnt + 16 * par; a.cnt_next = d->A.cnt + 16 * (par ^ 1);
    a.prof = dev_uprof().dev ? dev_uprof().dev + 16 : nullptr;
    // Launch shapes of the per-stream kernels.  S is the stream count of THIS GROUP, not of the batch (a batch of 1,024 streams is two
    // groups of 512: four wavefronts; 2,047 is 1,024 + 1,023: one group of each; av_msckf_batch_launch_shape reports what was launched).
    // From 1,024 streams of the group up ONE wavefront per stream: their phases are chains of short memory
    // round trips, and beside the front-end a 256-thread workgroup waits for a free slot on all four SIMDs of a CU at once (a 0.25-ms
    // kernel took 1.5 ms in the shared run: profiles/r05/README.md).  Below that the GPU is not full and what counts is the time ONE
    // stream takes: four wavefronts (one stream 0.59 against 0.78 ms per frame, 256 streams x 1,500 features 36 against 29 k frames/s).
    const int dk_wg = d->dk_wg ? d->dk_wg : (S >= 1024 ? 64 : 256);       // (AV_DK_WG=64|256 forces one: A/B runs, and the parity tests of the shape small groups do not take)
    d->launched_wg = dk_wg;
    dev_launch_predict(a, S, dk_wg, true, stm, dev_kouts(b).ir);
    AV_LAUNCH_CHECK();
    if (d->zupt_d) { dev_launch_zupt_detect(a, S, dev_zu_args(b->zupt, d->zupt_d), stm); AV_LAUNCH_CHECK(); }
    if ((rc = dev_phase(b, 0, stm, sl, a.cnt))) return rc;
    if (b->debug_capture && (rc = dev_debug_capture(b, 0, stm))) return rc;
    a.stacked = d->stacked0;
    // (the whole pruning phase of a stream as ONE workgroup -- five launches fewer -- was built and measured in round 4: 141.3 k against
    //  144.4 k frames/s, 5.5 against 5.0 ms of exclusive chain: a stream's ~150 candidates walk through the 16 teams of one workgroup
    //  instead of spreading over the chip.  Removed in round 5; profiles/r04/README.md keeps the numbers.)
    if ((rc = dev_launch_outs(false, b, a, dk_wg, stm))) return rc;
    if ((rc = dev_phase(b, 1, stm, sl, a.cnt))) return rc;
    if (b->debug_capture && (rc = dev_debug_capture(b, 1, stm))) return rc;
    a.stacked = d->stacked1;
    if ((rc = dev_launch_outs(true, b, a, dk_wg, stm))) return rc;
    if (d->zupt_d) { dev_launch_zupt_update(a, S, dev_zu_args(b->zupt, d->zupt_d), stm); AV_LAUNCH_CHECK(); }      // on the state the step leaves: the forecast starts from the corrected one
    if (sl.pend_d) {
        FcOut fc = dev_kouts(b).fc; fc.pend = sl.pend_d;
        dev_launch_forecast(a, S, fc, stm);
        AV_LAUNCH_CHECK();
    }
    AV_HIP(hipMemcpyAsync(sl.out_h, d->out_d, sizeof(double) * 12 * S, hipMemcpyDeviceToHost, stm));
    for (int i = 0; i < N_OUT; ++i) if (d->outs_d[i]) AV_HIP(hipMemcpyAsync(sl.outs_h[i], d->outs_d[i], OUTS[i].bytes(b->out_set) * S, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipMemcpyAsync(sl.cnt_h, a.cnt, sizeof(int) * 16, hipMemcpyDeviceToHost, stm));
    return AV_OK;
}

// wait for the step queued on slot k and hand its published poses to the caller (outs: where the step's optional outputs go, S times
// the entry's bytes per stream each; NULL: the step has no destination for that array and it is dropped)
int dev_finish(av_msckf_batch* b, int k, double* out, const StepOuts& outs)
{
    DevPath* d = &b->dev;
    DevSlot& sl = d->slot[k];
    if (!sl.in_flight) return AV_OK;
    AV_HIP(hipEventSynchronize(sl.done));
    sl.in_flight = false;
    memcpy(out, sl.out_h, sizeof(double) * 12 * b->S);
    for (int i = 0; i < N_OUT; ++i) if (outs.p[i] && sl.outs_h[i]) memcpy(outs.p[i], sl.outs_h[i], OUTS[i].bytes(b->out_set) * b->S);
    for (int i = 0; i < 16; ++i) d->hint[i] = sl.cnt_h[i];
    d->have_hint = true;
    for (int ph = 0; ph < 2; ++ph) if (sl.t_used[ph]) {       // the whole step has retired: both phases' event pairs of this slot are complete
        float ms = 0;
        if (hipEventElapsedTime(&ms, sl.t0[ph], sl.t1[ph]) == hipSuccess) b->w_chain_ms += ms; else ++b->w_chain_dropped;
        sl.t_used[ph] = false;
    }
    return AV_OK;
}

// Stream restart, device side: dk_restart over the n distinct streams of `list` (local indices, checked by the caller) on `stm`, then
// the counters those streams held, added to the group's own so that av_msckf_batch_counters keeps accumulating.  The caller has drained
// the group; the call returns when the kernel has run, so any later step or read-back, on whatever stream, finds the new state.
int dev_restart(av_msckf_batch* b, const int* list, int n, hipStream_t stm)
{
    DevPath* d = &b->dev;
    if (n <= 0 || d->cap == 0) return AV_OK;                 // before the first step there is no device state: the host's reset is all
    AV_HIP(hipSetDevice(b->device));
    memcpy(d->rs_list_h, list, sizeof(int) * (size_t)n);
    AV_HIP(hipMemcpyAsync(d->rs_list_d, d->rs_list_h, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, stm));
    DRestart r; memset(&r, 0, sizeof(r));
    r.list = d->rs_list_d; r.carry = d->rs_carry_d;
    for (int i = 0; i < 3; ++i) { r.v0[i] = b->vel0[i]; r.t_ci[i] = b->t_ci0[i]; r.gravity[i] = b->gravity0[i]; }
    for (int i = 0; i < 9; ++i) r.R_ic[i] = b->R_ic0[i];
    const KOuts o = dev_kouts(b);
    r.odom = o.odom; r.lm = o.lm; r.stats = o.stats; r.ir = o.ir; r.fc = o.fc; r.zupt = d->zupt_d;
    hipLaunchKernelGGL(dk_restart, dim3((unsigned)n), dim3(256), 0, stm, d->A, r);
    AV_LAUNCH_CHECK();
    AV_HIP(hipMemcpyAsync(d->rs_carry_h, d->rs_carry_d, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, stm));
    AV_HIP(hipStreamSynchronize(stm));
    for (int i = 0; i < n; ++i) { b->n_prune_stream_steps += d->rs_carry_h[2 * i]; b->n_two_pass_streams += d->rs_carry_h[2 * i + 1]; }
    return AV_OK;
}

const char* dev_fail_message(int code, int* av_code)
{
    *av_code = code == DFAIL_PIVOT ? AV_E_NUMERIC : AV_E_CAPACITY;
    switch (code) {
    case DFAIL_CAMS: return "stream exceeds the camera-state slots of its window";
    case DFAIL_FRAMES: return "more frames in the stream's window than the observation store holds (or a message wider than its capacity)";
    case DFAIL_STACK: return "stream stacks more blocks in one update than the back end holds (4096 blocks / the compression stage's row maps)";
    case DFAIL_PIVOT: return "a Cholesky factorisation of the stacked update met a non-positive or non-finite pivot (rank-deficient Gram matrix or corrupt covariance); update skipped, stream stopped";
    case DFAIL_TABLE: return "the stream's feature table is full";
    case DFAIL_ROWS: return "the lost features of one frame need more rows than the stream's block buffers and the shared overflow pool hold (AV_MSCKF_POOL_ROWS)";
    default: return "stream stopped";
    }
}

// read-only accessors of the resident state (call with no step in flight)
int dev_read_state(av_msckf_batch* b, int s, DState* D)
{
    AV_HIP(hipSetDevice(b->device));
    AV_HIP(hipMemcpy(D, b->dev.A.st + s, sizeof(DState), hipMemcpyDeviceToHost));
    return AV_OK;
}

}  // namespace
