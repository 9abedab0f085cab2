// msckf_mfma.inc -- the products of the batched update's back end on the fp64 matrix instruction (included by msckf.hip).
//
//   T^T = P[:, cols] H_thin^T        upd_tt_mfma_kernel       msckf.py:559-566 (K = P H^T S^-1 via the factor of S)
//   S   = H_thin P_cc H_thin^T + s^2 I   upd_s_mfma_kernel
//   Y   = L^-1 [T | r]               upd_fsolve_mfma_kernel   (blocked: 16 rows per step, the diagonal blocks by their inverses)
//   P  <- sym(P - Y^T Y), dx = Y^T y_r   upd_p_mfma_kernel    msckf.py:597-602
//
// Why (profiles/r05/mfma_f64_probe.json, round 5): v_mfma_f64_16x16x4_f64 runs at the same 78 TFLOP/s as v_fma_f64 and shares the
// SIMD with it -- a matrix instruction occupies the SIMD for 64 cycles, nothing overlaps -- so it buys no peak.  What it buys is
// everything AROUND the multiply-adds: the 64 x 64 LDS tile kernels it replaced (rounds 3-5, git 26affda) issued ~2 instructions per fused multiply-add (LDS
// reads of a 4 x 4 fp64 register tile are 64 B per lane and panel step: bound by LDS bandwidth at half the FMA rate; panel staging,
// barriers), left 30 % of every edge of a 141-row product empty, and ran at ~8 TFLOP/s.  One MFMA is ONE issue slot for 1,024
// multiply-adds with 16 B of operands per lane, read straight from global memory / L2 in the layout the matrices already have:
//   lane l = (lo = l & 15, hi = l >> 4):  A operand = A[i = lo][k = hi],  B operand = B[k = hi][j = lo],
//   result register r = D[row = hi + 4 r][col = lo]
// -- for every product here both operands are "row q of a row-major matrix, 16 consecutive entries": 128-byte segments.
// Register r of a result tile IS the B operand of k-step r of a following product (the probe checks this on the hardware): the
// forward substitution multiplies each 16 x 16 block of right-hand sides by the inverse of L's diagonal block without moving a lane.
//
// Work split: one WAVEFRONT per task (64-thread workgroups: no barriers, <= 128 registers so that a task fits beside the front-end's
// resident wavefronts), a task = a block of 2 x 2 tiles (32 x 32) of a product, or 16 right-hand sides of the substitution.  The
// 1-D grid maps workgroup id L to (stream, part) with all parts of a stream on ONE XCD (label L & 7, as the front-end's kernels do):
// the parts of a stream share their operands -- every part of upd_p reads Y -- and each XCD has its own L2.

typedef double av_v4d __attribute__((ext_vector_type(4)));
// at most 96 registers (five wavefronts per SIMD): a task then fits the hole ONE retiring LK wavefront leaves
#define AV_MFMA_CAP __attribute__((amdgpu_waves_per_eu(5, 8)))
// the factor kernels (one wavefront per stream, a dependent chain of ~50 memory round trips): 128 registers, nothing spilled
#define AV_MFMA_CAP_CHOL __attribute__((amdgpu_waves_per_eu(4, 8)))
__device__ __forceinline__ av_v4d av_mfma(double a, double b, av_v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// tiles per block edge, block edge.  2 x 2 tiles (32 x 32): four accumulators keep a task under 96 registers -- the hole ONE retiring
// LK wavefront leaves on a SIMD; 3 x 3 tiles need 130-190 and wait for two adjacent holes (0.5-1.0 ms per launch beside the front-end)
constexpr int MB = 2, MBW = 16 * MB;

__device__ __forceinline__ bool mfma_task(int parts, int S, int& stream, int& part)
{
    const int id = blockIdx.x, t = id >> 3;
    part = t % parts; stream = (t / parts) * 8 + (id & 7);
    return stream < S;
}
static inline unsigned mfma_grid(int parts, int S) { return (unsigned)parts * 8u * (unsigned)((S + 7) / 8); }
// lower-triangular block index -> (row block, column block), column <= row
__device__ __forceinline__ void mfma_tri(int part, int& tr, int& tc)
{
    tr = 0;
    while ((tr + 1) * (tr + 2) / 2 <= part) ++tr;
    tc = part - tr * (tr + 1) / 2;
}

// acc[mi][nj] += sum_{q < Q} A(q, mi) B(q, nj) for the tiles whose bit (mi * NJ + nj) of `skip` is clear.  loadA(q, mi) / loadB(q, nj):
// this lane's operand entry of k index q (q = 4 step + hi, always < Q: the tail is masked here).  ST k-steps are in flight ahead of
// the one being multiplied (3-4; 5-8 were measured and change nothing: the tasks are not bound by the latency of their operands).
template <int MI, int NJ, int ST, typename FA, typename FB>
__device__ __forceinline__ void mfma_block(int Q, FA loadA, FB loadB, av_v4d (&acc)[MI][NJ], unsigned skip)
{
    if (Q <= 0) return;
    const int hi = (int)threadIdx.x >> 4;
    const int steps = (Q + 3) >> 2;
    double a[ST][MI], b[ST][NJ];
    auto fetch = [&](int u, int s) {
        if (s >= steps) return;                               // (wave-uniform)
        const int q = 4 * s + hi;
        const bool in = q < Q;
        const int qc = in ? q : Q - 1;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) { const double v = loadA(qc, mi); a[u][mi] = in ? v : 0.0; }
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj) { const double v = loadB(qc, nj); b[u][nj] = in ? v : 0.0; }
    };
#pragma unroll
    for (int u = 0; u < ST; ++u) fetch(u, u);
    for (int s0 = 0; s0 < steps; s0 += ST) {
#pragma unroll
        for (int u = 0; u < ST; ++u) {
            if (s0 + u < steps) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int nj = 0; nj < NJ; ++nj)
                        if (!((skip >> (mi * NJ + nj)) & 1u)) acc[mi][nj] = av_mfma(a[u][mi], b[u][nj], acc[mi][nj]);
            }
            fetch(u, s0 + u + ST);
        }
    }
}

__device__ __forceinline__ int upd_rows_kept(const UpdArgsG& a) { return a.kdir > 0 ? a.kdir : upd_k(a.m, a.nc); }
constexpr int MFMA_MAXCOLS = 256;               // touched state columns per stream (6 per camera state of the window)

// T^T[c][r] = sum_q P[cols[q]][c] Wt[q][r]   (c < n, r < k), stored [n][ld] in a.T
__global__ AV_MFMA_CAP __launch_bounds__(64) void upd_tt_mfma_kernel(const UpdArgs* __restrict__ arr, int S, int bn, int bk)
{
    AV_FILTER_PRIO();
    int s, part;
    if (!mfma_task(bn * bk, S, s, part)) return;
    const UpdArgsG a = upd_load(arr, s);
    if (a.m <= 0 || a.mode != 0) return;
    const int k = upd_rows_kept(a), n = a.n, nc = a.nc, ld = a.ld;
    const int r0 = (part / bk) * MBW, c0 = (part % bk) * MBW;      // rows: state index, columns: stacked row
    if (r0 >= n || c0 >= k || nc > MFMA_MAXCOLS) return;
    __shared__ int scols[MFMA_MAXCOLS];
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    for (int q = lane; q < nc; q += 64) scols[q] = a.cols[q] * ld;
    __syncthreads();
    const size_t ldt = a.ldt;
    gcd_ptr pa[MB], pb[MB];
    unsigned skip = 0;
#pragma unroll
    for (int t = 0; t < MB; ++t) {
        pa[t] = AV_GD(a.P) + min(r0 + 16 * t + lo, n - 1);
        pb[t] = AV_GD(a.W) + min(c0 + 16 * t + lo, k - 1);
    }
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) if (r0 + 16 * mi >= n || c0 + 16 * nj >= k) skip |= 1u << (mi * MB + nj);
    av_v4d acc[MB][MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) acc[mi][nj] = av_v4d{0, 0, 0, 0};
    mfma_block<MB, MB, 3>(nc, [&](int q, int mi) { return pa[mi][scols[q]]; }, [&](int q, int nj) { return pb[nj][(size_t)q * ldt]; }, acc, skip);
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 16 * mi + hi + 4 * r, col = c0 + 16 * nj + lo;
                if (row < n && col < k) a.T[(size_t)row * ld + col] = acc[mi][nj][r];
            }
}

// S[r][c] = sum_q T^T[cols[q]][r] Wt[q][c] + s^2 [r == c]   (r, c < k; blocks on and below the diagonal, whole tiles)
__global__ AV_MFMA_CAP __launch_bounds__(64) void upd_s_mfma_kernel(const UpdArgs* __restrict__ arr, int S, int bk)
{
    AV_FILTER_PRIO();
    int s, part;
    if (!mfma_task(bk * (bk + 1) / 2, S, s, part)) return;
    const UpdArgsG a = upd_load(arr, s);
    if (a.m <= 0 || a.mode != 0) return;
    const int k = upd_rows_kept(a), nc = a.nc, ld = a.ld;
    int tr, tc;
    mfma_tri(part, tr, tc);
    const int r0 = tr * MBW, c0 = tc * MBW;
    if (r0 >= k || nc > MFMA_MAXCOLS) return;
    __shared__ int scols[MFMA_MAXCOLS];
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    for (int q = lane; q < nc; q += 64) scols[q] = a.cols[q] * ld;
    __syncthreads();
    const size_t ldt = a.ldt;
    gcd_ptr pa[MB], pb[MB];
    unsigned skip = 0;
#pragma unroll
    for (int t = 0; t < MB; ++t) {
        pa[t] = AV_GD(a.T) + min(r0 + 16 * t + lo, k - 1);
        pb[t] = AV_GD(a.W) + min(c0 + 16 * t + lo, k - 1);
    }
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) if (r0 + 16 * mi >= k || c0 + 16 * nj >= k || (tr == tc && nj > mi)) skip |= 1u << (mi * MB + nj);
    av_v4d acc[MB][MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) acc[mi][nj] = av_v4d{0, 0, 0, 0};
    mfma_block<MB, MB, 3>(nc, [&](int q, int mi) { return pa[mi][scols[q]]; }, [&](int q, int nj) { return pb[nj][(size_t)q * ldt]; }, acc, skip);
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) {
            if ((skip >> (mi * MB + nj)) & 1u) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 16 * mi + hi + 4 * r, col = c0 + 16 * nj + lo;
                if (row < k && col < k) a.Sbuf[(size_t)row * ld + col] = acc[mi][nj][r] + (row == col ? a.obs_noise : 0.0);
            }
        }
}

// Y = L^-1 [T | r_thin], 16 right-hand sides per wavefront (column c < n is row c of T^T, c == n is r_thin, solved in place),
// block row I (16 rows) at a time:   Y_I = Linv_II (B_I - sum_{J < I} L_IJ Y_J).
// L: the TRANSPOSED factor upd_chol_mfma_kernel leaves in the upper triangle of Sbuf (row q, entries i0 .. i0 + 15 = column q of L's
// block row: one 128-byte segment); LinvT: the transposed inverses of L's 16 x 16 diagonal blocks, block I at Pn + 256 I (Pn is free on
// the batched path: upd_p works in place; identity beyond row k).
// The block row just solved is the B operand of the next block row's last four k-steps as it stands in its result registers; the
// earlier ones are read back from Kt (this wavefront's own stores, long complete).
__global__ AV_MFMA_CAP __launch_bounds__(64) void upd_fsolve_mfma_kernel(const UpdArgs* __restrict__ arr, int S, int parts)
{
    AV_FILTER_PRIO();
    int s, part;
    if (!mfma_task(parts, S, s, part)) return;
    const UpdArgsG a = upd_load(arr, s);
    if (a.m <= 0 || a.mode != 0) return;
    const int k = upd_rows_kept(a), n = a.n, nc = a.nc, ld = a.ld;
    const int c0 = part * 16;
    if (c0 > n) return;
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    const int c = min(c0 + lo, n);
    const bool owner = c0 + lo <= n;
    const av_gptr<double> rcol = a.W + (size_t)nc * a.ldt;
    const av_gptr<const double> bsrc = c < n ? (av_gptr<const double>)(a.T + (size_t)c * ld) : (av_gptr<const double>)rcol;      // right-hand side c, by row
    const av_gptr<double> ybase = c < n ? a.Kt + c : rcol;
    const size_t ystride = c < n ? (size_t)ld : 1;
    const gcd_ptr Ls = AV_GD(a.Sbuf), Li = AV_GD(a.Pn);
    av_v4d yprev = {0, 0, 0, 0};
    for (int i0 = 0, I = 0; i0 < k; i0 += 16, ++I) {
        const int ia = min(i0 + lo, k - 1);
        const bool ain = i0 + lo < k;
        double rhs[4], li[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int i = i0 + hi + 4 * r; rhs[r] = bsrc[min(i, k - 1)]; li[r] = Li[I * 256 + (4 * r + hi) * 16 + lo]; }
        av_v4d g[1][1];
        g[0][0] = av_v4d{0, 0, 0, 0};
        mfma_block<1, 1, 4>(i0 - 16, [&](int q, int) { const double v = Ls[(size_t)q * ld + ia]; return ain ? v : 0.0; },
                            [&](int q, int) { return (double)ybase[(size_t)q * ystride]; }, g, 0u);
        av_v4d gg = g[0][0];
        if (I > 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double v = Ls[(size_t)(i0 - 16 + 4 * t + hi) * ld + ia];
                gg = av_mfma(ain ? v : 0.0, yprev[t], gg);
            }
        }
        av_v4d R;
#pragma unroll
        for (int r = 0; r < 4; ++r) R[r] = (i0 + hi + 4 * r < k) ? rhs[r] - gg[r] : 0.0;
        av_v4d y = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) y = av_mfma(li[t], R[t], y);
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int i = i0 + hi + 4 * r; if (i < k && owner) ybase[(size_t)i * ystride] = y[r]; }
        yprev = y;
    }
}

// P <- sym(P - Y^T Y) in place (msckf.py:597-602), delta_x = Y^T y_r by the stream's first task.  Blocks on and below the diagonal;
// the owner of an entry below the diagonal reads it and its mirror, writes both -- every unordered pair {(r,c), (c,r)} has one owner.
__global__ AV_MFMA_CAP __launch_bounds__(64) void upd_p_mfma_kernel(const UpdArgs* __restrict__ arr, int S, int bn)
{
    AV_FILTER_PRIO();
    int s, part;
    if (!mfma_task(bn * (bn + 1) / 2, S, s, part)) return;
    const UpdArgsG a = upd_load(arr, s);
    if (a.m <= 0 || a.mode != 0) return;
    const int k = upd_rows_kept(a), n = a.n, ld = a.ld;
    int tr, tc;
    mfma_tri(part, tr, tc);
    const int r0 = tr * MBW, c0 = tc * MBW;
    if (r0 >= n) return;
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    gcd_ptr pa[MB], pb[MB];
    unsigned skip = 0;
#pragma unroll
    for (int t = 0; t < MB; ++t) {
        pa[t] = AV_GD(a.Kt) + min(r0 + 16 * t + lo, n - 1);
        pb[t] = AV_GD(a.Kt) + min(c0 + 16 * t + lo, n - 1);
    }
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) if (r0 + 16 * mi >= n || c0 + 16 * nj >= n || (tr == tc && nj > mi)) skip |= 1u << (mi * MB + nj);
    av_v4d acc[MB][MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) acc[mi][nj] = av_v4d{0, 0, 0, 0};
    mfma_block<MB, MB, 3>(k, [&](int q, int mi) { return pa[mi][(size_t)q * ld]; }, [&](int q, int nj) { return pb[nj][(size_t)q * ld]; }, acc, skip);
    if (part == 0) {
        const auto rcol = a.W + (size_t)a.nc * a.ldt;
        for (int c = lane; c < n; c += 64) {
            double sacc = 0;
#pragma unroll 8
            for (int i = 0; i < k; ++i) sacc += a.Kt[(size_t)i * ld + c] * rcol[i];
            a.dx[c] = a.round > 0 ? a.dx[c] + sacc : sacc;
        }
    }
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nj = 0; nj < MB; ++nj) {
            if ((skip >> (mi * MB + nj)) & 1u) continue;
            const bool diag = tr == tc && mi == nj;
            double pr[4], pm[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 16 * mi + hi + 4 * r, col = c0 + 16 * nj + lo;
                const bool in = row < n && col < n && (!diag || row >= col);
                pr[r] = in ? a.P[(size_t)row * ld + col] : 0.0;
                pm[r] = in ? a.P[(size_t)col * ld + row] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 16 * mi + hi + 4 * r, col = c0 + 16 * nj + lo;
                const bool in = row < n && col < n && (!diag || row >= col);
                if (in) {
                    const double t = acc[mi][nj][r];
                    const double v = ((pr[r] - t) + (pm[r] - t)) / 2.;
                    a.P[(size_t)row * ld + col] = v;
                    if (row != col) a.P[(size_t)col * ld + row] = v;
                }
            }
        }
}

// Gram matrix of G = [Hc | r] (m x (nc + 1)) for the streams that stack more rows than a back-end pass keeps (msckf.hip, "Row compression
// WITHOUT a QR") as wave tasks: a 32 x 32 block of the lower triangle per wavefront, summed over ALL m rows in one fixed order (no
// slabs, no second pass), both operands "row q of G, 16 consecutive columns" gathered through the row map (Kt, as int) and the column
// list.  Result: lower triangle of Sbuf ([k1][ld]).  `list` / `n_list_dev`: the device-written list of the streams that compress; the
// tasks stride over it.
__global__ AV_MFMA_CAP __launch_bounds__(64) void upd_gram_mfma_kernel(const UpdArgs* __restrict__ arr, const int* __restrict__ list, const int* __restrict__ n_list_dev,
                                                           int n_list_host, int slots, int bk)
{
    AV_FILTER_PRIO();
    const int parts = bk * (bk + 1) / 2;
    const int id = blockIdx.x, t = id >> 3;
    const int part = t % parts, slot0 = (t / parts) * 8 + (id & 7);
    const int n_list = n_list_dev ? *n_list_dev : n_list_host;
    int tr, tc;
    mfma_tri(part, tr, tc);
    const int r0 = tr * MBW, c0 = tc * MBW;
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    __shared__ int srow[GRAM_CHUNK];
    for (int l = slot0; l < n_list; l += slots) {
        const UpdArgsG a = upd_load(arr, list[l]);
        if (!upd_front_needed(a)) continue;
        const int m = a.m, nc = a.nc, k1 = nc + 1, ld = a.ld;
        if (r0 >= k1) continue;
        gcd_ptr pa[MB], pb[MB];
        int sa[MB], sb[MB];
        unsigned skip = 0;
#pragma unroll
        for (int u = 0; u < MB; ++u) {
            const int ca = min(r0 + 16 * u + lo, nc), cb = min(c0 + 16 * u + lo, nc);
            pa[u] = ca < nc ? AV_GD(a.Hsrc) + AV_GI(a.cols)[ca] : AV_GD(a.rsrc);
            pb[u] = cb < nc ? AV_GD(a.Hsrc) + AV_GI(a.cols)[cb] : AV_GD(a.rsrc);
            sa[u] = ca < nc ? ld : 1; sb[u] = cb < nc ? ld : 1;
        }
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
#pragma unroll
            for (int nj = 0; nj < MB; ++nj) if (r0 + 16 * mi >= k1 || c0 + 16 * nj >= k1 || (tr == tc && nj > mi)) skip |= 1u << (mi * MB + nj);
        av_v4d acc[MB][MB];
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
#pragma unroll
            for (int nj = 0; nj < MB; ++nj) acc[mi][nj] = av_v4d{0, 0, 0, 0};
        for (int row0 = 0; row0 < m; row0 += GRAM_CHUNK) {
            const int rows = min(GRAM_CHUNK, m - row0);
            __syncthreads();                                 // (the previous piece of the row map is no longer read)
            const auto srcrow = (av_gptr<const int>)(a.Kt) + row0;
            for (int q = lane; q < rows; q += 64) srow[q] = srcrow[q];
            __syncthreads();
            mfma_block<MB, MB, 3>(rows, [&](int q, int mi) { return pa[mi][(size_t)srow[q] * sa[mi]]; }, [&](int q, int nj) { return pb[nj][(size_t)srow[q] * sb[nj]]; }, acc, skip);
        }
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
#pragma unroll
            for (int nj = 0; nj < MB; ++nj) {
                if ((skip >> (mi * MB + nj)) & 1u) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + 16 * mi + hi + 4 * r, col = c0 + 16 * nj + lo;
                    if (row < k1 && col <= row) a.Sbuf[(size_t)row * ld + col] = acc[mi][nj][r];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Cholesky S = L L^T by ONE wavefront per stream, blocked by 16: left-looking over block columns J,
//      tile(I, J) = S(I, J) - sum_{q < J} L(I, q) L(J, q)^T        (matrix instruction, operands from the factor's transposed image)
//      L(J, J)    = chol(tile(J, J)),  Linv_J = L(J, J)^-1         (16 x 16 in LDS, the wavefront's 64 lanes)
//      L(I, J)^T  = Linv_J tile(I, J)^T                            (matrix instruction: the tile, held TRANSPOSED, is the B operand as it stands)
// Output (what upd_fsolve_mfma_kernel reads): the TRANSPOSED factor in the upper triangle of Sbuf (row q, columns i >= q: L[i][q]),
// and LinvT blocks at Pn + 256 J.  The lower triangle of Sbuf keeps S.  Rows / columns at or beyond k: identity.
// Why one wavefront: a 256-thread kernel with the packed triangle in 74 KB of LDS (rounds 3-5: three barriers per 8 columns) holds four
// wave slots and half a CU's LDS for ~0.25 ms per stream, most of it waiting at barriers -- beside the front-end that is what displaces
// its wavefronts (0.49 ms per launch alone, 1.0 ms in the shared run); this one holds one slot for the time the dependent chain itself
// takes (0.35 ms in the shared run).
// ------------------------------------------------------------------------------------------------
constexpr int CH_TP = 17;                       // LDS pitch of the 16 x 16 tiles
// Cholesky of a 16 x 16 symmetric tile by one wavefront, the tile in REGISTERS in the result layout of the matrix instruction (lane
// (c = lane & 15, h = lane >> 4), register u = entry [h + 4 u][c]): per column j only the pivot column goes through LDS (16 values
// written by the four lanes that hold it, read back as each lane's row factors and column factor) -- one LDS round trip and two
// wavefront-local barriers per column, where a tile resident in LDS paid three dependent read-modify-write rounds.  Then the inverse
// of the factor, four lanes per column (rows h, h + 4, ..): column t of L is read ahead of the chain, the chain itself is one multiply,
// one broadcast across the four lanes and four multiply-adds per row t.  Leaves L (lower, garbage above) in A and L^-1 (lower, zeros
// above) in Ai, both LDS with pitch CH_TP.  Returns false (to every lane) on a pivot that is not positive and finite (replaced by 1).
__device__ __forceinline__ bool chol16_regs(av_v4d t, double* A, double* Ai, int lane)
{
    __shared__ double col[16], invd[16];
    bool ok = true;
    const int c = lane & 15, h = lane >> 4;
#pragma unroll 2
    for (int j = 0; j < 16; ++j) {
        if (c == j) {
#pragma unroll
            for (int u = 0; u < 4; ++u) col[h + 4 * u] = t[u];
        }
        __syncthreads();
        double d = col[j];
        if (!(d > 0.0) || !(d < 1.79e308)) { ok = false; d = 1.0; }
        const double inv = av_rsqrt_f64(d);
        const double lc = col[c] * inv;
        double li[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) li[u] = col[h + 4 * u] * inv;
        if (lane == 0) invd[j] = inv;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = h + 4 * u;
            if (c == j) t[u] = row > j ? li[u] : (row == j ? d * inv : t[u]);
            else if (c > j && row > j) t[u] = __builtin_fma(-li[u], lc, t[u]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) A[(h + 4 * u) * CH_TP + c] = t[u];
    __syncthreads();
    // inverse: column c of L^-1 by the four lanes (c, h): rows h + 4 u
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (h + 4 * u == c) ? 1.0 : 0.0;
#pragma unroll 1
    for (int tq = 0; tq < 4; ++tq) {                         // (rows 4 tq .. 4 tq + 3 live in register tq of the lanes h = 0 .. 3)
        const double vq = tq == 0 ? v[0] : (tq == 1 ? v[1] : (tq == 2 ? v[2] : v[3]));
        double vcur = vq;                                    // this lane's row h + 4 tq, kept current through the four steps below
#pragma unroll
        for (int tr = 0; tr < 4; ++tr) {
            const int tt = 4 * tq + tr;
            const double xt_own = vcur * invd[tt];           // valid on the lanes with h == tr
            const double xt = __shfl(xt_own, c + 16 * tr, 64);
            if (h == tr) Ai[tt * CH_TP + c] = tt < c ? 0.0 : xt;
            if (h > tr) vcur = __builtin_fma(-A[(h + 4 * tq) * CH_TP + tt], xt, vcur);       // row h + 4 tq > tt inside this group of four
#pragma unroll
            for (int u = 0; u < 4; ++u) if (u > tq) v[u] = __builtin_fma(-A[(h + 4 * u) * CH_TP + tt], xt, v[u]);
        }
    }
    __syncthreads();
    return ok;
}

// GRAM = false: S = H P H^T + s^2 I of the update (lower triangle of Sbuf, written by upd_s_mfma_kernel).
// GRAM = true: the bordered Gram matrix [A + E, b; b^T, 2 rho + 1] of the row compression (lower triangle of Sbuf, written by
// upd_gram_mfma_kernel), k = nc + 1.  E = 1e-12 max_i A_ii on every diagonal entry: relative to the LARGEST column, so a column that
// is (numerically) zero -- a camera whose block the stacked rows do not constrain -- still gets a pivot well above the rounding of the
// sums, instead of 1e-12 of its own rounding noise; the border pivot (rho - f^T f = the squared residual the columns cannot explain)
// only has to stay positive.  The
// factor leaves as the nc rows [F | f] of W that the back end reads: W[q][row] = L[q][row] (row <= q < nc), rcol[row] = L[nc][row].
template <bool GRAM>
__device__ __forceinline__ void chol_mfma_body(const UpdArgsG& a, const int k)
{
    const int ld = a.ld;
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    __shared__ double At[16 * CH_TP], Ai[16 * CH_TP];
    const av_gptr<double> Sb = a.Sbuf;
    const gcd_ptr Ls = AV_GD(a.Sbuf);
    const int nc = a.nc;
    const size_t ldt = a.ldt;
    const av_gptr<double> rcol = a.W + (size_t)nc * ldt;
    double eps = 0.0;
    if (GRAM) {
        double dloc = 0.0;
        for (int r = lane; r < nc; r += 64) dloc = fmax(dloc, Ls[(size_t)r * ld + r]);      // (a NaN on the diagonal is dropped by fmax here and caught by the pivot test)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) dloc = fmax(dloc, __shfl_xor(dloc, d, 64));
        eps = 1e-12 * dloc + 1e-300;
    }
    const int nb = (k + 15) >> 4;
    bool ok = true;
    // entry (r, c) of the matrix with the identity beyond k, read from the lower triangle
    auto s_at = [&](int r, int c) -> double {
        double v = Ls[(size_t)min(max(r, c), k - 1) * ld + min(min(r, c), k - 1)];
        if (GRAM && r == c) v = r < nc ? v + eps : 2.0 * v + 1.0;
        return (r < k && c < k) ? v : (r == c ? 1.0 : 0.0);
    };
#pragma unroll 1
    for (int J = 0; J < nb; ++J) {
        const int j0 = 16 * J;
        const int ja = min(j0 + lo, k - 1);
        const bool jin = j0 + lo < k;
        // ---- diagonal tile
        {
            av_v4d g[1][1], dt;
            g[0][0] = av_v4d{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) dt[r] = s_at(j0 + hi + 4 * r, j0 + lo);          // (requested ahead of the product: one memory round trip less per tile)
            mfma_block<1, 1, 4>(j0, [&](int q, int) { const double v = Ls[(size_t)q * ld + ja]; return jin ? v : 0.0; },
                                [&](int q, int) { const double v = Ls[(size_t)q * ld + ja]; return jin ? v : 0.0; }, g, 0u);
#pragma unroll
            for (int r = 0; r < 4; ++r) dt[r] -= g[0][0][r];
            __syncthreads();                                 // (the previous block column's readers of At / Ai are done)
            ok = chol16_regs(dt, At, Ai, lane) && ok;
            // transposed diagonal block -> upper triangle of Sbuf (row j0 + j', columns j0 + i' >= j'), LinvT block -> Pn
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jp = hi + 4 * r, ip = lo;
                if (ip >= jp && j0 + ip < k) Sb[(size_t)(j0 + jp) * ld + j0 + ip] = At[ip * CH_TP + jp];
                if (!GRAM) a.Pn[J * 256 + jp * 16 + ip] = Ai[ip * CH_TP + jp];             // LinvT[kk = jp][i = ip] = Linv[ip][jp]
                if (GRAM && j0 + ip < k && j0 + jp < nc) {                                  // row q = j0 + ip of [F | f], entry j0 + jp (zero above the diagonal)
                    const double v = ip >= jp ? At[ip * CH_TP + jp] : 0.0;
                    if (j0 + ip < nc) a.W[(size_t)(j0 + ip) * ldt + j0 + jp] = v; else rcol[j0 + jp] = v;
                }
            }
        }
        // ---- tiles below it, CC at a time, held transposed: T'[j'][i'] = tile(I, J)[i'][j']
        constexpr int CC = 2;
        double li[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) li[t] = Ai[lo * CH_TP + 4 * t + hi];                  // A operand of k-step t: Linv[i = lo][kk = 4 t + hi]
#pragma unroll 1
        for (int I0 = J + 1; I0 < nb; I0 += CC) {
            int ia[CC]; bool iin[CC]; unsigned skip = 0;
#pragma unroll
            for (int t = 0; t < CC; ++t) { ia[t] = min(16 * (I0 + t) + lo, k - 1); iin[t] = 16 * (I0 + t) + lo < k; if (I0 + t >= nb) skip |= 1u << t; }
            av_v4d g[1][CC], T0[CC];
#pragma unroll
            for (int t = 0; t < CC; ++t) {
                g[0][t] = av_v4d{0, 0, 0, 0};
#pragma unroll
                for (int r = 0; r < 4; ++r) T0[t][r] = ((skip >> t) & 1u) ? 0.0 : s_at(16 * (I0 + t) + lo, j0 + hi + 4 * r);      // (ahead of the product)
            }
            mfma_block<1, CC, 3>(j0, [&](int q, int) { const double v = Ls[(size_t)q * ld + ja]; return jin ? v : 0.0; },
                                 [&](int q, int t) { const double v = Ls[(size_t)q * ld + ia[t]]; return iin[t] ? v : 0.0; }, g, skip);
#pragma unroll
            for (int t = 0; t < CC; ++t) {
                if ((skip >> t) & 1u) continue;
                const int i0 = 16 * (I0 + t);
                av_v4d T;
#pragma unroll
                for (int r = 0; r < 4; ++r) T[r] = T0[t][r] - g[0][t][r];
                av_v4d x = {0, 0, 0, 0};
#pragma unroll
                for (int u = 0; u < 4; ++u) x = av_mfma(li[u], T[u], x);
#pragma unroll
                for (int r = 0; r < 4; ++r) if (j0 + hi + 4 * r < k && i0 + lo < k) {
                    Sb[(size_t)(j0 + hi + 4 * r) * ld + i0 + lo] = x[r];
                    if (GRAM) { if (i0 + lo < nc) a.W[(size_t)(i0 + lo) * ldt + j0 + hi + 4 * r] = x[r]; else rcol[j0 + hi + 4 * r] = x[r]; }
                }
            }
        }
        if (GRAM) {                                          // [F | f] above the diagonal: rows q of the blocks before J, entries of block J
            for (int e = lane; e < j0 * 16; e += 64) { const int q = e >> 4, c = j0 + (e & 15); if (c < nc) a.W[(size_t)q * ldt + c] = 0.0; }
        }
    }
    if (!ok) {
        // not positive definite to working precision, or not finite.  Update: L = 1e150 I with ZERO for the inverses of its diagonal blocks
        // (Y = Linv (..) = 0 exactly: delta_x = 0 and P keeps its bits; 1e-150 there left delta_x at 1e-300 of its size, not at zero);
        // compression: [F | f] = 0 (S = s^2 I, delta_x = 0, P unchanged).  The host stops the stream on the flag.
        if (lane == 0 && a.status) *a.status = UPD_BAD_PIVOT;
        if (GRAM) {
            for (int e = lane; e < nc * nc; e += 64) { const int q = e / nc, row = e - q * nc; a.W[(size_t)q * ldt + row] = 0.0; }
            for (int row = lane; row < nc; row += 64) rcol[row] = 0.0;
        } else {
            for (int e = lane; e < k * k; e += 64) { const int r = e / k, c = e - r * k; if (c >= r) Sb[(size_t)r * ld + c] = r == c ? 1e150 : 0.0; }
            for (int e = lane; e < nb * 256; e += 64) a.Pn[e] = 0.0;
        }
    }
}

__global__ AV_MFMA_CAP_CHOL __launch_bounds__(64) void upd_chol_mfma_kernel(const UpdArgs* __restrict__ arr, int S)
{
    AV_FILTER_PRIO();
    int s, part;
    if (!mfma_task(1, S, s, part)) return;
    const UpdArgsG a = upd_load(arr, s);
    if (a.m <= 0 || a.mode != 0) return;
    chol_mfma_body<false>(a, upd_rows_kept(a));
}
// the compression's factor: the streams of the device-written (or host-given) list, a wavefront each
__global__ AV_MFMA_CAP_CHOL __launch_bounds__(64) void upd_gram_chol_mfma_kernel(const UpdArgs* __restrict__ arr, const int* __restrict__ list, const int* __restrict__ n_list_dev, int n_list_host)
{
    AV_FILTER_PRIO();
    const int n_list = n_list_dev ? *n_list_dev : n_list_host;
    for (int l = blockIdx.x; l < n_list; l += gridDim.x) {
        const UpdArgsG a = upd_load(arr, list[l]);
        if (upd_front_needed(a)) chol_mfma_body<true>(a, a.nc + 1);
        __syncthreads();
    }
}
