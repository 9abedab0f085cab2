// ransac.hip -- two-point RANSAC on temporal matches (include/airvision.h: av_two_point_ransac is the specification).
//
// No counterpart in the reference: feature_tracker.py:135-136 sets both inlier vectors to all ones where this runs.
//
// Shape: one wavefront per problem, workgroups of one wavefront (the placement rule of DESIGN.md section 4: a small per-stream task
// beside the LK launches costs nothing when it is one wave of few registers).  Lanes stride over the pairs.
//   pass 1  undistort both points, rotate the first, keep (u1, u2) in LDS, sum |u1| + |u2|            (once per pair)
//   pass 2  scale, d, the 50-unit cut; the raw set is compacted IN PLACE in LDS as (c.x, c.y, c.z, pair index): position by
//           __ballot prefix count, so the raw set is in index order
//   models  lane k builds hypothesis k from two LDS reads
//   pass 3  every raw pair is read once and tested against all N models; lane k counts hypothesis k by ballot
//   marks   the best model's inlier set goes to a byte per pair in LDS; the caller compacts / stores it
// c_i lives in LDS: 32 bytes per pair (9.4 KB at 300 pairs), read twice after it was written.  Registers stay flat for any n (a
// register-resident c_i would need 8 VGPRs per 64 pairs: 40 at n = 300, 192 at 1,500), and recomputing it would run the
// undistortion -- the only expensive part: a division chain, for the equidistant model a Newton iteration and a tan -- three times.
#include <math.h>

#include "av_common.h"

namespace {

constexpr int RS_H = AV_RANSAC_MAX_HYPOTHESES;

__device__ __forceinline__ double rs_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ unsigned rs_wave_max(unsigned v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { unsigned o = (unsigned)__shfl_xor((int)v, m, 64); v = o > v ? o : v; }
    return v;
}

struct RsResult { int n_set, path; };

// One problem on the calling wavefront.  load(i, p1x, p1y, p2x, p2y) fetches pair i.  slot: LDS [n][4] doubles, model: LDS
// [RS_H][4] doubles, mark: LDS [n] bytes -- `bit` is OR-ed into mark[i] for every pair the problem keeps (the caller zeroes mark).
template <class Load>
__device__ __forceinline__ RsResult ransac_problem(int n, Load load, const CamModel& cam, const double* R, double thr, int N,
                                                   uint32_t seed, uint32_t frame, uint32_t camera,
                                                   double* slot, double* model, uint8_t* mark, uint8_t bit)
{
    const int lane = threadIdx.x;
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    RsResult res{0, AV_RANSAC_PATH_FEW};
    // ---- pass 1: steps 1, 2 and the sum of step 3; a lane takes one POINT at a time (point 2 i = p1_i, 2 i + 1 = p2_i)
    double acc = 0.0;
#pragma unroll 1
    for (int q = lane; q < 2 * n; q += 64) {
        const int i = q >> 1, second = q & 1;
        float p1x, p1y, p2x, p2y;
        load(i, p1x, p1y, p2x, p2y);
        double x, y;
        av_undistort(cam, I3, (double)(second ? p2x : p1x), (double)(second ? p2y : p1y), x, y);
        if (!second) {
            const double hx = (R[0] * x + R[1] * y) + R[2] * 1.0;
            const double hy = (R[3] * x + R[4] * y) + R[5] * 1.0;
            const double hz = (R[6] * x + R[7] * y) + R[8] * 1.0;
            x = hx / hz; y = hy / hz;
        }
        acc += sqrt(x * x + y * y);
        slot[2 * q] = x; slot[2 * q + 1] = y;
    }
    const double total = rs_wave_sum(acc);
    const double s = (sqrt(2.0) * (double)(2 * n)) / total;
    const double unit = (s * 2.0) / (cam.fx + cam.fy);
    const double cut = 50.0 * unit, thr_u = thr * unit;
    __syncthreads();
    // ---- pass 2: steps 3, 4, 7; raw set compacted in place (a chunk writes at or below the entries it has just read)
    int m = 0;
    double dsum = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        bool raw = false;
        double cx = 0, cy = 0, cz = 0, dn = 0;
        if (i < n) {
            const double ax = slot[4 * i] * s, ay = slot[4 * i + 1] * s, bx = slot[4 * i + 2] * s, by = slot[4 * i + 3] * s;
            const double dx = ax - bx, dy = ay - by;
            dn = sqrt(dx * dx + dy * dy);
            raw = !(dn > cut);
            cx = dy; cy = -dx; cz = ax * by - ay * bx;
        }
        const unsigned long long b = __ballot(raw);
        const int pos = m + __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (raw) {
            slot[4 * pos] = cx; slot[4 * pos + 1] = cy; slot[4 * pos + 2] = cz;
            reinterpret_cast<int*>(slot + 4 * pos + 3)[0] = i;
            dsum += dn;
        }
        m += __popcll(b);
    }
    __syncthreads();
    if (m < 3) return res;                                                   // step 5
    const double mean = rs_wave_sum(dsum) / (double)m;
    int kept = 0;
    if (mean < unit) {                                                       // step 6
        for (int j = lane; j < m; j += 64) {
            const double cx = slot[4 * j], cy = slot[4 * j + 1];
            const double dn = sqrt(cy * cy + cx * cx);                       // = sqrt(dx dx + dy dy) of pass 2, same bits
            if (!(dn > thr_u)) { mark[reinterpret_cast<const int*>(slot + 4 * j + 3)[0]] |= bit; ++kept; }
        }
        res.path = AV_RANSAC_PATH_STILL;
    } else {                                                                 // steps 8, 9
        bool valid = false;
        if (lane < N) {
            const uint32_t r0 = av_ransac_hash_inl(seed, frame, camera, (uint32_t)lane, 0u);
            const uint32_t r1 = av_ransac_hash_inl(seed, frame, camera, (uint32_t)lane, 1u);
            const uint32_t um = (uint32_t)m;
            const uint32_t a = r0 % um, bb = (a + 1u + r1 % (um - 1u)) % um;
            const double* ca = slot + 4 * a; const double* cb = slot + 4 * bb;
            const double n0 = fabs(ca[0]) + fabs(cb[0]), n1 = fabs(ca[1]) + fabs(cb[1]), n2 = fabs(ca[2]) + fabs(cb[2]);
            int j = 0; double nb = n0;
            if (n1 < nb) { j = 1; nb = n1; }
            if (n2 < nb) { j = 2; }
            const int p = j == 0 ? 1 : 0, q = j == 2 ? 1 : 2;
            const double det = ca[p] * cb[q] - ca[q] * cb[p];
            const double tp = (ca[q] * cb[j] - ca[j] * cb[q]) / det;
            const double tq = (ca[j] * cb[p] - ca[p] * cb[j]) / det;
            valid = det != 0.0 && isfinite(tp) && isfinite(tq);
            model[4 * lane + j] = 1.0; model[4 * lane + p] = tp; model[4 * lane + q] = tq;
            model[4 * lane + 3] = valid ? 1.0 : 0.0;
        }
        __syncthreads();
        int cnt = 0;
        for (int j0 = 0; j0 < m; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < m;
            const double cx = in ? slot[4 * j] : 0.0, cy = in ? slot[4 * j + 1] : 0.0, cz = in ? slot[4 * j + 2] : 0.0;
            for (int k = 0; k < N; ++k) {
                const double* t = model + 4 * k;
                const bool ok = in && t[3] != 0.0 && fabs((cx * t[0] + cy * t[1]) + cz * t[2]) < thr_u;
                const unsigned long long b = __ballot(ok);
                if (lane == k) cnt += __popcll(b);
            }
        }
        const bool qualifies = valid && !((double)cnt < 0.2 * (double)n);
        const unsigned best = rs_wave_max(qualifies ? ((unsigned)cnt << 8 | (unsigned)(63 - lane)) : 0u);      // most inliers, first k on ties
        res.path = AV_RANSAC_PATH_MODEL;
        if (best == 0u) {
            res.path |= AV_RANSAC_PATH_NONE;
        } else {
            const double* t = model + 4 * (63 - (int)(best & 255u));
            for (int j = lane; j < m; j += 64) {
                const double cx = slot[4 * j], cy = slot[4 * j + 1], cz = slot[4 * j + 2];
                if (fabs((cx * t[0] + cy * t[1]) + cz * t[2]) < thr_u) { mark[reinterpret_cast<const int*>(slot + 4 * j + 3)[0]] |= bit; ++kept; }
            }
        }
    }
    {
        int v = kept;
#pragma unroll
        for (int mm = 32; mm >= 1; mm >>= 1) v += __shfl_xor(v, mm, 64);
        res.n_set = v;
    }
    __syncthreads();
    return res;
}

// ---- the standalone operator: problem = blockIdx.x ---------------------------------------------------------------------------
__global__ __launch_bounds__(64, 5) void ransac_op_kernel(const float* pts1, const float* pts2, const int* off, const double* R, const int* camera,
                                                       const int* frame, CamModel cam, double thr, int N, uint32_t seed, int max_pairs,
                                                       uint8_t* markers, int* info)
{
    extern __shared__ double rs_lds[];
    __shared__ double model[RS_H * 4];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int o = off[b], n = off[b + 1] - o;
    if (n < 0 || n > max_pairs) {                                            // would not fit the LDS this launch was given
        if (info && lane < 2) info[2 * b + lane] = -1;
        return;
    }
    double* slot = rs_lds;
    uint8_t* mark = reinterpret_cast<uint8_t*>(rs_lds + 4 * (size_t)max_pairs);
    for (int i = lane; i < n; i += 64) mark[i] = 0;
    __syncthreads();
    const double* Rr = R + 9 * (size_t)b;
    const float* q1 = pts1 + 2 * (size_t)o; const float* q2 = pts2 + 2 * (size_t)o;
    auto load = [&](int i, float& p1x, float& p1y, float& p2x, float& p2y) {
        p1x = q1[2 * i]; p1y = q1[2 * i + 1]; p2x = q2[2 * i]; p2y = q2[2 * i + 1];
    };
    const RsResult r = ransac_problem(n, load, cam, Rr, thr, N, seed, frame ? (uint32_t)frame[b] : 0u, camera ? (uint32_t)camera[b] : 0u,
                                      slot, model, mark, (uint8_t)1);
    for (int i = lane; i < n; i += 64) markers[(size_t)o + i] = mark[i];
    if (info && lane == 0) { info[2 * b] = r.n_set; info[2 * b + 1] = r.path; }
}

// ---- the engine's stage: stream = blockIdx.x ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64, 5) void ransac_stage_kernel(RansacStage a)
{
    extern __shared__ double rs_lds[];
    __shared__ double model[RS_H * 4];
    const int s = blockIdx.x, lane = threadIdx.x;
    int* counts = a.counts + 4 * (size_t)s;
    const bool idle = a.slot_cur != nullptr && a.slot_cur[s] < 0;
    const int n = idle ? 0 : min(a.cur_count[s], a.NT);
    if (n == 0) {                                                            // first frame, lost everything, or no frame in this step
        if (lane < 4) counts[lane] = 0;
        return;
    }
    double* slot = rs_lds;
    uint8_t* mark = reinterpret_cast<uint8_t*>(rs_lds + 4 * (size_t)a.NT);
    for (int i = lane; i < n; i += 64) mark[i] = 0;
    __syncthreads();
    const size_t cb = (size_t)s * a.NT, pb = (size_t)s * a.MAXF;
    const uint32_t frame = (uint32_t)a.frame_no[s];
    int set0 = 0, set1 = 0, path = 0;
#pragma unroll 1
    for (int cam = 0; cam < 2; ++cam) {
        const float* prev = cam ? a.prev_p1 : a.prev_p0;
        const float* cur = cam ? a.cur_p1 : a.cur_p0;
        const double* Rr = a.Rpc + (size_t)s * 18 + 9 * cam;
        auto load = [&](int i, float& p1x, float& p1y, float& p2x, float& p2y) {
            const size_t src = pb + a.cur_src[cb + i];
            p1x = prev[2 * src]; p1y = prev[2 * src + 1]; p2x = cur[2 * (cb + i)]; p2y = cur[2 * (cb + i) + 1];
        };
        const RsResult r = ransac_problem(n, load, a.cam[cam], Rr, a.thr, a.N, a.seed, frame, (uint32_t)cam, slot, model, mark, (uint8_t)(1 << cam));
        if (cam == 0) { set0 = r.n_set; path = r.path; } else { set1 = r.n_set; path |= r.path << 4; }
    }
    // survivors = marked by both cameras; cur_* compacted in order (a chunk is read whole before any of it is written, at or below itself)
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < n && mark[i] == 3;
        long long id = 0; int life = 0, cell = 0; float x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (keep) {
            id = a.cur_id[cb + i]; life = a.cur_life[cb + i]; cell = a.cur_cell[cb + i];
            x0 = a.cur_p0[2 * (cb + i)]; y0 = a.cur_p0[2 * (cb + i) + 1]; x1 = a.cur_p1[2 * (cb + i)]; y1 = a.cur_p1[2 * (cb + i) + 1];
        }
        const unsigned long long b = __ballot(keep);
        const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (keep) {
            a.cur_id[cb + pos] = id; a.cur_life[cb + pos] = life; a.cur_cell[cb + pos] = cell;
            a.cur_p0[2 * (cb + pos)] = x0; a.cur_p0[2 * (cb + pos) + 1] = y0; a.cur_p1[2 * (cb + pos)] = x1; a.cur_p1[2 * (cb + pos) + 1] = y1;
        }
        base += __popcll(b);
        __syncthreads();
    }
    // (the detector's keep-out boxes are those of curr_features after the rejection, feature_adder.py:59-62: select_kernel reads this list)
    if (lane == 0) {
        a.cur_count[s] = base;
        counts[0] = base; counts[1] = set0; counts[2] = set1; counts[3] = path;
    }
}

size_t rs_lds_bytes(int max_pairs) { return ((size_t)max_pairs * 33 + 7) & ~(size_t)7; }

}  // namespace

int av_launch_ransac_stage(const RansacStage& a, hipStream_t st)
{
    hipLaunchKernelGGL(ransac_stage_kernel, dim3(a.S), dim3(64), rs_lds_bytes(a.NT), st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

AV_EXPORT uint32_t av_ransac_hash(uint32_t seed, uint32_t frame, uint32_t camera, uint32_t k, uint32_t draw)
{
    return av_ransac_hash_inl(seed, frame, camera, k, draw);
}

AV_EXPORT int av_ransac_num_hypotheses(double p)
{
    if (!(p > 0.0 && p < 1.0)) return 0;
    const double v = ceil(log(1.0 - p) / log(1.0 - 0.7 * 0.7));
    if (!(v >= 1.0)) return 1;
    return v > (double)AV_RANSAC_MAX_HYPOTHESES ? AV_RANSAC_MAX_HYPOTHESES : (int)v;
}

AV_EXPORT int av_two_point_ransac(const float* pts1_dev, const float* pts2_dev, const int32_t* off_dev, int n_problems, int max_pairs,
                                  const double* R_dev, const int32_t* camera_dev, const int32_t* frame_dev,
                                  const double* intr, const double* dist, int model, double inlier_error, double success_probability,
                                  uint32_t seed, uint8_t* markers_dev, int32_t* info_dev, void* stream)
{
    if (!off_dev || !R_dev || !intr || !dist || n_problems < 0 || max_pairs < 0 || (max_pairs > 0 && (!pts1_dev || !pts2_dev || !markers_dev))) {
        av_set_error("av_two_point_ransac: bad arguments");
        return AV_E_INVALID;
    }
    if (max_pairs > AV_RANSAC_MAX_PAIRS) { av_set_error("av_two_point_ransac: %d pairs in one problem, at most %d", max_pairs, AV_RANSAC_MAX_PAIRS); return AV_E_INVALID; }
    if (model != AV_DISTORTION_RADTAN && model != AV_DISTORTION_EQUIDISTANT) { av_set_error("av_two_point_ransac: unknown distortion model %d", model); return AV_E_INVALID; }
    const int N = av_ransac_num_hypotheses(success_probability);
    if (N <= 0 || !(inlier_error >= 0.0)) { av_set_error("av_two_point_ransac: success probability %g outside (0, 1) or negative inlier error", success_probability); return AV_E_INVALID; }
    if (n_problems == 0) return AV_OK;
    CamModel c{intr[0], intr[1], intr[2], intr[3], dist[0], dist[1], dist[2], dist[3], model};
    hipLaunchKernelGGL(ransac_op_kernel, dim3(n_problems), dim3(64), rs_lds_bytes(max_pairs), (hipStream_t)stream,
                       pts1_dev, pts2_dev, off_dev, R_dev, camera_dev, frame_dev, c, inlier_error, N, seed, max_pairs, markers_dev, info_dev);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
