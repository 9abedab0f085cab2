// frontend.hip -- the image front-end as a device-resident engine over S independent stereo streams.
//
// Reference being replaced (all under src/image_processing/):
//   pipeline.py:14-150            ImageProcessingPipeline.{__init__, imu_callback, stereo_callback}
//   imu_processor.py:22-67        IMU buffer, mean-gyro rotation prediction
//   feature_initializer.py:45-85  first frame: FAST -> stereo match all -> top-3/cell -> ids
//   feature_tracker.py:74-177     temporal LK, bounds mask, stereo re-match, re-bin, lifetime+1
//   stereo_matcher.py:33-115      predict -> LK fwd -> LK bwd -> gates (err<3, |dy|<20, bounds, epipolar)
//   feature_adder.py:52-108       FAST outside the 7x7 boxes of the tracked features, top-5/cell, stereo match, top-3/cell, ids
//   feature_pruner.py:8-19        per cell keep top-5 by lifetime (stable)
//   feature_publisher.py:90-121   undistort to normalised coords -> feature_msg
//
// The reference runs one stream, one frame at a time, with Python lists of FeatureMetaData.  Here
// the per-stream state (feature grid, ids, three padded pyramids) lives in HBM for all S
// streams; one call to av_frontend_step enqueues ~15 batched kernels (grid.y or block = stream) and
// never synchronises with the host.  Frames of one stream are a dependent chain (LK at t needs the
// points of t-1), streams are independent, so S is the parallel axis that fills 256 CUs.
//
// Order-sensitive list semantics of the reference are reproduced exactly:
//   * `select(...)` compactions keep order  -> ballot/popcount ordered compaction per stream
//   * Python's stable `sorted(key=response/lifetime, reverse=True)` -> explicit (key, insertion index)
//     total orders: FAST candidates by (score desc, raster asc), pruning by (lifetime desc, insertion)
//   * ids are handed out cell-major, response-descending inside a cell
//   * the 7x7 keep-out box of a tracked feature follows numpy slice semantics (no box at all when x<3 or y<3); the
//     reference paints the boxes into a byte image, select_kernel tests the detector's survivors against the feature list itself
#include <math.h>

#include <deque>
#include <mutex>
#include <new>
#include <vector>

#include "av_common.h"

namespace {

constexpr int CNT_BEFORE = 0, CNT_TRACKED = 1, CNT_MATCHED = 2, CNT_FAST = 3, CNT_CAND = 4, CNT_NEW = 5, CNT_PUB = 6, CNT_OVF = 7;
constexpr int NCNT = 8;
constexpr unsigned long long LIFE_MAX = 0xFFFFFFull;

// everything the glue kernels need, by value
struct FeDev {
    int S, w, h, C, grid_row, grid_col, gh, gw, gmin, gmax;
    int MAXF;        // capacity of a published grid  = C * gmax
    int NT;          // capacity of tracker work lists = MAXF
    int CC;          // capacity of the candidate list = max(max_corners, C * gmax)
    int cell_cap;    // capacity of one cell's FAST list
    int rbits;       // raster bits of the packed keypoint words (av_common.h): fixed at creation, 19 up to 2^19 pixels, else 24
    int NSORT;       // pow2 >= C * (gmax + gmin)
    CamModel cam0, cam1;
    double R0to1[9], E[9], I3[9];
    double epi_thr;
    // published grid, double buffered (index = parity)
    long long* feat_id[2]; int* feat_life[2]; float* feat_p0[2]; float* feat_p1[2]; int* feat_cell[2]; int* n_feat[2];
    long long* next_id; int* first_frame;
    const double* Hmat;                                   // [S][9]
    // temporal tracking
    float* trk_prev; float* trk_next; uint8_t* trk_status; int* trk_count;
    // survivors of temporal tracking, stereo-matched
    int* sv_src; float* sv_p0; float* sv_init; float* sv_p1; uint8_t* sv_st; float* sv_back; uint8_t* sv_st2; int* sv_count;
    // curr_features after the tracker (insertion order)
    long long* cur_id; int* cur_life; float* cur_p0; float* cur_p1; int* cur_cell; int* cur_count;
    int* cur_src;                                         // AV_FE_RANSAC: index of every curr feature in the previous grid (null without the flag)
    // FAST per-cell lists
    uint32_t* cell_kp; int* cell_count;
    uint32_t* tile_kp; int* tile_count; int n_tiles, tile_cap;      // FAST survivors per detector tile (fast.hip), binned into cells by select_kernel
    // candidates for new features
    uint32_t* cand_key; float* cand_p0; float* cand_init; float* cand_p1; uint8_t* cand_st; float* cand_back; uint8_t* cand_st2;
    uint8_t* cand_inl; int* cand_off; int* cand_count;
    int* r1_list; int* r2_list; int* r1_count; int* r2_count;      // lazy candidate matching: indices matched in round 1 / round 2
    // output
    long long* out_ids; double* out_uv; int* out_n;
    int* counters;
    // Shared frame store (av_frontend_frames_*): stream s reads storage entry slot_cur[s] of the FAST lists (and, through the maps
    // handed to the LK launches, of the images and pyramids); < 0 = the stream has no frame in this step: its workgroups return at
    // once and its state stays as it is.  Null = every stream owns entry s (av_frontend_step / _step_host).
    const int* slot_cur;
    // Static per-camera masks (av_frontend_set_masks): [w * h] bytes, 1 = scene, 0 = never scene, one per camera for ALL streams; null =
    // none set, and every kernel then does exactly what it did without them
    const uint8_t* smask0; const uint8_t* smask1;
};

__device__ __forceinline__ bool fe_idle(const FeDev& d, int s) { return d.slot_cur != nullptr && d.slot_cur[s] < 0; }

// ---- stream restart (include/airvision.h, "Stream restart"; av_frontend_restart; no step launches it): a thread per listed stream puts
//      its device state back to what av_frontend_create made: the next frame is an initialisation, ids begin again at 0, both grids are
//      empty, the counters read 0.  The grids' entries and the candidate arrays need nothing: the counts say how much of them
//      is read (the detector's keep-out boxes are rebuilt from curr_features in every step).  rs_counts: AV_FE_RANSAC's per-stream counts (null
//      without the stage).  (Ahead of the step's kernels in this file, so that each of them keeps its place behind its neighbour in the
//      code object.)
__global__ __launch_bounds__(64) void restart_kernel(FeDev d, const int* list, int n, int* rs_counts)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int s = list[i];
    if (s < 0 || s >= d.S) return;                           // (never: the entry checks; keeps a bad list inside the buffers)
    d.first_frame[s] = 1; d.next_id[s] = 0;
    d.n_feat[0][s] = 0; d.n_feat[1][s] = 0;
    for (int k = 0; k < NCNT; ++k) d.counters[s * NCNT + k] = 0;
    if (rs_counts) for (int k = 0; k < 4; ++k) rs_counts[4 * (size_t)s + k] = 0;
}

// the static mask byte under pixel coordinate (x, y): m[int(y)][int(x)], truncation (the reference's rule for its 7x7 mask,
// feature_adder.py:59-62).  The callers have tested the point against the image; the clamp only keeps a NaN inside the buffer.
__device__ __forceinline__ bool smask_valid(const FeDev& d, const uint8_t* m, float x, float y)
{
    const int xi = min(max((int)x, 0), d.w - 1), yi = min(max((int)y, 0), d.h - 1);
    return m[(size_t)yi * d.w + xi] != 0;
}

__device__ __forceinline__ int cell_of(const FeDev& d, float x, float y)
{
    // int(pt[1] / grid_h) * grid_col + int(pt[0] / grid_w)  (feature_tracker.py:144-146); float32 division
    return (int)(y / (float)d.gh) * d.grid_col + (int)(x / (float)d.gw);
}

// workgroup size of the per-stream glue kernels below: 256 threads, or 64 (one wavefront per stream: step_impl picks by batch size)
#define NTB ((int)blockDim.x)
#define NWB ((int)(blockDim.x >> 6))
// ordered compaction position inside the workgroup; `base` is a running total in registers
__device__ __forceinline__ int block_ordered_pos(bool flag, int& base, int* lds4)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long b = __ballot(flag);
    int lane_prefix = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) lds4[wv] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < NWB; ++i) { int c = lds4[i]; if (i < wv) off += c; tot += c; }
    int pos = base + off + lane_prefix;
    base += tot;
    __syncthreads();
    return pos;
}

// stereo_matcher.py:47-61: initial guess in cam1 = distort(undistort(p, R0to1)) with the cam0 model
__device__ __forceinline__ void stereo_init(const FeDev& d, float x, float y, float& ox, float& oy)
{
    double ux, uy;
    av_undistort(d.cam0, d.R0to1, (double)x, (double)y, ux, uy);
    float fx = (float)ux, fy = (float)uy;                      // undistortPoints output is float32
    double px, py;
    av_distort(d.cam0, (double)fx, (double)fy, px, py);
    ox = (float)px; oy = (float)py;                            // projectPoints output is float32
}

// stereo_matcher.py:75-113
constexpr int CAND_R1 = 5;      // candidates of a cell matched in round 1 (grid_min = 3 in the reference: + 2 spares)

__device__ __forceinline__ bool stereo_gate(const FeDev& d, float p0x, float p0y, float inx, float iny, float p1x, float p1y,
                                            uint8_t st, float bx, float by)
{
    (void)inx;
    if (!st) return false;
    float ex = p0x - bx, ey = p0y - by;
    float err = sqrtf(ex * ex + ey * ey);
    if (!(err < 3.f)) return false;
    float disp = fabsf(iny - p1y);
    if (!(disp < 20.f)) return false;
    if (p1x < 0 || p1x >= (float)d.w || p1y < 0 || p1y >= (float)d.h) return false;
    if (d.smask1 && !smask_valid(d, d.smask1, p1x, p1y)) return false;      // the cam1 point lies on a pixel that is never scene
    double ax, ay, bxx, byy;
    av_undistort(d.cam0, d.I3, (double)p0x, (double)p0y, ax, ay);
    av_undistort(d.cam0, d.I3, (double)p1x, (double)p1y, bxx, byy);
    double u0x = (double)(float)ax, u0y = (double)(float)ay, u1x = (double)(float)bxx;
    double l0 = (d.E[0] * u0x + d.E[1] * u0y) + d.E[2] * 1.0;
    double l1 = (d.E[3] * u0x + d.E[4] * u0y) + d.E[5] * 1.0;
    double err_epi = fabs(u1x * l0) / sqrt(l0 * l0 + l1 * l1);
    if (err_epi > d.epi_thr) return false;
    return true;
}

// ---- G1: predicted positions for temporal tracking (feature_tracker.py:86-101,159-177) --------
__global__ __launch_bounds__(256) void track_prepare_kernel(FeDev d, int par)
{
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (fe_idle(d, s)) return;
    const int n = d.n_feat[par][s];
    if (i == 0) { d.trk_count[s] = n; d.counters[s * NCNT + CNT_BEFORE] = n; }
    if (i >= n) return;
    const size_t k = (size_t)s * d.MAXF + i, t = (size_t)s * d.NT + i;
    float x = d.feat_p0[par][2 * k], y = d.feat_p0[par][2 * k + 1];
    const double* H = d.Hmat + s * 9;
    double h0 = (H[0] * (double)x + H[1] * (double)y) + H[2] * 1.0;
    double h1 = (H[3] * (double)x + H[4] * (double)y) + H[5] * 1.0;
    double h2 = (H[6] * (double)x + H[7] * (double)y) + H[8] * 1.0;
    d.trk_prev[2 * t] = x; d.trk_prev[2 * t + 1] = y;
    d.trk_next[2 * t] = (float)(h0 / h2); d.trk_next[2 * t + 1] = (float)(h1 / h2);
}

// ---- G2: bounds mask (+ static cam0 mask) + ordered compaction + stereo initial guess (feature_tracker.py:110-126) --
__global__ __launch_bounds__(256) void track_gate_kernel(FeDev d)
{
    __shared__ int lds4[4];
    const int s = blockIdx.x;
    if (fe_idle(d, s)) return;
    const int n = d.trk_count[s];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += NTB) {
        const int i = i0 + threadIdx.x;
        const size_t t = (size_t)s * d.NT + i;
        bool keep = false; float x = 0, y = 0;
        if (i < n) {
            x = d.trk_next[2 * t]; y = d.trk_next[2 * t + 1];
            keep = d.trk_status[t] != 0 && !(x < 0 || x > (float)(d.w - 1) || y < 0 || y > (float)(d.h - 1));
            if (keep && d.smask0) keep = smask_valid(d, d.smask0, x, y);      // tracked onto a cam0 pixel that is never scene
        }
        int pos = block_ordered_pos(keep, base, lds4);
        if (keep) {
            const size_t o = (size_t)s * d.NT + pos;
            d.sv_src[o] = i;
            d.sv_p0[2 * o] = x; d.sv_p0[2 * o + 1] = y;
            float ix, iy;
            stereo_init(d, x, y, ix, iy);
            d.sv_init[2 * o] = ix; d.sv_init[2 * o + 1] = iy;
            d.sv_p1[2 * o] = ix; d.sv_p1[2 * o + 1] = iy;
            d.sv_back[2 * o] = x; d.sv_back[2 * o + 1] = y;
        }
    }
    if (threadIdx.x == 0) { d.sv_count[s] = base; d.counters[s * NCNT + CNT_TRACKED] = base; }
}

// ---- G3: stereo gate of the survivors, re-bin into curr_features --------------------------------
// With AV_FE_RANSAC (d.cur_src set) the features also record where they came from in the previous grid, for the outlier-rejection
// stage that follows (ransac.hip) and compacts curr_features to those that survive it.
__global__ __launch_bounds__(256) void rebin_kernel(FeDev d, int par)
{
    __shared__ int lds4[4];
    const int s = blockIdx.x;
    if (fe_idle(d, s)) return;
    const int n = d.sv_count[s];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += NTB) {
        const int i = i0 + threadIdx.x;
        const size_t t = (size_t)s * d.NT + i;
        bool keep = false;
        if (i < n)
            keep = stereo_gate(d, d.sv_p0[2 * t], d.sv_p0[2 * t + 1], d.sv_init[2 * t], d.sv_init[2 * t + 1],
                               d.sv_p1[2 * t], d.sv_p1[2 * t + 1], d.sv_st[t], d.sv_back[2 * t], d.sv_back[2 * t + 1]);
        int pos = block_ordered_pos(keep, base, lds4);
        if (keep) {
            const size_t o = (size_t)s * d.NT + pos;
            const size_t src = (size_t)s * d.MAXF + d.sv_src[t];
            d.cur_id[o] = d.feat_id[par][src];
            d.cur_life[o] = d.feat_life[par][src] + 1;
            float x = d.sv_p0[2 * t], y = d.sv_p0[2 * t + 1];
            d.cur_p0[2 * o] = x; d.cur_p0[2 * o + 1] = y;
            d.cur_p1[2 * o] = d.sv_p1[2 * t]; d.cur_p1[2 * o + 1] = d.sv_p1[2 * t + 1];
            d.cur_cell[o] = cell_of(d, x, y);
            if (d.cur_src) d.cur_src[o] = d.sv_src[t];
        }
    }
    if (threadIdx.x == 0) { d.cur_count[s] = base; d.counters[s * NCNT + CNT_MATCHED] = base; }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// The 7x7 keep-out box of a tracked feature at p, numpy slice semantics (feature_adder.py:59-62): columns int(px) - 3 .. int(px) + 3,
// rows likewise, cut at the right and bottom border, and NO box when int(px) < 3 or int(py) < 3 (a negative slice start is an empty
// slice).  f(t, e) is called for every detector tile t the box touches -- at most 2 x 2, a box is smaller than a tile -- with the
// box's entry in that tile's list: its centre relative to the tile's origin, + 3 so that it is not negative, row << 8 | column.
template <class F>
__device__ __forceinline__ void keepout_tiles(const FeDev& d, int ntx, float px, float py, F f)
{
    const int fx = (int)px, fy = (int)py;
    if (fx < 3 || fy < 3) return;
    const int tx0 = (fx - 3) / AV_FAST_TW, tx1 = (min(fx, d.w - 4) + 3) / AV_FAST_TW;      // (a centre beyond the image, which the tracker's
    const int ty0 = (fy - 3) / AV_FAST_TH, ty1 = (min(fy, d.h - 4) + 3) / AV_FAST_TH;      //  gate rules out, has first > last: no tile)
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx)
            f(ty * ntx + tx, (uint16_t)(((fy - ty * AV_FAST_TH + 3) << 8) | (fx - tx * AV_FAST_TW + 3)));
}
static_assert(AV_FAST_TW >= 7 && AV_FAST_TH >= 7 && AV_FAST_TW + 6 <= 256 && AV_FAST_TH + 6 <= 256, "a box touches at most 2 x 2 tiles and its entry is two bytes");

// select_kernel's dynamic LDS: three per-cell arrays, one word per detector tile and the box lists, two bytes an entry and at most
// four entries a tracked feature (NT < 4,096: below 32 KB, 2.4 KB at 300 features).  A tile's word holds the detector's count of the
// tile in its low half and the end of the tile's box list in its high half: a count is at most a quarter of a tile's pixels, an end
// at most 4 NT < 2^14.  (A word each would not fit beside the lists for the largest image with the largest grid.)
size_t select_lds_bytes(const FeDev& d)
{
    return sizeof(int) * (size_t)(3 * d.C + 1 + d.n_tiles + 1) + sizeof(uint16_t) * 4 * (size_t)d.NT;
}
static_assert(AV_FAST_TW * AV_FAST_TH / 4 < 65536, "a tile's survivor count fits the low half of its word");

// ---- G5: per-cell top-grid_max FAST candidates (feature_adder.py:66-80) or all of them on the
//          first frame (feature_initializer.py:52-55), plus their stereo initial guess ----------
// The reference's detector drops the keypoints on a pixel inside a tracked feature's 7x7 box AFTER the non-max suppression (fast.hip
// header), reading a byte image the boxes were painted into.  Here no such image exists: the workgroup sorts the boxes of its
// stream's curr_features (after the outlier rejection, where that stage runs) into per-tile lists in LDS, and a survivor of detector
// tile t is tested against the few boxes that touch t.  The answer is a boolean, so the order of a list does not matter.
__global__ __launch_bounds__(256) void select_kernel(FeDev d)
{
    extern __shared__ int sm[];
    int* cnt = sm;               // [C]
    int* off = sm + d.C;         // [C+1]
    int* ccnt = off + d.C + 1;   // [C]   FAST keypoints per cell
    int* tile = ccnt + d.C;      // [n_tiles + 1] per detector tile: its survivor count | end of its box list << 16 (the list begins where the tile before ends)
    uint16_t* box = reinterpret_cast<uint16_t*>(tile + d.n_tiles + 1);           // [4 NT] the box lists, tile after tile
    const int s = blockIdx.x;
    if (fe_idle(d, s)) return;
    const int ts = d.slot_cur ? d.slot_cur[s] : s;              // storage entry of this frame's FAST lists
    const bool first = d.first_frame[s] != 0;
    // bin the detector's per-tile survivor lists into the per-cell lists (feature_adder.py:66-71: row = y / grid_height,
    // col = x / grid_width).  The cell lists are unordered; everything below orders by (response, raster) key.
    // Dense mapping, no search: slot j of a chunk is entry (j % BK) + kb of tile j / BK; a round issues BU independent loads
    // per thread (the list words); the box test and the binning of a word then run out of LDS.
    {
        __shared__ int tmax;
        const int nt = d.n_tiles, ntx = (d.w + AV_FAST_TW - 1) / AV_FAST_TW;
        const uint32_t rmask = (1u << d.rbits) - 1u;
        constexpr int BK = 32, BU = 5;
        if (threadIdx.x == 0) tmax = 0;
        for (int c = threadIdx.x; c < d.C; c += NTB) ccnt[c] = 0;
        int mx = 0;
        for (int t = threadIdx.x; t < nt; t += NTB) { const int n = d.tile_count[(size_t)ts * nt + t]; tile[t] = n; mx = max(mx, n); }
        __syncthreads();
        if (mx > 0) atomicMax(&tmax, mx);
        // the box lists, a counting sort by tile: count, exclusive prefix (one wavefront), fill -- a tile's cursor ends at its list's end.
        // Nothing tracked (first frame, everything lost): every list is empty.
        const int nf = min(d.cur_count[s], d.NT);
        const float* fp = d.cur_p0 + 2 * (size_t)s * d.NT;
        if (nf > 0) {
            for (int i = threadIdx.x; i < nf; i += NTB)
                keepout_tiles(d, ntx, fp[2 * i], fp[2 * i + 1], [&](int t, uint16_t) { atomicAdd(&tile[t], 1 << 16); });
            __syncthreads();
            if (threadIdx.x < 64) {
                const int lane = threadIdx.x;
                int carry = 0;
                for (int t0 = 0; t0 < nt; t0 += 64) {
                    const int t = t0 + lane, w = t < nt ? tile[t] : 0, v = w >> 16;
                    int incl = v;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
                    if (t < nt) tile[t] = (w & 0xFFFF) | ((carry + incl - v) << 16);
                    carry += __shfl(incl, 63, 64);
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < nf; i += NTB)
                keepout_tiles(d, ntx, fp[2 * i], fp[2 * i + 1], [&](int t, uint16_t e) { box[atomicAdd(&tile[t], 1 << 16) >> 16] = e; });
        }
        __syncthreads();
        const int maxcount = tmax;
        for (int kb = 0; kb < maxcount; kb += BK)
            for (int j0 = threadIdx.x; j0 < nt * BK; j0 += NTB * BU) {
                uint32_t word[BU]; int x[BU], y[BU]; bool ok[BU];
#pragma unroll
                for (int u = 0; u < BU; ++u) {
                    const int j = j0 + NTB * u, t = j / BK, k = kb + (j % BK);
                    ok[u] = j < nt * BK && k < (tile[min(t, nt - 1)] & 0xFFFF);
                    word[u] = ok[u] ? d.tile_kp[((size_t)ts * nt + t) * d.tile_cap + k] : 0u;
                }
#pragma unroll
                for (int u = 0; u < BU; ++u) {
                    const uint32_t raster = rmask - (word[u] & rmask);
                    y[u] = (int)(raster / (uint32_t)d.w); x[u] = (int)(raster % (uint32_t)d.w);
                }
#pragma unroll
                for (int u = 0; u < BU; ++u) {
                    if (!ok[u]) continue;
                    // inside a box of the survivor's own tile t (tiles are row-major, fast.hip)?  |x - fx| <= 3 and |y - fy| <= 3
                    const int t = (j0 + NTB * u) / BK;
                    const int sx = x[u] % AV_FAST_TW + 6, sy = y[u] % AV_FAST_TH + 6;
                    bool inside = false;
                    for (int q = t ? tile[t - 1] >> 16 : 0, qe = tile[t] >> 16; q < qe; ++q) {
                        const int e = box[q];
                        inside |= (unsigned)(sx - (e & 0xFF)) <= 6u && (unsigned)(sy - (e >> 8)) <= 6u;
                    }
                    if (inside) continue;
                    const int cell = (y[u] / d.gh) * d.grid_col + x[u] / d.gw;
                    const int idx = atomicAdd(&ccnt[cell], 1);
                    if (idx < d.cell_cap) d.cell_kp[((size_t)s * d.C + cell) * d.cell_cap + idx] = word[u];
                    else atomicOr(&d.counters[s * NCNT + CNT_OVF], 2);
                }
            }
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int c = 0; c < d.C; ++c) tot += ccnt[c]; d.counters[s * NCNT + CNT_FAST] = tot; }
    }
    for (int c = threadIdx.x; c < d.C; c += NTB) {
        int n = min(ccnt[c], d.cell_cap);
        cnt[c] = first ? n : min(n, d.gmax);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int c = 0; c < d.C; ++c) {
            off[c] = acc;
            int take = cnt[c];
            if (acc + take > d.CC) { take = d.CC - acc; atomicOr(&d.counters[s * NCNT + CNT_OVF], 4); }
            cnt[c] = take;
            acc += take;
        }
        off[d.C] = acc;
        d.cand_count[s] = acc;
        d.counters[s * NCNT + CNT_CAND] = acc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= d.C; c += NTB) d.cand_off[s * (d.C + 1) + c] = off[c];
    // Round 1 of the stereo matching (see cand_round2_kernel): the first R1 candidates of every cell, all of them on the first frame
    {
        __shared__ int r1n;
        if (threadIdx.x == 0) r1n = 0;
        __syncthreads();
        for (int c = threadIdx.x; c < d.C; c += NTB) {
            const int take = first ? cnt[c] : min(cnt[c], CAND_R1);
            const int base = atomicAdd(&r1n, take);                     // order of the list is irrelevant: results are written by index
            for (int r = 0; r < take; ++r) d.r1_list[(size_t)s * d.CC + base + r] = off[c] + r;
        }
        __syncthreads();
        if (threadIdx.x == 0) d.r1_count[s] = r1n;
    }

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = wv; c < d.C; c += NWB) {
        const uint32_t* list = d.cell_kp + ((size_t)s * d.C + c) * d.cell_cap;
        const int n = min(ccnt[c], d.cell_cap);
        const int take = cnt[c];
        uint32_t* dst = d.cand_key + (size_t)s * d.CC + off[c];
        if (first) {
            for (int i = lane; i < take; i += 64) dst[i] = list[i];
        } else {
            // the first 4 x 64 keys of the list live in registers for all `take` selection rounds (re-reading the list from HBM
            // every round made this kernel a chain of ~75 memory round trips per wavefront); longer lists read the rest per round
            constexpr int KR = 4;
            uint32_t kreg[KR];
#pragma unroll
            for (int u = 0; u < KR; ++u) kreg[u] = lane + 64 * u < n ? list[lane + 64 * u] : 0u;
            uint32_t last = 0xFFFFFFFFu;
            for (int r = 0; r < take; ++r) {
                uint32_t best = 0;
#pragma unroll
                for (int u = 0; u < KR; ++u) if (kreg[u] < last && kreg[u] > best) best = kreg[u];
                for (int i = lane + 64 * KR; i < n; i += 64) { uint32_t k = list[i]; if (k < last && k > best) best = k; }
                best = (uint32_t)wave_max_u64(best);
                if (lane == 0) dst[r] = best;
                last = best;
            }
        }
    }
    __syncthreads();
    const int total = off[d.C];
    for (int i = threadIdx.x; i < total; i += NTB) {
        const size_t o = (size_t)s * d.CC + i;
        const uint32_t rmask = (1u << d.rbits) - 1u;
        uint32_t raster = rmask - (d.cand_key[o] & rmask);
        float y = (float)(raster / (uint32_t)d.w), x = (float)(raster % (uint32_t)d.w);
        d.cand_p0[2 * o] = x; d.cand_p0[2 * o + 1] = y;
        float ix, iy;
        stereo_init(d, x, y, ix, iy);
        d.cand_init[2 * o] = ix; d.cand_init[2 * o + 1] = iy;
        d.cand_p1[2 * o] = ix; d.cand_p1[2 * o + 1] = iy;
        d.cand_back[2 * o] = x; d.cand_back[2 * o + 1] = y;
    }
}

// ---- G6: lazy stereo matching of the candidates.  feature_adder.py:80-108 matches every candidate (up to grid_max per
// cell) and then keeps, per cell, the grid_min inliers of highest response.  Candidates are sorted by response inside their
// cell, so once the first R1 of a cell hold grid_min inliers the rest of the cell cannot change the result: round 1 matches the
// first R1 = grid_min + 2 candidates of every cell, this kernel gates them and lists for round 2 the remaining candidates of
// the (rare) cells that are still short.  Same ids, same points, ~3x fewer candidate LK passes at grid_max = 15.
__global__ __launch_bounds__(256) void cand_round2_kernel(FeDev d)
{
    __shared__ int r2n;
    const int s = blockIdx.x;
    if (fe_idle(d, s)) return;
    const int* coff = d.cand_off + s * (d.C + 1);
    const bool first = d.first_frame[s] != 0;
    if (threadIdx.x == 0) r2n = 0;
    __syncthreads();
    for (int c = threadIdx.x; c < d.C; c += NTB) {
        const int b = coff[c], e = coff[c + 1];
        const int r1 = first ? (e - b) : min(e - b, CAND_R1);
        int inl = 0;
        for (int i = b; i < b + r1; ++i) {
            const size_t o = (size_t)s * d.CC + i;
            const bool ok = stereo_gate(d, d.cand_p0[2 * o], d.cand_p0[2 * o + 1], d.cand_init[2 * o], d.cand_init[2 * o + 1],
                                        d.cand_p1[2 * o], d.cand_p1[2 * o + 1], d.cand_st[o], d.cand_back[2 * o], d.cand_back[2 * o + 1]);
            d.cand_inl[o] = ok ? 1 : 0;
            inl += ok;
        }
        const bool more = inl < d.gmin && b + r1 < e;
        for (int i = b + r1; i < e; ++i) d.cand_inl[(size_t)s * d.CC + i] = more ? 2 : 0;      // 2 = matched in round 2, gated by finalize
        if (more) {
            const int base = atomicAdd(&r2n, e - b - r1);
            for (int i = b + r1; i < e; ++i) d.r2_list[(size_t)s * d.CC + base + (i - b - r1)] = i;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) d.r2_count[s] = r2n;
}

__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* k, int n)
{
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (n >> 1); t += NTB) {
                int lo = 2 * t - (t & (stride - 1));
                int hi = lo + stride;
                bool up = (lo & size) == 0;
                unsigned long long a = k[lo], b = k[hi];
                if ((a > b) == up) { k[lo] = b; k[hi] = a; }
            }
        }
    __syncthreads();
}

// ---- G7: new-feature selection + ids, prune, publish --------------------------------------------
//  feature_adder.py:82-108 / feature_initializer.py:57-85, feature_pruner.py:8-19,
//  feature_publisher.py:90-121, pipeline.py:145-148
__global__ __launch_bounds__(256) void finalize_kernel(FeDev d, int par)
{
    extern __shared__ unsigned long long smem64[];
    unsigned long long* keys = smem64;                               // [NSORT]
    int* ism = reinterpret_cast<int*>(keys + d.NSORT);
    int* sel = ism;                   ism += d.C * d.gmin;           // candidate index of selection (c, r)
    int* sel_n = ism;                 ism += d.C;
    int* sel_pre = ism;               ism += d.C + 1;
    int* trk_n = ism;                 ism += d.C;                    // tracked features per cell
    int* cell_start = ism;            ism += d.C + 1;                // start of each cell in the sorted order
    int* out_start = ism;             ism += d.C + 1;                // start of each cell in the pruned grid
    int* new_cand = ism;              ism += d.C * d.gmin;           // insertion rank -> candidate index
    int* flags = ism;                 ism += 4;                      // [0] has_new among published

    const int s = blockIdx.x;
    if (fe_idle(d, s)) { if (threadIdx.x == 0) d.out_n[s] = 0; return; }       // nothing published, grid untouched
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int T = d.cur_count[s];
    const int ncand = d.cand_count[s];
    const int* coff = d.cand_off + s * (d.C + 1);
    const int nxt = par ^ 1;

    // A. stereo gate of the candidates matched in round 2 (round 1 was gated by cand_round2_kernel; 0 = never needed)
    for (int i = threadIdx.x; i < ncand; i += NTB) {
        const size_t o = (size_t)s * d.CC + i;
        if (d.cand_inl[o] == 2) d.cand_inl[o] = stereo_gate(d, d.cand_p0[2 * o], d.cand_p0[2 * o + 1], d.cand_init[2 * o], d.cand_init[2 * o + 1],
                                    d.cand_p1[2 * o], d.cand_p1[2 * o + 1], d.cand_st[o], d.cand_back[2 * o], d.cand_back[2 * o + 1]) ? 1 : 0;
    }
    for (int c = threadIdx.x; c < d.C; c += NTB) trk_n[c] = 0;
    if (threadIdx.x == 0) flags[0] = 0;
    __syncthreads();

    // B. per cell: top grid_min inliers by (response desc, raster asc)
    for (int c = wv; c < d.C; c += NWB) {
        const int b = coff[c], e = coff[c + 1];
        uint32_t last = 0xFFFFFFFFu;
        int r = 0;
        for (; r < d.gmin; ++r) {
            unsigned long long best = 0;
            for (int i = b + lane; i < e; i += 64) {
                const size_t o = (size_t)s * d.CC + i;
                uint32_t k = d.cand_key[o];
                if (d.cand_inl[o] && k < last) {
                    unsigned long long v = ((unsigned long long)k << 32) | (uint32_t)i;
                    if (v > best) best = v;
                }
            }
            best = wave_max_u64(best);
            if (best == 0) break;
            if (lane == 0) sel[c * d.gmin + r] = (int)(best & 0xFFFFFFFFu);
            last = (uint32_t)(best >> 32);
        }
        if (lane == 0) sel_n[c] = r;
    }
    // D. tracked features per cell
    for (int i = threadIdx.x; i < T; i += NTB) atomicAdd(&trk_n[d.cur_cell[(size_t)s * d.NT + i]], 1);
    __syncthreads();

    // C. prefixes (C <= 256 cells: serial is fine)
    if (threadIdx.x == 0) {
        int a = 0, b = 0, o = 0;
        for (int c = 0; c < d.C; ++c) {
            sel_pre[c] = a; cell_start[c] = b; out_start[c] = o;
            int nc = trk_n[c] + sel_n[c];
            a += sel_n[c]; b += nc; o += min(nc, d.gmax);
        }
        sel_pre[d.C] = a; cell_start[d.C] = b; out_start[d.C] = o;
    }
    __syncthreads();
    const int n_new = sel_pre[d.C];
    const int M = T + n_new;

    // E. sort keys: cell | (lifetime key when the cell will be pruned) | insertion index
    for (int j = threadIdx.x; j < d.NSORT; j += NTB) keys[j] = ~0ull;
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += NTB) {
        const size_t o = (size_t)s * d.NT + i;
        const int c = d.cur_cell[o];
        const bool pruned = trk_n[c] + sel_n[c] > d.gmax;
        unsigned long long lk = pruned ? (LIFE_MAX - (unsigned long long)d.cur_life[o]) : 0ull;
        keys[i] = ((unsigned long long)c << 48) | (lk << 24) | (unsigned long long)i;
    }
    for (int q = threadIdx.x; q < d.C * d.gmin; q += NTB) {
        const int c = q / d.gmin, r = q - c * d.gmin;
        if (r < sel_n[c]) {
            const int ins = T + sel_pre[c] + r;
            new_cand[ins - T] = sel[q];
            const bool pruned = trk_n[c] + sel_n[c] > d.gmax;
            unsigned long long lk = pruned ? (LIFE_MAX - 1ull) : 0ull;
            keys[ins] = ((unsigned long long)c << 48) | (lk << 24) | (unsigned long long)ins;
        }
    }
    bitonic_sort_u64(keys, d.NSORT);

    // G. pruned grid of this frame, cell-major
    const long long id0 = d.next_id[s];
    for (int j = threadIdx.x; j < M; j += NTB) {
        const unsigned long long k = keys[j];
        const int c = (int)(k >> 48), ins = (int)(k & 0xFFFFFFull);
        const int rank = j - cell_start[c];
        if (rank >= d.gmax) continue;
        const size_t o = (size_t)s * d.MAXF + out_start[c] + rank;
        if (ins < T) {
            const size_t t = (size_t)s * d.NT + ins;
            d.feat_id[nxt][o] = d.cur_id[t];
            d.feat_life[nxt][o] = d.cur_life[t];
            d.feat_p0[nxt][2 * o] = d.cur_p0[2 * t]; d.feat_p0[nxt][2 * o + 1] = d.cur_p0[2 * t + 1];
            d.feat_p1[nxt][2 * o] = d.cur_p1[2 * t]; d.feat_p1[nxt][2 * o + 1] = d.cur_p1[2 * t + 1];
        } else {
            const size_t q = (size_t)s * d.CC + new_cand[ins - T];
            d.feat_id[nxt][o] = id0 + (ins - T);
            d.feat_life[nxt][o] = 1;
            d.feat_p0[nxt][2 * o] = d.cand_p0[2 * q]; d.feat_p0[nxt][2 * o + 1] = d.cand_p0[2 * q + 1];
            d.feat_p1[nxt][2 * o] = d.cand_p1[2 * q]; d.feat_p1[nxt][2 * o + 1] = d.cand_p1[2 * q + 1];
            flags[0] = 1;                                   // benign race: all writers store 1
        }
        d.feat_cell[nxt][o] = c;
    }
    __syncthreads();
    const int n_out = out_start[d.C];
    // feature_publisher.py:97-107 dtype rule: cam0 coordinates stay float64 iff any
    // published cam0 point is a FAST tuple (= a feature created this frame); cam1 is always float32.
    const bool f64 = flags[0] != 0;
    for (int j = threadIdx.x; j < n_out; j += NTB) {
        const size_t o = (size_t)s * d.MAXF + j;
        double u0, v0, u1, v1;
        av_undistort(d.cam0, d.I3, (double)d.feat_p0[nxt][2 * o], (double)d.feat_p0[nxt][2 * o + 1], u0, v0);
        av_undistort(d.cam1, d.I3, (double)d.feat_p1[nxt][2 * o], (double)d.feat_p1[nxt][2 * o + 1], u1, v1);
        if (!f64) { u0 = (double)(float)u0; v0 = (double)(float)v0; }
        d.out_ids[o] = d.feat_id[nxt][o];
        d.out_uv[4 * o] = u0; d.out_uv[4 * o + 1] = v0;
        d.out_uv[4 * o + 2] = (double)(float)u1; d.out_uv[4 * o + 3] = (double)(float)v1;
    }
    if (threadIdx.x == 0) {
        d.n_feat[nxt][s] = n_out;
        d.out_n[s] = n_out;
        d.next_id[s] = id0 + n_new;
        d.first_frame[s] = 0;
        d.counters[s * NCNT + CNT_NEW] = n_new;
        d.counters[s * NCNT + CNT_PUB] = n_out;
    }
}

// ---- host-side engine ---------------------------------------------------------------------------
struct ImuSample { double t; double w[3]; };

struct StreamHost {
    std::deque<ImuSample> imu;
    std::mutex mu;
    double t_prev = 0.0;
    bool first = true;
    int frame = 0;                     // frames this stream has been given so far (the RANSAC draw hash takes it)
};

inline void mat3_mul(const double* A, const double* B, double* o)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) + A[i * 3 + 2] * B[2 * 3 + j];
}

// cv::Rodrigues (vector -> matrix), as imu_processor.py:63-64 uses it
inline void rodrigues(const double* r, double* R)
{
    double theta = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    if (theta < 2.220446049250313e-16) { for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    double c = cos(theta), s = sin(theta), c1 = 1. - c, it = 1. / theta;
    double x = r[0] * it, y = r[1] * it, z = r[2] * it;
    double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int i = 0; i < 9; ++i) R[i] = (c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * rx[i];
}

}  // namespace

struct av_frontend {
    av_frontend_config cfg;
    int device = 0;
    FeDev d;
    av_pyr_layout lay;
    PyrGeom geom;
    LKParams lk;
    uint8_t* pyr = nullptr;            // [S][3][lay.bytes]
    // step_host staging: two slots of {pinned host, device} image pairs, a copy stream and events, so that the H2D copy of
    // frame k+1 runs behind the kernels of frame k (pinned double-buffered H2D of frame pairs)
    struct HostSlot { uint8_t* pin = nullptr; uint8_t* dev = nullptr; hipEvent_t copied = nullptr, consumed = nullptr; bool used = false; };
    HostSlot hs[3]; hipStream_t copy_stream = nullptr; int hs_next = 0;      // three: the slot of frame k is still read (as the previous cam0 image) by step k+1
    // Level 0 of a pyramid slot (0 / 1: cam0 of alternating frames, 2: cam1) is either the padded copy inside the slot
    // (l0_img = nullptr) or the caller's image itself, read in place by LK and FAST (zero copy).  In place is possible when the
    // image outlives the step that gets it: always for av_frontend_step_host (the library's own staging slots), and for
    // av_frontend_step when the engine was created with AV_FE_INPUTS_PERSIST (include/airvision.h).
    const uint8_t* l0_img[3] = {nullptr, nullptr, nullptr}; int64_t l0_stride[3] = {0, 0, 0};
    // av_frontend_prestage: the pyramids of the NEXT step's images are already built (same slots, same launch): that step skips its own launch
    bool pre_on = false, pre_wrote_l0 = true; const uint8_t* pre_img0 = nullptr; const uint8_t* pre_img1 = nullptr; int64_t pre_stride = 0;
    void* zero_region = nullptr; size_t zero_bytes = 0;
    // Shared frame store (av_frontend_frames_reserve / _upload / av_frontend_step_frames): every DISTINCT stereo frame of a sweep is
    // uploaded, pyramided and FAST-scanned once and stays resident; the streams that replay it -- the offset streams of one
    // sequence, run.bat:4-12 / dataset.py:206-214 -- only carry an index into the store.
    struct FrameStore {
        int n_slots = 0;
        uint8_t* img = nullptr;                  // [n_slots][2][w * h]: cam0, cam1 (level 0 is read in place)
        uint8_t* pyr = nullptr;                  // [n_slots][2][lay.bytes]
        uint32_t* tile_kp = nullptr; int* tile_count = nullptr;      // FAST survivor lists of cam0, per slot
        bool l0_in_place = true;                 // false if the pyramid launcher had to write padded level-0 copies (unaligned geometry)
        std::vector<int> prev;                   // host: slot of every stream's previous frame (-1: none yet)
        struct Up { uint8_t* pin = nullptr; int* idx_h = nullptr; int* idx_d = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false;
                    uint8_t* raw_d = nullptr;                                 // raw_d: grey_chain's `raw` when a stage writes the store; idx_h / idx_d then hold its `first` list behind the entries' own
                    uint16_t* k_h = nullptr; uint16_t* k_d = nullptr; };      // AV_FE_EXPOSURE: the upload's factors [2][cap], pinned and on the device, by position in the upload
        uint8_t* gray_d = nullptr; size_t gray_cap = 0;       // grey_chain's `gray_full` of ONE upload (uploads are serialised on the copy stream: one scratch serves the whole ring)
        uint8_t* mosaic_d = nullptr; size_t mosaic_cap = 0;   // grey_chain's `mosaic` of one upload, likewise (packed mosaics only)
        uint32_t* range_d = nullptr; size_t range_cap = 0;    // grey_chain's `range` of one upload, likewise (AV_GRAY16_AUTO only): histograms, then records
        Up up[4]; int up_next = 0;               // upload staging ring (pinned frames + the slot list of the upload's kernels)
        hipEvent_t uploaded = nullptr; bool any_upload = false;      // copy stream: the newest upload's kernels have finished
        hipEvent_t stepped = nullptr; bool any_step = false;          // step stream: the newest step has finished
        long long frames_uploaded = 0;
        std::vector<uint16_t> k;                 // AV_FE_EXPOSURE, host: [n_slots][2] the factors the frame in each entry was corrected with (0: none yet)
    } fs;
    AvResources res;                   // owns every device and pinned block, event and stream named in this structure
    double* dH = nullptr;
    PinnedRing<double, 8> hH;          // the step's homographies (+ store maps, + AV_FE_RANSAC's rotations and frame numbers) on their way to dH
    int parity = 0;                    // index of the "prev" grid buffer; cam0 prev pyramid slot
    std::vector<StreamHost> streams;
    bool any_first = true;
    // feature read-back: two pinned staging slots (n | ids | uv | counters) so that the copy of frame k can be in flight
    // behind the kernels of frame k+1 (av_frontend_read_features_begin / _end)
    struct ReadSlot { int* n = nullptr; long long* ids = nullptr; double* uv = nullptr; int* cnt = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
    ReadSlot rd[2];
    // optional HIP-event timing per kernel class (bench.py's roofline leg)
    bool timing = false;
    std::vector<hipEvent_t> ev; std::vector<int> ev_cls; size_t ev_used = 0;
    // AV_FE_RANSAC: the stage's arguments; Rpc / frame_no are uploaded with the homographies, behind them in the same staging slot
    bool ransac = false; RansacStage rs; int* rs_counts = nullptr;
    // AV_FE_CLAHE: the equalised level 0 of every frame, [3][S][w * h] laid out like the pyramid slots (0 / 1: cam0 of alternating
    // frames, 2: cam1), and the look-up tables of one launch [2 S][tiles][256]; the frame store keeps tables of its own (fs_lut)
    bool clahe = false; uint8_t* eq = nullptr; uint8_t* eq_lut = nullptr; uint8_t* fs_lut = nullptr;
    // pixel_format != AV_PIX_GRAY8: the frames are converted to 8-bit grey into the same level 0 (pixfmt.hip);
    // own_l0 = some stage of grey_chain is on, so the engine owns level 0; frame_bytes = av_pixfmt_frame_bytes of the frames the entry
    // points are handed (in_w x in_h of fmt).  mosaic: grey_chain's scratch of that name for the step paths, [2][S][in_w * in_h], with a
    // packed mosaic format only (the frame store: FrameStore::mosaic_d)
    int fmt = AV_PIX_GRAY8, fmt_shift = 8; int64_t frame_bytes = 0; bool own_l0 = false; uint8_t* mosaic = nullptr;
    // image_downscale = 2 / 4: the frames the entry points are handed are in_w x in_h and are binned into that level 0 (downscale.hip);
    // cfg then holds the PROCESSED size d.w x d.h and the calibration scaled to it.  The order of the stages: grey_chain.
    // gray_full: grey_chain's scratch of that name for the step paths, [2][S][in_w * in_h] (the frame store: FrameStore::gray_d)
    int ds = 1, in_w = 0, in_h = 0; uint8_t* gray_full = nullptr;
    // av_frontend_set_masks: the engine's two mask buffers ([w * h] each, allocated by the first call; d.smask0 / smask1 point at them
    // while a mask is set) and whether the engine has been handed a frame (step, prestage or frames_upload): masks are then refused
    uint8_t* smask_buf[2] = {nullptr, nullptr}; bool fed = false;
    // AV_FE_PHOTOMETRIC: the tables of the two cameras on the device -- ph_resp_buf [2][256] Q8 (allocated with the engine), ph_gain_buf
    // [in_w * in_h] Q12 per camera (allocated by the first av_frontend_set_photometric that brings one) -- and what the stage's launches are
    // handed, ph_resp / ph_gain: null = that part is the identity for that camera.  photo_set: the tables have been given (a step before that is refused)
    bool photo = false, photo_set = false; uint16_t* ph_resp_buf = nullptr; uint16_t* ph_gain_buf[2] = {nullptr, nullptr};
    const uint16_t* ph_resp[2] = {nullptr, nullptr}; const uint16_t* ph_gain[2] = {nullptr, nullptr};
    // AV_FE_EXPOSURE ("Exposure-time normalisation" in include/airvision.h): the stage is on with either flag (photo); photo_tables = the
    // engine has AV_FE_PHOTOMETRIC and wants its tables.  ex_pend: what av_frontend_next_exposure left for the next call that hands
    // frames over, [2][n] by camera.  The step paths: a pinned ring ex_h [2][S] with one event per slot, like hH, and the factors on the
    // device ex_d [2][S], copied on the call's own stream ahead of the stage's launch.  Host copies for av_frontend_read_exposure:
    // ex_slot_k [2][2][S] by cam0's pyramid slot (a prestaged frame's factors wait there for its step), ex_last [S][2] of every stream's last step
    bool expo = false, photo_tables = false, ex_pending = false;
    std::vector<uint16_t> ex_pend, ex_slot_k, ex_last; int ex_pend_n = 0;
    PinnedRing<uint16_t, 8> ex_h; uint16_t* ex_d = nullptr;
    // av_frontend_set_gray16_scale ("Range scaling of 16-bit grey" in include/airvision.h): the settings, and for
    // AV_GRAY16_AUTO the step paths' histograms [S][4096] (zero between launches) and records [2][S][4] -- by cam0's pyramid slot, so
    // that a prestaged frame does not replace the records of the step before it (the frame store: FrameStore::range_d)
    Range16 g16 = {AV_GRAY16_SHIFT, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr}; uint32_t* g16_hist = nullptr; uint32_t* g16_rec = nullptr;
    bool stepped = false, stepped_frames = false;      // a step has run (av_frontend_read_image has something to return); it read the frame store
    // av_frontend_restart: the index list of a call on its way to the device, four pinned slots with an event each and a device slot
    // [4][S] to match, taken at create so that a restart allocates nothing
    PinnedRing<int, 4> rs_h; int* rs_d = nullptr;

    explicit av_frontend(int S) : streams(S) {}
};

namespace {

// Rpc (optional): [cam0_R_p_c, cam1_R_p_c] of imu_processor.py:56-65, 18 doubles
int integrate_imu(av_frontend* fe, int s, double t_curr, double* H, double* Rpc = nullptr)
{
    // imu_processor.py:28-67 + feature_tracker.py:166-171
    StreamHost& sh = fe->streams[s];
    const av_frontend_config& c = fe->cfg;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (Rpc) for (int i = 0; i < 18; ++i) Rpc[i] = (i % 9) % 4 == 0 ? 1.0 : 0.0;
    {
        std::lock_guard<std::mutex> g(sh.mu);
        int ib = -1, ie = -1;
        const int n = (int)sh.imu.size();
        for (int i = 0; i < n; ++i) if (sh.imu[i].t >= sh.t_prev - 0.01) { ib = i; break; }
        for (int i = 0; i < n; ++i) if (sh.imu[i].t >= t_curr - 0.004) { ie = i; break; }
        if (ib >= 0 && ie >= 0) {
            double m[3] = {0, 0, 0};
            for (int i = ib; i < ie; ++i) { m[0] += sh.imu[i].w[0]; m[1] += sh.imu[i].w[1]; m[2] += sh.imu[i].w[2]; }
            int cnt = ie - ib;
            if (cnt > 0) { m[0] /= cnt; m[1] /= cnt; m[2] /= cnt; }
            // cam0_mean = R_cam0_imu.T @ mean
            const double* Rc = c.R_cam0_imu;
            double cm[3];
            for (int i = 0; i < 3; ++i) cm[i] = (Rc[0 * 3 + i] * m[0] + Rc[1 * 3 + i] * m[1]) + Rc[2 * 3 + i] * m[2];
            double dt = t_curr - sh.t_prev;
            double rv[3] = {cm[0] * dt, cm[1] * dt, cm[2] * dt};
            double Rr[9];
            rodrigues(rv, Rr);
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i * 3 + j] = Rr[j * 3 + i];      // .T
            if (Rpc) {
                const double* R1 = c.R_cam1_imu;
                double c1[3];
                for (int i = 0; i < 3; ++i) c1[i] = (R1[0 * 3 + i] * m[0] + R1[1 * 3 + i] * m[1]) + R1[2 * 3 + i] * m[2];
                double rv1[3] = {c1[0] * dt, c1[1] * dt, c1[2] * dt};
                double Rr1[9];
                rodrigues(rv1, Rr1);
                for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { Rpc[i * 3 + j] = R[i * 3 + j]; Rpc[9 + i * 3 + j] = Rr1[j * 3 + i]; }
            }
            sh.imu.erase(sh.imu.begin(), sh.imu.begin() + ie);
        }
    }
    const double fx = c.cam0_intrinsics[0], fy = c.cam0_intrinsics[1], cx = c.cam0_intrinsics[2], cy = c.cam0_intrinsics[3];
    double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    double Ki[9] = {1. / fx, 0, -cx / fx, 0, 1. / fy, -cy / fy, 0, 0, 1};
    double KR[9];
    mat3_mul(K, R, KR);
    mat3_mul(KR, Ki, H);
    return AV_OK;
}

// event pair around a launch group; classes: 0 pyramid, 1 LK, 2 FAST, 3 glue
struct Span {
    av_frontend* fe; hipStream_t st; bool on;
    Span(av_frontend* f, int cls, hipStream_t s) : fe(f), st(s), on(false)
    {
        if (fe->timing && fe->ev_used + 2 <= fe->ev.size()) {
            on = true;
            fe->ev_cls[fe->ev_used / 2] = cls;
            (void)hipEventRecord(fe->ev[fe->ev_used], st);
        }
    }
    ~Span()
    {
        if (on) { (void)hipEventRecord(fe->ev[fe->ev_used + 1], st); fe->ev_used += 2; }
    }
};

// the engine-owned level 0 (AV_FE_CLAHE, pixel_format != AV_PIX_GRAY8) that goes with pyramid slot `slot`
uint8_t* eq_slot(const av_frontend* fe, int slot) { return fe->eq + (size_t)slot * fe->d.S * fe->d.w * fe->d.h; }

// The grey stages between the frames an entry point is handed and level 0, enqueued on st: [convert] -> [photometric] -> [bin] ->
// [equalise], each only if the engine was created with it.  This is the one place a stage is wired; the step paths (input_stage) and the frame
// store's upload both come through here.
//   raw        n groups of frames as handed over (fe->fmt, in_w x in_h).  Its map is null, unless the frames already lie in the
//              entries of l0 (8-bit grey copied into the store): then it is l0 itself
//   l0         where a finished level 0 goes: the engine's eq slots, or the store's entries with the list that CLAHE, the pyramid and
//              FAST read and write them through (every group, none negative)
//   first      the list of the stage that first writes l0 (conversion or binning), or null: l0's list with -1 for every frame but
//              the last of an entry named twice
//   gray_full  the caller's full-size grey scratch, ahead of the binning when a conversion or the photometric stage feeds it
//   mosaic     the caller's 8-bit mosaic scratch, between the two passes of a packed mosaic's conversion (n frames per camera, no list)
//   lut        the look-up tables of one equalisation
//   range      gray16_scale = AV_GRAY16_AUTO: the caller's histograms [n][4096] (zero, and left zero) and records [n][4], by group
//   k0, k1     AV_FE_EXPOSURE: the exposure factors of the n groups on the device, one array per camera, by group; else null
// *level0 = the set the pyramid launch reads: l0 if any stage ran (fe->own_l0: the engine then owns level 0, which outlives the call
// whatever the caller's frames do), else raw.
int grey_chain(av_frontend* fe, const FrameSet& raw, int n, const FrameSet& l0, const int* first, const FrameSet& gray_full, const FrameSet& mosaic,
               uint8_t* lut, uint32_t* range_hist, uint32_t* range_rec, const uint16_t* k0, const uint16_t* k1, hipStream_t st, FrameSet* level0)
{
    const av_frontend_config& c = fe->cfg;
    const bool conv = fe->fmt != AV_PIX_GRAY8, bin = fe->ds > 1;
    const FrameSet l0_first{{l0.base[0], l0.base[1]}, l0.stride, first};
    FrameSet at = raw;                         // where the frames lie after the stages so far
    int rc;
    if (conv) {
        const FrameSet& to = bin ? gray_full : l0_first;
        if (fe->g16.mode != AV_GRAY16_SHIFT) {       // a window or the pair's own range instead of the shift (range16.hip): same target, same list
            Range16 r = fe->g16;
            r.hist = range_hist; r.rec = range_rec;
            if ((rc = av_launch_gray16_range(at, to, n, fe->in_w, fe->in_h, r, st))) return rc;
        } else if ((rc = av_launch_to_gray8(at, to, n, fe->in_w, fe->in_h, fe->fmt, fe->fmt_shift, st, &mosaic))) return rc;
        at = to;
    }
    if (fe->photo) {
        // after a conversion: in place on its target, through the list that target was written through (`first` for l0, none for
        // gray_full); without one: out of the raw frames, which are the caller's and are never written
        const FrameSet& to = conv ? at : bin ? gray_full : l0_first;
        if ((rc = av_launch_photometric(at, to, n, fe->in_w, fe->in_h, fe->ph_resp[0], fe->ph_resp[1], fe->ph_gain[0], fe->ph_gain[1], k0, k1, st))) return rc;
        at = to;
    }
    if (bin && (rc = av_launch_downscale(at, l0_first, n, fe->in_w, fe->in_h, fe->ds, st))) return rc;
    if (conv || bin || fe->photo) at = l0;
    if (fe->clahe) {
        if ((rc = av_launch_clahe(at, l0, n, fe->d.w, fe->d.h, c.clahe_clip_limit, c.clahe_tiles_x, c.clahe_tiles_y, lut, st))) return rc;
        at = l0;
    }
    *level0 = at;
    return AV_OK;
}

// The input stage of a step (step_impl, av_frontend_prestage): the grey chain into the engine's own level 0 (slots cur and 2 of eq),
// then the pyramids of both cameras' images into pyramid slots cur and 2.  One class-0 span.
// *wrote_l0 = false: level 0 stays the image itself (never asked for unless the inputs persist: the engine's own level 0 always does).
int input_stage(av_frontend* fe, const uint8_t* img0, const uint8_t* img1, int64_t img_stride, int cur, bool inputs_persist, hipStream_t st, bool* wrote_l0)
{
    const FeDev& d = fe->d;
    const int64_t hw = (int64_t)d.w * d.h, in_hw = (int64_t)fe->in_w * fe->in_h;
    Span sp(fe, 0, st);
    const uint16_t* k0 = nullptr; const uint16_t* k1 = nullptr;
    if (fe->expo) {                          // the pending factors (the entry point has checked them) go to the device ahead of the stage, on this stream
        const int S = d.S;
        uint16_t* ex_h = nullptr;
        int rc = fe->ex_h.take(&ex_h);
        if (rc) return rc;
        memcpy(ex_h, fe->ex_pend.data(), sizeof(uint16_t) * 2 * S);
        AV_HIP(hipMemcpyAsync(fe->ex_d, ex_h, sizeof(uint16_t) * 2 * S, hipMemcpyHostToDevice, st));
        if ((rc = fe->ex_h.sent(st))) return rc;
        memcpy(fe->ex_slot_k.data() + (size_t)cur * 2 * S, fe->ex_pend.data(), sizeof(uint16_t) * 2 * S);
        fe->ex_pending = false;
        k0 = fe->ex_d; k1 = fe->ex_d + S;
    }
    const FrameSet l0 = fe->own_l0 ? FrameSet{{eq_slot(fe, cur), eq_slot(fe, 2)}, hw, nullptr} : FrameSet{};
    const FrameSet gray = fe->gray_full ? FrameSet{{fe->gray_full, fe->gray_full + (size_t)d.S * in_hw}, in_hw, nullptr} : FrameSet{};
    const FrameSet mosaic = fe->mosaic ? FrameSet{{fe->mosaic, fe->mosaic + (size_t)d.S * in_hw}, in_hw, nullptr} : FrameSet{};
    FrameSet level0;
    int rc = grey_chain(fe, av_frames(img0, img1, img_stride), d.S, l0, nullptr, gray, mosaic, fe->eq_lut, fe->g16_hist,
                        fe->g16_rec ? fe->g16_rec + (size_t)cur * 4 * d.S : nullptr, k0, k1, st, &level0);
    if (rc) return rc;
    return av_launch_pyramid(level0, d.S, fe->geom, fe->pyr, 3 * fe->lay.bytes, fe->lay.bytes, cur, 2, st, !(inputs_persist || fe->own_l0), wrote_l0);
}

// pyramid slot `slot` of the engine (0 / 1: cam0 of alternating frames, 2: cam1) with the level 0 that was recorded for it
ImgView slot_view(const av_frontend* fe, int slot) { return ImgView{fe->pyr + slot * fe->lay.bytes, 3 * fe->lay.bytes, fe->l0_img[slot], fe->l0_stride[slot], nullptr}; }
// camera `cam` of the shared frame store: entry e at pyr + (2 e + cam) * bytes / img + (2 e + cam) * w * h, reached through `map`
ImgView store_view(const av_frontend* fe, int cam, const int* map)
{
    const int64_t hw = (int64_t)fe->d.w * fe->d.h;
    return ImgView{fe->fs.pyr + cam * fe->lay.bytes, 2 * fe->lay.bytes, fe->fs.l0_in_place ? fe->fs.img + cam * hw : nullptr, 2 * hw, map};
}

// slots != nullptr: the step reads the shared frame store (stream s: entry slots[s], < 0 = no frame in this step); img0 / img1 unused.
int step_impl(av_frontend* fe, const uint8_t* img0, const uint8_t* img1, int64_t img_stride, const double* ts, hipStream_t st, bool inputs_persist,
              const int32_t* slots = nullptr)
{
    FeDev d = fe->d;                         // by value: the kernels take it by value, the frame-store step patches a few fields
    const int S = d.S;
    const bool frames = slots != nullptr;
    AV_HIP(hipSetDevice(fe->device));
    // host: IMU rotation prediction -> homographies
    int rc;
    double* hH = nullptr;
    if ((rc = fe->hH.take(&hH))) return rc;
    bool any_first = false;
    int* hmap = reinterpret_cast<int*>(hH + (size_t)9 * S);      // [2][S] behind the homographies: this frame's / the previous frame's store entry
    double* hR = hH + (size_t)10 * S;                            // AV_FE_RANSAC: [S][18] rotations, then [S] frame numbers
    int* hframe = reinterpret_cast<int*>(hR + (size_t)18 * S);
    for (int s = 0; s < S; ++s) {
        StreamHost& sh = fe->streams[s];
        if (frames) {
            hmap[s] = slots[s] < 0 ? -1 : slots[s]; hmap[S + s] = fe->fs.prev[s];
            if (slots[s] < 0) {                  // no frame for this stream in this step: its IMU buffer, t_prev and grid stay as they are
                for (int i = 0; i < 9; ++i) hH[s * 9 + i] = (i % 4 == 0) ? 1.0 : 0.0;
                if (fe->ransac) { for (int i = 0; i < 18; ++i) hR[s * 18 + i] = (i % 9) % 4 == 0 ? 1.0 : 0.0; hframe[s] = sh.frame; }
                continue;
            }
            fe->fs.prev[s] = slots[s];
            if (fe->expo) { fe->ex_last[2 * s] = fe->fs.k[2 * (size_t)slots[s]]; fe->ex_last[2 * s + 1] = fe->fs.k[2 * (size_t)slots[s] + 1]; }
        }
        if (sh.first) {
            any_first = true;
            for (int i = 0; i < 9; ++i) hH[s * 9 + i] = (i % 4 == 0) ? 1.0 : 0.0;
            if (fe->ransac) for (int i = 0; i < 18; ++i) hR[s * 18 + i] = (i % 9) % 4 == 0 ? 1.0 : 0.0;
        } else {
            integrate_imu(fe, s, ts[s], hH + s * 9, fe->ransac ? hR + s * 18 : nullptr);
        }
        if (fe->ransac) hframe[s] = sh.frame;
        sh.frame += 1;
        sh.t_prev = ts[s];
        sh.first = false;
    }
    if (fe->ransac) AV_HIP(hipMemcpyAsync(fe->dH, hH, sizeof(double) * 28 * S + sizeof(int) * S, hipMemcpyHostToDevice, st));
    else AV_HIP(hipMemcpyAsync(fe->dH, hH, sizeof(double) * 9 * S + (frames ? sizeof(int) * 2 * S : 0), hipMemcpyHostToDevice, st));
    if ((rc = fe->hH.sent(st))) return rc;
    AV_HIP(hipMemsetAsync(fe->zero_region, 0, fe->zero_bytes, st));

    const int par = fe->parity;              // prev grid buffer / prev cam0 pyramid slot
    const int cur = par ^ 1;                 // curr cam0 pyramid slot (0/1), cam1 pyramid is slot 2
    ImgView prev0, cur0, cur1;               // cam0 of the previous frame, cam0 and cam1 of this one
    if (frames) {
        // pyramids, level-0 images and FAST lists of both cameras lie in the store, built when the frame was uploaded
        const int* map_cur = reinterpret_cast<const int*>(fe->dH + (size_t)9 * S);
        d.slot_cur = map_cur; d.tile_kp = fe->fs.tile_kp; d.tile_count = fe->fs.tile_count;
        if (fe->fs.any_upload) AV_HIP(hipStreamWaitEvent(st, fe->fs.uploaded, 0));      // the frames this step reads are in the store, pyramids and FAST lists with them
        prev0 = store_view(fe, 0, map_cur + S); cur0 = store_view(fe, 0, map_cur); cur1 = store_view(fe, 1, map_cur);
    } else {
        bool wrote_l0 = true;
        if (fe->pre_on && fe->pre_img0 == img0 && fe->pre_img1 == img1 && fe->pre_stride == img_stride) wrote_l0 = fe->pre_wrote_l0;      // built by av_frontend_prestage
        else if ((rc = input_stage(fe, img0, img1, img_stride, cur, inputs_persist, st, &wrote_l0))) return rc;
        fe->pre_on = false;
        if (fe->expo) for (int s = 0; s < S; ++s) { fe->ex_last[2 * s] = fe->ex_slot_k[((size_t)cur * 2 + 0) * S + s]; fe->ex_last[2 * s + 1] = fe->ex_slot_k[((size_t)cur * 2 + 1) * S + s]; }
        if (fe->own_l0) { img0 = eq_slot(fe, cur); img1 = eq_slot(fe, 2); img_stride = (int64_t)d.w * d.h; }      // from here on the engine's own grey (equalised) images are the step's inputs
        fe->l0_img[cur] = wrote_l0 ? nullptr : img0; fe->l0_img[2] = wrote_l0 ? nullptr : img1;
        fe->l0_stride[cur] = fe->l0_stride[2] = img_stride;
        prev0 = slot_view(fe, par); cur0 = slot_view(fe, cur); cur1 = slot_view(fe, 2);      // (first frame: nothing is tracked from prev0)
    }
    fe->fed = true;                          // the engine has a frame from here on (av_frontend_set_masks)

    auto lk = [&](const ImgView& I, const ImgView& J, const float* prev, float* next, uint8_t* status, const int* count, int cap, int launch_pts, const int* list) -> int {
        Span sp(fe, 1, st);
        return av_launch_lk(I, J, S, fe->geom, prev, next, status, count, cap, launch_pts, fe->lk, st, list);
    };
    // forward / backward stereo pair: p0 in camera A -> p1 in camera B, p1 -> back in camera A
    auto lk_pair = [&](const ImgView& A, const ImgView& B, const float* p0, float* p1, uint8_t* st1, float* back, uint8_t* st2, const int* count, int cap, int launch_pts, const int* list) -> int {
        const int e = lk(A, B, p0, p1, st1, count, cap, launch_pts, list);
        return e ? e : lk(B, A, p1, back, st2, count, cap, launch_pts, list);
    };
    // per-stream glue kernels: 256-thread workgroups.  (64, one wavefront per stream -- bit-exact, the kernels take any
    // workgroup size -- was measured in round 5: glue 0.78 against 0.66 ms alone, 0.94 against 1.07 beside the filter, and the detector next
    // to them 2.46 against 2.31: front-end alone 216.9 against 220.3 k, complete path 173.3 against 174.3 k.  profiles/r05/README.md)
    { Span sp(fe, 3, st);
      hipLaunchKernelGGL(track_prepare_kernel, dim3((d.NT + 255) / 256, S), dim3(256), 0, st, d, par);
      AV_LAUNCH_CHECK(); }
    if ((rc = lk(prev0, cur0, d.trk_prev, d.trk_next, d.trk_status, d.trk_count, d.NT, d.NT, nullptr))) return rc;
    { Span sp(fe, 3, st);
      hipLaunchKernelGGL(track_gate_kernel, dim3(S), dim3(256), 0, st, d);
      AV_LAUNCH_CHECK(); }
    if ((rc = lk_pair(cur0, cur1, d.sv_p0, d.sv_p1, d.sv_st, d.sv_back, d.sv_st2, d.sv_count, d.NT, d.NT, nullptr))) return rc;
    { Span sp(fe, 3, st);
      hipLaunchKernelGGL(rebin_kernel, dim3(S), dim3(256), 0, st, d, par);
      AV_LAUNCH_CHECK(); }
    if (fe->ransac) {                          // outlier rejection on the tracked features (ransac.hip), one wavefront per stream
        Span sp(fe, 3, st);
        RansacStage a = fe->rs;
        a.prev_p0 = d.feat_p0[par]; a.prev_p1 = d.feat_p1[par]; a.slot_cur = d.slot_cur;
        if ((rc = av_launch_ransac_stage(a, st))) return rc;
    }
    // (FAST on a second HIP stream beside the temporal / stereo LK launches -- it reads only the new cam0 image and is first needed by
    //  select_kernel -- was measured in round 5: front-end alone 196.6 k against 205.1 k frames/s, complete path 157.7 against 157.3 k:
    //  the LK launches slow down by more than the detector's time; profiles/r05/README.md)
    if (!frames) {                             // (frame store: FAST ran when the frame was uploaded)
        Span sp(fe, 2, st);
        if ((rc = av_launch_fast(cur0, &fe->geom, d.smask0, 0, S, d.w, d.h, fe->cfg.fast_threshold, d.rbits, nullptr, nullptr, 0, d.tile_kp, d.tile_count, d.counters + CNT_OVF, NCNT, st))) return rc;
    }
    { Span sp(fe, 3, st);
      hipLaunchKernelGGL(select_kernel, dim3(S), dim3(256), select_lds_bytes(d), st, d);
      AV_LAUNCH_CHECK(); }
    const int r1_launch = any_first ? d.CC : d.C * (d.gmax < CAND_R1 ? d.gmax : CAND_R1);
    if ((rc = lk_pair(cur0, cur1, d.cand_p0, d.cand_p1, d.cand_st, d.cand_back, d.cand_st2, d.r1_count, d.CC, r1_launch, d.r1_list))) return rc;
    { Span sp(fe, 3, st);
      hipLaunchKernelGGL(cand_round2_kernel, dim3(S), dim3(256), 0, st, d);
      AV_LAUNCH_CHECK(); }
    // round 2: the rest of the cells that are still short of inliers (usually none)
    if (d.gmax > CAND_R1 && (rc = lk_pair(cur0, cur1, d.cand_p0, d.cand_p1, d.cand_st, d.cand_back, d.cand_st2, d.r2_count, d.CC, d.C * (d.gmax - CAND_R1), d.r2_list))) return rc;
    size_t fin_lds = sizeof(unsigned long long) * d.NSORT + sizeof(int) * (2 * d.C * d.gmin + 2 * d.C + 3 * (d.C + 1) + 4);
    { Span sp(fe, 3, st);
      hipLaunchKernelGGL(finalize_kernel, dim3(S), dim3(256), fin_lds, st, d, par);
      AV_LAUNCH_CHECK(); }
    fe->parity = par ^ 1;
    fe->stepped = true; fe->stepped_frames = frames;
    if (frames) { AV_HIP(hipEventRecord(fe->fs.stepped, st)); fe->fs.any_step = true; }
    return AV_OK;
}

}  // namespace

AV_EXPORT int av_frontend_create(const av_frontend_config* cfg, int n_streams, int device, av_frontend** out)
{
    if (!cfg || !out || n_streams <= 0) { av_set_error("av_frontend_create: bad arguments"); return AV_E_INVALID; }
    if (cfg->width <= 0 || cfg->height <= 0 || (int64_t)cfg->width * cfg->height > AV_MAX_IMAGE_PIXELS) {
        av_set_error("av_frontend_create: the engine takes images of 1 .. AV_MAX_IMAGE_PIXELS = %d pixels (%d x %d)", AV_MAX_IMAGE_PIXELS, cfg->width, cfg->height);
        return AV_E_INVALID;
    }
    if (av_pixfmt_check(cfg->pixel_format, cfg->gray16_shift, "av_frontend_create")) return AV_E_INVALID;
    if (av_pixfmt_check_size(cfg->pixel_format, cfg->width, cfg->height, "av_frontend_create")) return AV_E_INVALID;
    // image_downscale: from here on `cfg` is the configuration of the PROCESSED image (binned size, calibration scaled to it, in the
    // order include/airvision.h gives); in_w x in_h is what the entry points are handed
    const int in_w = cfg->width, in_h = cfg->height;
    const int ds = cfg->image_downscale == 0 ? 1 : cfg->image_downscale;
    av_frontend_config scaled;
    if ((ds != 1 && ds != 2 && ds != 4) || cfg->reserved1 != 0) {
        av_set_error("av_frontend_create: image_downscale %d is none of 0, 1, 2, 4 (or reserved1 = %d is not 0)", cfg->image_downscale, cfg->reserved1);
        return AV_E_INVALID;
    }
    if (ds > 1) {
        if (in_w % ds || in_h % ds) { av_set_error("av_frontend_create: image_downscale %d does not divide %d x %d", ds, in_w, in_h); return AV_E_INVALID; }
        scaled = *cfg;
        scaled.width = in_w / ds; scaled.height = in_h / ds;
        const double f = (double)ds, half = (f - 1.0) / 2.0;
        for (double* k : {scaled.cam0_intrinsics, scaled.cam1_intrinsics}) { k[0] = k[0] / f; k[1] = k[1] / f; k[2] = (k[2] - half) / f; k[3] = (k[3] - half) / f; }
        scaled.norm_unit = scaled.norm_unit * f;
        av_pyr_layout probe;
        if (av_pyramid_layout(scaled.width, scaled.height, scaled.lk_levels, &probe)) {
            av_set_error("av_frontend_create: image_downscale %d leaves %d x %d, which does not hold %d pyramid levels larger than %d pixels", ds, scaled.width, scaled.height,
                         scaled.lk_levels, AV_PYR_BORDER);
            return AV_E_INVALID;
        }
        cfg = &scaled;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { av_set_error("av_frontend_create: no HIP device visible"); return AV_E_NODEVICE; }
    if (device < 0 || device >= ndev) { av_set_error("av_frontend_create: device %d out of range (%d visible)", device, ndev); return AV_E_INVALID; }
    const int C = cfg->grid_row * cfg->grid_col;
    if (cfg->grid_row <= 0 || cfg->grid_col <= 0 || C > 256 || cfg->grid_min_feature_num <= 0 || cfg->grid_max_feature_num <= 0 ||
        cfg->lk_levels < 1 || cfg->lk_levels > AV_MAX_LEVELS || cfg->max_corners <= 0) {
        av_set_error("av_frontend_create: unsupported configuration (grid %dx%d, levels %d)", cfg->grid_row, cfg->grid_col, cfg->lk_levels);
        return AV_E_INVALID;
    }
    AV_HIP(hipSetDevice(device));
    av_frontend* fe = new (std::nothrow) av_frontend(n_streams);
    if (!fe) { av_set_error("out of host memory"); return AV_E_INVALID; }
    fe->cfg = *cfg; fe->device = fe->res.device = device;
    int rc = av_pyramid_layout(cfg->width, cfg->height, cfg->lk_levels, &fe->lay);
    if (rc) { delete fe; return rc; }
    fe->geom = av_make_geom(fe->lay);
    fe->lk.win = cfg->lk_win;
    fe->lk.max_iter = cfg->lk_max_iter < 0 ? 0 : (cfg->lk_max_iter > 100 ? 100 : cfg->lk_max_iter);
    double e = cfg->lk_eps < 0 ? 0. : (cfg->lk_eps > 10. ? 10. : cfg->lk_eps);
    fe->lk.eps2 = e * e;
    fe->lk.min_eig = cfg->lk_min_eig;
    const bool ransac = (cfg->flags & AV_FE_RANSAC) != 0;
    const int rs_N = ransac ? av_ransac_num_hypotheses(cfg->ransac_success_probability) : 0;
    if (ransac && (C * cfg->grid_max_feature_num > AV_RANSAC_MAX_PAIRS || rs_N <= 0 || !(cfg->ransac_threshold >= 0.0))) {
        av_set_error("av_frontend_create: AV_FE_RANSAC needs grid_num * grid_max <= %d (%d), a success probability inside (0, 1) (%g) and a threshold >= 0 (%g)",
                     AV_RANSAC_MAX_PAIRS, C * cfg->grid_max_feature_num, cfg->ransac_success_probability, cfg->ransac_threshold);
        delete fe; return AV_E_INVALID;
    }
    const bool clahe = (cfg->flags & AV_FE_CLAHE) != 0;
    if (clahe && av_clahe_check(cfg->width, cfg->height, cfg->clahe_clip_limit, cfg->clahe_tiles_x, cfg->clahe_tiles_y, "av_frontend_create")) { delete fe; return AV_E_INVALID; }
    if (fe->lk.win < 3 || fe->lk.win > 31) { av_set_error("av_frontend_create: lk_win %d outside 3 .. 31", fe->lk.win); delete fe; return AV_E_INVALID; }      // 15: the 16-lane kernel; others: the general one

    FeDev& d = fe->d;
    memset(&d, 0, sizeof(d));
    const int S = n_streams, w = cfg->width, h = cfg->height;
    d.S = S; d.w = w; d.h = h; d.C = C; d.grid_row = cfg->grid_row; d.grid_col = cfg->grid_col;
    d.gh = (h + cfg->grid_row - 1) / cfg->grid_row;          // int(np.ceil(h / grid_row)), feature_tracker.py:70-71
    d.gw = (w + cfg->grid_col - 1) / cfg->grid_col;
    d.gmin = cfg->grid_min_feature_num; d.gmax = cfg->grid_max_feature_num;
    d.MAXF = C * d.gmax; d.NT = d.MAXF;
    d.CC = cfg->max_corners > C * d.gmax ? cfg->max_corners : C * d.gmax;
    // a cell's list holds every corner the cell can have -- strict 3 x 3 maxima: at most one per 2 x 2 block, so the bound grows with the
    // cell's area, whatever the image size -- unless the candidate list (max_corners) is shorter than that
    d.cell_cap = (d.gh * d.gw) / 4 + (d.gh + d.gw) / 4 + 64;
    if (d.cell_cap > d.CC) d.cell_cap = d.CC;
    d.rbits = av_kp_raster_bits(w, h);
    int ns = 2; while (ns < C * (d.gmax + d.gmin)) ns <<= 1;
    d.NSORT = ns;
    if (ns > 4096) { av_set_error("av_frontend_create: grid_num*(grid_max+grid_min) = %d exceeds 4096", C * (d.gmax + d.gmin)); delete fe; return AV_E_INVALID; }
    d.cam0 = CamModel{cfg->cam0_intrinsics[0], cfg->cam0_intrinsics[1], cfg->cam0_intrinsics[2], cfg->cam0_intrinsics[3],
                      cfg->cam0_distortion[0], cfg->cam0_distortion[1], cfg->cam0_distortion[2], cfg->cam0_distortion[3], cfg->cam0_distortion_model};
    d.cam1 = CamModel{cfg->cam1_intrinsics[0], cfg->cam1_intrinsics[1], cfg->cam1_intrinsics[2], cfg->cam1_intrinsics[3],
                      cfg->cam1_distortion[0], cfg->cam1_distortion[1], cfg->cam1_distortion[2], cfg->cam1_distortion[3], cfg->cam1_distortion_model};
    for (int i = 0; i < 9; ++i) { d.R0to1[i] = cfg->R0to1[i]; d.E[i] = cfg->E[i]; d.I3[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    d.epi_thr = cfg->stereo_threshold * cfg->norm_unit;

#define A(ptr, n) if ((rc = fe->res.dev(&(ptr), (size_t)(n)))) { av_frontend_destroy(fe); return rc; }
    for (int b = 0; b < 2; ++b) {
        A(d.feat_id[b], S * d.MAXF) A(d.feat_life[b], S * d.MAXF) A(d.feat_p0[b], 2 * S * d.MAXF) A(d.feat_p1[b], 2 * S * d.MAXF)
        A(d.feat_cell[b], S * d.MAXF) A(d.n_feat[b], S)
    }
    A(d.next_id, S)
    if ((rc = fe->res.dev(&d.first_frame, (size_t)S, 1))) { av_frontend_destroy(fe); return rc; }   // bytes 0x01 -> non-zero ints
    A(fe->dH, 9 * S + S + (ransac ? 19 * S : 0))      // + [2][S] ints: the frame-store maps of the step (step_impl); AV_FE_RANSAC: + [S][18] rotations, [S] frame numbers
    d.Hmat = fe->dH;
    A(d.trk_prev, 2 * S * d.NT) A(d.trk_next, 2 * S * d.NT) A(d.trk_status, S * d.NT)
    A(d.sv_src, S * d.NT) A(d.sv_p0, 2 * S * d.NT) A(d.sv_init, 2 * S * d.NT) A(d.sv_p1, 2 * S * d.NT) A(d.sv_st, S * d.NT)
    A(d.sv_back, 2 * S * d.NT) A(d.sv_st2, S * d.NT)
    A(d.cur_id, S * d.NT) A(d.cur_life, S * d.NT) A(d.cur_p0, 2 * S * d.NT) A(d.cur_p1, 2 * S * d.NT) A(d.cur_cell, S * d.NT)
    A(d.cell_kp, (size_t)S * C * d.cell_cap)
    av_fast_tiles(w, h, &d.n_tiles, &d.tile_cap);
    // select_kernel's LDS: a word per tile and the box lists (below 32 KB: NT < 4,096, checked above).  2^24 pixels in whole tiles are some 5,500
    // tiles, 22 KB, and the per-cell arrays 3 KB at most: only a strip a few rows high, all partial tiles, with thousands of features gets here.
    if (select_lds_bytes(d) + 64 > 64 * 1024) {
        av_set_error("av_frontend_create: %d x %d has %d detector tiles, with %d features more than the selection kernel's LDS holds", w, h, d.n_tiles, d.NT);
        av_frontend_destroy(fe); return AV_E_INVALID;
    }
    A(d.tile_kp, (size_t)S * d.n_tiles * d.tile_cap) A(d.tile_count, (size_t)S * d.n_tiles)
    A(d.cand_key, (size_t)S * d.CC) A(d.cand_p0, 2 * (size_t)S * d.CC) A(d.cand_init, 2 * (size_t)S * d.CC) A(d.cand_p1, 2 * (size_t)S * d.CC)
    A(d.cand_st, (size_t)S * d.CC) A(d.cand_back, 2 * (size_t)S * d.CC) A(d.cand_st2, (size_t)S * d.CC) A(d.cand_inl, (size_t)S * d.CC)
    A(d.cand_off, S * (C + 1))
    A(d.r1_list, (size_t)S * d.CC) A(d.r2_list, (size_t)S * d.CC) A(d.r1_count, S) A(d.r2_count, S)
    A(d.out_ids, S * d.MAXF) A(d.out_uv, 4 * S * d.MAXF) A(d.out_n, S)
    // per-step zeroed counters in one region: trk_count, sv_count, cur_count, cand_count, cell_count, counters
    {
        size_t n_int = (size_t)S * 4 + (size_t)S * C + (size_t)S * NCNT;
        int* z = nullptr;
        A(z, n_int)
        fe->zero_region = z; fe->zero_bytes = n_int * sizeof(int);
        d.trk_count = z; d.sv_count = z + S; d.cur_count = z + 2 * S; d.cand_count = z + 3 * S;
        d.cell_count = z + 4 * S; d.counters = z + 4 * S + (size_t)S * C;
    }
    A(fe->pyr, (size_t)S * 3 * fe->lay.bytes)
    if (ransac) {
        A(d.cur_src, S * d.NT) A(fe->rs_counts, 4 * S)
        RansacStage& a = fe->rs;
        memset(&a, 0, sizeof(a));
        a.S = S; a.NT = d.NT; a.MAXF = d.MAXF; a.cam[0] = d.cam0; a.cam[1] = d.cam1;
        a.cur_id = d.cur_id; a.cur_life = d.cur_life; a.cur_p0 = d.cur_p0; a.cur_p1 = d.cur_p1; a.cur_cell = d.cur_cell; a.cur_src = d.cur_src;
        a.cur_count = d.cur_count; a.counts = fe->rs_counts;
        a.Rpc = fe->dH + (size_t)10 * S; a.frame_no = reinterpret_cast<const int*>(fe->dH + (size_t)28 * S);
        a.thr = cfg->ransac_threshold; a.N = rs_N; a.seed = cfg->ransac_seed;
        fe->ransac = true;
    }
    fe->fmt = cfg->pixel_format; fe->fmt_shift = cfg->gray16_shift;
    fe->ds = ds; fe->in_w = in_w; fe->in_h = in_h; fe->frame_bytes = av_pixfmt_frame_bytes(fe->fmt, in_w, in_h);
    fe->photo_tables = (cfg->flags & AV_FE_PHOTOMETRIC) != 0; fe->expo = (cfg->flags & AV_FE_EXPOSURE) != 0;
    fe->photo = fe->photo_tables || fe->expo;          // either flag turns the stage on
    fe->own_l0 = clahe || fe->fmt != AV_PIX_GRAY8 || ds > 1 || fe->photo;
    if (fe->own_l0) A(fe->eq, (size_t)3 * S * w * h)
    if (ds > 1 && (fe->fmt != AV_PIX_GRAY8 || fe->photo)) A(fe->gray_full, (size_t)2 * S * in_w * in_h)
    if (fe->photo_tables) A(fe->ph_resp_buf, 2 * 256)
    if (fe->expo) {
        A(fe->ex_d, 2 * S)
        fe->ex_slot_k.assign((size_t)4 * S, 0); fe->ex_last.assign((size_t)2 * S, 0);
    }
    if (av_pixfmt_packed_depth(fe->fmt) && av_pixfmt_is_bayer(fe->fmt)) A(fe->mosaic, (size_t)2 * S * in_w * in_h)
    if (clahe) {
        A(fe->eq_lut, (size_t)2 * S * cfg->clahe_tiles_x * cfg->clahe_tiles_y * 256)
        fe->clahe = true;
    }
#undef A
    rc = fe->hH.create(fe->res, 9 * (size_t)S + S + (ransac ? 19 * (size_t)S : 0));
    if (!rc && fe->expo) rc = fe->ex_h.create(fe->res, 2 * (size_t)S);
    if (!rc && !(rc = fe->rs_h.create(fe->res, (size_t)S))) rc = fe->res.dev(&fe->rs_d, 4 * (size_t)S);
    for (int i = 0; i < 2 && !rc; ++i) {
        av_frontend::ReadSlot& r = fe->rd[i];
        if (!(rc = fe->res.pinned(&r.n, (size_t)S)) && !(rc = fe->res.pinned(&r.ids, (size_t)S * d.MAXF)) && !(rc = fe->res.pinned(&r.uv, 4 * (size_t)S * d.MAXF)) &&
            !(rc = fe->res.pinned(&r.cnt, (size_t)S * NCNT))) rc = fe->res.event(&r.ev, hipEventDisableTiming);
    }
    if (rc) { av_frontend_destroy(fe); return rc; }
    *out = fe;
    return AV_OK;
}

AV_EXPORT void av_frontend_destroy(av_frontend* fe) { delete fe; }      // (~AvResources waits for the device and releases)

AV_EXPORT int av_frontend_push_imu(av_frontend* fe, int stream, double timestamp, const double gyro[3])
{
    if (!fe || stream < 0 || stream >= fe->d.S || !gyro) { av_set_error("av_frontend_push_imu: bad arguments"); return AV_E_INVALID; }
    StreamHost& sh = fe->streams[stream];
    std::lock_guard<std::mutex> g(sh.mu);
    sh.imu.push_back(ImuSample{timestamp, {gyro[0], gyro[1], gyro[2]}});
    return AV_OK;
}

AV_EXPORT int av_frontend_push_imu_batch(av_frontend* fe, const int32_t* stream_idx, const double* timestamps,
                                         const double* gyro, int n)
{
    if (!fe || !stream_idx || !timestamps || !gyro || n < 0) { av_set_error("av_frontend_push_imu_batch: bad arguments"); return AV_E_INVALID; }
    for (int i = 0; i < n; ++i) {
        int rc = av_frontend_push_imu(fe, stream_idx[i], timestamps[i], gyro + 3 * (size_t)i);
        if (rc) return rc;
    }
    return AV_OK;
}

// AV_FE_PHOTOMETRIC: an engine with the flag takes no frame before it has its tables
static int photo_ready(const av_frontend* fe, const char* who)
{
    if (!fe->photo_tables || fe->photo_set) return AV_OK;
    av_set_error("%s: the engine was created with AV_FE_PHOTOMETRIC but has no tables yet: call av_frontend_set_photometric first", who);
    return AV_E_INVALID;
}

// AV_FE_EXPOSURE: every call that hands frames over leaves nothing pending when it returns, whatever it returns
struct ExpoDone {
    av_frontend* fe;
    ~ExpoDone() { if (fe) fe->ex_pending = false; }
};
// ... and one that runs the input stage on n frames needs the factors of exactly those (runs = false: the step after a prestage of the
// same images, which needs none and discards what is pending)
static int expo_ready(av_frontend* fe, const char* who, int n, bool runs)
{
    if (!fe->expo || !runs) return AV_OK;
    if (!fe->ex_pending) {
        av_set_error("%s: the engine was created with AV_FE_EXPOSURE and has no exposure factors for these frames: call av_frontend_next_exposure first", who);
        return AV_E_INVALID;
    }
    if (fe->ex_pend_n != n) {
        av_set_error("%s: av_frontend_next_exposure gave the factors of %d frames, this call hands over %d", who, fe->ex_pend_n, n);
        return AV_E_INVALID;
    }
    return AV_OK;
}

// The pyramids of the images the NEXT av_frontend_step will get, enqueued now (behind the step just enqueued): that step then starts
// with its tracking launch.  Same kernels, same slots, same results -- only their place in the stream moves.  A caller that hands a
// step's feature message to the batched filter AFTER this call (av_msckf_batch_submit_dev copies it on this stream) starts the
// filter's chain behind the pyramid kernels instead of beside them: the filter's first kernel (39 KB of LDS, 4 x 128 registers per
// stream) and the pyramid kernel (all 160 KB of LDS at six workgroups per CU) otherwise halve each other (profiles/r05/README.md).
// Needs AV_FE_INPUTS_PERSIST (the images are read again by the step itself); a step that comes with other images builds its own.
AV_EXPORT int av_frontend_prestage(av_frontend* fe, const uint8_t* img0_dev, const uint8_t* img1_dev, int64_t img_stride, void* stream)
{
    const ExpoDone done{fe};
    if (!fe || !img0_dev || !img1_dev || img_stride < fe->frame_bytes) { av_set_error("av_frontend_prestage: bad arguments"); return AV_E_INVALID; }
    if (!(fe->cfg.flags & AV_FE_INPUTS_PERSIST)) { av_set_error("av_frontend_prestage: the engine was created without AV_FE_INPUTS_PERSIST"); return AV_E_INVALID; }
    if (photo_ready(fe, "av_frontend_prestage") || expo_ready(fe, "av_frontend_prestage", fe->d.S, true)) return AV_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    AV_HIP(hipSetDevice(fe->device));
    bool wrote_l0 = true;
    const int rc = input_stage(fe, img0_dev, img1_dev, img_stride, fe->parity ^ 1, true, st, &wrote_l0);      // the slots the next step will call cur / 2
    if (rc) return rc;
    fe->fed = true;
    // (The detector's pass over the new cam0 image -- it reads nothing but the image -- enqueued here as well ran at its exclusive speed,
    //  1.55 ms against 2.3 beside the filter's back end, and the LK launches took what it gave back: 173.4-173.9 against 174.1-175.2 k
    //  frames/s.  profiles/r05/README.md)
    fe->pre_on = true; fe->pre_wrote_l0 = wrote_l0; fe->pre_img0 = img0_dev; fe->pre_img1 = img1_dev; fe->pre_stride = img_stride;
    return AV_OK;
}

AV_EXPORT int av_frontend_step(av_frontend* fe, const uint8_t* img0_dev, const uint8_t* img1_dev, int64_t img_stride,
                               const double* timestamps, void* stream)
{
    const ExpoDone done{fe};
    if (!fe || !img0_dev || !img1_dev || !timestamps || img_stride < fe->frame_bytes) {
        av_set_error("av_frontend_step: bad arguments");
        return AV_E_INVALID;
    }
    if (photo_ready(fe, "av_frontend_step")) return AV_E_INVALID;
    const bool prestaged = fe->pre_on && fe->pre_img0 == img0_dev && fe->pre_img1 == img1_dev && fe->pre_stride == img_stride;      // (step_impl: it then skips the stage)
    if (expo_ready(fe, "av_frontend_step", fe->d.S, !prestaged)) return AV_E_INVALID;
    return step_impl(fe, img0_dev, img1_dev, img_stride, timestamps, (hipStream_t)stream, (fe->cfg.flags & AV_FE_INPUTS_PERSIST) != 0);
}

AV_EXPORT int av_frontend_step_host(av_frontend* fe, const uint8_t* img0_host, const uint8_t* img1_host, int64_t img_stride,
                                    const double* timestamps, void* stream)
{
    const ExpoDone done{fe};
    if (!fe || !img0_host || !img1_host || !timestamps || img_stride < fe->frame_bytes) {
        av_set_error("av_frontend_step_host: bad arguments");
        return AV_E_INVALID;
    }
    if (photo_ready(fe, "av_frontend_step_host") || expo_ready(fe, "av_frontend_step_host", fe->d.S, true)) return AV_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t img_bytes = (size_t)fe->frame_bytes;                  // the staging slots carry the frames in their own format and size
    const int S = fe->d.S;
    AV_HIP(hipSetDevice(fe->device));
    av_frontend::HostSlot& h = fe->hs[fe->hs_next];
    fe->hs_next = (fe->hs_next + 1) % 3;
    int rc0;
    if (!fe->copy_stream && (rc0 = fe->res.stream(&fe->copy_stream, hipStreamNonBlocking, 0))) return rc0;
    if (!h.consumed) {                       // (the last of the four: a slot whose set-up failed halfway is set up again, what it got before stays with the owner)
        if ((rc0 = fe->res.pinned_bytes(&h.pin, 2 * img_bytes * S)) || (rc0 = fe->res.dev_bytes(&h.dev, 2 * img_bytes * S)) ||
            (rc0 = fe->res.event(&h.copied, hipEventDisableTiming)) || (rc0 = fe->res.event(&h.consumed, hipEventDisableTiming))) return rc0;
    }
    // the slot was filled three calls ago and last read two calls ago (as that step's previous cam0 image): wait for the
    // step recorded after it -- every earlier step on the stream has then retired too
    if (h.used) AV_HIP(hipEventSynchronize(h.consumed));
    // caller memory -> pinned slot (the caller's buffers are free again when this returns), all cores
#pragma omp parallel for schedule(static) num_threads(S >= 16 ? 8 : 1)
    for (int i = 0; i < 2 * S; ++i) {
        const int s2 = i >> 1, cam = i & 1;
        memcpy(h.pin + ((size_t)cam * S + s2) * img_bytes, (cam ? img1_host : img0_host) + (size_t)s2 * img_stride, img_bytes);
    }
    AV_HIP(hipMemcpyAsync(h.dev, h.pin, 2 * img_bytes * S, hipMemcpyHostToDevice, fe->copy_stream));
    AV_HIP(hipEventRecord(h.copied, fe->copy_stream));
    AV_HIP(hipStreamWaitEvent(st, h.copied, 0));
    const int rc = step_impl(fe, h.dev, h.dev + img_bytes * S, (int64_t)img_bytes, timestamps, st, true);      // staging slots outlive the next step
    if (rc) return rc;
    // `consumed` of the slot filled ONE call ago is recorded now: this step was the last reader of its cam0 image
    av_frontend::HostSlot& hp = fe->hs[(fe->hs_next + 1) % 3];
    if (hp.consumed) { AV_HIP(hipEventRecord(hp.consumed, st)); hp.used = true; }
    AV_HIP(hipEventRecord(h.consumed, st));
    h.used = true;
    return AV_OK;
}

// ---- shared frame store -------------------------------------------------------------------------------------------------
AV_EXPORT int av_frontend_frames_reserve(av_frontend* fe, int n_slots)
{
    if (!fe || n_slots <= 0) { av_set_error("av_frontend_frames_reserve: bad arguments"); return AV_E_INVALID; }
    av_frontend::FrameStore& fs = fe->fs;
    if (fs.n_slots) {
        if (n_slots <= fs.n_slots) return AV_OK;
        av_set_error("av_frontend_frames_reserve: the store holds %d entries and cannot grow (asked for %d)", fs.n_slots, n_slots);
        return AV_E_INVALID;
    }
    AV_HIP(hipSetDevice(fe->device));
    const FeDev& d = fe->d;
    const size_t hw = (size_t)d.w * d.h;
    int rc;
    if ((rc = fe->res.dev(&fs.img, (size_t)n_slots * 2 * hw)) || (rc = fe->res.dev(&fs.pyr, (size_t)n_slots * 2 * fe->lay.bytes)) ||
        (rc = fe->res.dev(&fs.tile_kp, (size_t)n_slots * d.n_tiles * d.tile_cap)) || (rc = fe->res.dev(&fs.tile_count, (size_t)n_slots * d.n_tiles))) return rc;
    if (fe->clahe && (rc = fe->res.dev(&fe->fs_lut, (size_t)n_slots * 2 * fe->cfg.clahe_tiles_x * fe->cfg.clahe_tiles_y * 256))) return rc;
    if ((rc = fe->res.event(&fs.uploaded, hipEventDisableTiming)) || (rc = fe->res.event(&fs.stepped, hipEventDisableTiming))) return rc;
    if (!fe->copy_stream && (rc = fe->res.stream(&fe->copy_stream, hipStreamNonBlocking, 0))) return rc;
    fs.prev.assign((size_t)d.S, -1);
    if (fe->expo) fs.k.assign((size_t)2 * n_slots, 0);
    fs.n_slots = n_slots;
    return AV_OK;
}

AV_EXPORT int av_frontend_frames_upload(av_frontend* fe, const int32_t* slots, int n, const uint8_t* img0_host, const uint8_t* img1_host,
                                        int64_t img_stride, void* stream)
{
    (void)stream;
    const ExpoDone done{fe};
    if (!fe || n < 0 || (n > 0 && (!slots || !img0_host || !img1_host)) || img_stride < fe->frame_bytes) {
        av_set_error("av_frontend_frames_upload: bad arguments");
        return AV_E_INVALID;
    }
    av_frontend::FrameStore& fs = fe->fs;
    if (!fs.n_slots) { av_set_error("av_frontend_frames_upload: no frame store (av_frontend_frames_reserve first)"); return AV_E_INVALID; }
    if (photo_ready(fe, "av_frontend_frames_upload")) return AV_E_INVALID;
    if (n == 0) return AV_OK;
    if (expo_ready(fe, "av_frontend_frames_upload", n, true)) return AV_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= fs.n_slots) { av_set_error("av_frontend_frames_upload: entry %d outside the store (%d entries)", slots[i], fs.n_slots); return AV_E_INVALID; }
    if (fe->clahe) {                 // the entries are equalised where they lie: one named twice would be equalised twice, or half
        std::vector<char> seen((size_t)fs.n_slots, 0);
        for (int i = 0; i < n; ++i) {
            if (seen[slots[i]]) { av_set_error("av_frontend_frames_upload: entry %d is named twice in one upload (not allowed with AV_FE_CLAHE)", slots[i]); return AV_E_INVALID; }
            seen[slots[i]] = 1;
        }
    }
    AV_HIP(hipSetDevice(fe->device));
    const FeDev& d = fe->d;
    const size_t hw = (size_t)d.w * d.h;
    const bool conv = fe->fmt != AV_PIX_GRAY8, bin = fe->ds > 1;
    const bool raw = conv || bin || fe->photo;                      // the frames go through a kernel on their way into the store
    const size_t in_hw = (size_t)fe->in_w * fe->in_h;
    const size_t fb = (size_t)fe->frame_bytes;                           // bytes of one camera's frame as the caller hands it over
    av_frontend::FrameStore::Up& u = fs.up[fs.up_next];
    fs.up_next = (fs.up_next + 1) % 4;
    if (u.used) AV_HIP(hipEventSynchronize(u.done));                // the staging area's previous upload has left it
    AvResources& res = fe->res;
    int rc;
    if ((size_t)n > u.cap) {
        u.cap = 0;                   // (a failure below leaves the entry empty: the next upload builds it again)
        res.free_pinned(u.pin); res.free_pinned(u.idx_h); res.free_dev(u.idx_d); res.free_dev(u.raw_d); res.free_pinned(u.k_h); res.free_dev(u.k_d);
        const size_t cap = (size_t)n + 16;
        if ((rc = res.pinned_bytes(&u.pin, cap * 2 * fb)) || (rc = res.pinned_bytes(&u.idx_h, (raw ? 2 : 1) * cap * sizeof(int))) ||
            (rc = res.dev_bytes(&u.idx_d, (raw ? 2 : 1) * cap * sizeof(int))) || (raw && (rc = res.dev_bytes(&u.raw_d, cap * 2 * fb))) ||
            (fe->expo && ((rc = res.pinned_bytes(&u.k_h, cap * 2 * sizeof(uint16_t))) || (rc = res.dev_bytes(&u.k_d, cap * 2 * sizeof(uint16_t))))) ||
            (!u.done && (rc = res.event(&u.done, hipEventDisableTiming)))) return rc;
        u.cap = cap;
    }
    // The store's scratches follow AvResources::regrow: earlier uploads' launches on the copy stream may still read the old block, so the
    // caller stalls once per growth (an upload larger than any before it), never otherwise
    if ((conv || fe->photo) && bin && (rc = res.regrow(&fs.gray_d, &fs.gray_cap, (size_t)n, 2 * in_hw, fe->copy_stream))) return rc;
    if (fe->mosaic && (rc = res.regrow(&fs.mosaic_d, &fs.mosaic_cap, (size_t)n, 2 * in_hw, fe->copy_stream))) return rc;      // a packed mosaic format
    if (fe->g16.mode == AV_GRAY16_AUTO && (size_t)n > fs.range_cap) {      // the histograms and records; zeroed once, on the copy stream
        if ((rc = res.regrow(&fs.range_d, &fs.range_cap, (size_t)n, AV_GRAY16_WORK_WORDS * sizeof(uint32_t), fe->copy_stream))) return rc;
        AV_HIP(hipMemsetAsync(fs.range_d, 0, fs.range_cap * AV_GRAY16_WORK_WORDS * sizeof(uint32_t), fe->copy_stream));
    }
#pragma omp parallel for schedule(static) num_threads(n >= 8 ? 8 : 1)
    for (int i = 0; i < 2 * n; ++i) {
        const int f = i >> 1, cam = i & 1;
        memcpy(u.pin + ((size_t)2 * f + cam) * fb, (cam ? img1_host : img0_host) + (size_t)f * img_stride, fb);
    }
    for (int i = 0; i < n; ++i) u.idx_h[i] = slots[i];
    if (raw) {                       // the list of the launch that writes the store: an entry named twice is written by its last frame only (what the copies of grey frames leave)
        std::vector<int> last((size_t)fs.n_slots, -1);
        for (int i = 0; i < n; ++i) last[slots[i]] = i;
        for (int i = 0; i < n; ++i) u.idx_h[n + i] = last[slots[i]] == i ? slots[i] : -1;
    }
    hipStream_t cs = fe->copy_stream;
    // The entries handed to an upload are free as of the newest ENQUEUED step (the caller's promise): the copies wait for that step
    // and run beside whatever the caller enqueues next -- upload the frames of step k + 1 before enqueueing step k and the two overlap.
    if (fs.any_step) AV_HIP(hipStreamWaitEvent(cs, fs.stepped, 0));
    AV_HIP(hipMemcpyAsync(u.idx_d, u.idx_h, sizeof(int) * (raw ? 2 : 1) * n, hipMemcpyHostToDevice, cs));
    if (fe->expo) {                  // the upload's factors travel with it: [2][n] by position; an entry keeps those of the last frame that names it
        memcpy(u.k_h, fe->ex_pend.data(), sizeof(uint16_t) * 2 * n);
        AV_HIP(hipMemcpyAsync(u.k_d, u.k_h, sizeof(uint16_t) * 2 * n, hipMemcpyHostToDevice, cs));
        for (int i = 0; i < n; ++i) { fs.k[2 * (size_t)slots[i]] = u.k_h[i]; fs.k[2 * (size_t)slots[i] + 1] = u.k_h[n + i]; }
        fe->ex_pending = false;
    }
    if (raw) AV_HIP(hipMemcpyAsync(u.raw_d, u.pin, (size_t)n * 2 * fb, hipMemcpyHostToDevice, cs));      // to the ring entry's device buffer in one copy: the grey chain takes them into their store entries
    for (int i = 0; i < n && !raw;) {                                // 8-bit grey at full size: straight into the entries, runs of consecutive ones in one copy
        int j = i + 1;
        while (j < n && slots[j] == slots[j - 1] + 1) ++j;
        AV_HIP(hipMemcpyAsync(fs.img + (size_t)slots[i] * 2 * hw, u.pin + (size_t)i * 2 * hw, (size_t)(j - i) * 2 * hw, hipMemcpyHostToDevice, cs));
        i = j;
    }
    // grey_chain as in a step, but indexed, in place in the store, on the copy stream and outside the step's timing spans.  With both
    // conversion and binning every frame of the upload goes to full-size grey in upload order and the binning picks the ones that
    // reach the store; AV_FE_CLAHE equalises the entries once, where they lie, before anything reads them (the tables by position in
    // this upload)
    const FrameSet l0{{fs.img, fs.img + hw}, (int64_t)(2 * hw), u.idx_d};
    const FrameSet gray = fs.gray_d ? FrameSet{{fs.gray_d, fs.gray_d + in_hw}, (int64_t)(2 * in_hw), nullptr} : FrameSet{};
    const FrameSet mosaic = fs.mosaic_d ? FrameSet{{fs.mosaic_d, fs.mosaic_d + in_hw}, (int64_t)(2 * in_hw), nullptr} : FrameSet{};
    FrameSet level0;
    if ((rc = grey_chain(fe, raw ? av_frames(u.raw_d, u.raw_d + fb, (int64_t)(2 * fb)) : l0, n, l0, raw ? u.idx_d + n : nullptr, gray, mosaic, fe->fs_lut,
                         fs.range_d, fs.range_d ? fs.range_d + fs.range_cap * 4096 : nullptr, fe->expo ? u.k_d : nullptr, fe->expo ? u.k_d + n : nullptr, cs, &level0))) return rc;
    bool wrote_l0 = true;
    if ((rc = av_launch_pyramid(level0, n, fe->geom, fs.pyr, 2 * fe->lay.bytes, fe->lay.bytes, 0, 1, cs, false, &wrote_l0))) return rc;
    fs.l0_in_place = !wrote_l0;
    fe->fed = true;                                 // the detector reads the masks now: from here on they stay (av_frontend_set_masks)
    if ((rc = av_launch_fast(store_view(fe, 0, u.idx_d), &fe->geom, d.smask0, 0, n, d.w, d.h, fe->cfg.fast_threshold, d.rbits,
                             nullptr, nullptr, 0, fs.tile_kp, fs.tile_count, nullptr, 0, cs))) return rc;
    AV_HIP(hipEventRecord(u.done, cs));
    AV_HIP(hipEventRecord(fs.uploaded, cs));
    u.used = true; fs.any_upload = true;
    fs.frames_uploaded += n;
    return AV_OK;
}

AV_EXPORT int av_frontend_step_frames(av_frontend* fe, const int32_t* slot_of_stream, const double* timestamps, void* stream)
{
    if (!fe || !slot_of_stream || !timestamps) { av_set_error("av_frontend_step_frames: bad arguments"); return AV_E_INVALID; }
    if (!fe->fs.n_slots) { av_set_error("av_frontend_step_frames: no frame store (av_frontend_frames_reserve first)"); return AV_E_INVALID; }
    for (int s = 0; s < fe->d.S; ++s)
        if (slot_of_stream[s] >= fe->fs.n_slots) { av_set_error("av_frontend_step_frames: stream %d: entry %d outside the store (%d entries)", s, slot_of_stream[s], fe->fs.n_slots); return AV_E_INVALID; }
    return step_impl(fe, nullptr, nullptr, 0, timestamps, (hipStream_t)stream, true, slot_of_stream);
}

// Stream restart (include/airvision.h, "Stream restart").  Host state is consumed inside the step calls, so it is reset at once; the
// device state by restart_kernel on `stream`, behind whatever the caller has enqueued there (a step, a prestage, a pending read-back)
// and ahead of the step it enqueues next.
AV_EXPORT int av_frontend_restart(av_frontend* fe, const int32_t* stream_idx, int n, void* stream)
{
    if (!fe || n < 0 || (n > 0 && !stream_idx)) { av_set_error("av_frontend_restart: bad arguments"); return AV_E_INVALID; }
    const int S = fe->d.S;
    for (int i = 0; i < n; ++i) if (stream_idx[i] < 0 || stream_idx[i] >= S) { av_set_error("av_frontend_restart: stream %d out of range", stream_idx[i]); return AV_E_INVALID; }
    if (n == 0) return AV_OK;
    hipStream_t st = (hipStream_t)stream;
    AV_HIP(hipSetDevice(fe->device));
    int* list = nullptr;
    int rc = fe->rs_h.take(&list);
    if (rc) return rc;
    int m = 0;
    std::vector<char> seen((size_t)S, 0);                    // a repeated index is listed once (the pinned slot holds S entries)
    for (int i = 0; i < n; ++i) {
        const int s = stream_idx[i];
        if (seen[s]) continue;
        seen[s] = 1;
        StreamHost& sh = fe->streams[s];
        {
            std::lock_guard<std::mutex> g(sh.mu);
            sh.imu.clear(); sh.t_prev = 0.0; sh.first = true; sh.frame = 0;
        }
        if (!fe->fs.prev.empty()) fe->fs.prev[s] = -1;
        list[m++] = s;
    }
    fe->any_first = true;
    int* list_d = fe->rs_d + (size_t)fe->rs_h.cur * S;
    AV_HIP(hipMemcpyAsync(list_d, list, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, st));
    if ((rc = fe->rs_h.sent(st))) return rc;
    hipLaunchKernelGGL(restart_kernel, dim3((m + 63) / 64), dim3(64), 0, st, fe->d, (const int*)list_d, m, fe->ransac ? fe->rs_counts : nullptr);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

AV_EXPORT int av_frontend_max_features(const av_frontend* fe) { return fe ? fe->d.MAXF : AV_E_INVALID; }

// The feature_msg of the last step where it lies on the device (consumed by av_msckf_batch_submit_dev)
AV_EXPORT int av_frontend_features_dev(av_frontend* fe, const int64_t** ids_dev, const double** uv_dev, const int32_t** n_dev, int* cap)
{
    if (!fe || !ids_dev || !uv_dev || !n_dev || !cap) { av_set_error("av_frontend_features_dev: bad arguments"); return AV_E_INVALID; }
    static_assert(sizeof(long long) == sizeof(int64_t), "feature ids");
    *ids_dev = reinterpret_cast<const int64_t*>(fe->d.out_ids); *uv_dev = fe->d.out_uv; *n_dev = fe->d.out_n; *cap = fe->d.MAXF;
    return AV_OK;
}

// Read-back in two halves.  _begin enqueues the device-to-host copies of the features published by the last step into
// pinned slot `slot` (0/1) behind everything already on `stream` and returns; _end waits for exactly those copies and
// unpacks them into the caller's arrays.  A caller that enqueues the NEXT step between the two keeps the GPU busy while
// it consumes this frame's features.
AV_EXPORT int av_frontend_read_features_begin(av_frontend* fe, int slot, void* stream)
{
    if (!fe || slot < 0 || slot > 1) { av_set_error("av_frontend_read_features_begin: bad arguments"); return AV_E_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    const FeDev& d = fe->d;
    av_frontend::ReadSlot& r = fe->rd[slot];
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipMemcpyAsync(r.n, d.out_n, sizeof(int) * d.S, hipMemcpyDeviceToHost, st));
    AV_HIP(hipMemcpyAsync(r.ids, d.out_ids, sizeof(long long) * d.S * d.MAXF, hipMemcpyDeviceToHost, st));
    AV_HIP(hipMemcpyAsync(r.uv, d.out_uv, sizeof(double) * 4 * d.S * d.MAXF, hipMemcpyDeviceToHost, st));
    AV_HIP(hipMemcpyAsync(r.cnt, d.counters, sizeof(int) * d.S * NCNT, hipMemcpyDeviceToHost, st));
    AV_HIP(hipEventRecord(r.ev, st));
    r.pending = true;
    return AV_OK;
}

AV_EXPORT int av_frontend_read_features_end(av_frontend* fe, int slot, int64_t* ids_out, double* uv_out, int32_t* n_out, int cap)
{
    if (!fe || slot < 0 || slot > 1 || !ids_out || !uv_out || !n_out || cap < fe->d.MAXF) { av_set_error("av_frontend_read_features_end: bad arguments"); return AV_E_INVALID; }
    const FeDev& d = fe->d;
    av_frontend::ReadSlot& r = fe->rd[slot];
    if (!r.pending) { av_set_error("av_frontend_read_features_end: no read-back was begun on slot %d", slot); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipEventSynchronize(r.ev));
    r.pending = false;
    int ovf = 0;
#pragma omp parallel for schedule(static) num_threads(d.S >= 64 ? 4 : 1) reduction(|:ovf)
    for (int s = 0; s < d.S; ++s) {
        const int n = r.n[s];
        n_out[s] = n;
        memcpy(ids_out + (size_t)s * cap, r.ids + (size_t)s * d.MAXF, sizeof(long long) * (size_t)n);
        memcpy(uv_out + (size_t)s * cap * 4, r.uv + (size_t)s * d.MAXF * 4, sizeof(double) * 4 * (size_t)n);
        ovf |= r.cnt[(size_t)s * NCNT + CNT_OVF];
    }
    if (ovf) { av_set_error("front-end device buffer overflow (flags 0x%x): raise max_corners", ovf); return AV_E_CAPACITY; }
    return AV_OK;
}

AV_EXPORT int av_frontend_read_features(av_frontend* fe, int64_t* ids_out, double* uv_out, int32_t* n_out, int cap, void* stream)
{
    int rc = av_frontend_read_features_begin(fe, 0, stream);
    if (rc) return rc;
    return av_frontend_read_features_end(fe, 0, ids_out, uv_out, n_out, cap);
}

AV_EXPORT int av_frontend_read_grid(av_frontend* fe, int stream_idx, int64_t* ids, int32_t* lifetime, int32_t* cell,
                                    float* pts, int cap, int32_t* n_out, int64_t* next_feature_id, void* stream)
{
    if (!fe || stream_idx < 0 || stream_idx >= fe->d.S || !ids || !lifetime || !cell || !pts || !n_out || cap < fe->d.MAXF) {
        av_set_error("av_frontend_read_grid: bad arguments");
        return AV_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    const FeDev& d = fe->d;
    const int b = fe->parity;        // after a step, parity indexes the grid just published
    const size_t o = (size_t)stream_idx * d.MAXF;
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipStreamSynchronize(st));
    int n = 0; long long nid = 0;
    AV_HIP(hipMemcpy(&n, d.n_feat[b] + stream_idx, sizeof(int), hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(&nid, d.next_id + stream_idx, sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<float> p0(2 * (size_t)d.MAXF), p1(2 * (size_t)d.MAXF);
    std::vector<long long> idv(d.MAXF);
    AV_HIP(hipMemcpy(idv.data(), d.feat_id[b] + o, sizeof(long long) * d.MAXF, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(lifetime, d.feat_life[b] + o, sizeof(int) * d.MAXF, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(cell, d.feat_cell[b] + o, sizeof(int) * d.MAXF, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(p0.data(), d.feat_p0[b] + 2 * o, sizeof(float) * 2 * d.MAXF, hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(p1.data(), d.feat_p1[b] + 2 * o, sizeof(float) * 2 * d.MAXF, hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) {
        ids[k] = idv[k];
        pts[4 * k] = p0[2 * k]; pts[4 * k + 1] = p0[2 * k + 1]; pts[4 * k + 2] = p1[2 * k]; pts[4 * k + 3] = p1[2 * k + 1];
    }
    *n_out = n;
    if (next_feature_id) *next_feature_id = nid;
    return AV_OK;
}

// [candidates matched in round 1, in round 2] of the last step for one stream (the lazy stereo matching of
// cand_round2_kernel): the LK point passes actually run for new-feature candidates.  Synchronises.
AV_EXPORT int av_frontend_read_match_counts(av_frontend* fe, int stream_idx, int32_t out[2], void* stream)
{
    if (!fe || !out || stream_idx < 0 || stream_idx >= fe->d.S) { av_set_error("av_frontend_read_match_counts: bad arguments"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    AV_HIP(hipMemcpy(out, fe->d.r1_count + stream_idx, sizeof(int), hipMemcpyDeviceToHost));
    AV_HIP(hipMemcpy(out + 1, fe->d.r2_count + stream_idx, sizeof(int), hipMemcpyDeviceToHost));
    return AV_OK;
}

AV_EXPORT int av_frontend_read_counters(av_frontend* fe, int stream_idx, int32_t out[8], void* stream)
{
    if (!fe || stream_idx < 0 || stream_idx >= fe->d.S || !out) { av_set_error("av_frontend_read_counters: bad arguments"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    AV_HIP(hipMemcpy(out, fe->d.counters + (size_t)stream_idx * NCNT, sizeof(int) * NCNT, hipMemcpyDeviceToHost));
    return AV_OK;
}

AV_EXPORT int av_frontend_read_ransac_counts(av_frontend* fe, int stream_idx, int32_t out[4], void* stream)
{
    if (!fe || stream_idx < 0 || stream_idx >= fe->d.S || !out) { av_set_error("av_frontend_read_ransac_counts: bad arguments"); return AV_E_INVALID; }
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (!fe->ransac) return AV_OK;
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    AV_HIP(hipMemcpy(out, fe->rs_counts + (size_t)stream_idx * 4, sizeof(int) * 4, hipMemcpyDeviceToHost));
    return AV_OK;
}

AV_EXPORT int av_frontend_read_image(av_frontend* fe, int stream_idx, int cam, uint8_t* out_host, void* stream)
{
    if (!fe || stream_idx < 0 || stream_idx >= fe->d.S || cam < 0 || cam > 1 || !out_host) { av_set_error("av_frontend_read_image: bad arguments"); return AV_E_INVALID; }
    if (!fe->own_l0) { av_set_error("av_frontend_read_image: the engine was created without AV_FE_CLAHE or AV_FE_PHOTOMETRIC, with 8-bit grey input and without image_downscale: level 0 is the caller's own image"); return AV_E_INVALID; }
    if (!fe->stepped) { av_set_error("av_frontend_read_image: no step has run yet"); return AV_E_INVALID; }
    if (cam == 1 && fe->pre_on && !fe->stepped_frames) {
        av_set_error("av_frontend_read_image: the cam1 image of the last step has been replaced by av_frontend_prestage (read it before prestaging)");
        return AV_E_INVALID;
    }
    const size_t hw = (size_t)fe->d.w * fe->d.h;
    const uint8_t* src;
    if (fe->stepped_frames) {                        // the last step read the frame store
        const int e = fe->fs.prev[stream_idx];
        if (e < 0) { av_set_error("av_frontend_read_image: stream %d has not had a frame yet", stream_idx); return AV_E_INVALID; }
        src = fe->fs.img + ((size_t)2 * e + cam) * hw;
    } else {
        src = fe->eq + ((size_t)(cam ? 2 : fe->parity) * fe->d.S + stream_idx) * hw;      // after a step, parity is the slot of the frame just used
    }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (fe->copy_stream) AV_HIP(hipStreamSynchronize(fe->copy_stream));
    AV_HIP(hipMemcpy(out_host, src, hw, hipMemcpyDeviceToHost));
    return AV_OK;
}

// ---- range scaling of 16-bit grey ("Range scaling of 16-bit grey" in include/airvision.h) -----------------------------------
AV_EXPORT int av_frontend_set_gray16_scale(av_frontend* fe, int scale, int lo, int hi, int clip_lo_ppm, int clip_hi_ppm, int min_span)
{
    if (!fe) { av_set_error("av_frontend_set_gray16_scale: bad arguments"); return AV_E_INVALID; }
    if (fe->fed) {
        av_set_error("av_frontend_set_gray16_scale: the engine has already been handed a frame (step, prestage or frames_upload): the frames in it "
                     "would disagree with the new scale; set the scale of an engine before its first frame");
        return AV_E_INVALID;
    }
    if (scale != AV_GRAY16_SHIFT) {
        if (av_range16_check(scale, lo, hi, clip_lo_ppm, clip_hi_ppm, min_span, "av_frontend_set_gray16_scale")) return AV_E_INVALID;
        if (fe->fmt != AV_PIX_GRAY16) {
            av_set_error("av_frontend_set_gray16_scale: gray16_scale %d ('%s') applies to pixel_format AV_PIX_GRAY16 ('gray16') only, not to %d ('%s')", scale,
                         scale == AV_GRAY16_WINDOW ? "window" : "auto", fe->fmt, av_pixfmt_name(fe->fmt));
            return AV_E_INVALID;
        }
    }
    if (scale == AV_GRAY16_AUTO && !fe->g16_rec) {      // histograms [S][4096] and records [2][S][4], zeroed; once per engine
        AV_HIP(hipSetDevice(fe->device));
        int rc;
        if ((rc = fe->res.dev(&fe->g16_hist, (size_t)fe->d.S * 4096)) || (rc = fe->res.dev(&fe->g16_rec, (size_t)2 * fe->d.S * 4))) return rc;
    }
    fe->g16.mode = scale; fe->g16.lo = lo; fe->g16.hi = hi; fe->g16.ppm_lo = clip_lo_ppm; fe->g16.ppm_hi = clip_hi_ppm; fe->g16.min_span = min_span;
    return AV_OK;
}

AV_EXPORT int av_frontend_read_range(av_frontend* fe, int32_t* range_out_host, void* stream)
{
    if (!fe || !range_out_host) { av_set_error("av_frontend_read_range: bad arguments"); return AV_E_INVALID; }
    if (fe->g16.mode == AV_GRAY16_SHIFT) { av_set_error("av_frontend_read_range: the engine scales 16-bit data by a fixed shift (no av_frontend_set_gray16_scale to a window or a range): there is no range"); return AV_E_INVALID; }
    if (!fe->stepped) { av_set_error("av_frontend_read_range: no step has run yet"); return AV_E_INVALID; }
    if (fe->stepped_frames) { av_set_error("av_frontend_read_range: the last step read the frame store, whose entries are shared by streams and keep no range"); return AV_E_INVALID; }
    const int S = fe->d.S;
    if (fe->g16.mode == AV_GRAY16_WINDOW) {
        for (int s = 0; s < S; ++s) { range_out_host[2 * s] = fe->g16.lo; range_out_host[2 * s + 1] = fe->g16.hi; }
        return AV_OK;
    }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipStreamSynchronize((hipStream_t)stream));
    std::vector<uint32_t> rec((size_t)4 * S);
    AV_HIP(hipMemcpy(rec.data(), fe->g16_rec + (size_t)fe->parity * 4 * S, rec.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));      // after a step, parity is the slot of the frame just used
    for (int s = 0; s < S; ++s) { range_out_host[2 * s] = (int32_t)rec[4 * s]; range_out_host[2 * s + 1] = (int32_t)rec[4 * s + 1]; }
    return AV_OK;
}

// ---- static per-camera masks ("Static masks" in include/airvision.h) ------------------------------------------------------
AV_EXPORT int av_frontend_set_masks(av_frontend* fe, const uint8_t* mask0_host, const uint8_t* mask1_host)
{
    if (!fe) { av_set_error("av_frontend_set_masks: bad arguments"); return AV_E_INVALID; }
    if (fe->fed) {
        av_set_error("av_frontend_set_masks: the engine has already been handed a frame (step, prestage or frames_upload): the corners found in it "
                     "would disagree with the new masks; set the masks of an engine before its first frame");
        return AV_E_INVALID;
    }
    AV_HIP(hipSetDevice(fe->device));
    FeDev& d = fe->d;
    const size_t hw = (size_t)d.w * d.h;
    const int f = fe->ds;
    const uint8_t* src[2] = {mask0_host, mask1_host};
    const uint8_t* set[2] = {nullptr, nullptr};
    std::vector<uint8_t> bin(hw);
    for (int cam = 0; cam < 2; ++cam) {
        if (!src[cam]) continue;
        // the mask of the processed image: a pixel is scene iff all f x f input pixels under it are; stored as 0 / 1
        for (int y = 0; y < d.h; ++y)
            for (int x = 0; x < d.w; ++x) {
                uint8_t v = 1;
                for (int j = 0; j < f; ++j)
                    for (int i = 0; i < f; ++i) v &= src[cam][(size_t)(y * f + j) * fe->in_w + (size_t)x * f + i] != 0;
                bin[(size_t)y * d.w + x] = v;
            }
        int rc;
        if (!fe->smask_buf[cam] && (rc = fe->res.dev(&fe->smask_buf[cam], hw))) return rc;
        AV_HIP(hipMemcpy(fe->smask_buf[cam], bin.data(), hw, hipMemcpyHostToDevice));
        set[cam] = fe->smask_buf[cam];
    }
    d.smask0 = set[0]; d.smask1 = set[1];
    return AV_OK;
}

AV_EXPORT int av_frontend_read_mask(av_frontend* fe, int cam, uint8_t* out_host)
{
    if (!fe || cam < 0 || cam > 1 || !out_host) { av_set_error("av_frontend_read_mask: bad arguments"); return AV_E_INVALID; }
    const uint8_t* m = cam ? fe->d.smask1 : fe->d.smask0;
    if (!m) { av_set_error("av_frontend_read_mask: no mask is set for camera %d", cam); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipMemcpy(out_host, m, (size_t)fe->d.w * fe->d.h, hipMemcpyDeviceToHost));
    return AV_OK;
}

// ---- photometric calibration ("Photometric calibration" in include/airvision.h) ----------------------------------------------
AV_EXPORT int av_frontend_set_photometric(av_frontend* fe, const uint16_t* response0_host, const uint16_t* gain0_host,
                                          const uint16_t* response1_host, const uint16_t* gain1_host)
{
    if (!fe) { av_set_error("av_frontend_set_photometric: bad arguments"); return AV_E_INVALID; }
    if (!fe->photo_tables) { av_set_error("av_frontend_set_photometric: the engine was created without AV_FE_PHOTOMETRIC"); return AV_E_INVALID; }
    if (fe->fed) {
        av_set_error("av_frontend_set_photometric: the engine has already been handed a frame (step, prestage or frames_upload): the frames in it "
                     "would disagree with the new tables; set the tables of an engine before its first frame");
        return AV_E_INVALID;
    }
    const uint16_t* resp[2] = {response0_host, response1_host};
    const uint16_t* gain[2] = {gain0_host, gain1_host};
    for (int cam = 0; cam < 2; ++cam)
        for (int i = 0; resp[cam] && i < 256; ++i)
            if (resp[cam][i] > AV_PHOTOMETRIC_RESPONSE_MAX) {
                av_set_error("av_frontend_set_photometric: response%d[%d] = %d is above %d (255 in Q8)", cam, i, (int)resp[cam][i], AV_PHOTOMETRIC_RESPONSE_MAX);
                return AV_E_INVALID;
            }
    AV_HIP(hipSetDevice(fe->device));
    const size_t in_hw = (size_t)fe->in_w * fe->in_h;
    // a camera without either part gets the identity response, so that one stage serves both cameras (with no part at all: the
    // identity stage).  The engine has no tables while the copies run: a call that fails half way leaves it refusing frames, not
    // holding half of the new tables
    fe->photo_set = false;
    for (int cam = 0; cam < 2; ++cam) { fe->ph_resp[cam] = nullptr; fe->ph_gain[cam] = nullptr; }
    uint16_t ident[256];
    for (int i = 0; i < 256; ++i) ident[i] = (uint16_t)(i << 8);
    const uint16_t* new_resp[2] = {nullptr, nullptr};
    const uint16_t* new_gain[2] = {nullptr, nullptr};
    for (int cam = 0; cam < 2; ++cam) {
        const bool bare = !resp[cam] && !gain[cam];
        const uint16_t* r = resp[cam] ? resp[cam] : bare ? ident : nullptr;
        if (r) {
            AV_HIP(hipMemcpy(fe->ph_resp_buf + 256 * cam, r, sizeof(ident), hipMemcpyHostToDevice));
            new_resp[cam] = fe->ph_resp_buf + 256 * cam;
        }
        if (gain[cam]) {
            int rc;
            if (!fe->ph_gain_buf[cam] && (rc = fe->res.dev(&fe->ph_gain_buf[cam], in_hw))) return rc;
            AV_HIP(hipMemcpy(fe->ph_gain_buf[cam], gain[cam], in_hw * sizeof(uint16_t), hipMemcpyHostToDevice));
            new_gain[cam] = fe->ph_gain_buf[cam];
        }
    }
    for (int cam = 0; cam < 2; ++cam) { fe->ph_resp[cam] = new_resp[cam]; fe->ph_gain[cam] = new_gain[cam]; }
    fe->photo_set = true;
    return AV_OK;
}

AV_EXPORT int av_frontend_read_photometric(av_frontend* fe, int cam, uint16_t* response_out_host, uint16_t* gain_out_host)
{
    if (!fe || cam < 0 || cam > 1) { av_set_error("av_frontend_read_photometric: bad arguments"); return AV_E_INVALID; }
    if (!fe->photo_tables || !fe->photo_set) { av_set_error("av_frontend_read_photometric: no tables are set (AV_FE_PHOTOMETRIC and av_frontend_set_photometric)"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    const size_t in_hw = (size_t)fe->in_w * fe->in_h;
    if (response_out_host) {
        if (fe->ph_resp[cam]) AV_HIP(hipMemcpy(response_out_host, fe->ph_resp[cam], 256 * sizeof(uint16_t), hipMemcpyDeviceToHost));
        else for (int i = 0; i < 256; ++i) response_out_host[i] = (uint16_t)(i << 8);
    }
    if (gain_out_host) {
        if (fe->ph_gain[cam]) AV_HIP(hipMemcpy(gain_out_host, fe->ph_gain[cam], in_hw * sizeof(uint16_t), hipMemcpyDeviceToHost));
        else for (size_t i = 0; i < in_hw; ++i) gain_out_host[i] = 4096;
    }
    return AV_OK;
}

// ---- exposure-time normalisation ("Exposure-time normalisation" in include/airvision.h) ----------------------------------------------
AV_EXPORT int av_frontend_next_exposure(av_frontend* fe, const uint16_t* k0_host, const uint16_t* k1_host, int n)
{
    if (!fe || !k0_host || !k1_host || n <= 0) { av_set_error("av_frontend_next_exposure: bad arguments (a null pointer, or n = %d)", n); return AV_E_INVALID; }
    if (!fe->expo) { av_set_error("av_frontend_next_exposure: the engine was created without AV_FE_EXPOSURE"); return AV_E_INVALID; }
    for (int i = 0; i < n; ++i)
        if (!k0_host[i] || !k1_host[i]) { av_set_error("av_frontend_next_exposure: the factor of cam%d of frame %d is 0 (1 .. 65535 in Q12)", k0_host[i] ? 1 : 0, i); return AV_E_INVALID; }
    fe->ex_pend.resize((size_t)2 * n);
    memcpy(fe->ex_pend.data(), k0_host, sizeof(uint16_t) * n);
    memcpy(fe->ex_pend.data() + n, k1_host, sizeof(uint16_t) * n);
    fe->ex_pend_n = n; fe->ex_pending = true;
    return AV_OK;
}

AV_EXPORT int av_frontend_read_exposure(av_frontend* fe, int stream_idx, uint16_t out2[2])
{
    if (!fe || !out2 || stream_idx < 0 || stream_idx >= fe->d.S) { av_set_error("av_frontend_read_exposure: bad arguments"); return AV_E_INVALID; }
    if (!fe->expo) { av_set_error("av_frontend_read_exposure: the engine was created without AV_FE_EXPOSURE"); return AV_E_INVALID; }
    if (!fe->stepped) { av_set_error("av_frontend_read_exposure: no step has run"); return AV_E_INVALID; }
    out2[0] = fe->ex_last[2 * (size_t)stream_idx]; out2[1] = fe->ex_last[2 * (size_t)stream_idx + 1];
    return AV_OK;
}

AV_EXPORT int av_frontend_enable_timing(av_frontend* fe, int max_spans)
{
    if (!fe || max_spans < 0) { av_set_error("av_frontend_enable_timing: bad arguments"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipDeviceSynchronize());
    for (size_t i = fe->ev.size(); i-- > 0;) fe->res.free_event(fe->ev[i]);
    fe->ev.clear(); fe->ev_cls.clear(); fe->ev_used = 0;
    fe->timing = max_spans > 0;
    for (int i = 0; i < 2 * max_spans; ++i) {
        hipEvent_t e = nullptr;
        int rc = fe->res.event(&e, hipEventDefault);
        if (rc) return rc;
        fe->ev.push_back(e);
    }
    fe->ev_cls.assign((size_t)max_spans, 0);
    return AV_OK;
}

AV_EXPORT int av_frontend_read_timing(av_frontend* fe, double ms_out[4], int32_t spans_out[4])
{
    if (!fe || !ms_out || !spans_out) { av_set_error("av_frontend_read_timing: bad arguments"); return AV_E_INVALID; }
    AV_HIP(hipSetDevice(fe->device));
    AV_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 4; ++i) { ms_out[i] = 0.0; spans_out[i] = 0; }
    for (size_t k = 0; k + 1 < fe->ev_used; k += 2) {
        float ms = 0.f;
        AV_HIP(hipEventElapsedTime(&ms, fe->ev[k], fe->ev[k + 1]));
        int c = fe->ev_cls[k / 2];
        ms_out[c] += (double)ms; spans_out[c] += 1;
    }
    fe->ev_used = 0;
    return AV_OK;
}
