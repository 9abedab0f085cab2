// bayer.hip -- raw colour-filter-array (Bayer mosaic) frames, 8- or 16-bit samples, to tightly packed 8-bit grey (gfx950).
// The definition is written out in include/airvision.h (av_to_gray8, "Bayer mosaics"): reduce the sample (16-bit: min(255, v >> shift)),
// extend by BORDER_REFLECT_101, bilinear R / G / B each times four from the 3 x 3 neighbourhood, grey = (9798 R4 + 19235 G4 + 3735 B4 +
// 65536) >> 17.  tests/bayer_ref.py states it in NumPy and both kernels are held to it bit for bit.
// For every site the grey value is a weighted sum of four numbers -- the centre c, the row neighbours' sum hs, the column neighbours' sum
// vs, the diagonal neighbours' sum ds -- and the weights depend only on the colour phase of (x & 1, y & 1): bayer_weights().  The pattern
// is therefore a launch argument (the phase of the R site), not a template parameter.
//   vector path    w % 16 == 0, every base and every applied stride a multiple of 16 bytes.  A lane owns 16 output columns and walks
//                  down BY_ROWS rows with a rolling window of three rows in registers: one uint4 load per row (two for 16-bit samples),
//                  the sample left and right of its 16 from the neighbouring lanes by wavefront shuffles (only the first and the last
//                  lane of a wavefront load it; at the image's edges it is the lane's own reflected sample), one uint4 store per row.
//                  Lanes run over (strip, column vector) of one image in row-major order, so a wavefront holds neighbouring vectors.
//                  The sums are taken on two 16-bit halves per dword (even and odd columns apart).
//   generic path   anything else: one pixel per lane, neighbouring lanes on neighbouring pixels, nine samples read per pixel.
// Both use the 1-D XCD-aware launch of the pyramid and CLAHE kernels: the workgroups of one image run on one XCD, so the two halo rows
// two strips share are fetched into one L2.  No LDS, 64-bit byte offsets, plain vector stores, never in place.
#include "av_common.h"

namespace {

constexpr int BY_LANE = 16;                    // output columns of one lane of the vector path = one 16-byte store
constexpr int BY_ROWS = 16;                    // output rows a lane walks down (tests/test_gpu_bayer_op.py assumes this value)
constexpr int BY_GEN = 256 * 16;               // pixels of one workgroup of the generic path

struct BayerArgs {
    FramePlace place;
    int w, h, shift;
    int rx, ry;                                    // the R site: (x & 1, y & 1) == (rx, ry); the B site is the opposite corner
    int nvx, items;                                // vector path: vectors per row, (strip, vector) items per image
};

// weights of (c, hs, vs, ds) at a site of phase px = (x & 1) ^ rx, py = (y & 1) ^ ry:
//   (0, 0) R site: R4 = 4c, G4 = hs + vs, B4 = ds      (1, 1) B site: B4 = 4c, G4 = hs + vs, R4 = ds
//   (1, 0) G site in an R row: G4 = 4c, R4 = 2 hs, B4 = 2 vs      (0, 1) G site in a B row: G4 = 4c, B4 = 2 hs, R4 = 2 vs
struct BayerW { uint32_t c, hs, vs, ds; };
__device__ __forceinline__ BayerW bayer_weights(int px, int py)
{
    constexpr uint32_t KR = 9798u, KG = 19235u, KB = 3735u;
    BayerW k;
    if (px == py) { k.c = 4u * (px ? KB : KR); k.hs = KG; k.vs = KG; k.ds = px ? KR : KB; }
    else { k.c = 4u * KG; k.hs = 2u * (py ? KB : KR); k.vs = 2u * (py ? KR : KB); k.ds = 0u; }
    return k;
}
__device__ __forceinline__ uint32_t bayer_grey(const BayerW& k, uint32_t c, uint32_t hs, uint32_t vs, uint32_t ds)
{
    return (k.c * c + k.hs * hs + k.vs * vs + k.ds * ds + 65536u) >> 17;      // at most 32768 * 1020 + 65536
}

template <typename T>
__device__ __forceinline__ uint32_t bayer_sample(const uint8_t* row, int x, int shift)
{
    const uint32_t v = reinterpret_cast<const T*>(row)[x];
    return sizeof(T) == 1 ? v : min(255u, v >> shift);
}

// workgroup -> (image, block of the image): all blocks of an image on one XCD (workgroups are dealt round-robin over the 8 XCDs).
// Placement only: any mapping is correct.
__device__ __forceinline__ bool bayer_place(const BayerArgs& a, int& img, int& blk)
{
    const int L = blockIdx.x, wg = L >> 3;
    img = (L & 7) + 8 * (wg / a.place.per);
    blk = wg % a.place.per;
    return img < a.place.n_img;
}

// one row of 16 reduced samples of a lane, even and odd columns apart, two per dword in 16-bit halves: e[j] = columns 4j, 4j + 2,
// o[j] = columns 4j + 1, 4j + 3; l = column -1 (an odd one), r = column 16 (an even one).  Sums of two rows keep the layout.
struct BayerRow { uint32_t e[4], o[4], l, r; };

__device__ __forceinline__ BayerRow bayer_add(const BayerRow& p, const BayerRow& q)
{
    BayerRow s;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.e[j] = p.e[j] + q.e[j]; s.o[j] = p.o[j] + q.o[j]; }
    s.l = p.l + q.l; s.r = p.r + q.r;
    return s;
}

// the 16 bytes of a row as loaded (16-bit samples reduced and packed first)
template <typename T>
__device__ __forceinline__ void bayer_load16(const uint8_t* p, int shift, uint32_t d[4])
{
    if (sizeof(T) == 1) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
        const uint4 q0 = reinterpret_cast<const uint4*>(p)[0], q1 = reinterpret_cast<const uint4*>(p)[1];
        const uint32_t v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a0 = min(255u, (v[2 * j] & 0xFFFFu) >> shift), a1 = min(255u, (v[2 * j] >> 16) >> shift);
            const uint32_t a2 = min(255u, (v[2 * j + 1] & 0xFFFFu) >> shift), a3 = min(255u, (v[2 * j + 1] >> 16) >> shift);
            d[j] = a0 | a1 << 8 | a2 << 16 | a3 << 24;
        }
    }
}

// Row y of the lane's 16 columns at x0 with its two outer samples.  Every lane of the wavefront calls this (the shuffles need them
// all); `left_own` / `right_own`: the column vector touches the image's edge there and the outer sample is the reflected s(1) / s(w - 2).
template <typename T>
__device__ __forceinline__ BayerRow bayer_fetch(const uint8_t* img, int64_t pitch, int y, int x0, int shift, int lane, bool left_own, bool right_own)
{
    const uint8_t* row = img + (int64_t)y * pitch;
    uint32_t d[4];
    bayer_load16<T>(row + (int64_t)x0 * sizeof(T), shift, d);
    uint32_t l = __shfl_up(d[3], 1) >> 24, r = __shfl_down(d[0], 1) & 255u;
    if (left_own) l = (d[0] >> 8) & 255u;
    else if (lane == 0) l = bayer_sample<T>(row, x0 - 1, shift);
    if (right_own) r = (d[3] >> 16) & 255u;
    else if (lane == 63) r = bayer_sample<T>(row, x0 + BY_LANE, shift);
    BayerRow q;
#pragma unroll
    for (int j = 0; j < 4; ++j) { q.e[j] = d[j] & 0x00FF00FFu; q.o[j] = (d[j] >> 8) & 0x00FF00FFu; }
    q.l = l; q.r = r;
    return q;
}

// sums of the left and right neighbours: for the even columns 4j, 4j + 2 the neighbours are the odd columns 4j - 1, 4j + 1 and 4j + 1,
// 4j + 3; for the odd columns 4j + 1, 4j + 3 they are the even columns 4j, 4j + 2 and 4j + 2, 4j + 4
__device__ __forceinline__ void bayer_sides(const BayerRow& q, uint32_t se[4], uint32_t so[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t lo = j ? q.o[j - 1] >> 16 : q.l, hi = j < 3 ? q.e[j + 1] << 16 : q.r << 16;
        se[j] = (q.o[j] << 16 | lo) + q.o[j];
        so[j] = q.e[j] + (q.e[j] >> 16 | hi);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bayer_to_gray8_kernel(BayerArgs a)
{
    int img, blk;
    FrameAt f;
    if (!bayer_place(a, img, blk) || !av_frame_at(a.place, img, f)) return;
    const uint8_t* src = f.src; uint8_t* dst = f.dst;
    const int item = blk * 256 + (int)threadIdx.x, lane = threadIdx.x & 63;
    const bool live = item < a.items;
    const int it = live ? item : a.items - 1;                     // idle lanes follow the last item: every lane takes part in the shuffles
    const int strip = it / a.nvx, vx = it - strip * a.nvx;
    const int x0 = vx * BY_LANE, y0 = strip * BY_ROWS, w = a.w, h = a.h;
    const int64_t pitch = (int64_t)w * sizeof(T);
    const bool lo = vx == 0, ro = vx == a.nvx - 1;
    // weights by column parity (0: even x) and row parity of y - y0 (y0 is even)
    BayerW k[2][2];
#pragma unroll
    for (int yp = 0; yp < 2; ++yp)
#pragma unroll
        for (int xp = 0; xp < 2; ++xp) k[yp][xp] = bayer_weights(xp ^ a.rx, yp ^ a.ry);
    auto refl = [h](int y) { return y < 0 ? -y : y >= h ? max(0, 2 * h - 2 - y) : y; };      // (rows past h are read only for rows that are not stored)
    BayerRow up = bayer_fetch<T>(src, pitch, refl(y0 - 1), x0, a.shift, lane, lo, ro);
    BayerRow cur = bayer_fetch<T>(src, pitch, refl(y0), x0, a.shift, lane, lo, ro);
#pragma unroll 2
    for (int i = 0; i < BY_ROWS; ++i) {
        const int y = y0 + i;
        const BayerRow dn = bayer_fetch<T>(src, pitch, refl(y + 1), x0, a.shift, lane, lo, ro);
        const BayerRow v = bayer_add(up, dn);
        uint32_t hse[4], hso[4], dse[4], dso[4];
        bayer_sides(cur, hse, hso);
        bayer_sides(v, dse, dso);
        const BayerW ke = k[i & 1][0], ko = k[i & 1][1];
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t g0 = bayer_grey(ke, cur.e[j] & 0xFFFFu, hse[j] & 0xFFFFu, v.e[j] & 0xFFFFu, dse[j] & 0xFFFFu);
            const uint32_t g1 = bayer_grey(ko, cur.o[j] & 0xFFFFu, hso[j] & 0xFFFFu, v.o[j] & 0xFFFFu, dso[j] & 0xFFFFu);
            const uint32_t g2 = bayer_grey(ke, cur.e[j] >> 16, hse[j] >> 16, v.e[j] >> 16, dse[j] >> 16);
            const uint32_t g3 = bayer_grey(ko, cur.o[j] >> 16, hso[j] >> 16, v.o[j] >> 16, dso[j] >> 16);
            o[j] = g0 | g1 << 8 | g2 << 16 | g3 << 24;
        }
        if (live && y < h) *reinterpret_cast<uint4*>(dst + (int64_t)y * w + x0) = make_uint4(o[0], o[1], o[2], o[3]);
        up = cur; cur = dn;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bayer_to_gray8_generic_kernel(BayerArgs a)
{
    int img, blk;
    FrameAt f;
    if (!bayer_place(a, img, blk) || !av_frame_at(a.place, img, f)) return;
    const uint8_t* src = f.src; uint8_t* dst = f.dst;
    const int w = a.w, h = a.h, npix = w * h;
    const int64_t pitch = (int64_t)w * sizeof(T);
    const int p0 = blk * BY_GEN;                                  // < 2^24
#pragma unroll 2
    for (int j = 0; j < BY_GEN / 256; ++j) {
        const int p = p0 + j * 256 + (int)threadIdx.x;
        if (p >= npix) break;
        const int y = p / w, x = p - y * w;
        const int xl = x ? x - 1 : 1, xr = x + 1 < w ? x + 1 : w - 2, yu = y ? y - 1 : 1, yd = y + 1 < h ? y + 1 : h - 2;
        const uint8_t* ru = src + (int64_t)yu * pitch; const uint8_t* rc = src + (int64_t)y * pitch; const uint8_t* rd = src + (int64_t)yd * pitch;
        const uint32_t c = bayer_sample<T>(rc, x, a.shift);
        const uint32_t hs = bayer_sample<T>(rc, xl, a.shift) + bayer_sample<T>(rc, xr, a.shift);
        const uint32_t vs = bayer_sample<T>(ru, x, a.shift) + bayer_sample<T>(rd, x, a.shift);
        const uint32_t ds = bayer_sample<T>(ru, xl, a.shift) + bayer_sample<T>(ru, xr, a.shift) + bayer_sample<T>(rd, xl, a.shift) + bayer_sample<T>(rd, xr, a.shift);
        dst[p] = (uint8_t)bayer_grey(bayer_weights((x & 1) ^ a.rx, (y & 1) ^ a.ry), c, hs, vs, ds);
    }
}

}  // namespace

int av_launch_bayer_to_gray8(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, int fmt, int shift, hipStream_t st)
{
    if (n_groups <= 0) return AV_OK;
    if (fmt < AV_PIX_BAYER_RGGB8 || fmt > AV_PIX_BAYER_GBRG16) { av_set_error("av_to_gray8: pixel format %d is no Bayer mosaic", fmt); return AV_E_INVALID; }
    if (w < 2 || h < 2) { av_set_error("av_to_gray8: a Bayer mosaic is at least 2 x 2 samples (%d x %d)", w, h); return AV_E_INVALID; }
    const bool wide = fmt >= AV_PIX_BAYER_RGGB16;
    const int pat = (fmt - AV_PIX_BAYER_RGGB8) & 3;               // rggb, bggr, grbg, gbrg
    BayerArgs a;
    memset(&a, 0, sizeof(a));
    a.w = w; a.h = h; a.shift = shift;
    a.rx = pat == 1 || pat == 2; a.ry = pat == 1 || pat == 3;
    const bool vec = (w % BY_LANE) == 0 && av_frames_vec16(src, dst, n_groups);
    int per = (int)(((int64_t)w * h + BY_GEN - 1) / BY_GEN);
    if (vec) {
        a.nvx = w / BY_LANE;
        a.items = a.nvx * ((h + BY_ROWS - 1) / BY_ROWS);
        per = (a.items + 255) / 256;
    }
    const unsigned n_wg = av_frame_place(&a.place, src, dst, n_groups, per, 8, "av_to_gray8", w, h);      // eight images interleaved: bayer_place
    if (!n_wg) return AV_E_INVALID;
    const dim3 grid(n_wg), block(256);
    if (vec) {
        if (wide) hipLaunchKernelGGL(bayer_to_gray8_kernel<uint16_t>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(bayer_to_gray8_kernel<uint8_t>, grid, block, 0, st, a);
    } else {
        if (wide) hipLaunchKernelGGL(bayer_to_gray8_generic_kernel<uint16_t>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(bayer_to_gray8_generic_kernel<uint8_t>, grid, block, 0, st, a);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}
