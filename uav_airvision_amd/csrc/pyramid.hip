// pyramid.hip -- padded u8 Gaussian pyramids for LK (gfx950).
//
// Replaces the pyrDown chain that cv2.calcOpticalFlowPyrLK rebuilds inside every call
// (reference: src/image_processing/pyramid_builder.py:22-48 is a pass-through, SURVEY.md F2;
// call sites feature_tracker.py:102, stereo_matcher.py:64,70).  Built ONCE per image here and
// kept resident; the prev-cam0 pyramid is reused by the next frame.
//
// Layout: every level is stored with a 16-pixel BORDER_REFLECT_101 frame (AV_PYR_BORDER), so the
// LK kernel never clamps or reflects a coordinate.  Both kernels are written as pure gathers over
// the PADDED destination: a destination pixel in the frame recomputes the value of the interior
// pixel it mirrors, so there is no scatter and no separate border pass.
//
// Roofline: streaming kernels by their bytes (level 0: w*h read + padded write; levels 1..3: 1/4, 1/16, 1/64 of that), but NOT
// at the HBM bound.  The fused kernels ran at 1.95x the time of a device-to-device copy of their bytes, held there by VALU
// instruction issue (786 and 2,074 instructions per wavefront); after their diet (337 and 1,055) they run at 1.46x the copy and
// wait on load latency instead (pyr_l0l1: 58 % of its wave cycles waiting, 20 % on issue).  profiles/pyramid_diet has the census,
// the counters and the times.  Integer arithmetic only: separable [1 4 6 4 1], (sum + 128) >> 8.
#include <limits.h>
#include <stdlib.h>

#include "av_common.h"

namespace {

struct PyrArgs {
    const uint8_t* img0;
    const uint8_t* img1;
    int64_t img_stride;
    int imgs_per_stream;               // 1 or 2
    uint8_t* pyr_base;
    int64_t stream_stride, slot_stride;
    int slot0, slot1;
    PyrGeom g;
    int n_img, tiles_x, tiles_y;       // pyr_l0l1_kernel: XCD-aware 1-D launch
    uint32_t per_magic, tx_magic;      // pyr_l0l1_kernel: pyr_magic of tiles_x * tiles_y and of tiles_x
    uint32_t m23[6];                   // pyr_l2l3_kernel: pyr_magic of its six row lengths (L23_*)
    const int* index;                  // optional: image group i (a "stream") is storage entry index[i] of img0 / img1 / pyr_base (shared frame store)
};

// n / d without the 25-instruction expansion of an integer division: m = ceil(2^32 / d) gives floor(n / d) = mulhi(n, m) exactly
// while n * d < 2^32 (the error of n * m / 2^32 against n / d is below n * d / (d * 2^32) < 1 / d).  m = 0 (d = 1, or a launch so
// large that the bound fails): divide.
inline uint32_t pyr_magic(uint32_t d, uint64_t n_max) { return (d >= 2 && n_max * d < (1ull << 32)) ? 0xFFFFFFFFu / d + 1u : 0u; }
__device__ __forceinline__ int pyr_div(int n, int d, uint32_t m) { return m ? (int)__umulhi((uint32_t)n, m) : n / d; }

// image number of the launch -> (storage entry, camera)
__device__ __forceinline__ void pyr_entry(const PyrArgs& a, int img, int& s, int& cam)
{
    const bool two = a.imgs_per_stream == 2;
    s = two ? img >> 1 : img; cam = two ? img & 1 : 0;
    if (a.index) s = a.index[s];
}

// ---- the filter of every fused level: four outputs from sixteen source bytes, then five rows of them into one dword ----
typedef unsigned short pyr_u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t pyr_u32x4 __attribute__((ext_vector_type(4)));
typedef pyr_u32x4 pyr_u32x4_a4 __attribute__((aligned(4)));           // sixteen bytes at a dword-aligned address
// row filter [1 4 6 4 1]: (dx, dy, dz, dw) hold source columns 2 x0 - 4 .. 2 x0 + 11 of one row; the sums of outputs x0 .. x0 + 3
// (each [1 4 6 4] as one v_dot4 plus the fifth tap) come back as two packed pairs of u16
__device__ __forceinline__ void pyr_row4(uint32_t dx, uint32_t dy, uint32_t dz, uint32_t dw, uint32_t& p01, uint32_t& p23)
{
    const uint32_t W4 = 0x04060401u;
    const uint32_t h0 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(dy, dx, 2), W4, (dy >> 16) & 0xFF, false);
    const uint32_t h1 = __builtin_amdgcn_udot4(dy, W4, dz & 0xFF, false);
    const uint32_t h2 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(dz, dy, 2), W4, (dz >> 16) & 0xFF, false);
    const uint32_t h3 = __builtin_amdgcn_udot4(dz, W4, dw & 0xFF, false);
    p01 = h0 | (h1 << 16); p23 = h2 | (h3 << 16);
}
// column filter [1 4 6 4 1] of five packed row sums, (sum + 128) >> 8, in packed 16-bit arithmetic (v_pk_add_u16, v_pk_lshlrev_b16,
// v_pk_mad_u16, v_pk_lshrrev_b16).  No lane overflows: a row sum is at most 16 * 255 = 4,080, a column sum at most 16 * 4,080 = 65,280,
// and 65,280 + 128 = 65,408 < 2^16; every partial sum is a sum of non-negative terms of that total.
__device__ __forceinline__ pyr_u16x2 pyr_col2(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t r4)
{
    const pyr_u16x2 a0 = __builtin_bit_cast(pyr_u16x2, r0), a1 = __builtin_bit_cast(pyr_u16x2, r1), a2 = __builtin_bit_cast(pyr_u16x2, r2),
                    a3 = __builtin_bit_cast(pyr_u16x2, r3), a4 = __builtin_bit_cast(pyr_u16x2, r4);
    const pyr_u16x2 six = {6, 6}, half = {128, 128}, two = {2, 2}, eight = {8, 8};
    return (a2 * six + half + ((a1 + a3) << two) + (a0 + a4)) >> eight;
}
__device__ __forceinline__ uint32_t pyr_col4(const uint32_t (&p01)[5], const uint32_t (&p23)[5])
{
    const uint32_t lo = __builtin_bit_cast(uint32_t, pyr_col2(p01[0], p01[1], p01[2], p01[3], p01[4]));
    const uint32_t hi = __builtin_bit_cast(uint32_t, pyr_col2(p23[0], p23[1], p23[2], p23[3], p23[4]));
    return __builtin_amdgcn_perm(hi, lo, 0x06040200u);             // bytes 0 and 2 of lo, then of hi
}

__device__ __forceinline__ uint8_t* pyr_of(const PyrArgs& a, int img)
{
    int s, cam;
    pyr_entry(a, img, s, cam);
    return a.pyr_base + s * a.stream_stride + (cam == 0 ? a.slot0 : a.slot1) * a.slot_stride;
}

// level 0: copy the tightly packed input image into the padded level, frame included.  One thread writes 16 bytes;
// chunks that lie inside the image (all but the 16-pixel frame columns) are one 16-byte load when rows are 16-aligned.
__global__ __launch_bounds__(256) void pad_level0_kernel(PyrArgs a)
{
    const int w = a.g.w[0], h = a.g.h[0], pitch = a.g.pitch[0];
    const int chunks_per_row = pitch >> 4;                   // pitch is a multiple of 16
    const int ph = h + 2 * AV_PYR_BORDER;
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= chunks_per_row * ph) return;
    int yp = q / chunks_per_row, xc = q - yp * chunks_per_row;
    int img = blockIdx.y;
    int s, cam;
    pyr_entry(a, img, s, cam);
    const uint8_t* src = (cam == 0 ? a.img0 : a.img1) + s * a.img_stride;
    uint8_t* dst = pyr_of(a, img) + a.g.off[0];
    int y = av_reflect101(yp - AV_PYR_BORDER, h);
    const uint8_t* row = src + (size_t)y * w;
    const int x0 = xc * 16 - AV_PYR_BORDER;
    uint4 out;
    if (x0 >= 0 && x0 + 16 <= w && ((w | (int)(a.img_stride & 15) | (int)(reinterpret_cast<uintptr_t>(src) & 15)) & 15) == 0) {
        out = *reinterpret_cast<const uint4*>(row + x0);
    } else {
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int x = av_reflect101(x0 + i, w);
            x = min(max(x, 0), w - 1);      // slack columns beyond w+32 (pitch rounding): any valid pixel
            o[i >> 2] |= (uint32_t)row[x] << (8 * (i & 3));
        }
        out = make_uint4(o[0], o[1], o[2], o[3]);
    }
    *reinterpret_cast<uint4*>(dst + (size_t)yp * pitch + xc * 16) = out;
}

// Levels 0 AND 1 in one pass over the input image: a 128 x 32 tile of the image (+ a 2-pixel halo, reflect-101 at the image
// border) is staged in LDS once; from it the workgroup writes its part of the padded level 0 (16-byte stores, the frame
// parts of border tiles gathered through the reflection), filters the 64 x 16 tile of level 1 (row filter by v_dot4 into
// u16 sums, packed 16-bit column filter, (sum + 128) >> 8) and writes it, plus the mirror images of those level-1 pixels that lie
// within 16 pixels of the image border (the frame of level 1).  The separate pad and first pyrDown kernels read the image and
// re-read the padded level 0 (0.8 MB per image through L2); here every input byte is read once.
// Instruction issue costs this kernel as much as its bytes (profiles/pyramid_diet), so everything that depends only on the tile (which
// borders it touches, whether its last column is ragged, which strips of level 1 have a mirror image) is decided once per
// workgroup from blockIdx, in scalar registers, and the common path of a thread is loads, LDS traffic and the two filters.
constexpr int FT_W = 128, FT_LP = FT_W + 8;        // LDS row: columns x0-4 .. x0+131
// tile height: 96 rows when the image height allows (100 staged rows of eight 16-byte chunks: up to four loads in flight per thread,
// 2.1 % halo rows), else 32
constexpr int FT_H_TALL = 96, FT_H_BASE = 32;
template <bool WRITE_L0, int FT_H>
__global__ __launch_bounds__(256) void pyr_l0l1_kernel(PyrArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t src[(FT_H + 4) * FT_LP];
    __shared__ __attribute__((aligned(16))) uint16_t hs[(FT_H + 4) * (FT_W / 2)];
    // the level-1 tile lives where the staged source rows were: their last reader is the row filter, a barrier ahead of the first write
    // (26.4 instead of 29.4 KB of LDS: six workgroups per CU instead of five)
    static_assert((FT_H / 2) * (FT_W / 2) <= (FT_H + 4) * FT_LP, "level-1 tile fits the source tile");
    uint8_t* const l1t = src;
    const int w = a.g.w[0], h = a.g.h[0], pitch0 = a.g.pitch[0];
    const int w1 = a.g.w[1], h1 = a.g.h[1], pitch1 = a.g.pitch[1];
    const int tid = threadIdx.x;
    // workgroup -> (image, tile): with the 1-D launch all tiles of an image run on ONE XCD (round-robin dispatch over 8 XCDs, an
    // L2 each): horizontally adjacent tiles share every 128-byte line a 752-byte image row lays across their boundary, and
    // vertically adjacent ones their 4 halo rows -- on eight L2s each of those lines is fetched once per XCD that meets it
    // (PMC: 2.3x the image bytes), on one L2 once.
    const int L = blockIdx.x, wg = L >> 3, per = a.tiles_x * a.tiles_y;
    const int grp = pyr_div(wg, per, a.per_magic);
    const int img = (L & 7) + 8 * grp;
    if (img >= a.n_img) return;
    const int tile = wg - grp * per;
    const int by = pyr_div(tile, a.tiles_x, a.tx_magic), bx = tile - by * a.tiles_x;
    const int x0 = bx * FT_W, y0 = by * FT_H;
    int s, cam;
    pyr_entry(a, img, s, cam);
    const uint8_t* in = (cam == 0 ? a.img0 : a.img1) + s * a.img_stride;
    uint8_t* base = pyr_of(a, img);
    uint8_t* d0 = base + a.g.off[0];
    uint8_t* d1 = base + a.g.off[1];
    uint32_t* srcw = reinterpret_cast<uint32_t*>(src);
    // what the tile touches: all of it the same for every thread of the workgroup
    const bool top = y0 == 0, bot = y0 + FT_H >= h, left = x0 == 0, right = x0 + FT_W >= w;
    const bool ragged = x0 + FT_W > w;                                    // the last tile column holds fewer than 128 image columns

    // ---- stage rows y0-2 .. y0+FT_H+1, columns x0-4 .. x0+131 (reflect-101 outside the image): per row eight 16-byte chunks
    //      of the tile's own columns, and the two halo dwords in a short pass of their own ----
    // Thread t owns chunk column t & 7 and walks rows t >> 3, + 32, + 64, + 96: one offset per item, a constant stride apart in every
    // tile that touches neither the top nor the bottom of the image (rows are reflected only there).  w is a multiple of 16, so a chunk
    // lies inside the image or wholly past it, and only the ragged column has chunks past it: those are gathered byte by byte.  The
    // loads of all items are issued before any is waited for -- as a plain loop the compiler waited (vmcnt(0)) inside every iteration,
    // i.e. one 16-byte load in flight per thread, far below what HBM latency x bandwidth needs per CU.  A chunk is ONE 16-byte load
    // whatever the alignment of the image: rows are dword-aligned (the launch condition), which is all global_load_dwordx4 asks for;
    // an image whose base or stride is no multiple of 16 only pays for the lines its chunks straddle.
    {
        constexpr int ROWS = FT_H + 4, NIT = (ROWS + 31) / 32;
        static_assert(2 * ROWS <= 256, "one thread per halo dword");
        const int j = tid & 7, r0 = tid >> 3;
        const int gx = x0 + 16 * j;
        const bool in_img = !ragged || gx < w;
        uint32_t ro[NIT];                                                 // byte offset of the item's row in the image
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            int y = y0 - 2 + r0 + 32 * u;
            if (top || bot) y = av_reflect101(min(y, h + 1), h);          // (rows past the staged ones of the last item: not loaded)
            ro[u] = (uint32_t)(y * w);
        }
        // halo dword of thread t: row t >> 1, left (columns x0-4 .. x0-1) or right (x0+128 .. x0+131)
        const int hr = tid >> 1, gh = (tid & 1) ? x0 + FT_W : x0 - 4;
        const bool hval = tid < 2 * ROWS, hin = gh >= 0 && gh + 4 <= w;
        int hy = y0 - 2 + hr;
        if (top || bot) hy = av_reflect101(min(hy, h + 1), h);
        const uint8_t* hrow = in + (uint32_t)(hy * w);
        uint32_t hv = 0;
        pyr_u32x4 q4[NIT];
        if (hval && hin) hv = *reinterpret_cast<const uint32_t*>(hrow + gh);
        if (in_img) {
#pragma unroll
            for (int u = 0; u < NIT; ++u)
                if (u < NIT - 1 || r0 + 32 * u < ROWS) q4[u] = *reinterpret_cast<const pyr_u32x4_a4*>(in + (ro[u] + (uint32_t)gx));
        } else {                                                          // chunk past the image (ragged column): mirror images
#pragma unroll
            for (int u = 0; u < NIT; ++u)
                if (u < NIT - 1 || r0 + 32 * u < ROWS) {
                    const uint8_t* row = in + ro[u];
                    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int b = 0; b < 16; ++b) { int x = av_reflect101(gx + b, w); x = min(max(x, 0), w - 1); v[b >> 2] |= (uint32_t)row[x] << (8 * (b & 3)); }
                    q4[u] = pyr_u32x4{v[0], v[1], v[2], v[3]};
                }
        }
        if (hval && !hin) {                                               // halo past the left or right border
#pragma unroll
            for (int b = 0; b < 4; ++b) { int x = av_reflect101(gh + b, w); x = min(max(x, 0), w - 1); hv |= (uint32_t)hrow[x] << (8 * b); }
        }
        if (hval) srcw[hr * (FT_LP / 4) + ((tid & 1) ? FT_LP / 4 - 1 : 0)] = hv;
#pragma unroll
        for (int u = 0; u < NIT; ++u)
            if (u < NIT - 1 || r0 + 32 * u < ROWS) {
                uint32_t* dst = srcw + (r0 + 32 * u) * (FT_LP / 4) + 1 + 4 * j;
                dst[0] = q4[u].x; dst[1] = q4[u].y; dst[2] = q4[u].z; dst[3] = q4[u].w;
            }
    }
    __syncthreads();

    // ---- padded level 0: destination rows / 16-byte chunks owned by this tile (interior + its share of the frame) ----
    //      (WRITE_L0 = false: level 0 stays the caller's image -- LK and FAST read it in place, lk.hip LKArgs::imgI -- which
    //       removes 401 KB of stores and the re-read of that copy per image: 44 % of this kernel's bytes)
    if (WRITE_L0) {
        const int tw = min(FT_W, w - x0);                                 // valid interior columns (multiple of 16 or the image's tail)
        const int nrow = FT_H + (top ? AV_PYR_BORDER : 0) + (bot ? AV_PYR_BORDER : 0);
        const int nch_in = (tw + 15) >> 4;
        const int nch = nch_in + (left ? 1 : 0) + (right ? (pitch0 - AV_PYR_BORDER - w + 15) / 16 : 0);
        for (int i = tid; i < nrow * nch; i += 256) {
            const int ri = i / nch, ci = i - ri * nch;
            // destination row (image coordinates): the tile's own rows first, then the frame rows above / below
            int yp;
            if (ri < FT_H) yp = y0 + ri;
            else if (top && ri < FT_H + AV_PYR_BORDER) yp = -(ri - FT_H + 1);
            else yp = h + (ri - FT_H - (top ? AV_PYR_BORDER : 0));
            if (yp >= h + AV_PYR_BORDER || (ri < FT_H && yp >= h)) continue;
            int xd;                                                        // first destination column of the chunk
            bool interior;
            if (ci < nch_in) { xd = x0 + 16 * ci; interior = true; }
            else if (left && ci == nch_in) { xd = -AV_PYR_BORDER; interior = false; }
            else { xd = w + 16 * (ci - nch_in - (left ? 1 : 0)); interior = false; }
            const int sy = av_reflect101(yp, h) - (y0 - 2);                // staged row of the source pixel row
            uint32_t o[4];
            if (interior && xd + 16 <= w) {
                const uint32_t* p = srcw + sy * (FT_LP / 4) + ((xd - x0 + 4) >> 2);
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3];
            } else {
                o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    int x = av_reflect101(xd + b, w); x = min(max(x, 0), w - 1);
                    o[b >> 2] |= (uint32_t)src[sy * FT_LP + (x - x0 + 4)] << (8 * (b & 3));
                }
            }
            *reinterpret_cast<uint4*>(d0 + (size_t)(yp + AV_PYR_BORDER) * pitch0 + (xd + AV_PYR_BORDER)) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }

    // ---- level 1: row filter [1 4 6 4 1] of the staged rows into u16 sums: 4 outputs per item from 16 staged bytes ----
    for (int i = tid; i < (FT_H + 4) * (FT_W / 8); i += 256) {
        const int r = i / (FT_W / 8), xq = i - r * (FT_W / 8);
        const uint2 lo = *reinterpret_cast<const uint2*>(src + r * FT_LP + 8 * xq);
        const uint2 hi = *reinterpret_cast<const uint2*>(src + r * FT_LP + 8 * xq + 8);
        uint32_t p01, p23;
        pyr_row4(lo.x, lo.y, hi.x, hi.y, p01, p23);
        *reinterpret_cast<uint2*>(hs + r * (FT_W / 2) + 4 * xq) = make_uint2(p01, p23);
    }
    __syncthreads();
    // column filter: thread t -> level-1 row yo = t / 16, columns 4 xq .. 4 xq + 3 of the tile: five 8-byte reads of packed sums
    for (int t_ = tid; t_ < (FT_H / 2) * (FT_W / 8); t_ += 256) {
        const int yo = t_ >> 4, xq = t_ & 15;
        const uint16_t* c = hs + (2 * yo) * (FT_W / 2) + 4 * xq;
        uint32_t p01[5], p23[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint2 v = *reinterpret_cast<const uint2*>(c + k * (FT_W / 2));
            p01[k] = v.x; p23[k] = v.y;
        }
        const uint32_t out = pyr_col4(p01, p23);
        *reinterpret_cast<uint32_t*>(l1t + yo * (FT_W / 2) + 4 * xq) = out;
        const int x1 = x0 / 2 + 4 * xq, y1 = y0 / 2 + yo;
        if (x1 < w1 && y1 < h1) *reinterpret_cast<uint32_t*>(d1 + (size_t)(y1 + AV_PYR_BORDER) * pitch1 + (x1 + AV_PYR_BORDER)) = out;
    }
    // ---- frame of level 1: the level-1 pixels of this tile that lie within 16 pixels of the border are mirrored outwards ----
    // Sources with a mirror image are columns 1 .. 16 (image at -x) and w1-17 .. w1-2 (at 2 (w1-1) - x), rows likewise; the parts of
    // those strips inside this tile are ranges known per workgroup, and only they are walked: the rows of the column strips, the whole
    // rows of the row strips (dword copies), and the corners.  A mirrored dword is stored whole when its four sources are this tile's
    // (the strip w1-17 .. w1-2 may begin in the tile column before the last), else byte by byte.
    const int X1 = x0 / 2, Y1 = y0 / 2;
    const int tx1 = min(X1 + FT_W / 2, w1), ty1 = min(Y1 + FT_H / 2, h1);          // the tile's level-1 pixels: [X1, tx1) x [Y1, ty1)
    const bool hasL = X1 == 0, hasR = tx1 - 1 >= w1 - 1 - AV_PYR_BORDER;
    const int rlo[3] = {Y1, max(Y1, 1), max(Y1, h1 - 1 - AV_PYR_BORDER)};          // identity, top strip, bottom strip (inclusive)
    const int rhi[3] = {ty1 - 1, min(ty1 - 1, AV_PYR_BORDER), min(ty1 - 1, h1 - 2)};
    if (hasL || hasR || rlo[1] <= rhi[1] || rlo[2] <= rhi[2]) {
        __syncthreads();
        const uint32_t* l1w = reinterpret_cast<const uint32_t*>(l1t);
#pragma unroll
        for (int rk = 0; rk < 3; ++rk) {
            const int ya = rlo[rk], nr = rhi[rk] - ya + 1;
            if (nr <= 0) continue;
            if (rk != 0) {                                                 // whole rows of a row strip
                for (int i = tid; i < nr * (FT_W / 8); i += 256) {
                    const int yy = ya + (i >> 4), q = i & 15;
                    const int yd = rk == 1 ? -yy : 2 * (h1 - 1) - yy;
                    if (X1 + 4 * q < tx1)
                        *reinterpret_cast<uint32_t*>(d1 + (size_t)(yd + AV_PYR_BORDER) * pitch1 + (X1 + 4 * q + AV_PYR_BORDER)) = l1w[(yy - Y1) * (FT_W / 8) + q];
                }
            }
#pragma unroll
            for (int ck = 1; ck < 3; ++ck) {                               // the sixteen mirrored columns left / right of these rows
                if (!(ck == 1 ? hasL : hasR)) continue;
                for (int i = tid; i < nr * 4; i += 256) {
                    const int yy = ya + (i >> 2), k = i & 3;
                    const int yd = rk == 0 ? yy : (rk == 1 ? -yy : 2 * (h1 - 1) - yy);
                    const int xd = ck == 1 ? 4 * k - AV_PYR_BORDER : w1 + 4 * k;             // destination columns xd .. xd + 3
                    const int xs = ck == 1 ? -xd : 2 * (w1 - 1) - xd;                      // ... mirror sources xs, xs - 1, xs - 2, xs - 3
                    const uint8_t* sp = l1t + (yy - Y1) * (FT_W / 2) + (xs - X1);
                    uint8_t* dp = d1 + (size_t)(yd + AV_PYR_BORDER) * pitch1 + (xd + AV_PYR_BORDER);
                    if (xs < tx1 && xs - 3 >= X1) {
                        *reinterpret_cast<uint32_t*>(dp) = (uint32_t)sp[0] | (uint32_t)sp[-1] << 8 | (uint32_t)sp[-2] << 16 | (uint32_t)sp[-3] << 24;
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (xs - c < tx1 && xs - c >= X1) dp[c] = sp[-c];
                    }
                }
            }
        }
    }
}

// level l (>= 1) from padded level l-1.
__global__ __launch_bounds__(256) void pyr_down_kernel(PyrArgs a, int level)
{
    const int w = a.g.w[level], h = a.g.h[level], pitch = a.g.pitch[level];
    const int spitch = a.g.pitch[level - 1];
    const int quads_per_row = pitch >> 2;
    const int ph = h + 2 * AV_PYR_BORDER;
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= quads_per_row * ph) return;
    int yp = q / quads_per_row, xq = q - yp * quads_per_row;
    uint8_t* base = pyr_of(a, blockIdx.y);
    const uint8_t* src = base + a.g.off[level - 1];
    uint8_t* dst = base + a.g.off[level];
    int y = av_reflect101(yp - AV_PYR_BORDER, h);
    // padded source rows 2y-2 .. 2y+2
    const uint8_t* r0 = src + (size_t)(2 * y - 2 + AV_PYR_BORDER) * spitch + AV_PYR_BORDER;
    uint32_t out = 0;
    const int x0 = xq * 4 - AV_PYR_BORDER;
    if (x0 >= 0 && x0 + 4 <= w) {
        // interior quad: source bytes 2*x0-2 .. 2*x0+8 of each row sit inside the 16 bytes at 2*x0-4 (dword aligned:
        // x0 is a multiple of 4, the padded pitch a multiple of 16).  Row filter [1 4 6 4] as one v_dot4 plus the fifth tap.
        int hs[4][5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint4 d = *reinterpret_cast<const uint4*>(r0 + (size_t)k * spitch + 2 * x0 - 4);
            const uint32_t t0 = __builtin_amdgcn_alignbyte(d.y, d.x, 2), t1 = d.y, t2 = __builtin_amdgcn_alignbyte(d.z, d.y, 2), t3 = d.z;
            const uint32_t W4 = 0x04060401u;
            hs[0][k] = (int)__builtin_amdgcn_udot4(t0, W4, (d.y >> 16) & 0xFF, false);
            hs[1][k] = (int)__builtin_amdgcn_udot4(t1, W4, d.z & 0xFF, false);
            hs[2][k] = (int)__builtin_amdgcn_udot4(t2, W4, (d.z >> 16) & 0xFF, false);
            hs[3][k] = (int)__builtin_amdgcn_udot4(t3, W4, d.w & 0xFF, false);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = hs[i][0] + hs[i][4] + 4 * (hs[i][1] + hs[i][3]) + 6 * hs[i][2];
            out |= (uint32_t)((v + 128) >> 8) << (8 * i);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int xp = xq * 4 + i;
            int x = av_reflect101(xp - AV_PYR_BORDER, w);
            x = min(max(x, 0), w - 1);
            const uint8_t* p = r0 + 2 * x;
            int hsum[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint8_t* r = p + (size_t)k * spitch;
                hsum[k] = (int)r[-2] + (int)r[2] + 4 * ((int)r[-1] + (int)r[1]) + 6 * (int)r[0];
            }
            int v = hsum[0] + hsum[4] + 4 * (hsum[1] + hsum[3]) + 6 * hsum[2];
            out |= (uint32_t)((v + 128) >> 8) << (8 * i);
        }
    }
    *reinterpret_cast<uint32_t*>(dst + (size_t)yp * pitch + xq * 4) = out;
}

// Levels 2 AND 3 of one image by one workgroup: level 2 is filtered from the padded level 1 (global) into LDS, level 3 from
// that LDS copy, and both 16-pixel frames are mirrored out of LDS.  The per-level gather kernel spends most of its time in the
// frame at these sizes (52 % of the padded level 3 is frame, every frame pixel re-filters 25 source bytes through the
// reflection); here a frame pixel is one LDS byte read.
// The LDS copy of level 2 carries a 2-pixel reflect-101 frame of its own (and 4 bytes ahead of each row, so that source column
// 8 q - 4 of an output quad is 8-byte aligned): level 3 is then filtered exactly like the other levels -- quads from sixteen bytes,
// v_dot4 rows, packed columns -- with no reflection.  The padded levels leave LDS as whole dwords in the interior columns; only
// the dwords of the frame columns (and a row's last, partial one) are gathered byte by byte through the reflection.  Every flat
// index is split into (row, dword) by a multiplication (pyr_div): the row lengths are not powers of two.
enum { L23_Q2 = 0, L23_Q3, L23_IN2, L23_FR2, L23_IN3, L23_FR3 };      // PyrArgs::m23
struct L23Layout { int q2, q3, lp2, lp3, l3_off, bytes; };             // LDS: level 2 [h2 + 4][lp2], then level 3 [h3][lp3]
__host__ __device__ inline L23Layout pyr_l23_layout(const PyrGeom& g)
{
    L23Layout l;
    l.q2 = (g.w[2] + 3) >> 2; l.q3 = (g.w[3] + 3) >> 2;
    l.lp2 = 8 * l.q3 + 8;                   // columns -4 .. 8 q3 + 3: the last quad of level 3 reads up to 8 (q3 - 1) + 11, and 4 q2 + 4 <= lp2
    l.lp3 = 4 * l.q3;
    l.l3_off = ((g.h[2] + 4) * l.lp2 + 15) & ~15;
    l.bytes = l.l3_off + g.h[3] * l.lp3;
    return l;
}

// one padded level out of its LDS copy (l: pixel (0, 0), rows lp bytes apart): the whole interior dwords of every padded row, then
// the others -- four of the left frame and the right frame with the row's tail and the pitch's slack
template <int T>
__device__ __forceinline__ void pyr_store_padded(const uint8_t* l, int lp, int w, int h, uint8_t* d, int pitch, uint32_t m_in, uint32_t m_fr, int tid)
{
    const int ph = h + 2 * AV_PYR_BORDER, nin = w >> 2, nfr = (pitch >> 2) - nin;
    for (int i = tid; i < nin * ph; i += T) {
        const int yp = pyr_div(i, nin, m_in), q = i - yp * nin;
        const int y = av_reflect101(yp - AV_PYR_BORDER, h);
        *reinterpret_cast<uint32_t*>(d + yp * pitch + (AV_PYR_BORDER + 4 * q)) = *reinterpret_cast<const uint32_t*>(l + y * lp + 4 * q);
    }
    for (int i = tid; i < nfr * ph; i += T) {
        const int yp = pyr_div(i, nfr, m_fr), q = i - yp * nfr;
        const int y = av_reflect101(yp - AV_PYR_BORDER, h);
        const int xs = q < 4 ? 4 * q - AV_PYR_BORDER : 4 * (nin + q - 4);          // image column of the dword's first byte
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) { int x = av_reflect101(xs + c, w); x = min(max(x, 0), w - 1); out |= (uint32_t)l[y * lp + x] << (8 * c); }
        *reinterpret_cast<uint32_t*>(d + yp * pitch + (xs + AV_PYR_BORDER)) = out;
    }
}

template <int L23_T>
__global__ __launch_bounds__(L23_T) void pyr_l2l3_kernel(PyrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds23[];
    const int p1 = a.g.pitch[1];
    const int w2 = a.g.w[2], h2 = a.g.h[2], p2 = a.g.pitch[2];
    const int w3 = a.g.w[3], h3 = a.g.h[3], p3 = a.g.pitch[3];
    const L23Layout lay = pyr_l23_layout(a.g);
    const int q2 = lay.q2, q3 = lay.q3, lp2 = lay.lp2, lp3 = lay.lp3;
    uint8_t* l2 = lds23 + 2 * lp2 + 4;                                // level-2 pixel (0, 0)
    uint8_t* l3 = lds23 + lay.l3_off;
    const int tid = threadIdx.x;
    uint8_t* base = pyr_of(a, blockIdx.x);
    // level-1 pixel (-4, -2): its frame is valid around it
    const uint8_t* s1 = base + a.g.off[1] + (AV_PYR_BORDER - 2) * p1 + (AV_PYR_BORDER - 4);
    // ---- level 2 interior: quads of 4 pixels from five 16-byte source segments (as pyr_down_kernel) ----
    for (int i = tid; i < q2 * h2; i += L23_T) {
        const int y = pyr_div(i, q2, a.m23[L23_Q2]), q = i - y * q2;
        const uint8_t* r0 = s1 + (uint32_t)(2 * y * p1 + 8 * q);
        uint32_t p01[5], p23[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint4 d = *reinterpret_cast<const uint4*>(r0 + k * p1);
            pyr_row4(d.x, d.y, d.z, d.w, p01[k], p23[k]);
        }
        *reinterpret_cast<uint32_t*>(l2 + y * lp2 + 4 * q) = pyr_col4(p01, p23);      // columns >= w2 of the last quad: overwritten below
    }
    __syncthreads();
    // ---- its 2-pixel frame: columns -2, -1, w2, w2 + 1 of every row, then rows -2, -1, h2, h2 + 1 with their frame columns ----
    for (int i = tid; i < 4 * h2; i += L23_T) {
        const int y = i >> 2, c = i & 3;
        const int xd = c < 2 ? c - 2 : w2 + c - 2;
        l2[y * lp2 + xd] = l2[y * lp2 + av_reflect101(xd, w2)];
    }
    __syncthreads();
    for (int i = tid; i < (lp2 >> 2); i += L23_T) {
        uint32_t* col = reinterpret_cast<uint32_t*>(lds23) + i;       // row r of level 2 is LDS row r + 2
        const int dw = lp2 >> 2;
        col[0] = col[4 * dw]; col[dw] = col[3 * dw];
        col[(h2 + 2) * dw] = col[h2 * dw]; col[(h2 + 3) * dw] = col[(h2 - 1) * dw];
    }
    __syncthreads();
    // ---- padded level 2 out of LDS ----
    pyr_store_padded<L23_T>(l2, lp2, w2, h2, base + a.g.off[2], p2, a.m23[L23_IN2], a.m23[L23_FR2], tid);
    // ---- level 3 interior from the framed LDS copy of level 2: rows 2 y - 2 .. 2 y + 2 are LDS rows 2 y .. 2 y + 4 ----
    // (the 1,440 quads of a 752 x 480 image are 22.5 wavefronts' worth: wavefronts without an item skip the loop, and the items are dealt
    //  from the LAST thread down, so that the partial last pass falls on the wavefronts that sat out the partial passes of the loops above)
    for (int i = L23_T - 1 - tid; i < q3 * h3; i += L23_T) {
        const int y = pyr_div(i, q3, a.m23[L23_Q3]), q = i - y * q3;
        const uint8_t* r0 = lds23 + 2 * y * lp2 + 8 * q;
        uint32_t p01[5], p23[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint2 lo = *reinterpret_cast<const uint2*>(r0 + k * lp2), hi = *reinterpret_cast<const uint2*>(r0 + k * lp2 + 8);
            pyr_row4(lo.x, lo.y, hi.x, hi.y, p01[k], p23[k]);
        }
        *reinterpret_cast<uint32_t*>(l3 + y * lp3 + 4 * q) = pyr_col4(p01, p23);      // columns >= w3 of the last quad are never read back
    }
    __syncthreads();
    pyr_store_padded<L23_T>(l3, lp3, w3, h3, base + a.g.off[3], p3, a.m23[L23_IN3], a.m23[L23_FR3], tid);
}

}  // namespace

PyrGeom av_make_geom(const av_pyr_layout& l)
{
    PyrGeom g;
    memset(&g, 0, sizeof(g));
    g.levels = l.levels;
    for (int i = 0; i < l.levels; ++i) {
        g.w[i] = l.w[i]; g.h[i] = l.h[i]; g.pitch[i] = l.pitch[i]; g.off[i] = (int)l.offset[i];
    }
    return g;
}

int av_launch_pyramid(const FrameSet& img, int n_groups,
                      const PyrGeom& g, uint8_t* pyr_base, int64_t stream_stride, int64_t slot_stride, int slot0, int slot1,
                      hipStream_t st, bool write_level0, bool* wrote_level0)
{
    if (wrote_level0) *wrote_level0 = true;
    if (n_groups <= 0) return AV_OK;
    PyrArgs a;
    a.img0 = img.base[0]; a.img1 = img.base[1]; a.img_stride = img.stride; a.imgs_per_stream = img.base[1] ? 2 : 1;
    a.pyr_base = pyr_base; a.stream_stride = stream_stride; a.slot_stride = slot_stride;
    a.slot0 = slot0; a.slot1 = slot1; a.g = g;
    a.n_img = 0; a.tiles_x = 0; a.tiles_y = 0; a.per_magic = 0; a.tx_magic = 0; a.index = img.map;
    memset(a.m23, 0, sizeof(a.m23));
    const int n_img = n_groups * a.imgs_per_stream;
    const int w = g.w[0], h = g.h[0];
    // the fused level-0 + level-1 kernel needs: dword-aligned rows, whole 32-row tiles, a last tile column that still holds the
    // 17 pixels its frame mirrors, images large enough that a pixel is never in two mirror bands
    const int FT_H = ((h % FT_H_TALL) == 0 && h >= 2 * FT_H_TALL) ? FT_H_TALL : FT_H_BASE;
    const bool fused = g.levels >= 2 && (w & 15) == 0 && (h % FT_H) == 0 && h >= 64 && w >= 64 && (w % FT_W == 0 || w % FT_W >= 20) &&
                       (img.stride & 3) == 0 && (reinterpret_cast<uintptr_t>(img.base[0]) & 3) == 0 && (reinterpret_cast<uintptr_t>(img.base[1]) & 3) == 0;
    if (fused) {
        const int tx = (w + FT_W - 1) / FT_W, ty = h / FT_H;
        a.n_img = n_img; a.tiles_x = tx; a.tiles_y = ty;
        dim3 grid((unsigned)(tx * ty) * 8u * (unsigned)((n_img + 7) / 8));
        a.per_magic = pyr_magic((uint32_t)(tx * ty), grid.x >> 3); a.tx_magic = pyr_magic((uint32_t)tx, (uint64_t)(tx * ty));
        if (FT_H == FT_H_TALL) {
            if (write_level0) hipLaunchKernelGGL((pyr_l0l1_kernel<true, FT_H_TALL>), grid, dim3(256), 0, st, a);
            else { hipLaunchKernelGGL((pyr_l0l1_kernel<false, FT_H_TALL>), grid, dim3(256), 0, st, a); if (wrote_level0) *wrote_level0 = false; }
        } else {
            if (write_level0) hipLaunchKernelGGL((pyr_l0l1_kernel<true, FT_H_BASE>), grid, dim3(256), 0, st, a);
            else { hipLaunchKernelGGL((pyr_l0l1_kernel<false, FT_H_BASE>), grid, dim3(256), 0, st, a); if (wrote_level0) *wrote_level0 = false; }
        }
        AV_LAUNCH_CHECK();
    } else {
        int chunks = (g.pitch[0] >> 4) * (g.h[0] + 2 * AV_PYR_BORDER);
        dim3 grid((chunks + 255) / 256, n_img);
        hipLaunchKernelGGL(pad_level0_kernel, grid, dim3(256), 0, st, a);
        AV_LAUNCH_CHECK();
    }
    // levels 2 + 3 by one workgroup per image when the level-2 image fits in LDS
    const size_t lds23 = g.levels == 4 ? ((((size_t)g.h[2] * ((g.w[2] + 3) & ~3) + 15) & ~(size_t)15) + (size_t)g.h[3] * ((g.w[3] + 3) & ~3) + 16) : 0;
    // (the same images as ever take it: the bound is on the two levels as such; the LDS copy of level 2 now has a frame, which can pass
    //  64 KB only for an image some forty times wider than high)
    const L23Layout l23 = pyr_l23_layout(g);
    const bool fused23 = g.levels == 4 && lds23 <= 60 * 1024 && (g.pitch[1] & 3) == 0 && l23.bytes <= 64 * 1024;
    int lbeg = fused ? 2 : 1;
    if (fused23) {
        if (!fused) {
            int quads = (g.pitch[1] >> 2) * (g.h[1] + 2 * AV_PYR_BORDER);
            dim3 grid((quads + 255) / 256, n_img);
            hipLaunchKernelGGL(pyr_down_kernel, grid, dim3(256), 0, st, a, 1);
            AV_LAUNCH_CHECK();
        }
        for (int l = 2; l <= 3; ++l) {
            const uint32_t ph = (uint32_t)(g.h[l] + 2 * AV_PYR_BORDER), nin = (uint32_t)(g.w[l] >> 2), nfr = (uint32_t)(g.pitch[l] >> 2) - nin;
            const uint32_t q = (uint32_t)(l == 2 ? l23.q2 : l23.q3);
            a.m23[l == 2 ? L23_Q2 : L23_Q3] = pyr_magic(q, (uint64_t)q * g.h[l]);
            a.m23[l == 2 ? L23_IN2 : L23_IN3] = pyr_magic(nin, (uint64_t)nin * ph);
            a.m23[l == 2 ? L23_FR2 : L23_FR3] = pyr_magic(nfr, (uint64_t)nfr * ph);
        }
        // (512- and 256-thread workgroups -- a 1,024-thread workgroup is sixteen waves, two of them fill a CU's wave slots -- measured
        //  0.961 / 0.969 ms of pyramid time per step against 0.973: within the noise, round 5, before the kernel's instruction diet)
        hipLaunchKernelGGL(pyr_l2l3_kernel<1024>, dim3(n_img), dim3(1024), (size_t)l23.bytes, st, a);
        AV_LAUNCH_CHECK();
        lbeg = g.levels;
    }
    for (int l = lbeg; l < g.levels; ++l) {
        int quads = (g.pitch[l] >> 2) * (g.h[l] + 2 * AV_PYR_BORDER);
        dim3 grid((quads + 255) / 256, n_img);
        hipLaunchKernelGGL(pyr_down_kernel, grid, dim3(256), 0, st, a, l);
        AV_LAUNCH_CHECK();
    }
    return AV_OK;
}

AV_EXPORT int av_pyramid_layout(int w, int h, int levels, av_pyr_layout* out)
{
    if (!out || levels < 1 || levels > AV_MAX_LEVELS || w <= 0 || h <= 0) {
        av_set_error("av_pyramid_layout: bad arguments (w=%d h=%d levels=%d)", w, h, levels);
        return AV_E_INVALID;
    }
    memset(out, 0, sizeof(*out));
    out->levels = levels;
    int64_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l < levels; ++l) {
        if (lw <= AV_PYR_BORDER || lh <= AV_PYR_BORDER) {
            av_set_error("av_pyramid_layout: level %d is %dx%d, too small for a %d-pixel reflect-101 frame", l, lw, lh, AV_PYR_BORDER);
            return AV_E_INVALID;
        }
        out->w[l] = lw; out->h[l] = lh;
        out->pitch[l] = ((lw + 2 * AV_PYR_BORDER) + 15) & ~15;
        out->offset[l] = off;
        off += (int64_t)out->pitch[l] * (lh + 2 * AV_PYR_BORDER);
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
    }
    out->bytes = (off + 255) & ~(int64_t)255;
    if (out->bytes > 0x7fffffff) { av_set_error("av_pyramid_layout: image too large"); return AV_E_INVALID; }
    return AV_OK;
}

static int pyramid_build(const char* who, const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, int levels,
                         uint8_t* pyr_dev, int64_t pyr_stride, void* stream, bool write_level0)
{
    av_pyr_layout lay;
    int rc = av_pyramid_layout(w, h, levels, &lay);
    if (rc) return rc;
    if (!img_dev || !pyr_dev || n_img < 0 || pyr_stride < lay.bytes || img_stride < (int64_t)w * h) {
        av_set_error("%s: bad arguments", who);
        return AV_E_INVALID;
    }
    return av_launch_pyramid(av_frames(img_dev, nullptr, img_stride), n_img, av_make_geom(lay), pyr_dev, pyr_stride, 0, 0, 0, (hipStream_t)stream, write_level0);
}

AV_EXPORT int av_pyramid_build(const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, int levels,
                               uint8_t* pyr_dev, int64_t pyr_stride, void* stream)
{
    return pyramid_build("av_pyramid_build", img_dev, img_stride, n_img, w, h, levels, pyr_dev, pyr_stride, stream, true);
}

AV_EXPORT int av_pyramid_build_levels(const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, int levels,
                                      uint8_t* pyr_dev, int64_t pyr_stride, void* stream)
{
    return pyramid_build("av_pyramid_build_levels", img_dev, img_stride, n_img, w, h, levels, pyr_dev, pyr_stride, stream, false);
}
