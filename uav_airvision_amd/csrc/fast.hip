// fast.hip -- FAST-9/16 corner detector with corner score and 3x3 non-max suppression (gfx950).
//
// Replaces cv2.FastFeatureDetector_create(threshold).detect(img, mask) (TYPE_9_16, NMS on):
//   src/image_processing/pipeline.py:23-25 (ctor), feature_initializer.py:52, feature_adder.py:64.
// Semantics follow OpenCV 4.x features2d/fast.cpp (FAST_t<16>) and fast_score.cpp
// (cornerScore<16>): a pixel is a corner when 9 contiguous pixels of the 16-pixel Bresenham
// circle are all brighter than v+t or all darker than v-t; score = the largest threshold for
// which it stays a corner = max over the 16 arcs of min|diff| - 1; keypoints are strict maxima
// of the score over their 8 neighbours; a 3-pixel border is never a corner; detect(img, mask)
// drops keypoints whose mask pixel is 0 AFTER detection.  Integer-exact.
//
// MI355X mapping: one 256-thread workgroup per 64x48 tile; the 72x56 pixel tile and the 72x50 score tile live in
// LDS (every image byte is read from HBM once + halo, scores never go to HBM).  Three phases per tile, all of them
// working on DWORDS of four horizontally adjacent pixels (byte-wide LDS reads were 4x the instructions):
//  (1) the 4-pixel necessary test: a lane reads the five dwords that hold the compass pixels of its four positions,
//      survivors are compacted into a wave-private LDS list with ballots (no atomics, no barrier before phase 2);
//  (2) the ~200-op corner score for the compacted candidates only (dense lanes instead of a divergent early-out);
//  (3) 3x3 non-max suppression, again a dword of four scores per lane with its eight neighbouring dwords; quads with no
//      positive score (most) leave after one read.
// Survivors go to an LDS list first.  The front-end engine takes them as PER-TILE lists (tile_kp / tile_count: plain
// coalesced stores, every tile writes its count, no atomics and nothing to wait for -- the returning global atomics of a
// per-cell list were a quarter of the kernel's time); its select kernel bins them into grid cells.  The stand-alone
// detector (av_fast_detect) appends them to one flat list per image with one returning atomic per tile.
// A survivor is one packed word, score << B | (2^B - 1 - raster) (av_common.h): B is an argument of the launch -- 19 for av_fast_detect and
// for engines of up to 2^19 pixels, whose words are what they always were, 24 for av_fast_detect_wide and larger engines.
// Bound: VALU instruction issue, not the image read (profiles/fast_diet/README.md).  The image is 0.74 GB per step of 2,048 stereo
// streams, 0.15 ms at the rate of a copy; the kernel takes 1.22 ms alone (8 x that), issues 778 VALU instructions per wavefront
// (phase 1 about 75 per 64 quads, phase 2 84 per 64 candidates of which 56 are the packed minima / maxima, phase 3 about 60 per
// 64 quads) and its wavefronts wait on instruction issue for 46 % of their cycles.
// So the bookkeeping around the arithmetic is kept out of the per-pixel path: a thread owns one dword column of the tile (one
// division in the kernel, every LDS address of staging and phase 1 is 4 * thread + a constant), which positions of a quad can be
// corners is a per-lane constant, the row / column / image-edge tests run only in the tiles where they can bind (decided per
// workgroup), a candidate is stored as the LDS offset of its pixel, and phase 3 claims its slots with one LDS atomic per wavefront.
#include <stdlib.h>

#include "av_common.h"

namespace {

constexpr int TW = AV_FAST_TW, TH = AV_FAST_TH;      // 64 x 48
constexpr int PW = TW + 8, PH = TH + 8;     // pixel tile: columns x0-4 .. x0+67 (pc = x - x0 + 4), rows y0-4 .. y0+51
constexpr int PWD = PW / 4;                 // 18 dwords per pixel row
constexpr int SP = PW, SH = TH + 2;         // score tile: column index = pc (same dword phase as the pixels), row sr = y - y0 + 1
constexpr int SPD = SP / 4;
constexpr int TCAP = TW * TH / 4;           // strict 3x3 maxima in one tile: at most one per 2x2 block

struct FastArgs {
    const uint8_t* img;
    int64_t img_stride;
    int img_pitch;
    int border;                 // valid pixels around the w x h image in every direction (padded pyramid level: AV_PYR_BORDER; raw image: 0)
    const uint8_t* mask;
    int64_t mask_stride;
    int w, h, threshold;
    int rbits;                  // raster bits of the packed words (av_common.h)
    uint32_t* kp; int* count; int cap;
    uint32_t* tile_kp; int* tile_count;          // [n_img][tiles][TCAP], [n_img][tiles] (tiles row-major: by * tiles_x + bx)
    int* overflow; int stat_stride;
    int n_img, tiles_x, tiles_y;                 // XCD-aware 1-D launch (fast_kernel)
    const int* index;                            // optional: image i of the launch is storage entry index[i] (shared frame store)
};

// Corner score of one candidate, the 16 ring differences two to a register (packed 16-bit lanes: ring position j in the low
// half, its antipode j + 8 in the high half, j = 0..7).  The circular sliding minima / maxima of cornerScore<16>
// (windows of 2, 4, then 9 = 4 + 4 + 1) become 8 packed operations per stage instead of 16: "the next position" of the pair
// (j, j + 8) is the pair (j + 1, j + 9), and past the end of the array it is an earlier pair with its halves swapped, which
// the packed instructions take for free through their operand half selects.
typedef short av_s2 __attribute__((ext_vector_type(2)));
// Three-input packed minima / maxima (round 5).  gfx950 has no three-input packed INTEGER min / max, but it has v_pk_minimum3_f16 /
// v_pk_maximum3_f16, and the order of non-negative half-precision bit patterns is the order of the integers they spell: the ring
// differences are biased into 1 .. 511 (subnormal patterns, kept as they are: the kernel runs with fp16 denormals on, the default),
// compared as halves, and un-biased at the end.  A window minimum of nine = min3(min4, min4, far) is then ONE instruction instead of
// two, and two windows fold into the running best at once: 56 packed operations per candidate instead of 80 (all of them half-rate
// instructions, profiles/r05/valu_issue_microbench.json).  Same integers, same scores: tests/test_gpu_ops.py.
typedef _Float16 av_h2 __attribute__((ext_vector_type(2)));
typedef unsigned short av_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ av_h2 h2_swap(av_h2 x) { return __builtin_shufflevector(x, x, 1, 0); }
__device__ __forceinline__ av_h2 h2_min(av_h2 a, av_h2 b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ av_h2 h2_max(av_h2 a, av_h2 b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ av_h2 h2_min3(av_h2 a, av_h2 b, av_h2 c) { return __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), c); }
__device__ __forceinline__ av_h2 h2_max3(av_h2 a, av_h2 b, av_h2 c) { return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c); }
__device__ __forceinline__ int fast_score(const uint8_t* c, int t)
{
    // c points at the centre pixel inside the LDS pixel tile (row stride PW)
    constexpr int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int DY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    constexpr int BIAS = 256;
    const int v = c[0];
    const av_us2 vb = {(unsigned short)(v + BIAS), (unsigned short)(v + BIAS)};
    av_h2 D[8];                                     // BIAS + v - ring[j], BIAS + v - ring[j + 8]: 1 .. 511
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const av_us2 pk = {(unsigned short)c[DY[j] * PW + DX[j]], (unsigned short)c[DY[j + 8] * PW + DX[j + 8]]};     // one byte load per half
        D[j] = __builtin_bit_cast(av_h2, vb - pk);
    }
    av_h2 L2[8], H2[8], L4[8], H4[8];               // min / max over 2 and over 4 consecutive ring positions
#pragma unroll
    for (int j = 0; j < 8; ++j) { const av_h2 nx = j < 7 ? D[j + 1] : h2_swap(D[0]); L2[j] = h2_min(D[j], nx); H2[j] = h2_max(D[j], nx); }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        L4[j] = h2_min(L2[j], j < 6 ? L2[j + 2] : h2_swap(L2[j - 6]));
        H4[j] = h2_max(H2[j], j < 6 ? H2[j + 2] : h2_swap(H2[j - 6]));
    }
    av_h2 lo9[8], hi9[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {                   // windows of 9: positions i..i+3, i+4..i+7, i+8
        const av_h2 far = h2_swap(D[j]);
        lo9[j] = h2_min3(L4[j], j < 4 ? L4[j + 4] : h2_swap(L4[j - 4]), far);
        hi9[j] = h2_max3(H4[j], j < 4 ? H4[j + 4] : h2_swap(H4[j - 4]), far);
    }
    av_h2 A = h2_max(lo9[0], lo9[1]), Bm = h2_min(hi9[0], hi9[1]);      // best arc of "centre brighter than ring by at least" / "darker" (negated)
#pragma unroll
    for (int j = 2; j < 8; j += 2) { A = h2_max3(A, lo9[j], lo9[j + 1]); Bm = h2_min3(Bm, hi9[j], hi9[j + 1]); }
    const av_us2 Au = __builtin_bit_cast(av_us2, A), Bu = __builtin_bit_cast(av_us2, Bm);
    const int m = max(max((int)Au.x, (int)Au.y) - BIAS, BIAS - min((int)Bu.x, (int)Bu.y));
    return m > t ? m - 1 : 0;
}

// A dword of four bytes -> 0xFF in every byte that is not zero (mask bytes: any non-zero value means "keep").
__device__ __forceinline__ uint32_t nz_bytes(uint32_t m)
{
    const uint32_t hb = (((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u;      // no carry leaves a byte: 0x7F + 0x7F = 0xFE
    return (hb >> 7) * 0xFFu;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void fast_kernel(FastArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t pix[PH * PW + 16];     // +16: the last quad of the last row reads one dword past it
    __shared__ __attribute__((aligned(16))) uint8_t sc[SH * SP];
    // candidate lists, one private segment per wavefront (a wavefront judges at most 64 lanes x 4 rows x 4 positions)
    constexpr int NQ = SH * PWD;                                  // 900 quad positions
    constexpr int SEG = ((NQ + 255) / 256) * 64 * 4;
    __shared__ uint16_t cand[4 * SEG];
    // workgroup -> (image, tile).  1-D launch: all tiles of an image on ONE XCD (workgroups are dealt round-robin
    // over the 8 XCDs, each with its own L2): neighbouring tiles share their halo rows and, with 752-byte image rows, most of
    // their 128-byte lines -- spread over eight L2s every line was fetched ~3.7x (PMC, profiles/r03), on one L2 once.
    const int L = blockIdx.x, wg = L >> 3, per = a.tiles_x * a.tiles_y;
    int img_i = (L & 7) + 8 * (wg / per);
    if (img_i >= a.n_img) return;
    const int tl = wg % per;
    const int by = tl / a.tiles_x, bx = tl - by * a.tiles_x;
    if (a.index) img_i = a.index[img_i];                     // storage entry of this image (shared frame store): image, mask and lists
    const uint8_t* img = a.img + img_i * a.img_stride;
    const int x0 = bx * TW, y0 = by * TH;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // Who owns what.  Staging and phase 1: thread t < 252 owns dword column cq = t % 18 of the pixel / score tile and rows
    // rq + 14 j (56 = 4 x 14 pixel rows, 50 score rows): the ONE division of the kernel, and every LDS address of the two stages
    // is 4 t plus a constant.  Phase 3: 256 = 16 x 16, thread t owns quad column q3 = t % 16 and rows t / 16 + 16 it.
    constexpr int NOWN = 14 * PWD;                              // 252
    const int rq = tid / PWD, cq = tid - rq * PWD;
    const bool owner = tid < NOWN;
    const int r3 = tid >> 4, q3 = tid & 15;
    // What can bind in this tile, decided once per workgroup: pixels past the right / bottom edge of the image (ragged), score rows
    // outside y in [3, h - 3) (edge_y).
    const bool ragged = x0 + TW > a.w || y0 + TH > a.h;
    const bool edge_y = y0 < 4 || y0 + TH + 4 > a.h;

    // pixel tile: 56 rows x 72 bytes from (x0-4, y0-4) (x0 is a multiple of 64, so x0-4 is dword aligned when pitch and base are)
    uint32_t* pixw = reinterpret_cast<uint32_t*>(pix);
    // allow[it]: which of the four pixels a lane judges in iteration it of phase 3 may become keypoints at all.  With a mask that
    // can be read as dwords it is the mask dword (a quad is then wholly inside or wholly outside the image: outside reads as 0),
    // fetched NOW, with the pixel tile: a mask read behind the non-max suppression was a dependent HBM round trip in the middle of
    // every tile.  Without one only a ragged tile has pixels to refuse (0xFF per pixel inside the image).  A tile that is neither
    // never looks at it.
    constexpr int NIT3 = (TW / 4) * TH / 256;
    uint32_t allow[NIT3];
    const bool mask_dw = a.mask && (((a.w | (int)(a.mask_stride & 3) | (int)(reinterpret_cast<uintptr_t>(a.mask) & 3)) & 3) == 0);
    const bool use_allow = mask_dw || ragged;
#pragma unroll
    for (int it = 0; it < NIT3; ++it) allow[it] = 0xFFFFFFFFu;
    if (mask_dw) {
        const int x = x0 + 4 * q3;
        const uint8_t* mp = a.mask + img_i * a.mask_stride + x;
#pragma unroll
        for (int it = 0; it < NIT3; ++it) {
            const int y = y0 + r3 + 16 * it;
            allow[it] = (x + 4 <= a.w && y < a.h) ? *reinterpret_cast<const uint32_t*>(mp + (size_t)y * a.w) : 0u;
        }
    } else if (ragged) {
#pragma unroll
        for (int it = 0; it < NIT3; ++it) {
            const int left = a.w - (x0 + 4 * q3);                  // pixels of the quad inside the image
            allow[it] = (y0 + r3 + 16 * it < a.h && left > 0) ? (left >= 4 ? 0xFFFFFFFFu : 0xFFFFFFFFu >> (8 * (4 - left))) : 0u;
        }
    }
    // Tile rows as dwords whenever rows, stride and base are dword aligned (then a dword lies wholly inside or wholly outside the
    // valid columns): all four loads of a thread are issued in one basic block -- as a loop the compiler waited for every load
    // before issuing the next (one dword in flight per thread).  A tile whose 72 x 56 pixels all exist (image or frame) adds a
    // constant row stride to one address; in the others rows above / below the valid rows are clamped and dwords left / right of
    // the valid columns read as zero.  Pixels outside the image never reach a valid output (corners need x, y in [3, dim - 3)),
    // so clamp vs reflect vs zero is immaterial.
    const bool dw_rows = ((a.img_pitch | a.w | (int)(a.img_stride & 3) | (int)(reinterpret_cast<uintptr_t>(a.img) & 3)) & 3) == 0;
    if (dw_rows) {
        if (owner) {
            constexpr int NLD = PH / 14;
            uint32_t v[NLD];
            const int xb = x0 - 4 + 4 * cq;
            const bool whole = y0 - 4 >= -a.border && y0 + TH + 4 <= a.h + a.border && x0 - 4 >= -a.border && x0 + TW + 4 <= a.w + a.border;
            if (whole) {
                const uint8_t* p = img + (ptrdiff_t)(y0 - 4 + rq) * a.img_pitch + xb;
#pragma unroll
                for (int j = 0; j < NLD; ++j) v[j] = *reinterpret_cast<const uint32_t*>(p + (ptrdiff_t)(14 * j) * a.img_pitch);
            } else {
                const bool in = xb >= -a.border && xb + 4 <= a.w + a.border;
#pragma unroll
                for (int j = 0; j < NLD; ++j) {
                    const int y = min(max(y0 - 4 + rq + 14 * j, -a.border), a.h + a.border - 1);
                    v[j] = *reinterpret_cast<const uint32_t*>(in ? img + (ptrdiff_t)y * a.img_pitch + xb : img);
                }
#pragma unroll
                for (int j = 0; j < NLD; ++j) v[j] = in ? v[j] : 0u;
            }
#pragma unroll
            for (int j = 0; j < NLD; ++j) pixw[tid + NOWN * j] = v[j];
        } else {
            pixw[PH * PWD + tid - NOWN] = 0;
        }
    } else {
        for (int i = tid; i < PH * PW; i += 256) {
            int r = i / PW, c = i - r * PW;
            int y = min(max(y0 - 4 + r, 0), a.h - 1), x = min(max(x0 - 4 + c, 0), a.w - 1);
            pix[i] = img[(size_t)y * a.img_pitch + x];
        }
        if (tid < 4) pixw[PH * PWD + tid] = 0;
    }
    // Which of the lane's four positions pc = 4 cq + k can be corners at all (bit 7 of byte k): columns 3 .. TW + 4 of the tile that
    // lie in x in [3, w - 3).  The column is the lane's for the whole of phase 1, so this is computed once.
    uint32_t V = 0;
    {
        const int lo = max(3, 7 - x0), hi = min(TW + 4, a.w - x0);          // x = x0 - 4 + pc in [3, w - 3)
#pragma unroll
        for (int k = 0; k < 4; ++k) V |= (4 * cq + k >= lo && 4 * cq + k <= hi) ? 0x80u << (8 * k) : 0u;
    }
    __syncthreads();
    // Phase 1: cheap necessary condition on the 4 compass pixels of the ring (any 9-arc contains at least two of them) for the
    // four positions pc = 4 cq .. 4 cq + 3 of score row sr = rq + 14 it (pixel row sr + 3): dwords U (3 rows up), D (3 rows down),
    // L, C, R of the row.  Quad i = sr * PWD + cq = tid + 252 it is dword i of the score tile and dword i + 3 PWD of the pixel tile.
    uint32_t* scw = reinterpret_cast<uint32_t*>(sc);
    uint16_t* seg = cand + wave * SEG;
    int wcnt = 0;                                   // candidates found by this wavefront so far (wavefront-uniform)
    const int t = a.threshold;
#pragma unroll
    for (int it = 0; it < (SH + 13) / 14; ++it) {
        const int i = tid + NOWN * it;
        uint32_t m = 0;                             // bit 7 of byte k: position k passes the test and can be a corner
        if (14 * (it + 1) <= SH ? owner : tid < (SH - 14 * it) * PWD) {
            scw[i] = 0;
            uint32_t Vr = V;
            if (edge_y) {
                const int y = y0 - 1 + rq + 14 * it;
                Vr = (y >= 3 && y < a.h - 3) ? V : 0u;
            }
            const uint32_t* rowc = pixw + i + 3 * PWD;
            // (the dword left of quad 0 belongs to the row above: it only feeds positions 0 .. 2, which V rules out)
            const uint32_t C = rowc[0], Lw = rowc[-1], R = rowc[1];
            const uint32_t U = rowc[-3 * PWD], D = rowc[3 * PWD];
            const uint32_t R3 = __builtin_amdgcn_alignbyte(R, C, 3), L3 = __builtin_amdgcn_alignbyte(C, Lw, 1);      // p[+3], p[-3] of the four positions
            // Packed 16-bit lanes, two pixels per register.  Any 9-arc of the 16-ring holds at least one pixel of EVERY
            // antipodal pair, so "centre brighter than one of (p0, p8) AND than one of (p4, p12)" -- or the same for darker --
            // is necessary for a corner (OpenCV's own first rejection tests):
            //   bright: min(max(d0, d8), max(d4, d12)) > t     dark: max(min(d0, d8), min(d4, d12)) < -t
            auto half = [](uint32_t x, int hi) -> av_s2 { return __builtin_bit_cast(av_s2, __builtin_amdgcn_perm(0, x, hi ? 0x0C030C02u : 0x0C010C00u)); };
            const av_s2 tt = {(short)t, (short)t}, zz = {0, 0};
            uint32_t fl[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const av_s2 c = half(C, hf);
                const av_s2 d0 = c - half(D, hf), d8 = c - half(U, hf), d4 = c - half(R3, hf), d12 = c - half(L3, hf);
                const av_s2 mb = __builtin_elementwise_min(__builtin_elementwise_max(d0, d8), __builtin_elementwise_max(d4, d12));
                const av_s2 md = __builtin_elementwise_max(__builtin_elementwise_min(d0, d8), __builtin_elementwise_min(d4, d12));
                const av_s2 val = __builtin_elementwise_max(mb, zz - md);
                fl[hf] = __builtin_bit_cast(uint32_t, tt - val);             // negative (bit 15 of its half set) iff val > t
            }
            m = __builtin_amdgcn_perm(fl[1], fl[0], 0x07050301u) & Vr;       // the four sign bytes side by side
        }
        // ordered compaction into this wavefront's own segment: no LDS atomic, no cross-lane broadcast.  A candidate is the byte
        // offset of its centre in the pixel tile (at most 3,815); its score byte lies 3 PW before that offset in the score tile.
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool hit = (m & (0x80u << (8 * k))) != 0;
            const unsigned long long b = __builtin_amdgcn_ballot_w64(hit);
            if (__builtin_amdgcn_inverse_ballot_w64(b)) (seg + wcnt)[__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u))] = (uint16_t)(4 * i + 3 * PW + k);
            wcnt += __popcll(b);
        }
    }
    // Phase 2: full corner score only for the candidates -- each wavefront scores its own list (the LDS traffic of one
    // wavefront is ordered, so no workgroup barrier is needed between the two phases)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = lane; k < wcnt; k += 64) {
        const int o = seg[k];
        sc[o - 3 * PW] = (uint8_t)fast_score(&pix[o], t);
    }
    __syncthreads();
    // Phase 3: 3x3 non-max suppression + mask; survivors go to an LDS list first so that the tile issues
    // ONE returning global atomic per output list it touches instead of one per keypoint.
    __shared__ uint32_t surv_word[TCAP];
    __shared__ int nsurv, flat_base;
    if (tid == 0) nsurv = 0;
    __syncthreads();
    // quads of the tile interior: columns pc = 4q .. 4q+3, q = 1 + q3 (x = x0 + 4 q3 ..), score rows sr = 1 + r3 + 16 it (y = y0 + r3 + 16 it)
    const uint32_t* s3 = scw + (r3 + 1) * SPD + 1 + q3;
    const uint32_t ones = (1u << a.rbits) - 1u;
    const uint32_t rb0 = ones - (uint32_t)((y0 + r3) * a.w + x0 + 4 * q3);       // raster part of the word of pixel 0 of the quad, it = 0
#pragma unroll
    for (int it = 0; it < NIT3; ++it) {
        const uint32_t* rowc = s3 + 16 * SPD * it;
        const uint32_t B = rowc[0];
        uint32_t gb = 0;                                      // byte k != 0: pixel k is a keypoint
        if (B != 0) {                                         // a positive score among the four pixels (most quads have none)
            // Byte w of the 6-byte window [pc-1 .. pc+4] of a score row is byte 3 of the dword before (w = 0), the row's dword (1 .. 4)
            // or byte 0 of the dword after (5); pixel k sees w = k (left), k + 1 (centre), k + 2 (right).  Strict 3x3 maximum test
            // for the four pixels at once, two pixels per register (packed u16), every pair one v_perm of the dwords as loaded.
            typedef unsigned short av_u2 __attribute__((ext_vector_type(2)));
            uint32_t A[3], M[3], N[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const uint32_t* rp = rowc + (d - 1) * SPD;
                A[d] = rp[-1]; M[d] = d == 1 ? B : rp[0]; N[d] = rp[1];
            }
            auto p01 = [&](int d) -> av_u2 { return __builtin_bit_cast(av_u2, __builtin_amdgcn_perm(M[d], A[d], 0x0C040C03u)); };
            auto p12 = [&](int d) -> av_u2 { return __builtin_bit_cast(av_u2, __builtin_amdgcn_perm(0, M[d], 0x0C010C00u)); };
            auto p23 = [&](int d) -> av_u2 { return __builtin_bit_cast(av_u2, __builtin_amdgcn_perm(0, M[d], 0x0C020C01u)); };
            auto p34 = [&](int d) -> av_u2 { return __builtin_bit_cast(av_u2, __builtin_amdgcn_perm(0, M[d], 0x0C030C02u)); };
            auto p45 = [&](int d) -> av_u2 { return __builtin_bit_cast(av_u2, __builtin_amdgcn_perm(N[d], M[d], 0x0C040C03u)); };
            // (scores are 0 .. 254: as half-precision bit patterns they order like the integers -- one v_pk_maximum3_f16 per three, see fast_score)
            auto mx3 = [](av_u2 x, av_u2 y, av_u2 z) -> av_u2 { return __builtin_bit_cast(av_u2, h2_max3(__builtin_bit_cast(av_h2, x), __builtin_bit_cast(av_h2, y), __builtin_bit_cast(av_h2, z))); };
            const av_u2 n01 = mx3(mx3(p01(0), p12(0), p23(0)), mx3(p01(2), p12(2), p23(2)), mx3(p01(1), p23(1), p23(1)));
            const av_u2 n23 = mx3(mx3(p23(0), p34(0), p45(0)), mx3(p23(2), p34(2), p45(2)), mx3(p23(1), p45(1), p45(1)));
            const av_u2 g01 = __builtin_elementwise_sub_sat(p12(1), n01), g23 = __builtin_elementwise_sub_sat(p34(1), n23);
            // half k & 1 of g(k >> 1) != 0: score > all 8 neighbours; the differences are below 256, their low bytes side by side
            gb = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, g23), __builtin_bit_cast(uint32_t, g01), 0x06040200u);
            if (use_allow) gb &= mask_dw ? nz_bytes(allow[it]) : allow[it];
            if (a.mask && !mask_dw && gb != 0) {              // a mask that only bytes can read: looked at for the keypoints alone
                const uint8_t* mp = a.mask + img_i * a.mask_stride + (size_t)(y0 + r3 + 16 * it) * a.w + x0 + 4 * q3;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((gb >> (8 * k)) & 0xFFu) gb = mp[k] != 0 ? gb : gb & ~(0xFFu << (8 * k));
            }
        }
        // one compaction per wavefront: a ballot per pixel position, the lane counts below, ONE LDS atomic by one lane for the lot
        unsigned long long bk[4];
        int tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { bk[k] = __builtin_amdgcn_ballot_w64(((gb >> (8 * k)) & 0xFFu) != 0); tot += __popcll(bk[k]); }
        if (tot == 0) continue;                               // (wavefront-uniform)
        int base = 0;
        if (lane == 0) base = atomicAdd(&nsurv, tot);         // LDS atomic; a tile has <= TCAP strict maxima
        base = __builtin_amdgcn_readfirstlane(base);
        const uint32_t rb = rb0 - (uint32_t)(16 * it * a.w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (__builtin_amdgcn_inverse_ballot_w64(bk[k])) {
                const int slot = __builtin_amdgcn_mbcnt_hi((unsigned)(bk[k] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bk[k], (unsigned)base));
                surv_word[slot] = (((B >> (8 * k)) & 0xFFu) << a.rbits) | (rb - k);
            }
            base += __popcll(bk[k]);
        }
    }
    __syncthreads();
    const int ns = nsurv;
    if (a.tile_kp) {
        const size_t tile = (size_t)img_i * (a.tiles_x * a.tiles_y) + by * a.tiles_x + bx;
        if (tid == 0) a.tile_count[tile] = ns;
        for (int q = tid; q < ns; q += 256) a.tile_kp[tile * TCAP + q] = surv_word[q];
        return;
    }
    if (ns == 0) return;
    if (tid == 0) flat_base = atomicAdd(&a.count[img_i], ns);
    __syncthreads();
    for (int q = tid; q < ns; q += 256) {
        const int idx = flat_base + q;
        if (idx < a.cap) a.kp[(size_t)img_i * a.cap + idx] = surv_word[q];
        else if (a.overflow) atomicOr(&a.overflow[img_i * a.stat_stride], 1);
    }
}

}  // namespace

void av_fast_tiles(int w, int h, int* tiles, int* tile_cap)
{
    *tiles = ((w + TW - 1) / TW) * ((h + TH - 1) / TH);
    *tile_cap = TCAP;
}

// Exactly one of (kp, count, cap) -- a flat list per image -- and (tile_kp, tile_count) -- per-tile lists, see av_fast_tiles -- is given.
int av_launch_fast(const ImgView& src, const PyrGeom* g, const uint8_t* mask, int64_t mask_stride,
                   int n_img, int w, int h, int threshold, int raster_bits,
                   uint32_t* kp, int* count, int cap, uint32_t* tile_kp, int* tile_count,
                   int* overflow, int stat_stride, hipStream_t st)
{
    if (n_img <= 0) return AV_OK;
    if (!src.img && !g) { av_set_error("av_fast_detect: a pyramid source needs its geometry"); return AV_E_INVALID; }
    if ((raster_bits != AV_KP_RASTER_BITS && raster_bits != AV_KP_RASTER_BITS_WIDE) || (int64_t)w * h > ((int64_t)1 << raster_bits)) {
        av_set_error("av_fast_detect: image %dx%d exceeds 2^%d pixels", w, h, raster_bits);
        return AV_E_INVALID;
    }
    const int64_t n_wg = (int64_t)((w + TW - 1) / TW) * ((h + TH - 1) / TH) * 8 * ((n_img + 7) / 8);
    if (n_wg * 256 > 0xFFFFFFFFll) {                       // a launch holds fewer than 2^32 threads
        av_set_error("av_fast_detect: %d images of %dx%d are more than one launch holds (%lld workgroups)", n_img, w, h, (long long)n_wg);
        return AV_E_INVALID;
    }
    FastArgs a;
    // the image in place, or level 0 of the pyramid: the same pixels with a frame (every tile but the right-most column then copies
    // whole dwords without clamping)
    if (src.img) { a.img = src.img; a.img_stride = src.img_stride; a.img_pitch = w; a.border = 0; }
    else { a.img = src.pyr + g->off[0] + (size_t)AV_PYR_BORDER * g->pitch[0] + AV_PYR_BORDER; a.img_stride = src.pyr_stride; a.img_pitch = g->pitch[0]; a.border = AV_PYR_BORDER; }
    a.mask = mask; a.mask_stride = mask_stride;
    a.w = w; a.h = h; a.threshold = threshold; a.rbits = raster_bits;
    a.kp = kp; a.count = count; a.cap = cap;
    a.tile_kp = tile_kp; a.tile_count = tile_count; a.overflow = overflow; a.stat_stride = stat_stride;
    const int tx = (w + TW - 1) / TW, ty = (h + TH - 1) / TH;
    a.n_img = n_img; a.tiles_x = tx; a.tiles_y = ty; a.index = src.map;
    dim3 grid((unsigned)(tx * ty) * 8u * (unsigned)((n_img + 7) / 8));
    // (An occupancy throttle -- unused dynamic LDS holding the detector to 6 / 5 / 4 workgroups per CU so that the filter's kernels find
    //  room beside it -- was measured in round 5: 156.9 / 154.7 / 149.7 k against 157.5 k frames/s.  profiles/r05/README.md)
    // (The same 64 x 48 tile worked by two / one wavefront instead of four -- a workgroup of fewer wavefronts is easier to place beside the
    //  filter's single-wavefront tasks -- measured in round 5: detector 1.71 / 2.43 against 1.51 ms alone, 2.60 / 3.38 against 2.21 ms in
    //  the shared run, 170.2 / 159.5 against 173.4 k frames/s: with 19 KB of LDS per tile the CU then holds half / a quarter of the
    //  wavefronts.  What the detector needs is a wavefront that walks a column of small tiles.  profiles/r05/README.md)
    hipLaunchKernelGGL(fast_kernel, grid, dim3(256), 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

namespace {

int fast_detect_impl(const uint8_t* img_dev, int64_t img_stride, const uint8_t* mask_dev, int64_t mask_stride,
                     int n_img, int w, int h, int threshold, int raster_bits, uint32_t* kp_dev, int32_t* count_dev, int cap, void* stream)
{
    if (!img_dev || !kp_dev || !count_dev || cap <= 0 || n_img < 0 || w < 7 || h < 7 || img_stride < (int64_t)w * h) {
        av_set_error("av_fast_detect: bad arguments");
        return AV_E_INVALID;
    }
    if ((int64_t)w * h > ((int64_t)1 << raster_bits)) {     // before anything is enqueued
        av_set_error("av_fast_detect: image %dx%d exceeds 2^%d pixels", w, h, raster_bits);
        return AV_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    AV_HIP(hipMemsetAsync(count_dev, 0, sizeof(int) * (size_t)n_img, st));
    return av_launch_fast(ImgView{nullptr, 0, img_dev, img_stride, nullptr}, nullptr, mask_dev, mask_stride, n_img, w, h, threshold, raster_bits,
                          kp_dev, count_dev, cap, nullptr, nullptr, nullptr, 0, st);
}

}  // namespace

AV_EXPORT int av_fast_detect(const uint8_t* img_dev, int64_t img_stride, const uint8_t* mask_dev, int64_t mask_stride,
                             int n_img, int w, int h, int threshold, uint32_t* kp_dev, int32_t* count_dev, int cap,
                             void* stream)
{
    return fast_detect_impl(img_dev, img_stride, mask_dev, mask_stride, n_img, w, h, threshold, AV_KP_RASTER_BITS, kp_dev, count_dev, cap, stream);
}

AV_EXPORT int av_fast_detect_wide(const uint8_t* img_dev, int64_t img_stride, const uint8_t* mask_dev, int64_t mask_stride,
                                  int n_img, int w, int h, int threshold, uint32_t* kp_dev, int32_t* count_dev, int cap,
                                  void* stream)
{
    return fast_detect_impl(img_dev, img_stride, mask_dev, mask_stride, n_img, w, h, threshold, AV_KP_RASTER_BITS_WIDE, kp_dev, count_dev, cap, stream);
}
