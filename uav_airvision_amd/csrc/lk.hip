// lk.hip -- pyramidal iterative Lucas-Kanade tracker for gfx950, 16 lanes per point.
//
// Replaces cv2.calcOpticalFlowPyrLK as the reference calls it (winSize 15x15, maxLevel 3,
// criteria (EPS|COUNT, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW, minEigThreshold 1e-4):
//   src/image_processing/feature_tracker.py:102-108   (temporal, prev cam0 -> curr cam0)
//   src/image_processing/stereo_matcher.py:64-68      (stereo forward, cam0 -> cam1)
//   src/image_processing/stereo_matcher.py:70-74      (stereo backward, cam1 -> cam0)
//   parameters: src/config.py:31-44
//
// Semantics follow OpenCV 4.x video/lkpyramid.cpp (LKTrackerInvoker): W_BITS = 14 fixed-point
// bilinear weights, I patch scaled by 32, Scharr derivatives of the FIRST image (zero outside
// the image), 2x2 normal equations in float, <= max_iter Newton steps per level with the
// eps^2 and the oscillation stop, status decided at level 0 only.
//
// MI355X mapping
//   * one DPP row (16 lanes) owns one point for all pyramid levels (levels are a dependent chain per
//     point, points are independent): 4 points per wavefront, 16 per 256-thread workgroup, no
//     inter-workgroup synchronisation, one launch per LK call for every stream of the batch.
//   * lane r of a row owns window row r (15 pixels; lane 15 only feeds the interpolation of row 14).
//     The I patch and its two derivative patches live in 45 VGPRs per lane per level.  The float
//     Newton update of a point is identical in all its lanes, so one VALU instruction serves 4 points
//     (an earlier one-wavefront-per-point version spent half of every iteration on that replicated math).
//   * windows are staged through LDS: per level one coalesced 18x24-byte stage of the I
//     neighbourhood and one 32x32-byte stage of J around the predicted position (aligned dword
//     loads); every Newton iteration then reads 5 dwords of its row from LDS and takes the row below
//     from the neighbouring lane (DPP row_shl).  The J tile is restaged only when the window drifts
//     more than ~6 px.  1152 B of LDS per point.
//   * Scharr derivatives are computed on the fly from the staged neighbourhood (packed 16-bit
//     arithmetic on the even columns, odd pairs by v_perm) instead of materialising OpenCV's int16x2
//     derivative image (saves 4 B/pixel/level of HBM traffic).
//   * pyramid levels carry a 16-pixel reflect-101 frame, so no tap is ever clamped.
//   * the window sums are sums of integers; they are accumulated exactly (int32 per lane; across the
//     16 lanes by a DPP butterfly whose last two steps run on 16-bit halves, recombined in fp64)
//     and rounded once, which makes the result independent of the reduction order and bit-identical
//     to the scalar CPU oracle.
// Bound: VALU issue (PMC: ~1,400 VALU instructions per point pass; the staged tiles come from
// L2/MALL: the padded pyramids of a stream are ~560 KB); HBM sees each pyramid once per frame.
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "av_common.h"
#include "lk_host.h"

namespace {

struct LKArgs {
    const uint8_t* pyrI;
    const uint8_t* pyrJ;
    int64_t stream_stride;
    PyrGeom g;
    const float* prev;
    float* next;
    uint8_t* status;
    const int* count;
    const int* index;           // optional [n_set][cap]: point j of set s is index[s*cap + j] (a subset of the point arrays)
    int cap;
    int max_iter;
    double eps2;
    // float forms of the two fp64 thresholds (av_launch_lk): minEig < min_eig (double) <=> minEig < min_eig_up, the smallest float
    // >= min_eig; the step-length test is decided in float outside (eps_lo, eps_hi) = eps2 (1 -+ 2^-18) and in fp64 inside
    float min_eig_up, eps_lo, eps_hi;
    // the 16-lane kernel's form of minEig < min_eig_up without the division: minEig = fl(num / (2 win^2)) < min_eig_up <=> num <
    // min_eig_num (av_lk_quotient_bound, lk_host.h: the division is monotone; NaN when the threshold is NaN: the test fails nothing).
    // It sits in what was padding ahead of the double: no other field moves.
    float min_eig_num;
    double min_eig;             // the general kernel's fp64 form
    int n_set, gx;              // XCD-aware 1-D launch of the 16-lane kernels: gx workgroups per point set, see lk_track_g16_body
    // Level 0 straight from the caller's image (w x h, tightly packed rows) instead of a padded copy in the pyramid: non-null =
    // the I (resp. J) side reads level 0 at img + set * img_stride, with BORDER_REFLECT_101 indexing for the few windows that
    // reach over the image border (what the padded level's frame holds).  Levels >= 1 always come from the padded pyramid.
    const uint8_t* imgI; const uint8_t* imgJ;
    int64_t imgI_stride, imgJ_stride;
    // Optional storage maps (the front-end's shared frame store, frontend.hip): point set s reads the pyramids / level-0 images of
    // storage entry mapI[s] (I side) and mapJ[s] (J side) instead of entry s; a negative entry = the set has no frame in this step
    // and tracks nothing.  Null = identity.
    const int* mapI; const int* mapJ;
    // diagnostic (AV_LK_PROF=1, lk_track_g16_prof_kernel): per-phase s_memtime sums over every wavefront of the launch
    unsigned long long* prof;
};

// phases of a wavefront's life in the 16-lane kernel, as the stamps cut it
enum { LKP_HEAD = 0, LKP_ISTAGE, LKP_SETUP, LKP_JSTAGE, LKP_ITER, LKP_N, LKP_WAVES = LKP_N, LKP_ITERS, LKP_RESTAGES, LKP_LEVELS, LKP_SLOTS };

// LDS traffic of one wave is ordered by issue; this keeps the compiler from moving a read of the
// staged tile above the (other lanes') writes that fill it.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#define AV_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

typedef short av_v2s __attribute__((ext_vector_type(2)));
// a.lo*b.lo + a.hi*b.hi + c on packed signed 16-bit halves (v_dot2c_i32_i16, full rate, exact)
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(av_v2s, a), __builtin_bit_cast(av_v2s, b), c, false);
}
// the same with the accumulator in its own register: v_dot2c (what the builtin selects) accumulates in place, so an
// accumulator that has to survive -- the per-pixel seeds, the rounding constants -- costs a v_mov per use; the VOP3P
// form takes it as a third source
__device__ __forceinline__ int dot2_keep(uint32_t a, uint32_t b, int c)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// The four W_BITS = 14 bilinear weights of the fractions (fa, fb), packed for v_dot2: wtop = (iw00 | iw01 << 16), wbot = (iw10 | iw11 << 16),
//   iw00 = rn((1 - fa)(1 - fb) 2^14), iw01 = rn(fa (1 - fb) 2^14), iw10 = rn((1 - fa) fb 2^14), iw11 = 2^14 - iw00 - iw01 - iw10
// (rn = round to nearest, ties to even: cvRound / __float2int_rn), without a conversion instruction.  Why this is exact:
//   * Range.  fa = x - floor(x) is computed in float: the exact difference lies in [0, 1), so its rounding lies in [0, 1] (1.0 only for a
//     tiny negative x such as -1e-7: floor = -1, x + 1 rounds to 1.0 -- the weights are then those of fa = 1, as with the conversions).
//     1 - fa, 1 - fb lie in [0, 1] too, every product of two of them in [0, 1], and the multiplication by 2^14 is exact: 0 <= p <= 2^14.
//   * Rounding.  p + 2^23 lies in [2^23, 2^23 + 2^14], inside the binade [2^23, 2^24) whose floats are the integers: the addition (round
//     to nearest even, the mode every kernel of this library runs in; -ffp-contract=off: it is not fused with the multiplication) returns
//     2^23 + n with n the integer nearest to p, and of two equally near ones the one with an even significand, which is the even n
//     because 2^23 is even.  That is rn(p).  The float 2^23 + n has the bits 0x4B000000 + n, n <= 2^14: the low half of the word IS n.
//   * iw11.  Only the low halves of the words are packed, and the low half of a difference depends on the low halves alone: the three
//     biases 0x4B000000 drop out, and a sum of the three weights above 2^14 (each rounded up) gives the same negative 16-bit value.
//   (A NaN coordinate from the caller is outside this argument and outside the contract: the oracle's floor of a NaN is undefined.)
__device__ __forceinline__ void lk_weights(float fa, float fb, uint32_t& wtop, uint32_t& wbot)
{
    const float ga = 1.f - fa, gb = 1.f - fb;
    const uint32_t u00 = __float_as_uint(ga * gb * (float)(1 << 14) + 0x1p23f);
    const uint32_t u01 = __float_as_uint(fa * gb * (float)(1 << 14) + 0x1p23f);
    const uint32_t u10 = __float_as_uint(ga * fb * (float)(1 << 14) + 0x1p23f);
    const uint32_t u11 = (uint32_t)(1 << 14) - (u00 + u01 + u10);
    wtop = __builtin_amdgcn_perm(u01, u00, 0x05040100u);
    wbot = __builtin_amdgcn_perm(u11, u10, 0x05040100u);
}

// base + rows * pitch of a wave-uniform image origin, as an opaque scalar value (see the staging loops of lk_track_g16_body), and the
// unaligned dword at a per-lane 32-bit offset from it.  The address goes through the asm as an integer and comes back as a pointer to
// GLOBAL memory (which every image of this library is): a generic pointer out of an asm statement would be loaded from with flat_load.
typedef const __attribute__((address_space(1))) uint8_t* av_gptr;
__device__ __forceinline__ av_gptr lk_row_base(const uint8_t* base, int rows, int pitch)
{
    uint64_t p = (uint64_t)base + (uint64_t)rows * (uint64_t)pitch;
    asm("" : "+s"(p));
    return (av_gptr)p;
}
__device__ __forceinline__ uint32_t lk_load_u32(av_gptr rowbase, uint32_t off)
{
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    return *(const __attribute__((address_space(1))) u32_unaligned*)(rowbase + off);
}

constexpr int TILE_ROWS = 24;     // staged J tile: 24 rows x 32 bytes (window 16 rows + 4 px of drift either way)
constexpr int TILE_COLS = 32;
constexpr int TPITCH = 36;        // LDS row pitch in bytes (9 dwords: the 16 rows of a point fall on 16 different banks)
constexpr int TILE_DWORDS = 240;  // >= 24 * 9, and == 16 mod 32: the two points of a 32-lane LDS access group use disjoint banks

// =================================================================================================
// 16 lanes per point: lane r of a DPP row owns window row r (15 pixels + the column right of them); lane 15 owns
// row 15, which only feeds the bilinear interpolation of row 14.  A lane builds ONLY its own row of the I patch
// and of the two Scharr derivative patches; the row below, which every bilinear sample needs, is read out of the
// next lane's registers by the DPP operand of v_dot2c_i32_i16 (row_shl:1) -- no second copy of the row, no
// v_mov_dpp, no second byte permute per pixel.  The float Newton update of a point is identical in all its
// lanes, so one VALU instruction serves 4 points.  Window sums stay exact: int32 per lane
// (15 x 8160 x 4080 < 2^31), split into 16-bit halves for the 16-lane DPP butterfly, recombined in fp64.
// =================================================================================================
typedef unsigned short av_v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(av_v2u, a) + __builtin_bit_cast(av_v2u, b)); }
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(av_v2u, a) - __builtin_bit_cast(av_v2u, b)); }
__device__ __forceinline__ uint32_t pk_mul(uint32_t a, unsigned short k) { av_v2u kk = {k, k}; return __builtin_bit_cast(uint32_t, __builtin_bit_cast(av_v2u, a) * kk); }

// exact sum S over the 16 lanes of a DPP row of an int32 that may overflow when summed (16-bit halves), returned as
// (float)(S * 2^-20) rounded ONCE -- the value of (float)((double)S * 2^-20), without the fp64 instructions: the two half sums are
// exact as floats (|hi| < 2^17, lo < 2^18), so is lo * 2^-20, and the fused multiply-add rounds the exact hi * 2^-4 + lo * 2^-20 =
// S * 2^-20 once.  (fp64 form: 2 x v_cvt_f64_i32, v_ldexp_f64, v_add_f64, v_ldexp_f64, v_cvt_f32_f64 per sum -- six half-rate
// instructions against two half-rate conversions, one multiply and one fused multiply-add here; five sums per Newton iteration and
// level set-up: profiles/r05/valu_issue_microbench.json.)
__device__ __forceinline__ float row_sum16_scaled(int v)
{
    // |v| <= 15 * 8160 * 4080 < 2^29: the sum over a quad still fits int32, the sum over 16 lanes does not
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    int lo = v & 0xFFFF, hi = v >> 16;
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xF, 0xF, false); // row_half_mirror
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xF, 0xF, false);
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xF, 0xF, false); // row_mirror
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xF, 0xF, false);
    return __builtin_fmaf((float)hi, 0x1p-4f, (float)lo * 0x1p-20f);
}

// The same value for a sum of SQUARES (a11, a22), in one unsigned butterfly.  Every lane's share is non-negative and at most
// 15 x 4080^2 = 249,696,000 (15 columns, |Ix|, |Iy| <= 4080), lane 15's share is zero (lk_patch_rows), so the total S over the row is at
// most 15 x 249,696,000 = 3,745,440,000 < 2^32: the four 32-bit additions do not wrap, v_cvt_f32_u32 rounds the exact S once (to
// nearest even), and the multiplication by 2^-20 is exact (S = 0 stays 0, S >= 1 gives >= 2^-20: no underflow) -- (float)(S * 2^-20)
// rounded once, what row_sum16_scaled returns, in 6 instructions instead of 12.  a12, b1 and b2 are signed: they stay with the halves.
__device__ __forceinline__ float row_sum_sq_scaled(int a)
{
    uint32_t v = (uint32_t)a;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);   // row_mirror
    return (float)v * 0x1p-20f;
}

// sqrtf(x), correctly rounded, for x = 0 or 2^-96 <= x < inf: the instructions the compiler's own correctly rounded sqrtf executes for
// such an x, without the ones that only serve other arguments.  The compiler's expansion (-fhip-fp32-correctly-rounded-divide-sqrt,
// subnormals kept) is: scale x by 2^32 if x < 2^-96 (compare, multiply, select); s = v_sqrt_f32 (1 ulp); the one-ulp fix-up below;
// scale back (multiply, select); return x itself if x is +-0 or +inf (class test, select).  For 2^-96 <= x < inf neither select
// takes its other arm, and what is left is exactly the lines below: the same instructions on the same values, the same result.  For
// x = +0 the compiler's form returns x = +0 through the class test; here s = v_sqrt_f32(+0) = +0, the neighbour below has the bits
// 0xFFFFFFFF, a NaN, so that its residual is a NaN and `<= 0` is false; the neighbour above is the smallest subnormal (or zero, if it
// were flushed), its residual fma(-tiny, 0, 0) = +0 and `> 0` is false: s = +0 stands.
// The caller's argument is (A11 - A22)^2 + 4 A12^2 with A11, A12, A22 multiples of 2^-20 below 2^12 in magnitude (row_sum16_scaled: an
// integer below 2^32 times 2^-20, rounded to 24 bits, which keeps it a multiple of 2^-20): the difference and A12 are 0 or at least
// 2^-20 in magnitude, the squares 0 or at least 2^-40, at most 2^26: x is +0 or in [2^-40, 2^27], inside the range above.
__device__ __forceinline__ float lk_sqrt_ranged(float x)
{
    float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);      // the neighbours of s
    const float vd = __builtin_fmaf(-sd, s, x), vu = __builtin_fmaf(-su, s, x);                                    // their residuals
    s = vd <= 0.f ? sd : s;
    s = vu > 0.f ? su : s;
    return s;
}

// Bilinear sample of five packed pixel (or derivative) pairs x_i = (v[c], v[c+1]) of this lane's row with the same
// pairs of the row below (next lane, DPP row_shl:1):  acc_i = x_i . wtop + below(x_i) . wbot + rnd.
// One asm statement, for two reasons: the compiler does not fold a DPP move into v_dot2c (it has a tied accumulator),
// and its hazard recogniser does not see into inline asm -- a DPP operand written by a VALU instruction needs 2 wait
// states, guaranteed here by issuing the plain dot products first.
//
// deriv5<G>: columns 5 G .. 5 G + 4 of BOTH derivative patches (they share the weights), returned as the packed column pairs the window
// sums want, (Ix[2p] | Ix[2p+1] << 16) and the same for Iy, WITHOUT a shift.  OpenCV's value is (S + 2^13) >> 14, S = the weighted sum
// of four Scharr values.  The caller hands in the Scharr values times 4 and 4 * 2^13 as rounding term, so that the accumulator is
// 4 S + 4 * 2^13 and  (4 S + 4 * 2^13) >> 16 == (S + 2^13) >> 14  (an arithmetic shift is the floor of the division, and
// floor(4 n / 2^16) = floor(n / 2^14) for every integer n): the wanted value is the HIGH half of the accumulator, which the v_perm that
// packs a pair takes directly (bytes 2, 3 of either word: selector 0x07060302; for the last, half-empty pair bytes 2, 3 and zeros:
// 0x0C0C0302).  Ranges: |Scharr| <= 16 x 255 = 4080, times 4 = 16,320 < 2^15, a signed 16-bit operand of v_dot2 like the weights
// (0 .. 2^14, iw11 >= -2); |accumulator| <= 16,320 x (2^14 + 4) + 2^15 < 2^29; the result, |.| <= 4080, fits the half it is taken from,
// sign included (the high half of a two's-complement word IS the word >> 16 as a 16-bit two's-complement number).
// The pairs straddle the groups of five (4|5, 9|10 do not: 4 is carried): group 0 hands accumulator 4 on to group 1 (cx, cy).
// Wait states: a v_dot2* result needs 3 before another VALU opcode reads it and 4 before one overwrites it, and the compiler does not
// know what wrote this statement's outputs.  The order below (x columns, then y columns, then the packs alternating x, y) leaves at
// least 4 instructions between every v_dot2c and the v_perm that reads or overwrites its result, and at least 4 after the last
// v_dot2c of the statement (group 0's carried y accumulator).
#define AV_DERIV_DOTS \
        "v_dot2_i32_i16 %0, %10, %20, %22\n\t" \
        "v_dot2_i32_i16 %1, %11, %20, %22\n\t" \
        "v_dot2_i32_i16 %2, %12, %20, %22\n\t" \
        "v_dot2_i32_i16 %3, %13, %20, %22\n\t" \
        "v_dot2_i32_i16 %4, %14, %20, %22\n\t" \
        "v_dot2_i32_i16 %5, %15, %20, %22\n\t" \
        "v_dot2_i32_i16 %6, %16, %20, %22\n\t" \
        "v_dot2_i32_i16 %7, %17, %20, %22\n\t" \
        "v_dot2_i32_i16 %8, %18, %20, %22\n\t" \
        "v_dot2_i32_i16 %9, %19, %20, %22\n\t" \
        "v_dot2c_i32_i16_dpp %0, %10, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %1, %11, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %2, %12, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %3, %13, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %4, %14, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %5, %15, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %6, %16, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %7, %17, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %8, %18, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_dot2c_i32_i16_dpp %9, %19, %21 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
template <int G>
__device__ __forceinline__ void deriv5(const uint32_t* gx, const uint32_t* gy, uint32_t wtop, uint32_t wbot, int rnd, uint32_t* ixx, uint32_t* iyy, uint32_t& cx, uint32_t& cy)
{
    uint32_t x0, x1, x2, x3, x4, y0, y1, y2, y3, y4;
    const uint32_t hi2 = 0x07060302u, hi1 = 0x0C0C0302u;
    if (G == 0) {            // columns 0 .. 4: pairs (0, 1), (2, 3); 4 is carried
        asm(AV_DERIV_DOTS
            "v_perm_b32 %0, %1, %0, %23\n\t"
            "v_perm_b32 %5, %6, %5, %23\n\t"
            "v_perm_b32 %2, %3, %2, %23\n\t"
            "v_perm_b32 %7, %8, %7, %23"
            : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3), "=&v"(y4)
            : "v"(gx[0]), "v"(gx[1]), "v"(gx[2]), "v"(gx[3]), "v"(gx[4]), "v"(gy[0]), "v"(gy[1]), "v"(gy[2]), "v"(gy[3]), "v"(gy[4]),
              "v"(wtop), "v"(wbot), "v"(rnd), "s"(hi2));
        ixx[0] = x0; iyy[0] = y0; ixx[1] = x2; iyy[1] = y2; cx = x4; cy = y4;
    } else if (G == 1) {     // columns 5 .. 9: pairs (4, 5), (6, 7), (8, 9)
        asm(AV_DERIV_DOTS
            "v_perm_b32 %0, %0, %24, %23\n\t"
            "v_perm_b32 %5, %5, %25, %23\n\t"
            "v_perm_b32 %1, %2, %1, %23\n\t"
            "v_perm_b32 %6, %7, %6, %23\n\t"
            "v_perm_b32 %3, %4, %3, %23\n\t"
            "v_perm_b32 %8, %9, %8, %23"
            : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3), "=&v"(y4)
            : "v"(gx[5]), "v"(gx[6]), "v"(gx[7]), "v"(gx[8]), "v"(gx[9]), "v"(gy[5]), "v"(gy[6]), "v"(gy[7]), "v"(gy[8]), "v"(gy[9]),
              "v"(wtop), "v"(wbot), "v"(rnd), "s"(hi2), "v"(cx), "v"(cy));
        ixx[2] = x0; iyy[2] = y0; ixx[3] = x1; iyy[3] = y1; ixx[4] = x3; iyy[4] = y3;
    } else {                 // columns 10 .. 14: pairs (10, 11), (12, 13), (14, the zero 16th column)
        asm(AV_DERIV_DOTS
            "v_perm_b32 %0, %1, %0, %23\n\t"
            "v_perm_b32 %5, %6, %5, %23\n\t"
            "v_perm_b32 %2, %3, %2, %23\n\t"
            "v_perm_b32 %7, %8, %7, %23\n\t"
            "v_perm_b32 %4, %4, %4, %24\n\t"
            "v_perm_b32 %9, %9, %9, %24"
            : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3), "=&v"(y4)
            : "v"(gx[10]), "v"(gx[11]), "v"(gx[12]), "v"(gx[13]), "v"(gx[14]), "v"(gy[10]), "v"(gy[11]), "v"(gy[12]), "v"(gy[13]), "v"(gy[14]),
              "v"(wtop), "v"(wbot), "v"(rnd), "s"(hi2), "s"(hi1));
        ixx[5] = x0; iyy[5] = y0; ixx[6] = x2; iyy[6] = y2; ixx[7] = x4; iyy[7] = y4;
    }
}
#undef AV_DERIV_DOTS

// The I patch itself is only ever used as the accumulator seed of the iteration's interpolation:
//   ((dot + R) >> 9) - ival == (dot + R - (ival << 9)) >> 9,  seed = R - (ival << 9),  ival << 9 == acc & ~511 (acc >= 0)
__device__ __forceinline__ void bilin5_seed(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4, uint32_t wtop, uint32_t wbot, int rnd,
                                            int& o0, int& o1, int& o2, int& o3, int& o4)
{
    asm("v_dot2_i32_i16 %0, %5, %10, %12\n\t"
        "v_dot2_i32_i16 %1, %6, %10, %12\n\t"
        "v_dot2_i32_i16 %2, %7, %10, %12\n\t"
        "v_dot2_i32_i16 %3, %8, %10, %12\n\t"
        "v_dot2_i32_i16 %4, %9, %10, %12\n\t"
        "v_dot2c_i32_i16_dpp %0, %5, %11 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %1, %6, %11 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %2, %7, %11 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %3, %8, %11 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %4, %9, %11 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_and_b32 %0, %13, %0\n\t"
        "v_and_b32 %1, %13, %1\n\t"
        "v_and_b32 %2, %13, %2\n\t"
        "v_and_b32 %3, %13, %3\n\t"
        "v_and_b32 %4, %13, %4\n\t"
        "v_sub_u32 %0, %14, %0\n\t"
        "v_sub_u32 %1, %14, %1\n\t"
        "v_sub_u32 %2, %14, %2\n\t"
        "v_sub_u32 %3, %14, %3\n\t"
        "v_sub_u32 %4, %14, %4"
        : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "=&v"(o4)
        // (the two constants in scalar registers: no 32-bit literal dwords in the instruction stream)
        : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(x4), "v"(wtop), "v"(wbot), "v"(rnd), "s"(0xfffffe00u), "s"(0x100u));
}

// a * b + c on the low 24 bits of a and b, ONE instruction (left to itself the compiler turns `c += __mul24(a, b)` chains into
// v_mul_i32_i24 + v_add3_u32 plus a sign-extension v_bfe per operand: 1.5 - 2x the instructions of the window loops)
__device__ __forceinline__ int mad24(int a, int b, int c)
{
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// 16 x 16 -> 32-bit multiply-add on selected halves: the x and y derivative of a pixel share one register (|Ix|, |Iy| <= 4080,
// |J - I| <= 8160 all fit 16 bits), which is what brings the kernel under 96 VGPRs
template <int HA, int HB>
__device__ __forceinline__ int mad16(uint32_t a, uint32_t b, int c)
{
    int r;
    if (HA == 0 && HB == 0) asm("v_mad_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    else if (HA == 0 && HB == 1) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,1,0,0]" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    else asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,1,0,0]" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The Newton iteration's version for five window columns c0..c0+4 of this lane's J row (16 bytes in T0..T3): byte pairs by
// v_perm, then as above with a per-column accumulator seed (rounding term minus the I sample):
//   d_i = ((J[c], J[c+1]) . wtop + below(...) . wbot + seed_i) >> 9
template <int C0>
__device__ __forceinline__ void jdiff5(uint32_t T0, uint32_t T1, uint32_t T2, uint32_t T3, uint32_t sel0, uint32_t sel1, uint32_t sel2, uint32_t sel3,
                                       uint32_t wtop, uint32_t wbot, int s0, int s1, int s2, int s3, int s4,
                                       int& d0, int& d1, int& d2, int& d3, int& d4)
{
    // column c reads bytes (c, c+1): dword q = c >> 2, byte o = c & 3; o == 3 takes byte 0 of the next dword
    uint32_t p0, p1, p2, p3, p4;
#define AV_TQ(c) (((c) >> 2) == 0 ? T0 : ((c) >> 2) == 1 ? T1 : ((c) >> 2) == 2 ? T2 : T3)
#define AV_TN(c) (((c) >> 2) == 0 ? T1 : ((c) >> 2) == 1 ? T2 : T3)         /* never needed for c >> 2 == 3 (bytes 12..15 only) */
#define AV_SL(c) (((c) & 3) == 0 ? sel0 : ((c) & 3) == 1 ? sel1 : ((c) & 3) == 2 ? sel2 : sel3)
    asm("v_perm_b32 %5, %10, %11, %20\n\t"
        "v_perm_b32 %6, %12, %13, %21\n\t"
        "v_perm_b32 %7, %14, %15, %22\n\t"
        "v_perm_b32 %8, %16, %17, %23\n\t"
        "v_perm_b32 %9, %18, %19, %24\n\t"
        "v_dot2_i32_i16 %0, %5, %25, %27\n\t"
        "v_dot2_i32_i16 %1, %6, %25, %28\n\t"
        "v_dot2_i32_i16 %2, %7, %25, %29\n\t"
        "v_dot2_i32_i16 %3, %8, %25, %30\n\t"
        "v_dot2_i32_i16 %4, %9, %25, %31\n\t"
        "v_dot2c_i32_i16_dpp %0, %5, %26 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %1, %6, %26 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %2, %7, %26 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %3, %8, %26 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_dot2c_i32_i16_dpp %4, %9, %26 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_ashrrev_i32 %0, 9, %0\n\t"
        "v_ashrrev_i32 %1, 9, %1\n\t"
        "v_ashrrev_i32 %2, 9, %2\n\t"
        "v_ashrrev_i32 %3, 9, %3\n\t"
        "v_ashrrev_i32 %4, 9, %4"
        : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&v"(d4), "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(p4)
        : "v"(AV_TN(C0)), "v"(AV_TQ(C0)), "v"(AV_TN(C0 + 1)), "v"(AV_TQ(C0 + 1)), "v"(AV_TN(C0 + 2)), "v"(AV_TQ(C0 + 2)),
          "v"(AV_TN(C0 + 3)), "v"(AV_TQ(C0 + 3)), "v"(AV_TN(C0 + 4)), "v"(AV_TQ(C0 + 4)),
          "s"(AV_SL(C0)), "s"(AV_SL(C0 + 1)), "s"(AV_SL(C0 + 2)), "s"(AV_SL(C0 + 3)), "s"(AV_SL(C0 + 4)),
          "v"(wtop), "v"(wbot), "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4));
#undef AV_TQ
#undef AV_TN
#undef AV_SL
}

// This lane's row of the I patch and of the two Scharr derivative patches from staged rows r .. r+2 of the window's 18 x 18-byte
// neighbourhood (load_row(t, B): the five dwords of staged row r + t; byte 0 of B[0] = window column -1, and B[4] holds the row's bytes
// 14 .. 17: the last two are the ones wanted), and the lane's share of the normal-equation sums.  lane_on: all ones in lanes 0 .. 14,
// zero in lane 15.
template <int WIN, typename LoadRow>
__device__ __forceinline__ void lk_patch_rows(LoadRow load_row, uint32_t wtop, uint32_t wbot, uint32_t lane_on, int ipx, int ipy, int w, int h, int r,
                                              int (&iv)[WIN], uint32_t (&ixx)[(WIN + 1) / 2], uint32_t (&iyy)[(WIN + 1) / 2], int& a11, int& a12, int& a22)
{
    constexpr int W_BITS = 14;
    a11 = 0; a12 = 0; a22 = 0;
    // staged byte index of window column c is c+1.  E[t][k] = (byte 2k | byte 2k+1 << 16) of staged row r+t; the window
    // pair (c, c+1) of the centre row is O1[k] = (byte 2k+1 | byte 2k+2 << 16) for c = 2k and E[1][k+1] for c = 2k+1.
    uint32_t E[3][9];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        uint32_t B[5];
        load_row(t, B);
#pragma unroll
        for (int k = 0; k < 9; ++k) {                // bytes 2k, 2k+1: of dword k >> 1 for k < 8; bytes 16, 17 are bytes 2, 3 of B[4]
            const int b0 = k < 8 ? 2 * k : 2;
            E[t][k] = __builtin_amdgcn_perm(0, B[k >> 1], 0x0C000C00u | (uint32_t)(b0 & 3) | ((uint32_t)((b0 & 3) + 1) << 16));
        }
    }
    // (hi half of x | lo half of y << 16): the pair one column to the right of x, given y = the next pair
    auto mid = [](uint32_t x, uint32_t y) -> uint32_t { return __builtin_amdgcn_perm(y, x, 0x05040302u); };
    // pixel pairs (c, c+1) of the centre row, c = 0..14
    uint32_t px[WIN];
#pragma unroll
    for (int k = 0; k < 8; ++k) px[2 * k] = mid(E[1][k], E[1][k + 1]);
#pragma unroll
    for (int k = 0; k < 7; ++k) px[2 * k + 1] = E[1][k + 1];
    // Scharr on the even window columns (pairs c = 2k, 2k+1); the odd-aligned pairs are byte permutes of those:
    //   gx[c] = t0[s+1] - t0[s-1],  gy[c] = (t1[s+1] + t1[s-1]) * 3 + t1[s] * 10,  s = c+1,
    //   t0 = (row above + row below) * 3 + row * 10,  t1 = row below - row above
    // Both are built TIMES 4 (deriv5 takes the high half of its accumulator instead of shifting it), inside the constants they are
    // multiplied by anyway: 4 t0 = (above + below) * 12 + row * 40 <= 16 x 255 x 4 = 16,320 < 2^16 as the unsigned half it is computed
    // in, 4 gx = 4 t0[s+1] - 4 t0[s-1] and 4 gy = (t1[s+1] + t1[s-1]) * 12 + t1[s] * 40 lie in [-16,320, 16,320], inside the signed
    // 16-bit range: the packed arithmetic is modulo 2^16, so each half holds the two's-complement form of exactly that value.
    uint32_t gxp[WIN + 1], gyp[WIN + 1];
    {
        uint32_t t0E[9], t1E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            t0E[k] = pk_add(pk_mul(pk_add(E[0][k], E[2][k]), 12), pk_mul(E[1][k], 40));
            t1E[k] = pk_sub(E[2][k], E[0][k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {                 // window columns (2k, 2k+1): centres O[k], left E[k], right E[k+1]
            gxp[2 * k] = pk_sub(t0E[k + 1], t0E[k]);
            gyp[2 * k] = pk_add(pk_mul(pk_add(t1E[k + 1], t1E[k]), 12), pk_mul(mid(t1E[k], t1E[k + 1]), 40));
        }
    }
    // the derivative image is zero outside the image: only windows at the border pay for the masks
    // 0 <= ipx && ipx + WIN < w as ONE unsigned compare per axis: a negative index is above 2^31 as unsigned and any limit below it; a level
    // no wider than the window has the limit 0, which nothing is below (the limits are wave-uniform: scalar)
    const bool inside = (unsigned)ipx < (unsigned)max(w - WIN, 0) && (unsigned)ipy < (unsigned)max(h - WIN, 0);
    if (__builtin_amdgcn_ballot_w64(!inside) != 0) {
        // the masks are built from an opaque copy of ipx made INSIDE the block: without it the compiler hoists the 60-odd
        // compares / selects of the mask values onto the common path and keeps only the 16 ANDs in here
        int ipx_o = ipx;
        asm volatile("" : "+v"(ipx_o));
        const bool rowin = (unsigned)(ipy + r) < (unsigned)h;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t m0 = (rowin && (unsigned)(ipx_o + 2 * k) < (unsigned)w) ? 0xFFFFu : 0u;
            const uint32_t m1 = (rowin && (unsigned)(ipx_o + 2 * k + 1) < (unsigned)w) ? 0xFFFF0000u : 0u;
            gxp[2 * k] &= (m0 | m1); gyp[2 * k] &= (m0 | m1);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        gxp[2 * k + 1] = mid(gxp[2 * k], gxp[2 * k + 2]);
        gyp[2 * k + 1] = mid(gyp[2 * k], gyp[2 * k + 2]);
    }
    // Lane 15 (row 15 feeds only the interpolation of row 14, through the DPP operand of the lane above, which is the pixel pair and not
    // a weight) interpolates its derivatives with zero weights and a zero rounding term: its Ix, Iy pairs are zero, and so are its shares
    // of a11 / a12 / a22 here and of b1 / b2 in every Newton iteration, with no select there.  The zeroing is an AND with the lane
    // mask (x & ~0 = x, x & 0 = 0: what the three selects did, at full rate and without VCC).
    const int rnd_i = 1 << (W_BITS - 6);
    const uint32_t wtop_d = wtop & lane_on, wbot_d = wbot & lane_on;
    const int rnd_d = (int)((4u << (W_BITS - 1)) & lane_on);                // 4 * 2^13: the derivatives come in times 4 (deriv5)
    // The derivative patches are kept as PAIRS of adjacent columns, (Ix[2p] | Ix[2p+1] << 16) and the same for Iy (|Ix|, |Iy| <= 4080;
    // the 16th column is zero): every window sum is then a chain of v_dot2_i32_i16 -- two columns per instruction -- instead of one
    // v_mad_i32_i16 per column (24 instead of 45 here, 16 + 7 pair packs instead of 30 in every Newton iteration; the same exact
    // integers, whatever the grouping).
#pragma unroll
    for (int c = 0; c < WIN; c += 5)
        bilin5_seed(px[c], px[c + 1], px[c + 2], px[c + 3], px[c + 4], wtop, wbot, rnd_i, iv[c], iv[c + 1], iv[c + 2], iv[c + 3], iv[c + 4]);
    uint32_t cx = 0, cy = 0;
    deriv5<0>(gxp, gyp, wtop_d, wbot_d, rnd_d, ixx, iyy, cx, cy);
    deriv5<1>(gxp, gyp, wtop_d, wbot_d, rnd_d, ixx, iyy, cx, cy);
    deriv5<2>(gxp, gyp, wtop_d, wbot_d, rnd_d, ixx, iyy, cx, cy);
#pragma unroll
    for (int p = 0; p < (WIN + 1) / 2; ++p) {
        a11 = dot2(ixx[p], ixx[p], a11);
        a12 = dot2(ixx[p], iyy[p], a12);
        a22 = dot2(iyy[p], iyy[p], a22);
    }
}

// PTS: points per workgroup (16 = four wavefronts, 4 = one).  The wavefronts of a workgroup share nothing -- every point has its own
// LDS tile and there is no barrier -- so the workgroup size is purely a placement matter: see lk_track_g16_kernel.
template <int WIN, int OCC, bool PROF = false, int PTS = 16>
__device__ __forceinline__ bool lk_track_g16_body(const LKArgs& a)
{
    static_assert(WIN == 15, "lane map is built for the reference's 15x15 window");
    __shared__ uint32_t tile_all[PTS][TILE_DWORDS];
    // phase stamps (PROF only): cycles since the previous stamp are booked on the phase that just ended
    unsigned pt[LKP_N] = {0, 0, 0, 0, 0}, plast = 0;             // 32-bit: a wavefront lives ~10^5 cycles
    unsigned pn_iter = 0, pn_restage = 0, pn_level = 0;
    unsigned long long rt0 = 0;
    if (PROF) { rt0 = __builtin_amdgcn_s_memrealtime(); plast = (unsigned)__builtin_readcyclecounter(); }
#define LK_STAMP(ph) do { if (PROF) { const unsigned t_ = (unsigned)__builtin_readcyclecounter(); pt[ph] += t_ - plast; plast = t_; } } while (0)
    const int g = threadIdx.x >> 4;                 // point slot of this 16-lane group inside the workgroup
    const int r = threadIdx.x & 15;                 // window row owned by this lane (row 15 only feeds row 14)
    uint32_t* tile = tile_all[g];
    // all ones in the lanes that own a window row, zero in lane 15 (lk_patch_rows); opaque, or the compiler turns the ANDs back into selects
    // (not volatile: a volatile asm counts as a store to anything, and the wave-uniform loads below it would leave the scalar unit)
    uint32_t lane_on = r < WIN ? ~0u : 0u;
    asm("" : "+v"(lane_on));
    // Workgroup -> (point set, block of 16 points).  The dispatcher deals workgroups round-robin over the 8 XCDs (linear id mod 8,
    // MI355X_MICROARCH.md "Workgroup dispatch"), and each XCD has its own L2: with the plain (block, set) grid the ~19 workgroups of
    // one stream land on all eight XCDs and every L2 fetches that stream's two pyramids (profiles/r03/fetch_calib.json, rows32: a
    // window gather in image order reads 2.6x the image bytes).  The 1-D launch keeps a set's workgroups on ONE XCD: id L ->
    // XCD label L & 7, set = label + 8 * ((L >> 3) / gx), block = (L >> 3) % gx.  Placement only: any mapping is correct.
    const int L = blockIdx.x, wg = L >> 3, s = (L & 7) + 8 * (wg / a.gx), bx = wg % a.gx;
    if (s >= a.n_set) return false;
    const int slot = bx * PTS + g;
    const int sI = a.mapI ? a.mapI[s] : s, sJ = a.mapJ ? a.mapJ[s] : s;      // storage entries of the two images (scalar loads)
    if (sI < 0 || sJ < 0) return false;
    // Without an index list the point of a slot is known before the set's count is: its loads are issued ahead of the count's (one
    // dependent memory round trip less at the head of every wavefront; a slot past the count reads a valid entry and leaves)
    const bool direct = a.index == nullptr && slot < a.cap;
    float prevx0 = 0.f, prevy0 = 0.f, curx = 0.f, cury = 0.f;
    if (direct) {
        const size_t p0 = (size_t)s * a.cap + slot;
        prevx0 = a.prev[2 * p0]; prevy0 = a.prev[2 * p0 + 1]; curx = a.next[2 * p0]; cury = a.next[2 * p0 + 1];
    }
    const int n = min(a.count[s], a.cap);
    if (slot >= n) return false;                    // uniform per 16-lane group
    const int pidx = a.index ? a.index[(size_t)s * a.cap + slot] : slot;

    const uint8_t* PI = a.pyrI + sI * a.stream_stride;
    const uint8_t* PJ = a.pyrJ + sJ * a.stream_stride;
    const size_t pi = (size_t)s * a.cap + pidx;
    if (!direct) { prevx0 = a.prev[2 * pi]; prevy0 = a.prev[2 * pi + 1]; curx = a.next[2 * pi]; cury = a.next[2 * pi + 1]; }
    const float halfWin = (WIN - 1) * 0.5f;
    bool ok = true;
    // byte-pair selectors of v_perm: (byte o, byte o+1) zero-extended into the two 16-bit halves; o+1 == 4 = byte 0 of the next dword
    const uint32_t sel0 = 0x0C010C00u, sel1 = 0x0C020C01u, sel2 = 0x0C030C02u, sel3 = 0x0C040C03u;

    for (int level = a.g.levels - 1; level >= 0; --level) {
        const int w = a.g.w[level], h = a.g.h[level], pitch = a.g.pitch[level];
        const int col_lo = -AV_PYR_BORDER, col_hi = pitch - AV_PYR_BORDER;
        const float scale = __int_as_float((127 - level) << 23);       // 2^-level (written as 1. / (1 << level) it is an fp64 division per level)
        float pvx = prevx0 * scale, pvy = prevy0 * scale;
        // the guess is scaled by 2^-level at the top level and doubled below it: ONE wave-uniform factor, chosen on the scalar unit (the
        // asm keeps it in a scalar register: left alone the compiler selects it per lane, through VCC); the products are the same
        uint32_t gmul = level == a.g.levels - 1 ? (uint32_t)(127 - level) << 23 : 0x40000000u;
        asm("" : "+s"(gmul));
        curx = curx * __uint_as_float(gmul); cury = cury * __uint_as_float(gmul);
        pvx -= halfWin; pvy -= halfWin;
        // The floor stays a float for the fraction: an index that passes the bounds test is below 2^12 in magnitude, (float)(int)floor
        // is the floor itself.  The bounds test is -WIN <= i < size as ONE unsigned compare per axis on the index biased by WIN (an
        // index beyond int range converts saturated, and INT_MAX + WIN / INT_MIN + WIN both land above any size + WIN as unsigned).
        const float fpx = floorf(pvx), fpy = floorf(pvy);
        const int ipx = (int)fpx, ipy = (int)fpy;
        const unsigned wlim = (unsigned)(w + WIN), hlim = (unsigned)(h + WIN);
        if ((unsigned)ipx + WIN >= wlim || (unsigned)ipy + WIN >= hlim) {
            if (level == 0) ok = false;
            continue;
        }
        uint32_t wtop, wbot;
        lk_weights(pvx - fpx, pvy - fpy, wtop, wbot);

        // ---- stage the 18 x 18-byte neighbourhood of the I window: rows ipy-1 .., bytes ipx-1 .. ipx+16 of each as five dwords
        //      read at their (unaligned) byte address, so that every staged row starts at window column -1.  All bytes lie inside
        //      the padded pyramid row: ipx - 1 >= -16 and ipx + 16 <= w + 15 (the 5th dword is fetched 2 bytes early and stored as it
        //      is: it holds bytes 14 .. 17 of the row, lk_patch_rows takes its upper two).
        // Lane map of both staging loops: lane r handles dword (r & 7) of rows 2k + (r >> 3): the global address is a
        // wave-uniform base (padded level origin + 2k rows, scalar) plus ONE per-lane 32-bit offset, the LDS address one
        // per-lane base plus an immediate -- no per-load index arithmetic on the vector unit.  lk_row_base makes the row base opaque
        // in a scalar register pair: handed the sum, the compiler re-associates it into (origin + lane offset) + row step, a chain of
        // 64-bit vector additions per load.  The per-lane offsets are non-negative (bounds tests above, 16-pixel frame), below 2^31.
        const int sub = r >> 3, dwl = r & 7;
        const uint32_t tofs = (uint32_t)(sub * (TPITCH / 4) + dwl);
        LK_STAMP(LKP_HEAD);
        if (PROF) ++pn_level;
        wave_lds_sync();
        {
            // source of this level's I rows: the padded pyramid level (origin at row -16, column -16, frame included) or, for
            // level 0 in place, the caller's image (origin at pixel (0, 0), no frame: windows over the border take the slow path)
            const bool extI = level == 0 && a.imgI != nullptr;                      // wave-uniform
            const uint8_t* L0 = extI ? a.imgI + (size_t)sI * (size_t)a.imgI_stride : PI + a.g.off[level];
            const int pI = extI ? w : pitch, bI = extI ? 0 : AV_PYR_BORDER;
            const bool act = dwl < 5;                                    // 5 of the 8 slots of a row carry a dword
            if (!extI || (ipx >= 1 && ipx + 16 < w && ipy >= 1 && ipy + 16 < h)) {
                const uint32_t loff = (uint32_t)(__mul24(ipy - 1 + sub + bI, pI) + (ipx - 1 + bI) + (dwl < 4 ? 4 * dwl : 14));
                uint32_t sv[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {                               // 18 rows
                    sv[k] = 0;
                    if (act) sv[k] = lk_load_u32(lk_row_base(L0, 2 * k, pI), loff);
                }
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    if (act) tile[tofs + 2 * k * (TPITCH / 4)] = sv[k];
            } else if (act) {
                // the window reaches over the image border: the bytes the padded level's BORDER_REFLECT_101 frame would hold (the fifth
                // dword: row bytes 16, 17 in ITS bytes 2, 3, where the fast path has them; its lower half is never read)
                const int xb = ipx - 1 + (dwl < 4 ? 4 * dwl : 16), nbyte = dwl < 4 ? 4 : 2, bsh = dwl < 4 ? 0 : 16;
#pragma unroll 1
                for (int k = 0; k < 9; ++k) {
                    const uint8_t* row = L0 + (size_t)av_reflect101(ipy - 1 + sub + 2 * k, h) * (size_t)w;
                    uint32_t v = 0;
#pragma unroll 1
                    for (int bb = 0; bb < nbyte; ++bb) v |= (uint32_t)row[av_reflect101(xb + bb, w)] << (8 * bb + bsh);
                    tile[tofs + 2 * k * (TPITCH / 4)] = v;
                }
            }
        }
        wave_lds_sync();
        LK_STAMP(LKP_ISTAGE);

        // ---- this lane's row of the I patch and of the Scharr patches: staged rows r..r+2, 18 bytes of each -------------
        int iv[WIN];
        uint32_t ixx[(WIN + 1) / 2], iyy[(WIN + 1) / 2];      // (Ix[2p] | Ix[2p+1] << 16), the same for Iy: pairs of window columns
        int a11, a12, a22;
        lk_patch_rows<WIN>([&](int t, uint32_t (&B)[5]) {
                               const uint32_t* rowp = tile + __mul24(r + t, TPITCH / 4);
#pragma unroll
                               for (int k = 0; k < 5; ++k) B[k] = rowp[k];
                           }, wtop, wbot, lane_on, ipx, ipy, w, h, r, iv, ixx, iyy, a11, a12, a22);
        const float A11 = row_sum_sq_scaled(a11);
        const float A12 = row_sum16_scaled(a12);
        const float A22 = row_sum_sq_scaled(a22);
        float D = A11 * A22 - A12 * A12;
        // minEig = eigNum / (2 WIN^2) is only ever compared with the threshold: fl(eigNum / 450) < min_eig_up <=> eigNum < min_eig_num
        // (av_lk_quotient_bound, computed by lk_fill_args: the correctly rounded division by a positive constant is monotone).  eigNum is
        // finite here (|A| < 2^12), so neither side meets a NaN of its own; a NaN threshold gives a NaN bound, and both forms are false.
        const float eigNum = A22 + A11 - lk_sqrt_ranged((A11 - A22) * (A11 - A22) + 4.f * A12 * A12);
        if (eigNum < a.min_eig_num || D < 1.1920928955078125e-7f) {
            if (level == 0) ok = false;
            continue;
        }
        D = 1.f / D;

        // ---- Newton iterations.  ONE exit, at the bottom, and every loop-carried value (wx, wy, their floors, the previous step, the
        //      tile origin) updated in place: a point that is done simply drops out of the loop's execution mask with its state where the
        //      step left it, and what distinguished the former four exits is settled once, after the loop:
        //        converged / oscillating / trip limit ("soft"): the position stands, status untouched; oscillation takes half the last
        //        step back; out of the image before the next trip (tested where that trip's floor is computed, at the bottom, and for
        //        the first trip ahead of the loop): level 0 fails.
        //      (With a `break` per case the compiler carried a copy of every state register per exit around the loop: 14 register moves
        //      and ~45 execution-mask instructions per trip.)
        float wx = curx - halfWin, wy = cury - halfWin;
        if (a.max_iter <= 0) continue;                         // wave-uniform: no trip, no bounds test
        float fx = floorf(wx), fy = floorf(wy);
        int inx = (int)fx, iny = (int)fy;
        if ((unsigned)inx + WIN >= wlim || (unsigned)iny + WIN >= hlim) {
            if (level == 0) ok = false;
            continue;
        }
        float pdx = 0.f, pdy = 0.f;
        int X0 = -(1 << 30), Y0 = 0;                           // no tile yet: inx - X0 is beyond any drift, the first trip stages
        bool osc = false, soft = false;
        LK_STAMP(LKP_SETUP);
        for (int j = 0;;) {
            if (PROF) ++pn_iter;
            int dx0 = inx - X0, dy0 = iny - Y0;
            if ((unsigned)dx0 > (unsigned)(TILE_COLS - 17) || (unsigned)dy0 > (unsigned)(TILE_ROWS - 16)) {
                X0 = min(max((inx - 6) & ~3, col_lo), col_hi - TILE_COLS);
                Y0 = min(max(iny - 4, -AV_PYR_BORDER), h + AV_PYR_BORDER - TILE_ROWS);
                LK_STAMP(LKP_ITER);
                if (PROF) ++pn_restage;
                wave_lds_sync();
                {
                    const bool extJ = level == 0 && a.imgJ != nullptr;              // wave-uniform
                    const uint8_t* LJ0 = extJ ? a.imgJ + (size_t)sJ * (size_t)a.imgJ_stride : PJ + a.g.off[level];
                    const int pJ = extJ ? w : pitch, bJ = extJ ? 0 : AV_PYR_BORDER;
                    if (!extJ || (X0 >= 0 && X0 + TILE_COLS <= w && Y0 >= 0 && Y0 + TILE_ROWS <= h)) {
                        const uint32_t joff = (uint32_t)(__mul24(Y0 + sub + bJ, pJ) + X0 + bJ + 4 * dwl);
                        uint32_t sv[TILE_ROWS / 2];
#pragma unroll
                        for (int k = 0; k < TILE_ROWS / 2; ++k)        // 24 rows x 8 dwords
                            sv[k] = lk_load_u32(lk_row_base(LJ0, 2 * k, pJ), joff);
#pragma unroll
                        for (int k = 0; k < TILE_ROWS / 2; ++k) tile[tofs + 2 * k * (TPITCH / 4)] = sv[k];
                    } else {
#pragma unroll 1
                        for (int k = 0; k < TILE_ROWS / 2; ++k) {
                            const uint8_t* row = LJ0 + (size_t)av_reflect101(Y0 + sub + 2 * k, h) * (size_t)w;
                            uint32_t v = 0;
#pragma unroll 1
                            for (int bb = 0; bb < 4; ++bb) v |= (uint32_t)row[av_reflect101(X0 + 4 * dwl + bb, w)] << (8 * bb);
                            tile[tofs + 2 * k * (TPITCH / 4)] = v;
                        }
                    }
                }
                wave_lds_sync();
                LK_STAMP(LKP_JSTAGE);
                dx0 = inx - X0; dy0 = iny - Y0;
            }
            lk_weights(wx - fx, wy - fy, wtop, wbot);

            // this lane's J row (dy0 + r): 16 pixels starting at byte dx0 -> 5 aligned dwords -> 4 byte-aligned dwords
            const int sh = dx0 & 3;
            const uint32_t* rp = tile + __mul24(dy0 + r, TPITCH / 4) + (dx0 >> 2);
            uint32_t d0 = rp[0], d1 = rp[1], d2 = rp[2], d3 = rp[3], d4 = rp[4];
            const uint32_t T0 = __builtin_amdgcn_alignbyte(d1, d0, sh), T1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
            const uint32_t T2 = __builtin_amdgcn_alignbyte(d3, d2, sh), T3 = __builtin_amdgcn_alignbyte(d4, d3, sh);
            int df[WIN];
            jdiff5<0>(T0, T1, T2, T3, sel0, sel1, sel2, sel3, wtop, wbot, iv[0], iv[1], iv[2], iv[3], iv[4], df[0], df[1], df[2], df[3], df[4]);
            jdiff5<5>(T0, T1, T2, T3, sel0, sel1, sel2, sel3, wtop, wbot, iv[5], iv[6], iv[7], iv[8], iv[9], df[5], df[6], df[7], df[8], df[9]);
            jdiff5<10>(T0, T1, T2, T3, sel0, sel1, sel2, sel3, wtop, wbot, iv[10], iv[11], iv[12], iv[13], iv[14], df[10], df[11], df[12], df[13], df[14]);
            int b1 = 0, b2 = 0;
#pragma unroll
            for (int p = 0; p < (WIN + 1) / 2; ++p) {
                // (|J - I| <= 8160 fits 16 bits; the high half of the last pair multiplies the zero 16th column: df[14] goes in as it is)
                const uint32_t dp = 2 * p + 1 < WIN ? __builtin_amdgcn_perm((uint32_t)df[2 * p + 1 < WIN ? 2 * p + 1 : 0], (uint32_t)df[2 * p], 0x05040100u) : (uint32_t)df[2 * p];
                b1 = dot2(dp, ixx[p], b1);
                b2 = dot2(dp, iyy[p], b2);
            }
            const float fb1 = row_sum16_scaled(b1);
            const float fb2 = row_sum16_scaled(b2);
            const float dx = (A12 * fb2 - A22 * fb1) * D;
            const float dy = (A12 * fb1 - A11 * fb2) * D;
            wx += dx; wy += dy;
            // delta.ddot(delta) <= eps^2 is an fp64 test in OpenCV.  e32 lies within 2^-22 (relative) of the exact dx^2 + dy^2, so outside
            // (eps_lo, eps_hi) the float compare decides the same way; inside (once in ~10^5 iterations) the fp64 form does.
            const float e32 = __builtin_fmaf(dx, dx, dy * dy);
            bool conv = e32 <= a.eps_lo;
            if (__builtin_amdgcn_ballot_w64(e32 > a.eps_lo && e32 < a.eps_hi) != 0) {
                asm volatile("; fp64 step test");          // keeps the block a branch (if-converted, its fp64 instructions ran every iteration)
                conv = (double)dx * dx + (double)dy * dy <= a.eps2;
            }
            // |x| < 0.01 (double) for a float x <=> |x| <= 0.01f: 0.01f = 0.00999999977... < 0.01 < the next float up
            osc = !conv && j > 0 && fabsf(dx + pdx) <= 0.01f && fabsf(dy + pdy) <= 0.01f;
            pdx = dx; pdy = dy;
            ++j;
            soft = conv || osc || j >= a.max_iter;
            // the next trip's floors and its bounds test
            fx = floorf(wx); fy = floorf(wy);
            inx = (int)fx; iny = (int)fy;
            if (soft || (unsigned)inx + WIN >= wlim || (unsigned)iny + WIN >= hlim) break;
        }
        if (!soft && level == 0) ok = false;
        curx = wx + halfWin; cury = wy + halfWin;
        if (osc) { curx -= pdx * 0.5f; cury -= pdy * 0.5f; }
        LK_STAMP(LKP_ITER);
    }
    if (r == 0) {
        a.next[2 * pi] = curx;
        a.next[2 * pi + 1] = cury;
        a.status[pi] = ok ? 1 : 0;
    }
    if (PROF) {
        LK_STAMP(LKP_HEAD);
        // one record per wavefront: its first lane books the wave's clock; iteration / level counts are the maxima over its points
        // (what the wave executed); every point leader books its own counts for the per-point means
        unsigned wi = pn_iter, wr = pn_restage, wl = pn_level;
#pragma unroll
        for (int d = 16; d < 64; d <<= 1) { wi = max(wi, (unsigned)__shfl_xor((int)wi, d, 64)); wr = max(wr, (unsigned)__shfl_xor((int)wr, d, 64)); wl = max(wl, (unsigned)__shfl_xor((int)wl, d, 64)); }
        // (every wavefront stamps; one workgroup in 61 books: 10^7 same-address atomics per launch made the profiled kernel 9x slower)
        const bool book = blockIdx.x % 61 == 0;
        if (book && (threadIdx.x & 63) == 0) {
            for (int k = 0; k < LKP_N; ++k) atomicAdd(a.prof + k, (unsigned long long)pt[k]);
            atomicAdd(a.prof + LKP_WAVES, 1ull);
            atomicAdd(a.prof + LKP_SLOTS + 3, __builtin_amdgcn_s_memrealtime() - rt0);      // the same span on the constant 100 MHz clock
            atomicAdd(a.prof + LKP_ITERS, (unsigned long long)wi);
            atomicAdd(a.prof + LKP_RESTAGES, (unsigned long long)wr);
            atomicAdd(a.prof + LKP_LEVELS, (unsigned long long)wl);
        }
        if (book && r == 0) { atomicAdd(a.prof + LKP_SLOTS, 1ull); atomicAdd(a.prof + LKP_SLOTS + 1, (unsigned long long)pn_iter); atomicAdd(a.prof + LKP_SLOTS + 2, (unsigned long long)pn_restage); }
    }
#undef LK_STAMP
    return true;
}

// (Round 5, archived -- profiles/r05/lk_dma_experiment.md, code in git 741c321: both stagings by LDS-DMA, the J tile requested before
//  the patch set-up and the next level's I neighbourhood before the iterations.  Bit-exact, the wavefront's life 13 % shorter, the
//  launch 1.7 % LONGER (0.955 vs 0.939 ms): at five wavefronts per SIMD the other four already fill the slots a staging wavefront
//  leaves; the kernel is bound by VALU issue.)
// 96 VGPRs: 5 waves per SIMD without spills (the kernel is VALU-issue bound: 4 -> 5 waves bought 1 %, a 6-wave build with
// 11 spilled values lost 5 %).
// One wavefront (four points) per workgroup: the wavefronts of this kernel share nothing, so the workgroup size is a placement matter
// only -- and it matters twice.  (1) A 256-thread workgroup holds its four slots until its SLOWEST wavefront is done (the points of a
// launch take 3 .. 30 Newton iterations); single wavefronts hand their slot back one by one: front-end alone 0.917 -> 0.862 ms per
// launch (211.1 -> 220.5 k frames/s).  (2) A 256-thread workgroup needs a free slot on all four SIMDs of a CU at once: beside the
// filter's single-wavefront tasks, each of which takes ONE slot on ONE SIMD, a CU with three free slots starts nothing -- every
// resident filter wavefront can keep a whole LK workgroup out: complete path 161.6 -> 168.9 k.  (profiles/r05/README.md)
template <int WIN> __global__ __launch_bounds__(64, 5) void lk_track_g16_kernel(LKArgs a) { lk_track_g16_body<WIN, 5, false, 4>(a); }
// (Two wavefronts per workgroup lie in between: front-end alone 218.3 k against 220.2 k, complete path 166.2 against 168.7 k.
//  profiles/r05/README.md)
// (Forward and backward pass of a stereo match as ONE launch -- the 16 lanes that tracked a point forward track it back, three launches
//  fewer per front-end step -- was built and measured in round 5: front-end alone 207.9 / 206.2 k against 206.1 / 206.8 k frames/s, one
//  stream 0.649 against 0.645 ms per frame: nothing, removed.  profiles/r05/README.md)
// (a four-wave build that leaves 128 register rows per SIMD to the filter's kernels: 146.7 k against 152.8 k frames/s, round 4)
// AV_LK_PROF=1: the same body, four wavefronts (16 points) per workgroup, with s_memtime stamps at the phase boundaries (I staging /
// patch set-up / J staging / Newton iterations), summed over the wavefronts of every launch and printed at exit
// (profiles/r05/lk_phase_stamps.txt).
template <int WIN> __global__ __launch_bounds__(256, 5) void lk_track_g16_prof_kernel(LKArgs a) { lk_track_g16_body<WIN, 5, true>(a); }

static unsigned long long* g_lk_prof = nullptr;
static void lk_prof_report()
{
    if (!g_lk_prof) return;
    unsigned long long h[LKP_SLOTS + 4];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, g_lk_prof, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
    static const char* names[LKP_N] = {"head+tail", "I staging", "set-up", "J staging", "iterations"};
    double tot = 0;
    for (int k = 0; k < LKP_N; ++k) tot += (double)h[k];
    const double nw = (double)h[LKP_WAVES];
    fprintf(stderr, "AV_LK_PROF: %.0f wavefronts booked (one workgroup in 61), %.0f s_memtime ticks per wavefront = %.1f us on the 100 MHz clock: %.0f ticks per us\n",
            nw, tot / nw, (double)h[LKP_SLOTS + 3] / nw / 100., tot / ((double)h[LKP_SLOTS + 3] / 100.));
    for (int k = 0; k < LKP_N; ++k) fprintf(stderr, "AV_LK_PROF:   %-10s %8.0f ticks per wavefront  %5.1f %%\n", names[k], (double)h[k] / nw, 100. * (double)h[k] / tot);
    fprintf(stderr, "AV_LK_PROF: per wavefront (max over its 4 points): %.2f levels, %.2f iterations, %.2f J stagings; per point: %.2f iterations, %.2f J stagings\n",
            (double)h[LKP_LEVELS] / nw, (double)h[LKP_ITERS] / nw, (double)h[LKP_RESTAGES] / nw,
            (double)h[LKP_SLOTS + 1] / (double)h[LKP_SLOTS], (double)h[LKP_SLOTS + 2] / (double)h[LKP_SLOTS]);
}


// =================================================================================================
// Any other window (config.win_size, src/config.py:35-38; 3 <= win <= 31): one WAVEFRONT per point, the win x win window
// pixels dealt over the 64 lanes (at most 16 per lane, the I / Ix / Iy values of a lane's pixels in registers), the same
// arithmetic in the same order as the 16-lane kernel and the oracle: W_BITS = 14 bilinear weights, Scharr derivatives of the
// first image taken at integer pixels (BORDER_REFLECT_101 neighbours inside the image, zero outside), exact integer window
// sums (int64 per lane, butterfly over the wavefront) rounded once, float Newton steps.  Pixels are read straight from the
// padded pyramid level (or the caller's image for level 0) through the cache -- this is the general path, not the fast one.
// =================================================================================================
constexpr int LKG_MAX_WIN = 31, LKG_PER_LANE = (LKG_MAX_WIN * LKG_MAX_WIN + 63) / 64;

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct LKLevel { const uint8_t* base; int pitch, w, h; };      // base = address of pixel (0, 0)
__device__ __forceinline__ int lkg_pix(const LKLevel& L, int x, int y) { return L.base[(size_t)av_reflect101_any(y, L.h) * L.pitch + av_reflect101_any(x, L.w)]; }

__global__ __launch_bounds__(256) void lk_track_generic_kernel(LKArgs a, int WIN)
{
    constexpr int W_BITS = 14;
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.y, slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int sI = a.mapI ? a.mapI[s] : s, sJ = a.mapJ ? a.mapJ[s] : s;
    if (sI < 0 || sJ < 0) return;
    const int n = min(a.count[s], a.cap);
    if (slot >= n) return;                                   // wave-uniform
    const int pidx = a.index ? a.index[(size_t)s * a.cap + slot] : slot;
    const size_t pi = (size_t)s * a.cap + pidx;
    const float prevx0 = a.prev[2 * pi], prevy0 = a.prev[2 * pi + 1];
    float curx = a.next[2 * pi], cury = a.next[2 * pi + 1];
    const float halfWin = (WIN - 1) * 0.5f;
    const int win2 = WIN * WIN;
    const double FLT_SCALE_D = 1.0 / (1 << 20);
    bool ok = true;
    for (int level = a.g.levels - 1; level >= 0; --level) {
        const int w = a.g.w[level], h = a.g.h[level];
        LKLevel LI, LJ;
        {
            const bool extI = level == 0 && a.imgI != nullptr, extJ = level == 0 && a.imgJ != nullptr;
            const int pitch = a.g.pitch[level];
            LI.base = extI ? a.imgI + (size_t)sI * (size_t)a.imgI_stride : a.pyrI + sI * a.stream_stride + a.g.off[level] + (size_t)AV_PYR_BORDER * pitch + AV_PYR_BORDER;
            LI.pitch = extI ? w : pitch; LI.w = w; LI.h = h;
            LJ.base = extJ ? a.imgJ + (size_t)sJ * (size_t)a.imgJ_stride : a.pyrJ + sJ * a.stream_stride + a.g.off[level] + (size_t)AV_PYR_BORDER * pitch + AV_PYR_BORDER;
            LJ.pitch = extJ ? w : pitch; LJ.w = w; LJ.h = h;
        }
        const float scale = (float)(1. / (1 << level));
        float pvx = prevx0 * scale, pvy = prevy0 * scale;
        if (level == a.g.levels - 1) { curx = curx * scale; cury = cury * scale; }
        else                         { curx = curx * 2.f;   cury = cury * 2.f; }
        pvx -= halfWin; pvy -= halfWin;
        const int ipx = (int)floorf(pvx), ipy = (int)floorf(pvy);
        if (ipx < -WIN || ipx >= w || ipy < -WIN || ipy >= h) {
            if (level == 0) ok = false;
            continue;
        }
        float fa = pvx - ipx, fb = pvy - ipy;
        int iw00 = __float2int_rn((1.f - fa) * (1.f - fb) * (1 << W_BITS));
        int iw01 = __float2int_rn(fa * (1.f - fb) * (1 << W_BITS));
        int iw10 = __float2int_rn((1.f - fa) * fb * (1 << W_BITS));
        int iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
        // ---- I patch and derivative patches of this lane's window pixels
        short iv[LKG_PER_LANE], ixv[LKG_PER_LANE], iyv[LKG_PER_LANE];
        long long sA11 = 0, sA12 = 0, sA22 = 0;
#pragma unroll
        for (int t = 0; t < LKG_PER_LANE; ++t) {
            const int idx = lane + 64 * t;
            iv[t] = 0; ixv[t] = 0; iyv[t] = 0;
            if (idx < win2) {
                const int y = idx / WIN, x = idx - y * WIN, X = ipx + x, Y = ipy + y;
                // 4 x 4 neighbourhood (X-1 .. X+2, Y-1 .. Y+2), reflected: the four bilinear taps and their Scharr stencils
                int P[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) P[r][c] = lkg_pix(LI, X - 1 + c, Y - 1 + r);
                const int ival = AV_DESCALE(P[1][1] * iw00 + P[1][2] * iw01 + P[2][1] * iw10 + P[2][2] * iw11, W_BITS - 5);
                // derivative at the integer pixel (X + cx, Y + cy), cx, cy in {0, 1}: zero outside the image (calc() pads the derivative
                // image with BORDER_CONSTANT), else Scharr over reflected neighbours.  The stencil of (X+cx, Y+cy) needs pixels
                // X+cx-1 .. X+cx+1: for cx = 1 that is X .. X+2, all inside P; reflection of a neighbour of an INSIDE pixel equals the
                // reflected read already taken (reflect101 is applied per coordinate).
                int dxv[2][2], dyv[2][2];
#pragma unroll
                for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                    for (int cx = 0; cx < 2; ++cx) {
                        const bool in = (unsigned)(X + cx) < (unsigned)w && (unsigned)(Y + cy) < (unsigned)h;
                        // t0(c) = (above + below) * 3 + centre * 10, t1(c) = below - above, at columns cx-1 .. cx+1 (P columns cx .. cx+2)
                        int t0[3], t1[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k) { t0[k] = (P[cy][cx + k] + P[cy + 2][cx + k]) * 3 + P[cy + 1][cx + k] * 10; t1[k] = P[cy + 2][cx + k] - P[cy][cx + k]; }
                        dxv[cy][cx] = in ? (int)(short)(t0[2] - t0[0]) : 0;
                        dyv[cy][cx] = in ? (int)(short)((t1[2] + t1[0]) * 3 + t1[1] * 10) : 0;
                    }
                const int ix = AV_DESCALE(dxv[0][0] * iw00 + dxv[0][1] * iw01 + dxv[1][0] * iw10 + dxv[1][1] * iw11, W_BITS);
                const int iy = AV_DESCALE(dyv[0][0] * iw00 + dyv[0][1] * iw01 + dyv[1][0] * iw10 + dyv[1][1] * iw11, W_BITS);
                iv[t] = (short)ival; ixv[t] = (short)ix; iyv[t] = (short)iy;
                sA11 += (long long)ixv[t] * ixv[t]; sA12 += (long long)ixv[t] * iyv[t]; sA22 += (long long)iyv[t] * iyv[t];
            }
        }
        const float A11 = (float)((double)wave_sum_i64(sA11) * FLT_SCALE_D);
        const float A12 = (float)((double)wave_sum_i64(sA12) * FLT_SCALE_D);
        const float A22 = (float)((double)wave_sum_i64(sA22) * FLT_SCALE_D);
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * WIN * WIN);
        if ((double)minEig < a.min_eig || D < 1.1920928955078125e-7f) {
            if (level == 0) ok = false;
            continue;
        }
        D = 1.f / D;
        float wx = curx - halfWin, wy = cury - halfWin;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_iter; ++j) {
            const int inx = (int)floorf(wx), iny = (int)floorf(wy);
            if (inx < -WIN || inx >= w || iny < -WIN || iny >= h) {
                if (level == 0) ok = false;
                break;
            }
            fa = wx - inx; fb = wy - iny;
            iw00 = __float2int_rn((1.f - fa) * (1.f - fb) * (1 << W_BITS));
            iw01 = __float2int_rn(fa * (1.f - fb) * (1 << W_BITS));
            iw10 = __float2int_rn((1.f - fa) * fb * (1 << W_BITS));
            iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
            long long sb1 = 0, sb2 = 0;
#pragma unroll
            for (int t = 0; t < LKG_PER_LANE; ++t) {
                const int idx = lane + 64 * t;
                if (idx < win2) {
                    const int y = idx / WIN, x = idx - y * WIN, X = inx + x, Y = iny + y;
                    const int diff = AV_DESCALE(lkg_pix(LJ, X, Y) * iw00 + lkg_pix(LJ, X + 1, Y) * iw01 + lkg_pix(LJ, X, Y + 1) * iw10 + lkg_pix(LJ, X + 1, Y + 1) * iw11, W_BITS - 5) - iv[t];
                    sb1 += (long long)diff * ixv[t]; sb2 += (long long)diff * iyv[t];
                }
            }
            const float fb1 = (float)((double)wave_sum_i64(sb1) * FLT_SCALE_D);
            const float fb2 = (float)((double)wave_sum_i64(sb2) * FLT_SCALE_D);
            const float dx = (A12 * fb2 - A22 * fb1) * D;
            const float dy = (A12 * fb1 - A11 * fb2) * D;
            wx += dx; wy += dy;
            curx = wx + halfWin; cury = wy + halfWin;
            if ((double)dx * dx + (double)dy * dy <= a.eps2) break;
            if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                curx -= dx * 0.5f; cury -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
    }
    if (lane == 0) {
        a.next[2 * pi] = curx;
        a.next[2 * pi + 1] = cury;
        a.status[pi] = ok ? 1 : 0;
    }
}

}  // namespace

static int lk_fill_args(LKArgs& a, const ImgView& I, const ImgView& J, const PyrGeom& g,
                        const float* prev, float* next, uint8_t* status, const int* count, int cap,
                        const LKParams& p, const int* index)
{
    if (p.win < 3 || p.win > LKG_MAX_WIN) { av_set_error("av_lk_track: winSize %d outside 3 .. %d", p.win, LKG_MAX_WIN); return AV_E_INVALID; }
    assert(I.pyr_stride == J.pyr_stride);        // the kernels step both pyramids by LKArgs::stream_stride
    a.pyrI = I.pyr; a.pyrJ = J.pyr; a.stream_stride = I.pyr_stride; a.g = g;
    // cv::buildOpticalFlowPyramid stops at the first level whose successor would be no larger than the window in either
    // dimension (OpenCV 4.x lkpyramid.cpp: `if (sz.width <= winSize.width || sz.height <= winSize.height) return level`);
    // level 0 is always tracked.  Not reached by the reference's 752 x 480 / 15 / 3.
    for (int l = 1; l < a.g.levels; ++l)
        if (a.g.w[l] <= p.win || a.g.h[l] <= p.win) { a.g.levels = l; break; }
    a.prev = prev; a.next = next; a.status = status; a.count = count; a.index = index; a.cap = cap;
    a.max_iter = p.max_iter; a.eps2 = p.eps2;
    a.min_eig_up = (float)p.min_eig;
    if ((double)a.min_eig_up < p.min_eig) a.min_eig_up = nextafterf(a.min_eig_up, INFINITY);
    a.min_eig_num = av_lk_quotient_bound(a.min_eig_up, (float)(2 * p.win * p.win));      // read by the 16-lane kernel (win == 15) only
    if (p.eps2 >= 1e-30) { a.eps_lo = (float)(p.eps2 * (1. - 0x1p-18)); a.eps_hi = (float)(p.eps2 * (1. + 0x1p-18)); }
    else { a.eps_lo = -1.f; a.eps_hi = INFINITY; }                 // e32 may underflow: every test in fp64
    a.min_eig = p.min_eig;
    a.imgI = I.img; a.imgJ = J.img; a.imgI_stride = I.img_stride; a.imgJ_stride = J.img_stride; a.mapI = I.map; a.mapJ = J.map; a.prof = nullptr;
    a.n_set = 0; a.gx = 0;
    return AV_OK;
}

static bool lk_prof_on()
{
    static const bool prof = [] {
        const char* e = getenv("AV_LK_PROF");
        if (!(e && atoi(e) == 1)) return false;
        if (hipMalloc(&g_lk_prof, sizeof(unsigned long long) * (LKP_SLOTS + 4)) != hipSuccess) { g_lk_prof = nullptr; return false; }
        (void)hipMemset(g_lk_prof, 0, sizeof(unsigned long long) * (LKP_SLOTS + 4));
        (void)hipDeviceSynchronize();
        atexit(lk_prof_report);
        return true;
    }();
    return prof;
}

// grid of the 16-lane kernels: XCD-aware 1-D launch (lk_track_g16_body)
static dim3 lk_g16_grid(LKArgs& a, int n_set, int launch_pts, int pts_per_wg)
{
    a.n_set = n_set; a.gx = (launch_pts + pts_per_wg - 1) / pts_per_wg;
    return dim3((unsigned)a.gx * 8u * (unsigned)((n_set + 7) / 8));
}

int av_launch_lk(const ImgView& I, const ImgView& J, int n_set, const PyrGeom& g,
                 const float* prev, float* next, uint8_t* status, const int* count, int cap, int launch_pts,
                 const LKParams& p, hipStream_t st, const int* index)
{
    if (n_set <= 0 || launch_pts <= 0) return AV_OK;
    LKArgs a;
    int rc = lk_fill_args(a, I, J, g, prev, next, status, count, cap, p, index);
    if (rc) return rc;
    if (launch_pts > cap) launch_pts = cap;
    if (p.win != 15) {           // any other window of config.win_size: the general kernel (one wavefront per point)
        a.n_set = n_set; a.gx = 0;
        hipLaunchKernelGGL(lk_track_generic_kernel, dim3((launch_pts + 3) / 4, n_set), dim3(256), 0, st, a, p.win);
        AV_LAUNCH_CHECK();
        return AV_OK;
    }
    const bool prof = lk_prof_on();
    const int wgp = prof ? 256 : 64;             // one wavefront per workgroup; the profiling kernel: four
    const dim3 grid = lk_g16_grid(a, n_set, launch_pts, wgp / 16);
    a.prof = g_lk_prof;
    if (prof) hipLaunchKernelGGL(lk_track_g16_prof_kernel<15>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(lk_track_g16_kernel<15>, grid, dim3(64), 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// av_lk_track and av_lk_track_images: the latter reads level 0 in place from the two image arrays (the engine's way), the former from the pyramids
static int lk_track_api(const uint8_t* imgI_dev, const uint8_t* imgJ_dev, int64_t img_stride,
                        const uint8_t* pyrI_dev, const uint8_t* pyrJ_dev, int64_t pyr_stride, int n_set,
                        int w, int h, int levels,
                        const float* prev_dev, float* next_dev, uint8_t* status_dev, const int32_t* count_dev, int cap,
                        int win, int max_iter, double eps, double min_eig_threshold, void* stream)
{
    av_pyr_layout lay;
    int rc = av_pyramid_layout(w, h, levels, &lay);
    if (rc) return rc;
    if (!pyrI_dev || !pyrJ_dev || !prev_dev || !next_dev || !status_dev || !count_dev || cap <= 0 || n_set < 0 ||
        pyr_stride < lay.bytes) {
        av_set_error("av_lk_track: bad arguments");
        return AV_E_INVALID;
    }
    LKParams p;
    p.win = win;
    p.max_iter = max_iter < 0 ? 0 : (max_iter > 100 ? 100 : max_iter);        // as calc() clamps criteria.maxCount
    double e = eps < 0 ? 0. : (eps > 10. ? 10. : eps);
    p.eps2 = e * e;
    p.min_eig = min_eig_threshold;
    return av_launch_lk(ImgView{pyrI_dev, pyr_stride, imgI_dev, img_stride, nullptr}, ImgView{pyrJ_dev, pyr_stride, imgJ_dev, img_stride, nullptr}, n_set, av_make_geom(lay),
                        prev_dev, next_dev, status_dev, count_dev, cap, cap, p, (hipStream_t)stream);
}

AV_EXPORT int av_lk_track(const uint8_t* pyrI_dev, const uint8_t* pyrJ_dev, int64_t pyr_stride, int n_set,
                          int w, int h, int levels,
                          const float* prev_dev, float* next_dev, uint8_t* status_dev, const int32_t* count_dev, int cap,
                          int win, int max_iter, double eps, double min_eig_threshold, void* stream)
{
    return lk_track_api(nullptr, nullptr, 0, pyrI_dev, pyrJ_dev, pyr_stride, n_set, w, h, levels, prev_dev, next_dev, status_dev, count_dev, cap,
                        win, max_iter, eps, min_eig_threshold, stream);
}

AV_EXPORT int av_lk_track_images(const uint8_t* imgI_dev, const uint8_t* imgJ_dev, int64_t img_stride,
                                 const uint8_t* pyrI_dev, const uint8_t* pyrJ_dev, int64_t pyr_stride, int n_set,
                                 int w, int h, int levels,
                                 const float* prev_dev, float* next_dev, uint8_t* status_dev, const int32_t* count_dev, int cap,
                                 int win, int max_iter, double eps, double min_eig_threshold, void* stream)
{
    if (!imgI_dev || !imgJ_dev || w <= 0 || h <= 0 || img_stride < (int64_t)w * h) {
        av_set_error("av_lk_track_images: bad arguments");
        return AV_E_INVALID;
    }
    return lk_track_api(imgI_dev, imgJ_dev, img_stride, pyrI_dev, pyrJ_dev, pyr_stride, n_set, w, h, levels, prev_dev, next_dev, status_dev, count_dev, cap,
                        win, max_iter, eps, min_eig_threshold, stream);
}
