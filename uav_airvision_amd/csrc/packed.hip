// packed.hip -- packed 10 / 12-bit camera transports (PFNC Mono10p / Mono12p, MIPI CSI-2 RAW10 / RAW12) to tightly packed 8-bit samples
// (gfx950).  The byte layouts and the value rule are written out in include/airvision.h ("Packed 10 / 12-bit transports");
// tests/packed_ref.py states them in NumPy and the kernel is held to it bit for bit.  A streaming pass (stream_pass.h) over groups (4
// samples in 5 bytes, or 2 in 3; a row is whole groups, so the image is): the unit is one group, a lane's span is what is whole
// vectors on both sides -- 12-bit: 32 samples, three uint4 loads in, two uint4 stores out; 10-bit: 64 samples, five in, four out.
// Every sample goes through the GRAY16 rule on its left-justified value: s = min(255, (v << (16 - d)) >> shift).  For a packed mosaic
// that is all this file does: the reduced 8-bit mosaic goes to a scratch and bayer.hip's 8-bit kernels run on it unchanged.
#include "stream_pass.h"

namespace {

constexpr int PK_P = 0, PK_CSI2 = 1;           // LAYOUT: PFNC "p" (little-endian bit stream, LSB first) / MIPI CSI-2 (high bytes first, low bits in the group's last byte)

struct PackArgs {
    FramePlace place;
    int npix, vec;                                 // (stream_pass.h)
    int shift;
};

template <int DEPTH> struct PkGeom {
    static constexpr int GPX = DEPTH == 10 ? 4 : 2;        // samples of a group
    static constexpr int GB = DEPTH == 10 ? 5 : 3;         // bytes of a group
    static constexpr int SPAN = DEPTH == 10 ? 64 : 32;     // samples of one lane's span in the aligned body
    static constexpr int IN_VEC = SPAN * DEPTH / 128;      // 5 / 3 uint4 in
    static constexpr int OUT_VEC = SPAN / 16;              // 4 / 2 uint4 out
};

template <int DEPTH>
__device__ __forceinline__ uint32_t pk_reduce(uint32_t v, int shift) { return min(255u, (v << (16 - DEPTH)) >> shift); }

__device__ __forceinline__ uint32_t pk_byte(const uint32_t* d, int b) { return (d[b >> 2] >> (8 * (b & 3))) & 255u; }

// sample k of a span held in dwords d[] (k and everything derived from it are compile-time constants after unrolling)
template <int DEPTH, int LAYOUT>
__device__ __forceinline__ uint32_t pk_sample(const uint32_t* d, int k)
{
    constexpr uint32_t mask = (1u << DEPTH) - 1u;
    if (LAYOUT == PK_P) {
        const int bit = k * DEPTH, w = bit >> 5, o = bit & 31;
        uint32_t v = d[w] >> o;
        if (o + DEPTH > 32) v |= d[w + 1] << (32 - o);
        return v & mask;
    }
    using G = PkGeom<DEPTH>;
    const int g = k / G::GPX, j = k - g * G::GPX;
    constexpr int low = DEPTH - 8;                         // 2 / 4 low bits per sample in the group's last byte
    return pk_byte(d, G::GB * g + j) << low | ((pk_byte(d, G::GB * g + G::GPX) >> (low * j)) & ((1u << low) - 1u));
}

// one group, byte by byte: GB bytes in, GPX bytes out
template <int DEPTH, int LAYOUT>
__device__ __forceinline__ void pk_group(const uint8_t* p, uint8_t* q, int shift)
{
    using G = PkGeom<DEPTH>;
    uint32_t d[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < G::GB; ++i) d[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
#pragma unroll
    for (int j = 0; j < G::GPX; ++j) q[j] = (uint8_t)pk_reduce<DEPTH>(pk_sample<DEPTH, LAYOUT>(d, j), shift);
}

template <int DEPTH, int LAYOUT>
struct PackOp {
    using Args = PackArgs;
    using G = PkGeom<DEPTH>;
    static constexpr int SPAN = G::SPAN, UNIT = G::GPX, UNROLL = 2;
    static constexpr bool IMAGE_MINOR = false;
    int shift;
    __device__ __forceinline__ PackOp(const PackArgs& a, const FrameAt&, int, int) : shift(a.shift) {}
    __device__ __forceinline__ void span(const uint8_t* src, uint8_t* dst, int p) const
    {
        const uint4* in = reinterpret_cast<const uint4*>(src + (int64_t)(p / G::GPX) * G::GB);      // SPAN samples are whole vectors: 48 p / 32 or 80 p / 64 bytes in
        uint32_t d[4 * G::IN_VEC];
#pragma unroll
        for (int i = 0; i < G::IN_VEC; ++i) { const uint4 q = in[i]; d[4 * i] = q.x; d[4 * i + 1] = q.y; d[4 * i + 2] = q.z; d[4 * i + 3] = q.w; }
        uint32_t o[4 * G::OUT_VEC];
#pragma unroll
        for (int i = 0; i < 4 * G::OUT_VEC; ++i) o[i] = 0u;
#pragma unroll
        for (int k = 0; k < G::SPAN; ++k) o[k >> 2] |= pk_reduce<DEPTH>(pk_sample<DEPTH, LAYOUT>(d, k), shift) << (8 * (k & 3));
        uint4* out = reinterpret_cast<uint4*>(dst + p);
#pragma unroll
        for (int i = 0; i < G::OUT_VEC; ++i) out[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    }
    __device__ __forceinline__ void unit(const uint8_t* src, uint8_t* dst, int q) const { pk_group<DEPTH, LAYOUT>(src + (int64_t)q * G::GB, dst + (int64_t)q * G::GPX, shift); }
};

}  // namespace

int av_launch_unpack_to_gray8(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, int fmt, int shift, hipStream_t st)
{
    if (n_groups <= 0) return AV_OK;
    const int depth = av_pixfmt_packed_depth(fmt);
    if (!depth || av_pixfmt_frame_bytes(fmt, w, h) == 0) { av_set_error("av_to_gray8: %d x %d of pixel format %d is no packed frame of whole groups", w, h, fmt); return AV_E_INVALID; }
    const bool csi2 = av_pixfmt_packed_csi2(fmt);
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.npix = w * h; a.shift = shift;
    a.vec = av_frames_vec16(src, dst, n_groups);
    const int block = 256 * (depth == 10 ? PkGeom<10>::SPAN : PkGeom<12>::SPAN);      // samples of one workgroup
    const unsigned n_wg = av_frame_place(&a.place, src, dst, n_groups, (a.npix + block - 1) / block, 1, "av_to_gray8", w, h);
    if (!n_wg) return AV_E_INVALID;
    const dim3 grid(n_wg), blockdim(256);
    if (depth == 10) {
        if (csi2) hipLaunchKernelGGL((stream_pass_kernel<PackOp<10, PK_CSI2>>), grid, blockdim, 0, st, a);
        else hipLaunchKernelGGL((stream_pass_kernel<PackOp<10, PK_P>>), grid, blockdim, 0, st, a);
    } else {
        if (csi2) hipLaunchKernelGGL((stream_pass_kernel<PackOp<12, PK_CSI2>>), grid, blockdim, 0, st, a);
        else hipLaunchKernelGGL((stream_pass_kernel<PackOp<12, PK_P>>), grid, blockdim, 0, st, a);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}
