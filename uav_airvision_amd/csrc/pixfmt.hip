// pixfmt.hip -- camera frames of the other pixel formats (16-bit grey, RGB / BGR, RGBA / BGRA) to tightly packed 8-bit grey (gfx950).
// The arithmetic is written out in include/airvision.h (av_to_gray8); tests/pixfmt_ref.py states it in NumPy and the kernel is held
// to it bit for bit.  A streaming pass (stream_pass.h): a lane's span is 16 pixels, 2 / 3 / 4 uint4 loads in and one uint4 store out;
// the unit is one pixel.  Never in place.
#include "stream_pass.h"

namespace {

constexpr int PF_LANE = 16;                    // output pixels of one lane = one 16-byte store

struct PixArgs {
    FramePlace place;
    int npix, vec;                                 // (stream_pass.h)
    int shift;
};

__host__ __device__ constexpr int pf_bytes(int fmt) { return fmt == AV_PIX_GRAY8 ? 1 : fmt == AV_PIX_GRAY16 ? 2 : (fmt == AV_PIX_RGB8 || fmt == AV_PIX_BGR8) ? 3 : 4; }

__device__ __forceinline__ uint32_t pf_luma(uint32_t r, uint32_t g, uint32_t b) { return (9798u * r + 19235u * g + 3735u * b + 16384u) >> 15; }
__device__ __forceinline__ uint32_t pf_byte(const uint32_t* d, int b) { return (d[b >> 2] >> (8 * (b & 3))) & 255u; }

// one pixel, byte by byte (16-bit samples are in host byte order: little endian, like the device)
template <int FMT>
__device__ __forceinline__ uint8_t pf_pixel(const uint8_t* p, int shift)
{
    if (FMT == AV_PIX_GRAY16) return (uint8_t)min(255u, ((uint32_t)p[0] | (uint32_t)p[1] << 8) >> shift);
    constexpr bool bgr = FMT == AV_PIX_BGR8 || FMT == AV_PIX_BGRA8;
    return (uint8_t)pf_luma(p[bgr ? 2 : 0], p[1], p[bgr ? 0 : 2]);
}

// 16 pixels from whole vectors
template <int FMT>
__device__ __forceinline__ uint4 pf_group(const uint4* in, int shift)
{
    constexpr int B = pf_bytes(FMT);
    constexpr bool bgr = FMT == AV_PIX_BGR8 || FMT == AV_PIX_BGRA8;
    uint32_t d[4 * B];
#pragma unroll
    for (int i = 0; i < B; ++i) { const uint4 q = in[i]; d[4 * i] = q.x; d[4 * i + 1] = q.y; d[4 * i + 2] = q.z; d[4 * i + 3] = q.w; }
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < PF_LANE; ++k) {
        uint32_t v;
        if (FMT == AV_PIX_GRAY16) v = min(255u, ((d[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) >> shift);
        else v = pf_luma(pf_byte(d, B * k + (bgr ? 2 : 0)), pf_byte(d, B * k + 1), pf_byte(d, B * k + (bgr ? 0 : 2)));
        o[k >> 2] |= v << (8 * (k & 3));
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

template <int FMT>
struct PixOp {
    using Args = PixArgs;
    static constexpr int SPAN = PF_LANE, UNIT = 1, UNROLL = 4, B = pf_bytes(FMT);
    static constexpr bool IMAGE_MINOR = false;
    int shift;
    __device__ __forceinline__ PixOp(const PixArgs& a, const FrameAt&, int, int) : shift(a.shift) {}
    __device__ __forceinline__ void span(const uint8_t* src, uint8_t* dst, int p) const
    {
        *reinterpret_cast<uint4*>(dst + p) = pf_group<FMT>(reinterpret_cast<const uint4*>(src + (int64_t)p * B), shift);
    }
    __device__ __forceinline__ void unit(const uint8_t* src, uint8_t* dst, int p) const { dst[p] = pf_pixel<FMT>(src + (int64_t)p * B, shift); }
};

}  // namespace

int av_pixfmt_bytes(int fmt)
{
    if (fmt >= AV_PIX_BAYER_RGGB8 && fmt <= AV_PIX_BAYER_GBRG16) return fmt >= AV_PIX_BAYER_RGGB16 ? 2 : 1;      // one sample per pixel (bayer.hip)
    return fmt >= AV_PIX_GRAY8 && fmt <= AV_PIX_BGRA8 ? pf_bytes(fmt) : 0;
}

// the packed transports (packed.hip): grey 32 .. 35 and mosaics 40 .. 55, in the order 10p, 12p, 10_csi2, 12_csi2
static int pk_kind(int fmt)
{
    if (fmt >= AV_PIX_GRAY10P && fmt <= AV_PIX_GRAY12_CSI2) return fmt - AV_PIX_GRAY10P;
    if (fmt >= AV_PIX_BAYER_RGGB10P && fmt <= AV_PIX_BAYER_GBRG12_CSI2) return (fmt - AV_PIX_BAYER_RGGB10P) >> 2;
    return -1;
}
int av_pixfmt_packed_depth(int fmt) { const int k = pk_kind(fmt); return k < 0 ? 0 : (k & 1) ? 12 : 10; }
bool av_pixfmt_packed_csi2(int fmt) { return pk_kind(fmt) >= 2; }
bool av_pixfmt_is_bayer(int fmt) { return (fmt >= AV_PIX_BAYER_RGGB8 && fmt <= AV_PIX_BAYER_GBRG16) || (fmt >= AV_PIX_BAYER_RGGB10P && fmt <= AV_PIX_BAYER_GBRG12_CSI2); }

const char* av_pixfmt_name(int fmt)
{
    static const char* const plain[] = {"gray8", "gray16", "rgb8", "bgr8", "rgba8", "bgra8"};
    static const char* const kind[] = {"10p", "12p", "10_csi2", "12_csi2"};
    static const char* const pat[] = {"rggb", "bggr", "grbg", "gbrg"};
    static thread_local char text[32];
    const int k = pk_kind(fmt);
    if (fmt >= AV_PIX_GRAY8 && fmt <= AV_PIX_BGRA8) return plain[fmt];
    if (k >= 0 && fmt < AV_PIX_BAYER_RGGB10P) snprintf(text, sizeof(text), "gray%s", kind[k]);
    else if (k >= 0) snprintf(text, sizeof(text), "bayer_%s%s", pat[fmt & 3], kind[k]);
    else if (av_pixfmt_bytes(fmt)) snprintf(text, sizeof(text), "bayer_%s%d", pat[fmt & 3], 8 * av_pixfmt_bytes(fmt));
    else snprintf(text, sizeof(text), "unknown");
    return text;
}

AV_EXPORT int64_t av_pixfmt_frame_bytes(int pixel_format, int w, int h)
{
    if (w <= 0 || h <= 0) return 0;
    const int depth = av_pixfmt_packed_depth(pixel_format);
    if (!depth) return (int64_t)w * h * av_pixfmt_bytes(pixel_format);
    if (w % (depth == 10 ? 4 : 2)) return 0;                       // a row is whole groups: 4 samples in 5 bytes, 2 in 3
    return (int64_t)w * h * depth / 8;
}

int av_pixfmt_check(int fmt, int shift, const char* who)
{
    if (av_pixfmt_bytes(fmt) == 0 && av_pixfmt_packed_depth(fmt) == 0) {
        av_set_error("%s: unknown pixel format %d (AV_PIX_GRAY8 = 0 .. AV_PIX_BGRA8 = 5, AV_PIX_BAYER_RGGB8 = 16 .. AV_PIX_BAYER_GBRG16 = 23, AV_PIX_GRAY10P = 32 .. "
                     "AV_PIX_GRAY12_CSI2 = 35, AV_PIX_BAYER_RGGB10P = 40 .. AV_PIX_BAYER_GBRG12_CSI2 = 55)", who, fmt);
        return AV_E_INVALID;
    }
    if (shift < 0 || shift > 8) { av_set_error("%s: gray16 shift %d outside 0 .. 8", who, shift); return AV_E_INVALID; }
    return AV_OK;
}

int av_pixfmt_check_size(int fmt, int w, int h, const char* who)
{
    const int depth = av_pixfmt_packed_depth(fmt);
    if (depth && w > 0 && h > 0 && av_pixfmt_frame_bytes(fmt, w, h) == 0) {
        av_set_error("%s: a row of %s is whole groups of %d samples: width %d is not (%d x %d)", who, av_pixfmt_name(fmt), depth == 10 ? 4 : 2, w, w, h);
        return AV_E_INVALID;
    }
    return AV_OK;
}

int av_launch_to_gray8(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, int fmt, int shift, hipStream_t st, const FrameSet* mosaic)
{
    if (n_groups <= 0) return AV_OK;
    if (av_pixfmt_packed_depth(fmt)) {             // packed.hip; a packed mosaic in two passes: its reduced 8-bit mosaic into `mosaic`, bayer.hip's 8-bit kernels on that
        if (!av_pixfmt_is_bayer(fmt)) return av_launch_unpack_to_gray8(src, dst, n_groups, w, h, fmt, shift, st);
        if (!mosaic || !mosaic->base[0] || (src.base[1] && !mosaic->base[1])) { av_set_error("av_to_gray8: a packed mosaic (pixel format %d) needs a mosaic scratch", fmt); return AV_E_INVALID; }
        if (w < 2 || h < 2) { av_set_error("av_to_gray8: a Bayer mosaic is at least 2 x 2 samples (%d x %d)", w, h); return AV_E_INVALID; }
        const int rc = av_launch_unpack_to_gray8(src, *mosaic, n_groups, w, h, fmt, shift, st);
        return rc ? rc : av_launch_bayer_to_gray8(*mosaic, dst, n_groups, w, h, AV_PIX_BAYER_RGGB8 + (fmt & 3), 8, st);
    }
    if (fmt >= AV_PIX_BAYER_RGGB8) return av_launch_bayer_to_gray8(src, dst, n_groups, w, h, fmt, shift, st);      // a 3 x 3 stencil over rows: bayer.hip
    PixArgs a;
    memset(&a, 0, sizeof(a));
    a.npix = w * h; a.shift = shift;
    a.vec = av_frames_vec16(src, dst, n_groups);
    const unsigned n_wg = av_frame_place(&a.place, src, dst, n_groups, (a.npix + 256 * PF_LANE - 1) / (256 * PF_LANE), 1, "av_to_gray8", w, h);
    if (!n_wg) return AV_E_INVALID;
    const dim3 grid(n_wg), block(256);
    switch (fmt) {
    case AV_PIX_GRAY16: hipLaunchKernelGGL(stream_pass_kernel<PixOp<AV_PIX_GRAY16>>, grid, block, 0, st, a); break;
    case AV_PIX_RGB8:   hipLaunchKernelGGL(stream_pass_kernel<PixOp<AV_PIX_RGB8>>, grid, block, 0, st, a); break;
    case AV_PIX_BGR8:   hipLaunchKernelGGL(stream_pass_kernel<PixOp<AV_PIX_BGR8>>, grid, block, 0, st, a); break;
    case AV_PIX_RGBA8:  hipLaunchKernelGGL(stream_pass_kernel<PixOp<AV_PIX_RGBA8>>, grid, block, 0, st, a); break;
    case AV_PIX_BGRA8:  hipLaunchKernelGGL(stream_pass_kernel<PixOp<AV_PIX_BGRA8>>, grid, block, 0, st, a); break;
    default: av_set_error("av_to_gray8: no conversion kernel for pixel format %d", fmt); return AV_E_INVALID;
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}

AV_EXPORT int av_to_gray8(const void* img_dev, int64_t img_stride_bytes, int n_img, int w, int h, int pixel_format, int shift,
                          uint8_t* out_dev, int64_t out_stride, void* stream)
{
    int rc = av_pixfmt_check(pixel_format, shift, "av_to_gray8");
    if (rc) return rc;
    if (w <= 0 || h <= 0 || (int64_t)w * h > AV_MAX_IMAGE_PIXELS) { av_set_error("av_to_gray8: w * h must be 1 .. AV_MAX_IMAGE_PIXELS = 2^24 (%d x %d)", w, h); return AV_E_INVALID; }
    if ((rc = av_pixfmt_check_size(pixel_format, w, h, "av_to_gray8"))) return rc;
    const bool bayer = av_pixfmt_is_bayer(pixel_format), packed = av_pixfmt_packed_depth(pixel_format) != 0;
    if (bayer && (w < 2 || h < 2)) { av_set_error("av_to_gray8: a Bayer mosaic is at least 2 x 2 samples (%d x %d)", w, h); return AV_E_INVALID; }
    const int64_t npix = (int64_t)w * h, in_bytes = av_pixfmt_frame_bytes(pixel_format, w, h);
    if (!img_dev || !out_dev || n_img < 0 || img_stride_bytes < in_bytes || out_stride < npix) {
        av_set_error("av_to_gray8: bad arguments (n_img %d, strides %lld / %lld bytes for %d x %d %s frames of %lld bytes)", n_img, (long long)img_stride_bytes,
                     (long long)out_stride, w, h, av_pixfmt_name(pixel_format), (long long)in_bytes);
        return AV_E_INVALID;
    }
    if (n_img == 0) return AV_OK;
    const uint8_t* in = static_cast<const uint8_t*>(img_dev);
    hipStream_t st = (hipStream_t)stream;
    if (pixel_format == AV_PIX_GRAY8 && in == out_dev && img_stride_bytes == out_stride) return AV_OK;      // the identity in place: nothing to do
    if (av_spans_overlap(in, img_stride_bytes, in_bytes, out_dev, out_stride, npix, n_img)) { av_set_error("av_to_gray8: out_dev overlaps the input (the conversion does not work in place)"); return AV_E_INVALID; }
    if (pixel_format == AV_PIX_GRAY8) {            // the identity out of place: a strided copy
        AV_HIP(hipMemcpy2DAsync(out_dev, (size_t)out_stride, in, (size_t)img_stride_bytes, (size_t)npix, (size_t)n_img, hipMemcpyDeviceToDevice, st));
        return AV_OK;
    }
    const FrameSet src = av_frames(in, nullptr, img_stride_bytes), dst{{out_dev, nullptr}, out_stride, nullptr};
    if (packed && bayer) {                         // the operator owns no scratch: one for this call, freed once the stream has passed it (the call waits)
        AvScratch scratch;
        const int64_t mstride = (npix + 15) & ~(int64_t)15;      // whole vectors apart: the vector paths of both passes stay open to a batch
        if ((rc = scratch.alloc((size_t)n_img * mstride))) return rc;
        const FrameSet mosaic{{static_cast<uint8_t*>(scratch.p), nullptr}, mstride, nullptr};
        rc = av_launch_to_gray8(src, dst, n_img, w, h, pixel_format, shift, st, &mosaic);
        const hipError_t done = hipStreamSynchronize(st);
        if (!rc && done != hipSuccess) { av_set_error("av_to_gray8: %s", hipGetErrorString(done)); return AV_E_HIP; }
        return rc;
    }
    return av_launch_to_gray8(src, dst, n_img, w, h, pixel_format, shift, st);
}
