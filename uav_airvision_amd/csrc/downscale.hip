// downscale.hip -- 2 x 2 / 4 x 4 binning of tightly packed 8-bit grey frames (gfx950).
// The definition is written out in include/airvision.h (av_downscale): out(x, y) = (sum of the f x f input block + f * f / 2) >> 2 log2 f,
// integers only, no border rule (the input is exactly f w x f h).  tests/downscale_ref.py states it in NumPy and both kernels are held
// to it bit for bit.
//   vector path    w % 16 == 0 (w: the OUTPUT width), every base and every applied stride a multiple of 16 bytes.  A lane owns 16 output
//                  pixels of one output row: f rows x f uint4 loads in, one uint4 store out.  The horizontal sums are taken on two
//                  16-bit halves per dword -- (d & 0x00FF00FF) + ((d >> 8) & 0x00FF00FF) holds p0 + p1 and p2 + p3 of the dword's four
//                  pixels -- and the rows are added in that layout; f = 4 then adds the two halves.  The largest value is
//                  16 * 255 + 8 = 4088: it fits a half.  Lanes run over (output row, column vector) of one image in row-major order,
//                  so a wavefront holds neighbouring vectors.
//   generic path   anything else: one output pixel per lane, neighbouring lanes on neighbouring pixels, f * f bytes read per pixel.
// Workgroups are dealt image-major like the conversion kernels of pixfmt.hip: this is a pure streaming pass in which no two workgroups
// share a byte, so the XCD-aware placement of the stencil kernels (bayer.hip, clahe.hip: halo rows of one image into one L2) has
// nothing to gather.  No LDS, 64-bit byte offsets, plain vector stores, never in place.
#include "av_common.h"

namespace {

constexpr int DS_LANE = 16;                    // output pixels of one lane of the vector path = one 16-byte store
constexpr int DS_GEN = 256 * 16;               // output pixels of one workgroup of the generic path

struct DsArgs {
    FramePlace place;
    int W;                                         // input width = f * w (the input's row pitch)
    int w, h;                                      // output size
    int nvx, items;                                // vector path: vectors per output row, (row, vector) items per image
};

template <int F>
__global__ __launch_bounds__(256) void downscale_kernel(DsArgs a)
{
    const int img = blockIdx.x / a.place.per, blk = blockIdx.x - img * a.place.per;
    FrameAt f;
    if (!av_frame_at(a.place, img, f)) return;
    const uint8_t* src = f.src; uint8_t* dst = f.dst;
    const int item = blk * 256 + (int)threadIdx.x;                // < 2^24 / 16
    if (item >= a.items) return;
    const int y = item / a.nvx, vx = item - y * a.nvx;
    constexpr int ND = 4 * F;                                     // dwords of one input row of the lane: 16 F pixels
    uint32_t acc[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) acc[j] = 0u;
    const uint8_t* p = src + (int64_t)(F * y) * a.W + (int64_t)vx * (DS_LANE * F);
#pragma unroll
    for (int r = 0; r < F; ++r) {
        const uint4* row = reinterpret_cast<const uint4*>(p + (int64_t)r * a.W);
#pragma unroll
        for (int k = 0; k < F; ++k) {
            const uint4 q = row[k];
            const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * k + j] += (d[j] & 0x00FF00FFu) + ((d[j] >> 8) & 0x00FF00FFu);
        }
    }
    uint32_t o[4];
    if (F == 2) {                                                 // a dword holds two finished sums: output pixels 2 j, 2 j + 1
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t u = ((acc[2 * m] + 0x00020002u) >> 2) & 0x00FF00FFu, v = ((acc[2 * m + 1] + 0x00020002u) >> 2) & 0x00FF00FFu;
            o[m] = (u & 255u) | (u >> 16) << 8 | (v & 255u) << 16 | (v >> 16) << 24;
        }
    } else {                                                      // the two halves of a dword are the halves of one output pixel
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            uint32_t s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const uint32_t t = acc[4 * m + j]; s[j] = ((t & 0xFFFFu) + (t >> 16) + 8u) >> 4; }
            o[m] = s[0] | s[1] << 8 | s[2] << 16 | s[3] << 24;
        }
    }
    *reinterpret_cast<uint4*>(dst + (int64_t)y * a.w + (int64_t)vx * DS_LANE) = make_uint4(o[0], o[1], o[2], o[3]);
}

template <int F>
__global__ __launch_bounds__(256) void downscale_generic_kernel(DsArgs a)
{
    const int img = blockIdx.x / a.place.per, blk = blockIdx.x - img * a.place.per;
    FrameAt f;
    if (!av_frame_at(a.place, img, f)) return;
    const uint8_t* src = f.src; uint8_t* dst = f.dst;
    const int w = a.w, npix = a.w * a.h;
    const int p0 = blk * DS_GEN;                                  // < 2^24
#pragma unroll 2
    for (int j = 0; j < DS_GEN / 256; ++j) {
        const int p = p0 + j * 256 + (int)threadIdx.x;
        if (p >= npix) break;
        const int y = p / w, x = p - y * w;
        const uint8_t* q = src + (int64_t)(F * y) * a.W + F * x;
        uint32_t s = F * F / 2;
#pragma unroll
        for (int r = 0; r < F; ++r)
#pragma unroll
            for (int k = 0; k < F; ++k) s += q[(int64_t)r * a.W + k];
        dst[p] = (uint8_t)(s >> (F == 2 ? 2 : 4));
    }
}

// the one rule that picks the kernel (av_launch_downscale; av_downscale_vector_path reports it); w: the output width
bool ds_vector_ok(const FrameSet& src, const FrameSet& dst, int n_groups, int w) { return (w % DS_LANE) == 0 && av_frames_vec16(src, dst, n_groups); }

}  // namespace

int av_launch_downscale(const FrameSet& src, const FrameSet& dst, int n_groups, int W, int H, int f, hipStream_t st)
{
    if (n_groups <= 0) return AV_OK;
    if ((f != 2 && f != 4) || W <= 0 || H <= 0 || W % f || H % f) { av_set_error("av_downscale: factor %d does not bin %d x %d (2 or 4, dividing both sides)", f, W, H); return AV_E_INVALID; }
    DsArgs a;
    memset(&a, 0, sizeof(a));
    a.W = W; a.w = W / f; a.h = H / f;
    const bool vec = ds_vector_ok(src, dst, n_groups, a.w);
    int per = (int)(((int64_t)a.w * a.h + DS_GEN - 1) / DS_GEN);
    if (vec) {
        a.nvx = a.w / DS_LANE;
        a.items = a.nvx * a.h;
        per = (a.items + 255) / 256;
    }
    const unsigned n_wg = av_frame_place(&a.place, src, dst, n_groups, per, 1, "av_downscale", W, H);
    if (!n_wg) return AV_E_INVALID;
    const dim3 grid(n_wg), block(256);
    if (vec) {
        if (f == 2) hipLaunchKernelGGL(downscale_kernel<2>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(downscale_kernel<4>, grid, block, 0, st, a);
    } else {
        if (f == 2) hipLaunchKernelGGL(downscale_generic_kernel<2>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(downscale_generic_kernel<4>, grid, block, 0, st, a);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}

AV_EXPORT int av_downscale(const uint8_t* img_dev, int64_t img_stride, int n_img, int W, int H, int factor,
                           uint8_t* out_dev, int64_t out_stride, void* stream)
{
    if (factor != 2 && factor != 4) { av_set_error("av_downscale: factor %d is neither 2 nor 4", factor); return AV_E_INVALID; }
    if (W <= 0 || H <= 0 || (int64_t)W * H > AV_MAX_IMAGE_PIXELS) { av_set_error("av_downscale: W * H must be 1 .. AV_MAX_IMAGE_PIXELS = 2^24 (%d x %d)", W, H); return AV_E_INVALID; }
    if (W % factor || H % factor) { av_set_error("av_downscale: %d x %d is not divisible by the factor %d", W, H, factor); return AV_E_INVALID; }
    const int64_t in_bytes = (int64_t)W * H, out_bytes = in_bytes / (factor * factor);
    if (!img_dev || !out_dev || n_img < 0 || img_stride < in_bytes || out_stride < out_bytes) {
        av_set_error("av_downscale: bad arguments (n_img %d, strides %lld / %lld bytes for %d x %d by %d)", n_img, (long long)img_stride, (long long)out_stride, W, H, factor);
        return AV_E_INVALID;
    }
    if (n_img == 0) return AV_OK;
    if (av_spans_overlap(img_dev, img_stride, in_bytes, out_dev, out_stride, out_bytes, n_img)) { av_set_error("av_downscale: out_dev overlaps the input (the binning does not work in place)"); return AV_E_INVALID; }
    return av_launch_downscale(av_frames(img_dev, nullptr, img_stride), FrameSet{{out_dev, nullptr}, out_stride, nullptr}, n_img, W, H, factor, (hipStream_t)stream);
}

AV_EXPORT int av_downscale_vector_path(const uint8_t* img_dev, int64_t img_stride, int n_img, int W, int factor, const uint8_t* out_dev, int64_t out_stride)
{
    if ((factor != 2 && factor != 4) || W <= 0 || W % factor || n_img <= 0) return 0;
    return ds_vector_ok(av_frames(img_dev, nullptr, img_stride), av_frames(out_dev, nullptr, out_stride), n_img, W / factor) ? 1 : 0;
}
