// photometric.hip -- photometric calibration of 8-bit grey frames: inverse response table and vignette gain map (gfx950).
// The arithmetic is written out in include/airvision.h ("Photometric calibration"); tests/photometric_ref.py states it in NumPy and the
// kernel is held to it bit for bit:
//     out = min(255, (response[p] * gain[x] + (1 << 19)) >> 20)        response Q8 (absent: p << 8), gain Q12 (absent: 4096)
// A streaming pass (stream_pass.h): a lane's span is 16 pixels -- one uint4 of pixels and two uint4 of gains in, 16 table look-ups,
// one uint4 out -- and the unit is one pixel.  The aligned body needs the gain bases to be whole 16-byte vectors too (ph_vector_ok).
// The 512-byte response table of the workgroup's camera is staged into LDS once per workgroup (256 lanes, one entry each).
// With per-frame exposure factors ("Exposure-time normalisation" in include/airvision.h; tests/exposure_ref.py) the table a workgroup
// stages is its image's own: r'[p] = min(65280, (response[p] * k + 2048) >> 12), k uint16 Q12 of the image's group and camera -- the
// whole per-pixel cost of the factor; span() and unit() do not know of it.  Those instances always use the LDS table.
// In place (src == dst, same list) is correct: a lane reads its own pixels before it writes them and no lane reads another's.
// Workgroup order: image-minor (id = block * n_img + image).  The gain map is one per camera for ALL images of a launch, so the
// workgroups in flight at any time read the same few KB of it from L2 while the pixels stream; with the image-major order of
// pixfmt.hip every image would walk the whole map (4.6 MB per camera at 1920 x 1200, more than one L2) on its own.
#include "stream_pass.h"

namespace {

constexpr int PH_LANE = 16;                    // pixels of one lane = one 16-byte store

struct PhArgs {
    FramePlace place;
    int npix, vec;                                 // (stream_pass.h; vec: the gain bases are whole vectors as well)
    const uint16_t* resp0; const uint16_t* resp1;  // [256] Q8 per camera
    const uint16_t* gain0; const uint16_t* gain1;  // [npix] Q12 per camera
    const uint16_t* k0; const uint16_t* k1;        // [n_groups] Q12 per camera: exposure factors by group of the launch (instances with HAS_EXPOSURE)
};

__shared__ uint16_t ph_tab[256];               // the response table of the workgroup's camera (instances with one), or of its image (HAS_EXPOSURE)

__device__ __forceinline__ uint32_t ph_out(uint32_t r, uint32_t g) { return min(255u, (r * g + (1u << 19)) >> 20); }      // r <= 65280: r * g + 2^19 < 2^32

template <bool HAS_RESPONSE, bool HAS_GAIN, bool HAS_EXPOSURE>
struct PhOp {
    using Args = PhArgs;
    static constexpr int SPAN = PH_LANE, UNIT = 1, UNROLL = 4;
    static constexpr bool IMAGE_MINOR = true;
    const uint16_t* gain;
    __device__ __forceinline__ PhOp(const PhArgs& a, const FrameAt& f, int, int tid) : gain(f.cam ? a.gain1 : a.gain0)
    {
        if constexpr (HAS_EXPOSURE) {
            const uint32_t k = (f.cam ? a.k1 : a.k0)[f.g];                        // 65280 * 65535 + 2048 < 2^32
            const uint32_t base = HAS_RESPONSE ? (uint32_t)(f.cam ? a.resp1 : a.resp0)[tid] : (uint32_t)tid << 8;
            ph_tab[tid] = (uint16_t)min(65280u, (base * k + 2048u) >> 12);
            __syncthreads();
        } else if constexpr (HAS_RESPONSE) {
            ph_tab[tid] = (f.cam ? a.resp1 : a.resp0)[tid];
            __syncthreads();
        }
    }
    __device__ __forceinline__ uint32_t resp(uint32_t p) const
    {
        if constexpr (HAS_RESPONSE || HAS_EXPOSURE) return ph_tab[p];
        else return p << 8;
    }
    __device__ __forceinline__ void span(const uint8_t* src, uint8_t* dst, int p) const
    {
        const uint4 q = *reinterpret_cast<const uint4*>(src + p);
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        uint32_t gw[8];
        if (HAS_GAIN) {
            const uint4* gp = reinterpret_cast<const uint4*>(gain + p);
            const uint4 g0 = gp[0], g1 = gp[1];
            gw[0] = g0.x; gw[1] = g0.y; gw[2] = g0.z; gw[3] = g0.w; gw[4] = g1.x; gw[5] = g1.y; gw[6] = g1.z; gw[7] = g1.w;
        }
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < PH_LANE; ++k) {
            const uint32_t px = (d[k >> 2] >> (8 * (k & 3))) & 255u;
            const uint32_t gk = HAS_GAIN ? (gw[k >> 1] >> (16 * (k & 1))) & 0xFFFFu : 4096u;
            o[k >> 2] |= ph_out(resp(px), gk) << (8 * (k & 3));
        }
        *reinterpret_cast<uint4*>(dst + p) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __device__ __forceinline__ void unit(const uint8_t* src, uint8_t* dst, int p) const { dst[p] = (uint8_t)ph_out(resp(src[p]), HAS_GAIN ? (uint32_t)gain[p] : 4096u); }
};

// the one rule that picks the body (av_launch_photometric; av_photometric_vector_path reports it)
bool ph_vector_ok(const FrameSet& src, const FrameSet& dst, int n_groups, const uint16_t* gain0, const uint16_t* gain1)
{
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return av_frames_vec16(src, dst, n_groups) && al16(gain0) && al16(gain1);
}

int ph_launch(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, const uint16_t* resp0, const uint16_t* resp1,
              const uint16_t* gain0, const uint16_t* gain1, const uint16_t* k0, const uint16_t* k1, hipStream_t st)
{
    PhArgs a;
    memset(&a, 0, sizeof(a));
    a.npix = w * h;
    a.resp0 = resp0; a.resp1 = resp1; a.gain0 = gain0; a.gain1 = gain1; a.k0 = k0; a.k1 = k1;
    a.vec = ph_vector_ok(src, dst, n_groups, gain0, gain1);
    const unsigned n_wg = av_frame_place(&a.place, src, dst, n_groups, (a.npix + 256 * PH_LANE - 1) / (256 * PH_LANE), 1, "av_photometric", w, h);
    if (!n_wg) return AV_E_INVALID;
    const dim3 grid(n_wg), block(256);
    if (k0) {
        if (resp0 && gain0) hipLaunchKernelGGL((stream_pass_kernel<PhOp<true, true, true>>), grid, block, 0, st, a);
        else if (resp0) hipLaunchKernelGGL((stream_pass_kernel<PhOp<true, false, true>>), grid, block, 0, st, a);
        else if (gain0) hipLaunchKernelGGL((stream_pass_kernel<PhOp<false, true, true>>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((stream_pass_kernel<PhOp<false, false, true>>), grid, block, 0, st, a);
    } else if (resp0 && gain0) hipLaunchKernelGGL((stream_pass_kernel<PhOp<true, true, false>>), grid, block, 0, st, a);
    else if (resp0) hipLaunchKernelGGL((stream_pass_kernel<PhOp<true, false, false>>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((stream_pass_kernel<PhOp<false, true, false>>), grid, block, 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

int av_launch_photometric(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, const uint16_t* resp0, const uint16_t* resp1,
                          const uint16_t* gain0, const uint16_t* gain1, const uint16_t* k0, const uint16_t* k1, hipStream_t st)
{
    if (n_groups <= 0) return AV_OK;
    if (src.map && src.map != dst.map) { av_set_error("av_photometric: a listed source is read through the destination's list"); return AV_E_INVALID; }
    const bool two = src.base[1] != nullptr;
    if (two && (k0 != nullptr) != (k1 != nullptr)) { av_set_error("av_photometric: exposure factors for one camera of two"); return AV_E_INVALID; }
    if (!two) {
        if (!resp0 && !gain0 && !k0) { av_set_error("av_photometric: neither a response table nor a gain map nor exposure factors"); return AV_E_INVALID; }
        return ph_launch(src, dst, n_groups, w, h, resp0, nullptr, gain0, nullptr, k0, nullptr, st);
    }
    if ((resp0 != nullptr) == (resp1 != nullptr) && (gain0 != nullptr) == (gain1 != nullptr)) {      // both cameras have the same parts: one launch
        if (!resp0 && !gain0 && !k0) { av_set_error("av_photometric: neither a response table nor a gain map nor exposure factors"); return AV_E_INVALID; }
        return ph_launch(src, dst, n_groups, w, h, resp0, resp1, gain0, gain1, k0, k1, st);
    }
    // the cameras differ in which parts they have: one launch per camera, each with its own kernel and its own factors (a camera with
    // no part at all is the identity: copied if it is not in place)
    const uint16_t* resp[2] = {resp0, resp1};
    const uint16_t* gain[2] = {gain0, gain1};
    const uint16_t* k[2] = {k0, k1};
    for (int cam = 0; cam < 2; ++cam) {
        const FrameSet s1{{src.base[cam], nullptr}, src.stride, src.map}, d1{{dst.base[cam], nullptr}, dst.stride, dst.map};
        if (resp[cam] || gain[cam] || k[cam]) {
            const int rc = ph_launch(s1, d1, n_groups, w, h, resp[cam], nullptr, gain[cam], nullptr, k[cam], nullptr, st);
            if (rc) return rc;
        } else if (src.base[cam] != dst.base[cam] || src.stride != dst.stride) {
            av_set_error("av_photometric: a camera without tables next to one with tables is only taken in place");
            return AV_E_INVALID;
        }
    }
    return AV_OK;
}

static int ph_check(const char* who, const void* in_dev, const void* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride, bool quiet)
{
    if (w <= 0 || h <= 0 || (int64_t)w * h > AV_MAX_IMAGE_PIXELS) {
        if (!quiet) av_set_error("%s: w * h must be 1 .. AV_MAX_IMAGE_PIXELS = 2^24 (%d x %d)", who, w, h);
        return AV_E_INVALID;
    }
    const int64_t npix = (int64_t)w * h;
    if (!in_dev || !out_dev || n < 0 || in_stride < npix || out_stride < npix) {
        if (!quiet) av_set_error("%s: bad arguments (n %d, strides %lld / %lld bytes for %d x %d)", who, n, (long long)in_stride, (long long)out_stride, w, h);
        return AV_E_INVALID;
    }
    return AV_OK;
}

// av_photometric and av_photometric_exposure: the same checks, `who` in the texts; k_dev null = no exposure factors
static int ph_operator(const char* who, const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                       const uint16_t* response_dev, const uint16_t* gain_dev, bool takes_k, const uint16_t* k_dev, void* stream)
{
    int rc = ph_check(who, in_dev, out_dev, n, w, h, in_stride, out_stride, false);
    if (rc) return rc;
    if (!response_dev && !gain_dev && !k_dev) {
        av_set_error("%s: neither a response table nor a gain map%s", who, takes_k ? " nor exposure factors (all three null)" : " (both null)");
        return AV_E_INVALID;
    }
    if (n == 0) return AV_OK;
    const int64_t npix = (int64_t)w * h;
    const bool in_place = in_dev == out_dev && (n == 1 || in_stride == out_stride);      // (one image applies no stride)
    if (!in_place && av_spans_overlap(in_dev, in_stride, npix, out_dev, out_stride, npix, n)) {
        av_set_error("%s: out_dev overlaps the input without being the input itself (in place needs the same address and stride)", who);
        return AV_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    if (response_dev) {                            // an entry above 65280 would overflow the 32-bit product: checked here, once per call (blocking for 512 bytes)
        uint16_t tab[256];
        AV_HIP(hipMemcpyAsync(tab, response_dev, sizeof(tab), hipMemcpyDeviceToHost, st));
        AV_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < 256; ++i)
            if (tab[i] > AV_PHOTOMETRIC_RESPONSE_MAX) { av_set_error("%s: response[%d] = %d is above %d (255 in Q8)", who, i, (int)tab[i], AV_PHOTOMETRIC_RESPONSE_MAX); return AV_E_INVALID; }
    }
    return av_launch_photometric(av_frames(in_dev, nullptr, in_stride), FrameSet{{out_dev, nullptr}, out_stride, nullptr}, n, w, h,
                                 response_dev, nullptr, gain_dev, nullptr, k_dev, nullptr, st);
}

AV_EXPORT int av_photometric(const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                             const uint16_t* response_dev, const uint16_t* gain_dev, void* stream)
{
    return ph_operator("av_photometric", in_dev, out_dev, n, w, h, in_stride, out_stride, response_dev, gain_dev, false, nullptr, stream);
}

AV_EXPORT int av_photometric_exposure(const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                                      const uint16_t* response_dev, const uint16_t* gain_dev, const uint16_t* k_dev, void* stream)
{
    return ph_operator("av_photometric_exposure", in_dev, out_dev, n, w, h, in_stride, out_stride, response_dev, gain_dev, true, k_dev, stream);
}

AV_EXPORT int av_photometric_vector_path(const uint8_t* in_dev, uint8_t* out_dev, int n, int w, int h, int64_t in_stride, int64_t out_stride,
                                         const uint16_t* response_dev, const uint16_t* gain_dev)
{
    if (ph_check("av_photometric_vector_path", in_dev, out_dev, n, w, h, in_stride, out_stride, true) || n == 0 || (!response_dev && !gain_dev)) return 0;
    return ph_vector_ok(av_frames(in_dev, nullptr, in_stride), av_frames(out_dev, nullptr, out_stride), n, gain_dev, nullptr) ? 1 : 0;
}
