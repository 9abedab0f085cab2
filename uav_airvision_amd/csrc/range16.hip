// range16.hip -- 16-bit grey frames to 8-bit grey through a window (lo, hi) instead of a fixed shift: a window given by the caller
// ('window') or taken per stereo pair from a 4,096-bin histogram of v >> 4 ('auto') (gfx950).  The arithmetic is written out in
// include/airvision.h ("Range scaling of 16-bit grey"); tests/range16_ref.py states it in NumPy and the kernels are held to it bit for
// bit.  Integer arithmetic only; the histogram is summed with integer atomics, so the result does not depend on their order.
//   range16_hist_kernel    several 256-thread workgroups per image, each over R16_CHUNK samples: a 4,096 x uint32 histogram in LDS
//                          (16 KB), then its non-zero bins added to the group's histogram in global memory.  A lane reads 8 samples
//                          as one 16-byte vector and counts a run of equal bins before it touches LDS (a thermal frame sits in a few
//                          bins: neighbouring samples mostly share one); sample by sample for the ragged end and unaligned launches
//   range16_pick_kernel    one wavefront per group, 64 lanes x 64 bins: prefix sums across the wavefront, b_lo and b_hi, the
//                          minimum-span rule, the record {lo, hi, m}; the group's histogram is left zeroed for the next launch
//   apply                  a streaming pass (stream_pass.h): a lane's span is 16 pixels, two 16-byte loads in and one store out;
//                          the unit is one pixel.  Its state is the group's record (or the caller's window)
// A group is the images of one FrameSet group (one camera or the two of a stereo pair, pooled).  All byte offsets are 64-bit.
#include "stream_pass.h"

namespace {

constexpr int R16_BINS = 4096;
static_assert(R16_BINS + 4 == AV_GRAY16_WORK_WORDS, "a group's histogram and record are what the header promises");
constexpr int R16_CHUNK = 65536;               // samples of one histogram workgroup: 32 rounds of 256 lanes x 8 samples
constexpr int R16_LANE = 16;                   // output pixels of one lane of the apply kernel = one 16-byte store

struct Range16Args {
    FramePlace place;                              // (n_src: the images pooled into one group)
    int npix, vec;                                 // (stream_pass.h; the histogram: the source's alignment alone)
    uint32_t* hist;                                // [groups][R16_BINS], zero between launches
    uint32_t* rec;                                 // [groups][4]: lo, hi, m, 0; apply: null = the window below for every group
    uint32_t k_lo, k_hi, min_span;                 // pick: samples that may saturate at each end, smallest span
    uint32_t lo, hi, m;                            // apply without records
    int32_t* range_out;                            // apply: [groups][2] (lo, hi) of every group that is written; or null
};

__device__ __forceinline__ uint32_t r16_sample(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }      // host byte order: little endian
__device__ __forceinline__ uint32_t r16_map(uint32_t v, uint32_t lo, uint32_t hi, uint32_t m) { return min(255u, ((min(max(v, lo), hi) - lo) * m + 32768u) >> 16); }

__global__ __launch_bounds__(256) void range16_hist_kernel(Range16Args a)
{
    __shared__ uint32_t bins[R16_BINS];
    const int img = blockIdx.x / a.place.per, blk = blockIdx.x - img * a.place.per;
    FrameAt f;
    if (!av_frame_at(a.place, img, f)) return;      // (no destination: f.dst is not used)
    const uint8_t* src = f.src;
    const int tid = threadIdx.x, g = f.g;
    for (int b = tid; b < R16_BINS; b += 256) bins[b] = 0u;
    __syncthreads();
    const int p0 = blk * R16_CHUNK, p1 = min(a.npix, p0 + R16_CHUNK);      // < 2^24
    if (a.vec) {
        for (int p = p0 + tid * 8; p + 8 <= p1; p += 256 * 8) {
            const uint4 q = *reinterpret_cast<const uint4*>(src + (int64_t)p * 2);
            const uint32_t d[4] = {q.x, q.y, q.z, q.w};
            uint32_t run = (d[0] & 0xFFFFu) >> 4, cnt = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t b = ((d[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) >> 4;
                if (b != run) { atomicAdd(&bins[run], cnt); run = b; cnt = 0u; }
                ++cnt;
            }
            atomicAdd(&bins[run], cnt);
        }
        if (p1 == a.npix) {                                                  // the image's ragged end: its last npix % 8 samples
            const int q = (a.npix & ~7) + tid;
            if (q < a.npix && q >= p0) atomicAdd(&bins[r16_sample(src + (int64_t)q * 2) >> 4], 1u);
        }
    } else {
        for (int p = p0 + tid; p < p1; p += 256) atomicAdd(&bins[r16_sample(src + (int64_t)p * 2) >> 4], 1u);
    }
    __syncthreads();
    uint32_t* hist = a.hist + (size_t)g * R16_BINS;
    for (int b = tid; b < R16_BINS; b += 256) {
        const uint32_t c = bins[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

__global__ __launch_bounds__(64) void range16_pick_kernel(Range16Args a)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    if (av_frame_entry(a.place, g) < 0) return;
    uint4* mine = reinterpret_cast<uint4*>(a.hist + (size_t)g * R16_BINS + lane * 64);      // bins 64 lane .. 64 lane + 63
    uint32_t v[64];
#pragma unroll
    for (int i = 0; i < 16; ++i) { const uint4 q = mine[i]; v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w; }
#pragma unroll
    for (int i = 0; i < 16; ++i) mine[i] = make_uint4(0u, 0u, 0u, 0u);                       // zero again for the next launch
    uint32_t sum = 0u;
#pragma unroll
    for (int i = 0; i < 64; ++i) sum += v[i];
    uint32_t incl = sum;                                                                    // inclusive prefix over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    const uint32_t total = __shfl(incl, 63);
    const uint32_t below = incl - sum, above = total - incl;                                // samples in the lanes before / after this one
    // b_lo: the smallest bin with hist[0 .. b].sum() > k_lo; b_hi: the largest with hist[b .. 4095].sum() > k_hi.  One lane holds each.
    int b_lo = -1, b_hi = -1;
    if (below <= a.k_lo && a.k_lo < incl) {
        uint32_t c = below;
#pragma unroll
        for (int i = 0; i < 64; ++i) { c += v[i]; if (b_lo < 0 && c > a.k_lo) b_lo = lane * 64 + i; }
    }
    if (above <= a.k_hi && a.k_hi < above + sum) {
        uint32_t c = above;
#pragma unroll
        for (int i = 63; i >= 0; --i) { c += v[i]; if (b_hi < 0 && c > a.k_hi) b_hi = lane * 64 + i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { b_lo = max(b_lo, __shfl_xor(b_lo, o)); b_hi = max(b_hi, __shfl_xor(b_hi, o)); }      // every other lane holds -1
    if (b_lo < 0 || b_hi < 0) return;                                                       // an empty histogram: no record
    if (lane == 0) {
        uint32_t lo = 16u * (uint32_t)b_lo, hi = 16u * (uint32_t)b_hi + 15u;
        if (hi - lo < a.min_span) {
            // max(0, min(lo - need / 2, 65535 - min_span)) in signed arithmetic (every term is below 2^17): the unsigned form
            // lo >= need / 2 ? min(lo - need / 2, top) : 0 lost its guard in the compiler's output and wrapped to the upper clamp
            const int need = (int)a.min_span - (int)(hi - lo);
            lo = (uint32_t)max(0, min((int)lo - (need >> 1), 65535 - (int)a.min_span));
            hi = lo + a.min_span;
        }
        const uint32_t span = hi - lo;
        uint32_t* r = a.rec + 4 * (size_t)g;
        r[0] = lo; r[1] = hi; r[2] = ((255u << 16) + (span >> 1)) / span; r[3] = 0u;
    }
}

__device__ __forceinline__ uint4 r16_group(const uint4* in, uint32_t lo, uint32_t hi, uint32_t m)
{
    const uint4 q0 = in[0], q1 = in[1];
    const uint32_t d[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < R16_LANE; ++k) o[k >> 2] |= r16_map((d[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, lo, hi, m) << (8 * (k & 3));
    return make_uint4(o[0], o[1], o[2], o[3]);
}

struct Range16Op {
    using Args = Range16Args;
    static constexpr int SPAN = R16_LANE, UNIT = 1, UNROLL = 4;
    static constexpr bool IMAGE_MINOR = false;
    uint32_t lo, hi, m;
    __device__ __forceinline__ Range16Op(const Range16Args& a, const FrameAt& f, int blk, int tid) : lo(a.lo), hi(a.hi), m(a.m)
    {
        if (a.rec) { const uint32_t* r = a.rec + 4 * (size_t)f.g; lo = r[0]; hi = r[1]; m = r[2]; }
        if (a.range_out && blk == 0 && f.cam == 0 && tid == 0) { a.range_out[2 * f.g] = (int32_t)lo; a.range_out[2 * f.g + 1] = (int32_t)hi; }
    }
    __device__ __forceinline__ void span(const uint8_t* src, uint8_t* dst, int p) const
    {
        *reinterpret_cast<uint4*>(dst + p) = r16_group(reinterpret_cast<const uint4*>(src + (int64_t)p * 2), lo, hi, m);
    }
    __device__ __forceinline__ void unit(const uint8_t* src, uint8_t* dst, int p) const { dst[p] = (uint8_t)r16_map(r16_sample(src + (int64_t)p * 2), lo, hi, m); }
};

}  // namespace

int av_range16_check(int mode, int lo, int hi, int ppm_lo, int ppm_hi, int min_span, const char* who)
{
    if (mode != AV_GRAY16_WINDOW && mode != AV_GRAY16_AUTO) { av_set_error("%s: gray16 scale %d is neither AV_GRAY16_WINDOW (1) nor AV_GRAY16_AUTO (2)", who, mode); return AV_E_INVALID; }
    if (mode == AV_GRAY16_WINDOW && !(0 <= lo && lo < hi && hi <= 65535)) { av_set_error("%s: gray16 window (%d, %d) does not satisfy 0 <= lo < hi <= 65535", who, lo, hi); return AV_E_INVALID; }
    if (mode == AV_GRAY16_AUTO && (ppm_lo < 0 || ppm_hi < 0 || (int64_t)ppm_lo + ppm_hi > AV_GRAY16_MAX_CLIP_PPM)) {
        av_set_error("%s: gray16 auto clip (%d, %d) ppm: both are >= 0 and their sum is at most %d", who, ppm_lo, ppm_hi, AV_GRAY16_MAX_CLIP_PPM);
        return AV_E_INVALID;
    }
    if (mode == AV_GRAY16_AUTO && (min_span < 16 || min_span > 65535)) { av_set_error("%s: gray16 auto minimum span %d outside 16 .. 65535", who, min_span); return AV_E_INVALID; }
    return AV_OK;
}

int av_launch_gray16_range(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, const Range16& r, hipStream_t st)
{
    if (n_groups <= 0) return AV_OK;
    Range16Args a;
    memset(&a, 0, sizeof(a));
    a.npix = w * h;
    a.hist = r.hist; a.range_out = r.range_out;
    const int per_hist = (a.npix + R16_CHUNK - 1) / R16_CHUNK, per_apply = (a.npix + 256 * R16_LANE - 1) / (256 * R16_LANE);
    const unsigned n_wg = av_frame_place(&a.place, src, dst, n_groups, per_apply, 1, "av_to_gray8_range", w, h);      // the larger of the two grids
    if (!n_wg) return AV_E_INVALID;
    if (r.mode == AV_GRAY16_AUTO) {
        if (!r.hist || !r.rec) { av_set_error("av_to_gray8_range: AV_GRAY16_AUTO needs a histogram and a record buffer"); return AV_E_INVALID; }
        const int64_t N = (int64_t)a.npix * a.place.n_src;                                          // samples of a group: 64 bits on the host
        a.k_lo = (uint32_t)(N * r.ppm_lo / 1000000); a.k_hi = (uint32_t)(N * r.ppm_hi / 1000000); a.min_span = (uint32_t)r.min_span;
        a.rec = r.rec;
        a.place.per = per_hist;
        a.vec = av_frames_vec16(src, FrameSet{{nullptr, nullptr}, 0, dst.map}, n_groups);      // the histogram reads only: the source's alignment alone
        hipLaunchKernelGGL(range16_hist_kernel, dim3((unsigned)(per_hist * a.place.n_img)), dim3(256), 0, st, a);
        AV_LAUNCH_CHECK();
        hipLaunchKernelGGL(range16_pick_kernel, dim3((unsigned)n_groups), dim3(64), 0, st, a);
        AV_LAUNCH_CHECK();
    } else {
        const uint32_t span = (uint32_t)(r.hi - r.lo);
        a.lo = (uint32_t)r.lo; a.hi = (uint32_t)r.hi; a.m = ((255u << 16) + span / 2) / span;
    }
    a.place.per = per_apply;
    a.vec = av_frames_vec16(src, dst, n_groups);
    hipLaunchKernelGGL(stream_pass_kernel<Range16Op>, dim3(n_wg), dim3(256), 0, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

AV_EXPORT int av_to_gray8_range(const void* img_dev, int64_t img_stride_bytes, int n_img, int w, int h, int mode, int lo, int hi,
                                int ppm_lo, int ppm_hi, int min_span, int pool, const int32_t* index_dev,
                                uint8_t* out_dev, int64_t out_stride, int32_t* range_dev, uint32_t* work_dev, void* stream)
{
    int rc = av_range16_check(mode, lo, hi, ppm_lo, ppm_hi, min_span, "av_to_gray8_range");
    if (rc) return rc;
    if (w <= 0 || h <= 0 || (int64_t)w * h > AV_MAX_IMAGE_PIXELS) { av_set_error("av_to_gray8_range: w * h must be 1 .. AV_MAX_IMAGE_PIXELS = 2^24 (%d x %d)", w, h); return AV_E_INVALID; }
    const int64_t npix = (int64_t)w * h;
    if (!img_dev || !out_dev || n_img < 0 || (pool != 1 && pool != 2) || n_img % pool || img_stride_bytes < 2 * npix || out_stride < npix) {
        av_set_error("av_to_gray8_range: bad arguments (n_img %d in groups of %d, strides %lld / %lld bytes for %d x %d frames of %lld bytes)", n_img, pool,
                     (long long)img_stride_bytes, (long long)out_stride, w, h, (long long)(2 * npix));
        return AV_E_INVALID;
    }
    if (n_img == 0) return AV_OK;
    const uint8_t* in = static_cast<const uint8_t*>(img_dev);
    hipStream_t st = (hipStream_t)stream;
    if (!index_dev && av_spans_overlap(in, img_stride_bytes, 2 * npix, out_dev, out_stride, npix, n_img)) {
        av_set_error("av_to_gray8_range: out_dev overlaps the input (the conversion does not work in place)");
        return AV_E_INVALID;
    }
    const int n_groups = n_img / pool;
    const FrameSet src = av_frames(in, pool == 2 ? in + img_stride_bytes : nullptr, pool * img_stride_bytes);
    const FrameSet dst{{out_dev, pool == 2 ? out_dev + out_stride : nullptr}, pool * out_stride, index_dev};
    Range16 r;
    r.mode = mode; r.lo = lo; r.hi = hi; r.ppm_lo = ppm_lo; r.ppm_hi = ppm_hi; r.min_span = min_span; r.hist = nullptr; r.rec = nullptr; r.range_out = range_dev;
    if (mode != AV_GRAY16_AUTO) return av_launch_gray16_range(src, dst, n_groups, w, h, r, st);
    if (work_dev) {                                // the caller's histograms and records: nothing is allocated, nothing waits
        r.hist = work_dev; r.rec = work_dev + (size_t)n_groups * R16_BINS;
        return av_launch_gray16_range(src, dst, n_groups, w, h, r, st);
    }
    // without them: histograms and records for this call, freed once the stream has passed them (the call waits)
    AvScratch scratch;
    const size_t words = (size_t)n_groups * AV_GRAY16_WORK_WORDS;
    if ((rc = scratch.alloc(words * sizeof(uint32_t)))) return rc;
    uint32_t* buf = static_cast<uint32_t*>(scratch.p);
    hipError_t done = hipMemsetAsync(buf, 0, words * sizeof(uint32_t), st);
    r.hist = buf; r.rec = buf + (size_t)n_groups * R16_BINS;
    if (done == hipSuccess) rc = av_launch_gray16_range(src, dst, n_groups, w, h, r, st);
    const hipError_t waited = hipStreamSynchronize(st);
    if (!rc && (done != hipSuccess || waited != hipSuccess)) { av_set_error("av_to_gray8_range: %s", hipGetErrorString(done != hipSuccess ? done : waited)); return AV_E_HIP; }
    return rc;
}
