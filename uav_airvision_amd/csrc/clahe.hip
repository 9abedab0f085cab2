// clahe.hip -- contrast-limited adaptive histogram equalisation of 8-bit images (gfx950).  The definition is written out in
// include/airvision.h (av_clahe); tests/clahe_ref.py states it in NumPy and the kernels are held to it bit for bit.
//   clahe_lut_kernel:   one workgroup per (image, tile): histogram of the tile of the padded image in LDS (one sub-histogram per
//                       wavefront), clip, redistribute, 256-bin prefix sum, 256 bytes out.
//   clahe_apply_kernel: one workgroup per (image, band of rows, chunk of the band).  A band is the set of rows that interpolate between
//                       the same two tile rows; their 2 * tiles_x look-up tables lie in LDS, the pixels go through as whole dwords.
// Both use the 1-D launch of the pyramid kernel: all workgroups of an image run on one XCD, so the tables the first kernel wrote are
// in the L2 the second one reads, and the lines two tiles share are fetched once.
#include "av_common.h"

namespace {

constexpr int CL_ROWS = 16;            // image rows per apply workgroup (a band of th rows is cut into ceil(th / CL_ROWS) chunks)

struct ClaheArgs {
    FramePlace place;                              // (the list on both sides)
    uint8_t* lut;                                  // [n_img][tiles_y * tiles_x][256], by launch image
    int w, h, tiles_x, tiles_y, tw, th;
    int clip;                                      // 0: no clipping
    float scale, inv_tw, inv_th;
    int chunks;                                    // apply: chunks per band
    int dwords;                                    // rows, strides and bases are whole dwords
};

__device__ __forceinline__ uint32_t clahe_round_u8(float v)      // saturate_u8(round half to even)
{
    return (uint32_t)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void clahe_lut_kernel(ClaheArgs a)
{
    __shared__ int hist[4][256];
    __shared__ int part[8];
    const int L = blockIdx.x, wg = L >> 3;
    const int per = a.place.per;
    const int img = (L & 7) + 8 * (wg / per);
    FrameAt f;
    if (img >= a.place.n_img || !av_frame_at(a.place, img, f)) return;
    const int tile = wg % per;
    const int by = tile / a.tiles_x, bx = tile - by * a.tiles_x;
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint8_t* src = f.src;
    for (int i = tid; i < 4 * 256; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    int* my = hist[wave];
    const int x0 = bx * a.tw, y0 = by * a.th;
    const int xe = min(x0 + a.tw, a.w);            // end of the tile's columns that lie inside the image
    int xg = x0;                                   // columns from here on are read one by one, mirrored
    if (a.dwords && x0 < xe) {
        const int d0 = x0 >> 2, nd = ((xe + 3) >> 2) - d0;
        for (int it = tid; it < a.th * nd; it += 256) {
            const int r = it / nd, j = it - r * nd;
            const int yy = av_reflect101_any(y0 + r, a.h);
            const uint32_t q = *reinterpret_cast<const uint32_t*>(src + (size_t)yy * a.w + 4 * (d0 + j));
            const int xb = 4 * (d0 + j);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (xb + b >= x0 && xb + b < xe) atomicAdd(&my[(q >> (8 * b)) & 255u], 1);
        }
        xg = xe;
    }
    const int ng = x0 + a.tw - xg;
    for (int it = tid; it < a.th * ng; it += 256) {
        const int r = it / ng, j = it - r * ng;
        const int yy = av_reflect101_any(y0 + r, a.h), xx = av_reflect101_any(xg + j, a.w);
        atomicAdd(&my[src[(size_t)yy * a.w + xx]], 1);
    }
    __syncthreads();
    int hv = ((hist[0][tid] + hist[1][tid]) + hist[2][tid]) + hist[3][tid];
    const int lane = tid & 63;
    if (a.clip > 0) {
        int ex = max(hv - a.clip, 0);
        hv = min(hv, a.clip);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o);
        if (lane == 0) part[wave] = ex;
        __syncthreads();
        const int clipped = (part[0] + part[1]) + (part[2] + part[3]);
        const int batch = clipped >> 8, residual = clipped - (batch << 8);
        hv += batch;
        if (residual) {
            const int step = max(256 / residual, 1);
            const int k = tid / step;
            if (k * step == tid && k < residual) hv += 1;
        }
    }
    // inclusive prefix sum over the 256 bins: within the wavefront by shuffles, across the four by their totals
    int sum = hv;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(sum, o);
        if (lane >= o) sum += t;
    }
    if (lane == 63) part[4 + wave] = sum;
    __syncthreads();
    for (int v = 0; v < wave; ++v) sum += part[4 + v];
    uint32_t b = clahe_round_u8((float)sum * a.scale);
    b |= (uint32_t)__shfl_down((int)b, 1) << 8;
    b |= (uint32_t)__shfl_down((int)b, 2) << 16;
    if ((tid & 3) == 0) *reinterpret_cast<uint32_t*>(a.lut + ((size_t)img * per + tile) * 256 + tid) = b;
}

// first row whose unclamped upper tile row floor(y / th - 0.5) is >= k, in the kernel's own float arithmetic
__device__ __forceinline__ int clahe_band_start(int k, int th, float inv_th, int h)
{
    if (k < 0) return 0;
    int c = ((2 * k + 1) * th + 1) >> 1;
    if (c > h) c = h;
    while (c > 0 && (int)floorf((float)(c - 1) * inv_th - 0.5f) >= k) --c;
    while (c < h && (int)floorf((float)c * inv_th - 0.5f) < k) ++c;
    return c;
}

__device__ __forceinline__ uint32_t clahe_pixel(const uint8_t* l1, const uint8_t* l2, uint32_t v, int x, const ClaheArgs& a, float ya, float ya1)
{
    const float txf = (float)x * a.inv_tw - 0.5f;
    const float fl = floorf(txf);
    const float xa = txf - fl, xa1 = 1.0f - xa;
    const int t1 = (int)fl;
    const int i1 = max(t1, 0) * 256 + (int)v, i2 = min(t1 + 1, a.tiles_x - 1) * 256 + (int)v;
    const float top = (float)l1[i1] * xa1 + (float)l1[i2] * xa;
    const float bot = (float)l2[i1] * xa1 + (float)l2[i2] * xa;
    return clahe_round_u8(top * ya1 + bot * ya);
}

__global__ __launch_bounds__(256) void clahe_apply_kernel(ClaheArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t luts[];      // [2][tiles_x][256]
    const int L = blockIdx.x, wg = L >> 3;
    const int img = (L & 7) + 8 * (wg / a.place.per);
    FrameAt f;
    if (img >= a.place.n_img || !av_frame_at(a.place, img, f)) return;
    const int sub = wg % a.place.per;
    const int band = sub / a.chunks - 1, chunk = sub - (band + 1) * a.chunks;      // band: the unclamped upper tile row, -1 .. tiles_y - 1
    const int yb = clahe_band_start(band, a.th, a.inv_th, a.h), ye = clahe_band_start(band + 1, a.th, a.inv_th, a.h);
    const int ya0 = yb + chunk * CL_ROWS, ya1r = min(ya0 + CL_ROWS, ye);
    if (ya0 >= ya1r) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint8_t* src = f.src; uint8_t* dst = f.dst;
    const int ty1 = max(band, 0), ty2 = min(band + 1, a.tiles_y - 1);
    const int row_bytes = a.tiles_x * 256;
    {
        const uint4* g1 = reinterpret_cast<const uint4*>(a.lut + ((size_t)img * a.tiles_y + ty1) * row_bytes);
        const uint4* g2 = reinterpret_cast<const uint4*>(a.lut + ((size_t)img * a.tiles_y + ty2) * row_bytes);
        uint4* s = reinterpret_cast<uint4*>(luts);
        const int n16 = row_bytes >> 4;
        for (int i = tid; i < n16; i += 256) { s[i] = g1[i]; s[n16 + i] = g2[i]; }
    }
    __syncthreads();
    const uint8_t* l1 = luts; const uint8_t* l2 = luts + row_bytes;
    for (int y = ya0 + wave; y < ya1r; y += 4) {
        const float tyf = (float)y * a.inv_th - 0.5f;
        const float ya = tyf - floorf(tyf), yaa1 = 1.0f - ya;
        const uint8_t* in = src + (size_t)y * a.w; uint8_t* out = dst + (size_t)y * a.w;
        if (a.dwords) {
            const int nd = a.w >> 2;
            for (int c = lane; c < nd; c += 64) {
                const uint32_t q = reinterpret_cast<const uint32_t*>(in)[c];
                uint32_t o = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) o |= clahe_pixel(l1, l2, (q >> (8 * b)) & 255u, 4 * c + b, a, ya, yaa1) << (8 * b);
                reinterpret_cast<uint32_t*>(out)[c] = o;
            }
        } else {
            for (int x = lane; x < a.w; x += 64) out[x] = (uint8_t)clahe_pixel(l1, l2, in[x], x, a, ya, yaa1);
        }
    }
}

}  // namespace

int av_clahe_check(int w, int h, double clip_limit, int tiles_x, int tiles_y, const char* who)
{
    // w * h <= AV_MAX_IMAGE_PIXELS = 2^24 is what keeps the arithmetic exact: a tile has at most 2^24 pixels (one tile, nothing padded),
    // so every histogram bin, the clipped total and every prefix sum is an int of at most 2^24, and (float)sum is that integer itself;
    // scale = 255.0f / (float)area with (float)area exact as well.  No product of 255 and a count is ever formed in integers.
    if (w <= 0 || h <= 0 || (int64_t)w * h > AV_MAX_IMAGE_PIXELS || tiles_x < 1 || tiles_x > AV_CLAHE_MAX_TILES || tiles_y < 1 || tiles_y > AV_CLAHE_MAX_TILES ||
        !(clip_limit >= 0.0)) {
        av_set_error("%s: CLAHE needs 1 <= tiles <= %d (%d x %d), a clip limit >= 0 (%g) and w * h <= 2^24 (%d x %d)", who, AV_CLAHE_MAX_TILES,
                     tiles_x, tiles_y, clip_limit, w, h);
        return AV_E_INVALID;
    }
    return AV_OK;
}

int av_launch_clahe(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, double clip_limit, int tiles_x, int tiles_y,
                    uint8_t* lut, hipStream_t st)
{
    if (n_groups <= 0) return AV_OK;
    if (src.map != dst.map) { av_set_error("av_clahe: a listed set is read and written through one list"); return AV_E_INVALID; }
    ClaheArgs a;
    memset(&a, 0, sizeof(a));
    a.lut = lut; a.w = w; a.h = h; a.tiles_x = tiles_x; a.tiles_y = tiles_y;
    const int wp = w % tiles_x ? w + tiles_x - w % tiles_x : w, hp = h % tiles_y ? h + tiles_y - h % tiles_y : h;
    a.tw = wp / tiles_x; a.th = hp / tiles_y;
    const int area = a.tw * a.th;
    a.clip = 0;
    if (clip_limit > 0.0) {                    // a limit of the whole tile or more clips nothing: it is held there, inside int
        const double c = clip_limit * area / 256;
        a.clip = c >= (double)area ? area : ((int)c > 1 ? (int)c : 1);
    }
    a.scale = 255.0f / (float)area;
    a.inv_tw = 1.0f / (float)a.tw; a.inv_th = 1.0f / (float)a.th;
    auto al4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; };
    a.dwords = (w & 3) == 0 && (src.stride & 3) == 0 && (dst.stride & 3) == 0 && al4(src.base[0]) && al4(src.base[1]) && al4(dst.base[0]) && al4(dst.base[1]);
    // both kernels interleave eight images over the XCDs; the apply launch is the larger: a launch holds fewer than 2^32 threads
    a.chunks = (a.th + 2 + CL_ROWS - 1) / CL_ROWS;      // a band has th rows, one more or less where 1.0f / th rounds a boundary row across
    const int per_lut = tiles_x * tiles_y, per_apply = (tiles_y + 1) * a.chunks;
    const unsigned n_apply = av_frame_place(&a.place, src, dst, n_groups, per_apply, 8, "av_clahe", w, h, 0xFFFFFFFFll / 256);
    if (!n_apply) return AV_E_INVALID;
    a.place.per = per_lut;
    hipLaunchKernelGGL(clahe_lut_kernel, dim3(n_apply / per_apply * per_lut), dim3(256), 0, st, a);
    AV_LAUNCH_CHECK();
    a.place.per = per_apply;
    hipLaunchKernelGGL(clahe_apply_kernel, dim3(n_apply), dim3(256), (size_t)2 * tiles_x * 256, st, a);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

AV_EXPORT int av_clahe(const uint8_t* img_dev, int64_t img_stride, int n_img, int w, int h, double clip_limit, int tiles_x, int tiles_y,
                       uint8_t* out_dev, int64_t out_stride, uint8_t* lut_dev, void* stream)
{
    int rc = av_clahe_check(w, h, clip_limit, tiles_x, tiles_y, "av_clahe");
    if (rc) return rc;
    if (!img_dev || !out_dev || n_img < 0 || img_stride < (int64_t)w * h || out_stride < (int64_t)w * h) {
        av_set_error("av_clahe: bad arguments (n_img %d, strides %lld / %lld for %d x %d)", n_img, (long long)img_stride, (long long)out_stride, w, h);
        return AV_E_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(lut_dev) & 15) { av_set_error("av_clahe: lut_dev must be 16-byte aligned (the tables are stored and loaded as whole vectors)"); return AV_E_INVALID; }
    if (n_img == 0) return AV_OK;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* lut = lut_dev;
    if (!lut) {
        hipError_t e = hipMallocAsync((void**)&lut, (size_t)n_img * tiles_x * tiles_y * 256, st);
        if (e != hipSuccess) { av_set_error("av_clahe: no memory for the look-up tables (%s)", hipGetErrorString(e)); return AV_E_HIP; }
    }
    rc = av_launch_clahe(av_frames(img_dev, nullptr, img_stride), FrameSet{{out_dev, nullptr}, out_stride, nullptr}, n_img, w, h, clip_limit, tiles_x, tiles_y, lut, st);
    if (!lut_dev) (void)hipFreeAsync(lut, st);
    return rc;
}
