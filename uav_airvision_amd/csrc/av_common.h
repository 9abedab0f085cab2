// av_common.h -- shared declarations of libairvision_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/airvision.h"

#define AV_EXPORT extern "C" __attribute__((visibility("default")))

// ---- error plumbing ---------------------------------------------------------------------------
#include "av_resources.h"          // av_set_error, AV_HIP; the owner of device memory, pinned memory, events and streams
#define AV_LAUNCH_CHECK()                                                                         \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess) {                                                                   \
            av_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
            return AV_E_HIP;                                                                      \
        }                                                                                         \
    } while (0)

// ---- pyramid geometry passed by value to kernels ----------------------------------------------
struct PyrGeom {
    int levels;
    int w[AV_MAX_LEVELS], h[AV_MAX_LEVELS], pitch[AV_MAX_LEVELS];
    int off[AV_MAX_LEVELS];      // byte offset of padded (0,0) of each level (fits int)
};
PyrGeom av_make_geom(const av_pyr_layout& l);

// ---- camera model, by value -------------------------------------------------------------------
struct CamModel {
    double fx, fy, cx, cy, k1, k2, p1, p2;       // equidistant: k1, k2, p1, p2 hold the model's k1 .. k4
    int model;                                    // AV_DISTORTION_RADTAN (0) / AV_DISTORTION_EQUIDISTANT (1)
};

// packed FAST keypoint word: score << B | (2^B - 1 - raster), B = the raster bits of the launch.  B = 19 is the documented format of
// av_fast_detect and what the engine uses for images of up to 2^19 pixels; B = 24 (av_fast_detect_wide, larger engines) holds any
// raster below AV_MAX_IMAGE_PIXELS.  A FAST score is at most 254, so the largest 24-bit word is 0xFEFFFFFF: every word lies strictly
// between the two sentinels of the selection loops, 0 and 0xFFFFFFFF (a word is 0 only for score 0 at the last pixel, which lies in the
// 3-pixel border and is never a corner).  Words order by (score, then raster descending) in either format.
#define AV_KP_RASTER_BITS 19
#define AV_KP_RASTER_BITS_WIDE 24
static_assert((1 << AV_KP_RASTER_BITS_WIDE) == AV_MAX_IMAGE_PIXELS, "the wide keypoint word holds every raster of the largest image");
static_assert(((254ull << AV_KP_RASTER_BITS_WIDE) | ((1ull << AV_KP_RASTER_BITS_WIDE) - 1ull)) < 0xFFFFFFFFull, "the largest keypoint word stays below the sentinel");
inline int av_kp_raster_bits(int w, int h) { return (int64_t)w * h <= (1 << AV_KP_RASTER_BITS) ? AV_KP_RASTER_BITS : AV_KP_RASTER_BITS_WIDE; }

// ---- draw hash of the two-point RANSAC (written out in include/airvision.h; host and device) ---
#ifdef __HIPCC__
#define AV_HD __host__ __device__
#else
#define AV_HD
#endif
AV_HD inline uint32_t av_ransac_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
AV_HD inline uint32_t av_ransac_hash_inl(uint32_t seed, uint32_t frame, uint32_t camera, uint32_t k, uint32_t draw)
{
    return av_ransac_mix(av_ransac_mix(av_ransac_mix(seed + 0x9e3779b9u) ^ frame) ^ (camera << 16 | k << 1 | draw));
}

#ifdef __HIPCC__
// cv::borderInterpolate(p, len, BORDER_REFLECT_101) for |overshoot| < len
__device__ __forceinline__ int av_reflect101(int p, int len)
{
    if (p < 0) p = -p;
    if (p >= len) p = 2 * len - 2 - p;
    return p;
}
// the same for any overshoot (cv::borderInterpolate loops): the general LK kernel's windows reach win + 1 pixels past a level
// that may be only win + 1 pixels wide
__device__ __forceinline__ int av_reflect101_any(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do { p = p < 0 ? -p : 2 * len - 2 - p; } while ((unsigned)p >= (unsigned)len);
    return p;
}

// cv2.undistortPoints core: 5 fixed-point iterations of the radtan inverse, then R*[x y 1].
// Expression order follows OpenCV's cvUndistortPointsInternal; fp64, no contraction.
// cv2.fisheye.undistortPoints core (camera_model.py:41-43): Newton's method on theta (1 + k1 theta^2 + ...) = theta_d, at most 10 steps,
// eps 1e-8 (OpenCV 4.x fisheye.cpp, default TermCriteria), then scale = tan(theta) / theta_d and R * [x y 1].  Parity unpinned
// (the CPU checker holds the same restatement; tan from the device math library vs libm: a few ulp).
__device__ __forceinline__ void av_undistort_fisheye(const CamModel& c, const double* R, double u, double v, double& ox, double& oy)
{
    const double pwx = (u - c.cx) / c.fx, pwy = (v - c.cy) / c.fy;
    const double half_pi = 3.1415926535897932384626433832795 / 2.;
    double theta_d = sqrt(pwx * pwx + pwy * pwy);
    theta_d = fmin(fmax(-half_pi, theta_d), half_pi);
    bool converged = false;
    double theta = theta_d, scale = 0.0;
    if (fabs(theta_d) > 1e-8) {
#pragma unroll 1
        for (int j = 0; j < 10; ++j) {
            const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta6 * theta2;
            const double k0_theta2 = c.k1 * theta2, k1_theta4 = c.k2 * theta4, k2_theta6 = c.p1 * theta6, k3_theta8 = c.p2 * theta8;
            const double theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                     (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabs(theta_fix) < 1e-8) { converged = true; break; }
        }
        scale = tan(theta) / theta_d;
    } else {
        converged = true;
    }
    const bool flipped = (theta_d < 0 && theta > 0) || (theta_d > 0 && theta < 0);
    if (converged && !flipped) {
        const double pux = pwx * scale, puy = pwy * scale;
        const double xx = R[0] * pux + R[1] * puy + R[2];
        const double yy = R[3] * pux + R[4] * puy + R[5];
        const double ww = R[6] * pux + R[7] * puy + R[8];
        ox = xx / ww; oy = yy / ww;
    } else {
        ox = -1000000.0; oy = -1000000.0;
    }
}
// cv2.fisheye.distortPoints (camera_model.py:69-70), alpha = 0
__device__ __forceinline__ void av_distort_fisheye(const CamModel& c, double x, double y, double& ou, double& ov)
{
    const double r2 = x * x + y * y, r = sqrt(r2);
    const double theta = atan(r);
    const double theta2 = theta * theta, theta3 = theta2 * theta, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const double theta_d = theta + c.k1 * theta3 + c.k2 * theta5 + c.p1 * theta7 + c.p2 * theta9;
    const double inv_r = r > 1e-8 ? 1.0 / r : 1;
    const double cdist = r > 1e-8 ? theta_d * inv_r : 1;
    ou = x * cdist * c.fx + c.cx;
    ov = y * cdist * c.fy + c.cy;
}

__device__ __forceinline__ void av_undistort(const CamModel& c, const double* R, double u, double v, double& ox, double& oy)
{
    if (c.model == 1) { av_undistort_fisheye(c, R, u, v, ox, oy); return; }
    const double ifx = 1. / c.fx, ify = 1. / c.fy;
    double x = (u - c.cx) * ifx, y = (v - c.cy) * ify;
    const double x0 = x, y0 = y;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        double r2 = x * x + y * y;
        double icdist = 1. / (1 + ((0 * r2 + c.k2) * r2 + c.k1) * r2);
        if (icdist < 0) { x = (u - c.cx) * ifx; y = (v - c.cy) * ify; break; }
        double deltaX = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
        double deltaY = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    double xx = R[0] * x + R[1] * y + R[2];
    double yy = R[3] * x + R[4] * y + R[5];
    double ww = 1. / (R[6] * x + R[7] * y + R[8]);
    ox = xx * ww;
    oy = yy * ww;
}

// cv2.projectPoints with zero rvec/tvec on (x, y, 1): radtan forward + K.
__device__ __forceinline__ void av_distort(const CamModel& c, double x, double y, double& ou, double& ov)
{
    if (c.model == 1) { av_distort_fisheye(c, x, y, ou, ov); return; }
    double r2 = x * x + y * y, r4 = r2 * r2;
    double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    double cdist = 1 + c.k1 * r2 + c.k2 * r4;
    double xd = x * cdist + c.p1 * a1 + c.p2 * a2;
    double yd = y * cdist + c.p1 * a3 + c.p2 * a1;
    ou = xd * c.fx + c.cx;
    ov = yd * c.fy + c.cy;
}
#endif  // __HIPCC__

// ---- kernel launchers (defined in the .hip files, used by ops_api and the engine) -------------
// Where one camera's frames lie for an LK or FAST launch: set (LK) / image (FAST) s is storage entry e = map ? map[s] : s.
struct ImgView {
    const uint8_t* pyr; int64_t pyr_stride;      // padded pyramid of entry e at pyr + e * pyr_stride
    const uint8_t* img; int64_t img_stride;      // level 0 read in place, w-pitched, at img + e * img_stride; null: level 0 of the pyramid
    const int* map;                              // shared frame store (LK: a negative entry = the set has no frame in this step); or null
};

// Where the frames of one stage of the input chain lie (the producer side of ImgView): camera c of group g at base[c] + e * stride
// bytes with e = map ? map[g] : g; base[1] null = one camera.  A launcher reads its source set and writes its destination set, and
// a launch has ONE list, its destination's.  A group whose entry is negative is skipped.  A source without a map is read at
// g * stride (conversion, binning, range scaling, photometric out of the caller's frames); a source with a map -- always the
// destination's own -- is read at e like the destination (photometric in place in a listed set, CLAHE, the pyramid; the last two are
// handed no negative entry).  This is the whole rule; FramePlace / av_frame_at below are its one implementation.
struct FrameSet {
    uint8_t* base[2]; int64_t stride;
    const int* map;                              // device, one int per group; or null
};
// (a set that is only read may be made from const pointers: nothing writes through a launcher's source)
inline FrameSet av_frames(const uint8_t* b0, const uint8_t* b1, int64_t stride, const int* map = nullptr)
{
    return FrameSet{{const_cast<uint8_t*>(b0), const_cast<uint8_t*>(b1)}, stride, map};
}

// The device side of a (src, dst) pair of FrameSets, by value: the first member of every input stage's argument record.  Image i of
// a launch is camera i % n_src of group i / n_src; how a kernel maps blockIdx.x onto (image, block of the image) is its own.
struct FramePlace {
    const uint8_t* src0; const uint8_t* src1;
    uint8_t* dst0; uint8_t* dst1;
    int64_t src_stride, dst_stride;              // bytes between the groups of one camera
    const int* index;                            // the destination's list, or null
    int n_src;                                   // 1 or 2
    int src_listed;                              // the source has the list too
    int n_img;                                   // n_groups * n_src
    int per;                                     // workgroups per image (of the kernel launched)
};
// Fills p and returns the workgroups of the launch, per * n_img with n_img rounded up to a multiple of img_round (8 for the kernels
// that interleave eight images over the XCDs); 0 with the error set (who, w x h in the text) if that is more than max_wg.
inline unsigned av_frame_place(FramePlace* p, const FrameSet& src, const FrameSet& dst, int n_groups, int per, int img_round,
                               const char* who, int w, int h, int64_t max_wg = 0x7FFFFFFFll)
{
    p->src0 = src.base[0]; p->src1 = src.base[1]; p->dst0 = dst.base[0]; p->dst1 = dst.base[1];
    p->src_stride = src.stride; p->dst_stride = dst.stride; p->index = dst.map;
    p->n_src = src.base[1] ? 2 : 1; p->src_listed = src.map != nullptr; p->n_img = n_groups * p->n_src; p->per = per;
    const int64_t n_wg = (int64_t)per * ((p->n_img + img_round - 1) / img_round * img_round);
    if (n_wg > max_wg) { av_set_error("%s: %d images of %d x %d are more than one launch holds", who, p->n_img, w, h); return 0u; }
    return (unsigned)n_wg;
}
#ifdef __HIPCC__
// storage entry of group g; negative: the group is skipped
__device__ __forceinline__ int64_t av_frame_entry(const FramePlace& p, int g) { return p.index ? p.index[g] : g; }
// image img of the launch: its camera, its group and where it is read and written; false = its group is skipped
struct FrameAt { int cam, g; const uint8_t* src; uint8_t* dst; };
__device__ __forceinline__ bool av_frame_at(const FramePlace& p, int img, FrameAt& f)
{
    f.cam = img % p.n_src; f.g = img / p.n_src;
    const int64_t e = av_frame_entry(p, f.g);
    if (e < 0) return false;
    f.src = (f.cam ? p.src1 : p.src0) + (p.src_listed ? e : (int64_t)f.g) * p.src_stride;
    f.dst = (f.cam ? p.dst1 : p.dst0) + e * p.dst_stride;
    return true;
}
#endif

// The vector bodies of the input stages (stream_pass.h, bayer.hip, downscale.hip, the histogram of range16.hip) load and store whole
// 16-byte vectors: every base, and every stride that is applied, has to be a multiple of 16.  One group at its own place (no list)
// applies no stride.  The width condition of each kernel stays with its launcher.
inline bool av_frames_vec16(const FrameSet& src, const FrameSet& dst, int n_groups)
{
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool strides16 = (n_groups == 1 && !src.map && !dst.map) || ((src.stride & 15) == 0 && (dst.stride & 15) == 0);
    return strides16 && al16(src.base[0]) && al16(src.base[1]) && al16(dst.base[0]) && al16(dst.base[1]);
}
// n frames of in_bytes at in + i * in_stride against n of out_bytes at out + i * out_stride: do the two spans share a byte?  (The
// refusal of the operators that do not work in place.)
inline bool av_spans_overlap(const void* in, int64_t in_stride, int64_t in_bytes, const void* out, int64_t out_stride, int64_t out_bytes, int n)
{
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + (uint64_t)(n - 1) * in_stride + in_bytes;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uint64_t)(n - 1) * out_stride + out_bytes;
    return o0 < i1 && i0 < o1;
}

// pyramid.hip: the pyramids of n_groups images of one camera or of two (img: read in place, its map is also the list of the pyramid
// side: group i reads / writes storage entry img.map[i] of the image and pyramid arrays)
int av_launch_pyramid(const FrameSet& img, int n_groups,
                      const PyrGeom& g, uint8_t* pyr_base, int64_t stream_stride, int64_t slot_stride, int slot0, int slot1,
                      hipStream_t st, bool write_level0 = true, bool* wrote_level0 = nullptr);
// write_level0 = false: levels 1.. only, level 0 stays the caller's image (honoured by the fused kernel; *wrote_level0 tells)

// lk.hip
struct LKParams {
    int win, max_iter;
    double eps2, min_eig;
};
// I -> J; the two views share one pyramid stride (LKArgs::stream_stride)
int av_launch_lk(const ImgView& I, const ImgView& J, int n_set, const PyrGeom& g,
                 const float* prev, float* next, uint8_t* status, const int* count, int cap, int launch_pts,
                 const LKParams& p, hipStream_t st, const int* index = nullptr);

// fast.hip
constexpr int AV_FAST_TW = 64, AV_FAST_TH = 48;                      // the detector's tile: tile (x / TW, y / TH), row-major, holds pixel (x, y)
void av_fast_tiles(int w, int h, int* tiles, int* tile_cap);         // tile count of a w x h image, entries per tile list
// scans src.img in place, or -- src.img null -- the interior of level 0 of src.pyr with its AV_PYR_BORDER-pixel frame (g: its geometry;
// may be null when src.img is given); image i of the launch is storage entry src.map[i] of the image, the mask and the lists
// raster_bits: AV_KP_RASTER_BITS (w * h <= 2^19) or AV_KP_RASTER_BITS_WIDE (w * h <= AV_MAX_IMAGE_PIXELS): the format of the words written
int av_launch_fast(const ImgView& src, const PyrGeom* g, const uint8_t* mask, int64_t mask_stride,
                   int n_img, int w, int h, int threshold, int raster_bits,
                   uint32_t* kp, int* count, int cap,                               // flat output (ops API) or NULL
                   uint32_t* tile_kp, int* tile_count,                              // per-tile output (front-end engine) or NULL
                   int* overflow, int stat_stride, hipStream_t st);

// ransac.hip: the engine's outlier-rejection stage (AV_FE_RANSAC), one single-wavefront workgroup per stream: both camera problems,
// ordered compaction of cur_* to the survivors, cur_count, counts[s][4]
struct RansacStage {
    int S, NT, MAXF;
    CamModel cam[2];
    const float* prev_p0; const float* prev_p1;      // the previous grid [S][MAXF][2]
    long long* cur_id; int* cur_life; float* cur_p0; float* cur_p1; int* cur_cell; const int* cur_src; int* cur_count;
    const double* Rpc;                               // [S][2][9]: cam0_R_p_c, cam1_R_p_c
    const int* frame_no;                             // [S]
    const int* slot_cur;                             // frame-store step: < 0 = the stream idles (null otherwise)
    int* counts;                                     // [S][4]
    double thr; int N; uint32_t seed;
};
int av_launch_ransac_stage(const RansacStage& a, hipStream_t st);

// clahe.hip: equalise n_groups images of one camera or of two (FrameSet; the list on both sides).  dst may be src.
// lut: [n_groups * cameras][tiles_y * tiles_x][256] scratch (the look-up tables of the launch, camera-minor).
// av_clahe_check: the argument limits of av_clahe, with `who` in the text.
int av_clahe_check(int w, int h, double clip_limit, int tiles_x, int tiles_y, const char* who);
int av_launch_clahe(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, double clip_limit, int tiles_x, int tiles_y,
                    uint8_t* lut, hipStream_t st);

// pixfmt.hip: n_groups frames of one camera or of two, of pixel format fmt (AV_PIX_*, not GRAY8), to tightly packed 8-bit grey
// (FrameSet; the list on the destination only, a negative entry skips the group).  Never in place.
// av_pixfmt_bytes: bytes per pixel, 0 = unknown format; av_pixfmt_check: the limits of format and shift, with `who` in the text.
// Packed 10 / 12-bit transports have no whole bytes per pixel (av_pixfmt_bytes gives 0 for them as for an unknown code): they are
// known by av_pixfmt_packed_depth (10 / 12; 0 = not packed), av_pixfmt_packed_csi2 (MIPI CSI-2 byte order instead of PFNC "p") and sized
// by av_pixfmt_frame_bytes (include/airvision.h), which is what sizes a frame of ANY format.  av_pixfmt_is_bayer: a mosaic, packed or
// not (its pattern is fmt & 3).  av_pixfmt_name: config.image_format's name of a code (a thread-local text).  av_pixfmt_check_size: a
// packed format's rows are whole groups, with `who` and the format's name in the text.
// A packed mosaic is converted in two passes and needs `mosaic`, a scratch set of n_groups frames of w * h bytes per camera (no list).
int av_pixfmt_bytes(int fmt);
int av_pixfmt_packed_depth(int fmt);
bool av_pixfmt_packed_csi2(int fmt);
bool av_pixfmt_is_bayer(int fmt);
const char* av_pixfmt_name(int fmt);
int av_pixfmt_check(int fmt, int shift, const char* who);
int av_pixfmt_check_size(int fmt, int w, int h, const char* who);
int av_launch_to_gray8(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, int fmt, int shift, hipStream_t st, const FrameSet* mosaic = nullptr);
// packed.hip: the same for the packed transports, every sample reduced to 8 bits (a packed mosaic: its reduced 8-bit mosaic)
int av_launch_unpack_to_gray8(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, int fmt, int shift, hipStream_t st);
// bayer.hip: the same for the Bayer mosaic formats (AV_PIX_BAYER_*), w >= 2 and h >= 2; av_launch_to_gray8 hands them on
int av_launch_bayer_to_gray8(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, int fmt, int shift, hipStream_t st);
// downscale.hip: 2 x 2 / 4 x 4 binning (f = 2 or 4) of n_groups tightly packed W x H grey frames of one camera or of two into tightly
// packed (W / f) x (H / f) ones; W % f == 0 and H % f == 0.  Sets and list as av_launch_to_gray8.  Never in place.
int av_launch_downscale(const FrameSet& src, const FrameSet& dst, int n_groups, int W, int H, int f, hipStream_t st);
// photometric.hip: photometric calibration of n_groups tightly packed w x h grey frames of one camera or of two ("Photometric
// calibration" in include/airvision.h): out = min(255, (resp[p] * gain[x] + 2^19) >> 20), resp* [256] Q8 and gain* [w * h] Q12 on the
// device, one per camera, null = that part is the identity (at least one part is given; cameras that differ in their parts take one
// launch each).  Sets and list as av_launch_to_gray8 -- the destination's list, a negative entry skips the group -- but dst may be src:
// a source with a list (the destination's own) is read through it, which is the in-place call on a listed set.
// k0 / k1: the exposure factors of the launch ("Exposure-time normalisation"), uint16 [n_groups] Q12 on the device, by GROUP of the
// launch (not by entry of a list), one array per camera; null = off (both or neither for two cameras).  With them no table is required.
int av_launch_photometric(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, const uint16_t* resp0, const uint16_t* resp1,
                          const uint16_t* gain0, const uint16_t* gain1, const uint16_t* k0, const uint16_t* k1, hipStream_t st);
// range16.hip: n_groups 16-bit grey frames of one camera or of two to tightly packed 8-bit grey through a window instead of a shift
// ("Range scaling of 16-bit grey" in include/airvision.h).  Sets and list as av_launch_to_gray8 -- the destination's list, a negative
// entry skips the group (its histogram, its record and its pixels).  A group is the images of one FrameSet group: the two cameras'
// frames are pooled into one histogram and share one record.  AV_GRAY16_AUTO: hist [n_groups][4096] is zero on entry and zero again when
// the launches have run, rec [n_groups][4] receives {lo, hi, m, 0} by group (not by entry); AV_GRAY16_WINDOW reads neither.  range_out
// (or null): int32 [n_groups][2], (lo, hi) of every group that is written.  Three launches (one for a window) on st, no host wait.
// av_range16_check: the limits of the settings a mode reads, with `who` in the text.
struct Range16 {
    int mode, lo, hi, ppm_lo, ppm_hi, min_span;
    uint32_t* hist; uint32_t* rec; int32_t* range_out;
};
int av_range16_check(int mode, int lo, int hi, int ppm_lo, int ppm_hi, int min_span, const char* who);
int av_launch_gray16_range(const FrameSet& src, const FrameSet& dst, int n_groups, int w, int h, const Range16& r, hipStream_t st);
