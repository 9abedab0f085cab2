// stream_pass.h -- the one kernel of the input stages that are pure streaming passes (gfx950): pixfmt.hip, packed.hip, photometric.hip
// and the apply pass of range16.hip.  An image is one run of npix output pixels (rows are tightly packed on both sides); a 256-thread
// workgroup takes 256 lane spans of it; no lane reads what another writes, so a pass whose operation allows it is correct in place.
//   aligned body   a.vec: every base, and every stride that is applied, is a whole 16-byte vector (av_frames_vec16; an operation
//                  with more vector operands adds them to the rule).  A lane owns one span -- whole vectors on both sides, lane i's
//                  after lane i - 1's -- and Op::span() takes it with vector loads and stores.  The ragged end of the image, less
//                  than a span, is taken unit by unit by the one lane it falls to.
//   unit-wise      every other launch: one unit per lane and round, neighbouring lanes on neighbouring units, byte loads and stores.
// Which image and which block of it a workgroup takes is blockIdx.x split image-major (id = image * per + block) or image-minor
// (id = block * n_img + image); where the image lies is av_frame_at (av_common.h).  All byte offsets are 64-bit: 2^24 pixels x 4 B x
// thousands of streams passes 2^32.
//
// An operation Op provides
//   Args                 the kernel's argument record: `FramePlace place; int npix, vec;` and whatever is its own
//   SPAN, UNIT           output pixels of a lane's span (a multiple of 16) and of the indivisible unit (1, or a packed group; an
//                        image is whole units)
//   UNROLL               rounds of the unit-wise loop that are unrolled together (SPAN / UNIT rounds in all)
//   IMAGE_MINOR          the workgroup order
//   Op(a, f, blk, tid)   its state for the workgroup's image (every lane of the workgroup constructs it: it may hold a barrier)
//   span(src, dst, p)    pixels p .. p + SPAN - 1 of the image at src / dst, p a multiple of SPAN
//   unit(src, dst, u)    unit u of it: pixels u * UNIT .. u * UNIT + UNIT - 1
#pragma once
#include "av_common.h"

template <typename Op>
__global__ __launch_bounds__(256) void stream_pass_kernel(typename Op::Args a)
{
    int img, blk;
    if (Op::IMAGE_MINOR) { blk = blockIdx.x / a.place.n_img; img = blockIdx.x - blk * a.place.n_img; }
    else { img = blockIdx.x / a.place.per; blk = blockIdx.x - img * a.place.per; }
    FrameAt f;
    if (!av_frame_at(a.place, img, f)) return;
    const int tid = threadIdx.x;
    const Op op(a, f, blk, tid);
    const int p0 = blk * (256 * Op::SPAN);                        // < 2^24
    const int n_unit = a.npix / Op::UNIT;
    if (a.vec) {
        const int p = p0 + tid * Op::SPAN;
        if (p + Op::SPAN <= a.npix) op.span(f.src, f.dst, p);
        else for (int u = p / Op::UNIT; u < n_unit; ++u) op.unit(f.src, f.dst, u);      // the image's ragged end: one lane, less than a span
        return;
    }
    const int u0 = p0 / Op::UNIT;
#pragma unroll Op::UNROLL
    for (int j = 0; j < Op::SPAN / Op::UNIT; ++j) {
        const int u = u0 + j * 256 + tid;
        if (u < n_unit) op.unit(f.src, f.dst, u);
    }
}
