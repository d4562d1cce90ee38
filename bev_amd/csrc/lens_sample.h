// lens_sample.h -- what the two lens warps (warp_lens.hip: OpenCV's rational model; warp_fisheye.hip: the equidistant one) share from the
// lens step on: the sampler that guards each tap against the frame and the inlier's sampler.  (The kernels' body is lens_lane.inc.)  The
// frame is flat_frame.h, the blend lens_pixel.h.
#pragma once
#include "warp_lens.h"
#include "lens_pixel.h"

namespace bevwarp {
namespace {

// (Args: kernel arguments with the source's sides and strides and the border pixel bv_u8 / bv_f -- LensArgs, or the supersampled warp's)
template <typename T, int C, class Args>
__device__ __forceinline__ Pixel<T, C> border_pixel(const Args& a) {
    Pixel<T, C> p;
    if constexpr (sizeof(T) == 1) {
        p.packed = a.bv_u8;
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = a.bv_f[k];
    }
    return p;
}

// an inlier's taps: all four are source pixels
template <typename T, int C, int INTERP>
__device__ __forceinline__ Pixel<T, C> sample_inside(const uint8_t* __restrict__ frame, int64_t rs, int sx, int sy, int fx, int fy, bool vec) {
    const uint8_t* r0 = frame + (int64_t)sy * rs;
    if (INTERP == kNearest) return load_pixel<T, C>(r0, sx, vec);
    const uint8_t* r1 = r0 + rs;
    return blend_taps<T, C>(load_pixel<T, C>(r0, sx, vec), load_pixel<T, C>(r0, sx + 1, vec), load_pixel<T, C>(r1, sx, vec), load_pixel<T, C>(r1, sx + 1, vec), fx, fy);
}

// The constant border: a tap inside the frame is its pixel, a tap outside -- every tap of an invalid pixel -- the border pixel; a pixel
// whose four taps are all outside is the border value itself.  Every tap is loaded from the CLAMPED position (always a source pixel, also
// for the lanes past the row's end) and replaced afterwards, so the loads are unconditional and all issue before the first wait.
template <typename T, int C, int INTERP, class Args>
__device__ __forceinline__ Pixel<T, C> sample_guarded(const Args& a, const uint8_t* __restrict__ frame, int sx, int sy, int fx, int fy, bool valid, bool vec) {
    const Pixel<T, C> b = border_pixel<T, C>(a);
    const int w = a.src_w, h = a.src_h;
    const bool xin0 = (unsigned)sx < (unsigned)w, yin0 = (unsigned)sy < (unsigned)h;
    const int cx0 = min(max(sx, 0), w - 1), cy0 = min(max(sy, 0), h - 1);
    const uint8_t* r0 = frame + (int64_t)cy0 * a.src_rs;
    if (INTERP == kNearest) {
        const Pixel<T, C> p = load_pixel<T, C>(r0, cx0, vec);
        return (valid && xin0 && yin0) ? p : b;
    }
    const bool xin1 = (unsigned)(sx + 1) < (unsigned)w, yin1 = (unsigned)(sy + 1) < (unsigned)h;
    const int cx1 = min(max(sx + 1, 0), w - 1), cy1 = min(max(sy + 1, 0), h - 1);
    const uint8_t* r1 = frame + (int64_t)cy1 * a.src_rs;
    const Pixel<T, C> t00 = load_pixel<T, C>(r0, cx0, vec), t01 = load_pixel<T, C>(r0, cx1, vec);
    const Pixel<T, C> t10 = load_pixel<T, C>(r1, cx0, vec), t11 = load_pixel<T, C>(r1, cx1, vec);
    const Pixel<T, C> out = blend_taps<T, C>((valid && xin0 && yin0) ? t00 : b, (valid && xin1 && yin0) ? t01 : b, (valid && xin0 && yin1) ? t10 : b,
                                             (valid && xin1 && yin1) ? t11 : b, fx, fy);
    // (8-bit pixels: the blend of four border pixels is the border pixel)
    const bool all_out = !valid || !(xin0 || xin1) || !(yin0 || yin1);
    return (sizeof(T) == 4 && all_out) ? b : out;
}

}  // namespace
}  // namespace bevwarp
