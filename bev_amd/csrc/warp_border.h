// Internal interface of the border-mode warp (warp_border.hip, bevwarp_warp_border): OpenCV's REPLICATE, REFLECT, WRAP,
// REFLECT_101 and TRANSPARENT borders.  BORDER_CONSTANT never comes here: it is bevwarp_warp.  Not installed.
#pragma once
#include "flat_frame.h"

namespace bevwarp {

// OpenCV's values (cv::BorderTypes)
constexpr int kBorderReplicate = 1;
constexpr int kBorderReflect = 2;
constexpr int kBorderWrap = 3;
constexpr int kBorderReflect101 = 4;
constexpr int kBorderTransparent = 5;

struct BorderArgs : FrameArgs {  // (the launch geometry, the destination and the matrices: flat_frame.h)
    const uint8_t* src;
    int64_t src_fs, src_rs;       // bytes
    int src_h, src_w;
    // index remap of the modes that take a remainder: period, an offset (a multiple of the period) that makes every
    // saturated tap index non-negative, and the period's magic -- per axis
    uint32_t per_x, off_x, mag_x, per_y, off_y, mag_y;
    int src_vec_ok;               // 8-bit, 2 / 4 channels: every source pixel is 2- / 4-byte aligned (one load per tap)
};

namespace {
// borderInterpolate(p, n, MODE) in closed form for p in [-32768, 32768] (a saturated index, or one past it):
//   REPLICATE clamp; WRAP p mod n; REFLECT q = p mod 2n, q < n ? q : 2n-1-q; REFLECT_101 q = p mod (2n-2), q < n ? q : 2n-2-q.
// per = the period (n, 2n, 2n - 2; 1 for REFLECT_101 of n == 1, which maps everything to 0), off = a multiple of it that makes
// p + off non-negative, mag = fast_div's magic of per for p + off <= off + 32768.
template <int MODE>
__device__ __forceinline__ int border_index(int p, int n, uint32_t per, uint32_t off, uint32_t mag) {
    if (MODE == kBorderReplicate) return min(max(p, 0), n - 1);
    const uint32_t u = (uint32_t)(p + (int)off);
    const int q = (int)(u - fast_div(u, mag, per) * per);
    if (MODE == kBorderWrap) return q;
    if (MODE == kBorderReflect) return q < n ? q : (int)per - 1 - q;
    return q < n ? q : (int)per - q;  // REFLECT_101
}
}  // namespace

hipError_t launch_warp_border(const BorderArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
