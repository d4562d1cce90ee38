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

hipError_t launch_warp_border(const BorderArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
