// Internal interface of the border-mode warp (warp_border.hip, bevwarp_warp_border): OpenCV's REPLICATE, REFLECT, WRAP,
// REFLECT_101 and TRANSPARENT borders.  BORDER_CONSTANT never comes here: it is bevwarp_warp.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevwarp {

// OpenCV's values (cv::BorderTypes)
constexpr int kBorderReplicate = 1;
constexpr int kBorderReflect = 2;
constexpr int kBorderWrap = 3;
constexpr int kBorderReflect101 = 4;
constexpr int kBorderTransparent = 5;

// One destination row segment of 4 pixels per lane, a wave per row, four rows per workgroup; the grid is flat:
// item t -> frame t / tiles_per_frame, tile (t mod tiles_per_frame) -> (tile row, tile column).
constexpr int kBorderPPL = 4;
constexpr int kBorderTileW = 64 * kBorderPPL;
constexpr int kBorderTileH = 4;

struct BorderArgs {
    const uint8_t* src;
    uint8_t* dst;
    const double* minv;           // device, inverse matrices
    int64_t src_fs, src_rs;       // bytes
    int64_t dst_fs, dst_rs;
    int src_h, src_w, dst_h, dst_w;
    int m_stride;                 // 9 (one matrix per frame) or 0 (shared)
    int bw0;                      // evaluation block width of the reference algorithm
    int tiles_x, tiles_per_frame;
    uint32_t bw0_magic, tx_magic, tpf_magic;  // fast_div magics (0 = divide)
    // index remap of the modes that take a remainder: period, an offset (a multiple of the period) that makes every
    // saturated tap index non-negative, and the period's magic -- per axis
    uint32_t per_x, off_x, mag_x, per_y, off_y, mag_y;
    int dst_vec_ok;               // destination layout admits the wide stores (the rule of bevwarp_warp)
    int src_vec_ok;               // 8-bit, 2 / 4 channels: every source pixel is 2- / 4-byte aligned (one load per tap)
};

hipError_t launch_warp_border(const BorderArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
