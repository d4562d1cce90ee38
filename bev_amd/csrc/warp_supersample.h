// Internal interface of the supersampled warp (warp_supersample.hip, bevwarp_warp_border under BEVWARP_SUPERSAMPLE_*): every destination
// pixel is the average of the k x k pixels that bevwarp_warp_border writes on the k times finer grid.  The launch geometry is the border
// kernel's on the DESTINATION grid; bw0 and its magic describe the FINE grid's evaluation blocks.  Not installed.
#pragma once
#include "warp_border.h"

namespace bevwarp {

constexpr int kBorderConstant = 0;  // (cv::BORDER_CONSTANT: here a mode of the kernel, not a delegation to bevwarp_warp)

struct SupersampleArgs : BorderArgs {  // (per_*, off_*, mag_* are unused by the constant border)
    double inv_k, centre;       // 1 / k and c = (1 - k) / (2 k): the fine matrix's two constants, both exact
    int log2k;                  // 1, 2, 3
    float bv_f[4];              // the border value per channel, float32 pixels
    uint32_t bv_u8;             // ... and saturate_cast<uchar> of it, packed: byte k = channel k
};

hipError_t launch_warp_supersample(const SupersampleArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
