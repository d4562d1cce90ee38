// Internal interface of the lens warp (warp_lens.hip, bevwarp_warp_lens): the perspective warp of frames as a distorted camera
// delivers them -- OpenCV's rational lens model folded into the coordinate chain, BORDER_CONSTANT and BORDER_TRANSPARENT.  The launch
// geometry and the source's layout flag are the border kernel's.  Not installed.
#pragma once
#include "warp_border.h"

namespace bevwarp {

struct LensArgs : BorderArgs {  // (minv holds M_ray: destination pixel -> normalised undistorted camera plane; per_*, off_*, mag_* are unused)
    double lens[12];            // fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 (OpenCV's order)
    double r2_max;              // pixels whose r^2 exceeds it (or is NaN) are outside; +inf: no limit
    float bv_f[4];              // the border value per channel, float32 pixels
    uint32_t bv_u8;             // ... and saturate_cast<uchar> of it, packed: byte k = channel k
};

hipError_t launch_warp_lens(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream);
// ... under BEVWARP_LENS_FISHEYE (warp_fisheye.hip): lens holds fx, fy, cx, cy, k1, k2, k3, k4 and four zeros, r2_max holds theta_max
hipError_t launch_warp_fisheye(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream);

}  // namespace bevwarp
