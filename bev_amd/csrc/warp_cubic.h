// Internal interface of the bicubic warp (warp_cubic.hip; BEVWARP_CUBIC through bevwarp_warp and bevwarp_warp_border), all six
// border modes, BORDER_CONSTANT included.  The launch geometry and the layout flags are the border kernel's.  Not installed.
#pragma once
#include "warp_border.h"

namespace bevwarp {

struct CubicArgs : BorderArgs {  // (per_*, off_*, mag_*: cubic::window_period -- the 4-tap window reaches one index further than a saturated one)
    float cv_f[4];               // the border value per channel (BORDER_CONSTANT; 0 for every other mode), float32 pixels
    int cv_u8[4];                // ... and saturate_cast<uchar> of it, 8-bit pixels
    // (as cubic_sample.h's sampler takes the border value from either args struct)
    __device__ __forceinline__ int cv_int(int k) const { return cv_u8[k]; }
    __device__ __forceinline__ float cv_float(int k) const { return cv_f[k]; }
};

hipError_t launch_warp_cubic(const CubicArgs& a, int dtype, int channels, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
