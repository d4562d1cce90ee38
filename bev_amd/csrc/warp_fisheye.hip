// warp_fisheye.hip -- bevwarp_warp_lens under BEVWARP_LENS_FISHEYE: the lens warp (warp_lens.hip) with the equidistant lens step where the
// rational one stood -- destination pixel -> ray in the camera's frame (M_ray, NOT divided by its depth: a ray at or beyond 90 degrees from
// the optical axis is a pixel like any other) -> angle -> raw pixel -> one sample.  The same formats, borders, frame (flat_frame.h),
// samplers and lane (lens_sample.h); the step is fisheye_pixel.h.  See DESIGN.md section 4.23.
// a.lens: fx, fy, cx, cy, k1..k4, four zeros; a.r2_max carries theta_max.  Wave-uniform, in scalar registers.
#include "lens_sample.h"
#include "fisheye_pixel.h"

namespace bevwarp {
namespace {

template <typename T, int C, int INTERP, bool TRANSPARENT>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_fisheye_kernel(const LensArgs a) {
#define BEVWARP_LENS_STEP fisheye_pixel
#include "lens_lane.inc"
#undef BEVWARP_LENS_STEP
}

template <typename T, int INTERP, bool TRANSPARENT>
void launch_c(const LensArgs& a, int channels, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    switch (channels) {
        case 1: hipLaunchKernelGGL((warp_fisheye_kernel<T, 1, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((warp_fisheye_kernel<T, 2, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((warp_fisheye_kernel<T, 3, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((warp_fisheye_kernel<T, 4, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
    }
}

template <typename T, int INTERP>
void launch_mode(const LensArgs& a, int channels, bool transparent, dim3 grid, hipStream_t stream) {
    if (transparent)
        launch_c<T, INTERP, true>(a, channels, grid, stream);
    else
        launch_c<T, INTERP, false>(a, channels, grid, stream);
}

}  // namespace

hipError_t launch_warp_fisheye(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    if (dtype == 0)
        (interp == kNearest ? launch_mode<uint8_t, kNearest> : launch_mode<uint8_t, kLinear>)(a, channels, transparent, grid, stream);
    else
        (interp == kNearest ? launch_mode<float, kNearest> : launch_mode<float, kLinear>)(a, channels, transparent, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
