// warp_lens.hip -- the perspective warp of frames as a distorted camera delivers them (bevwarp_warp_lens): destination pixel ->
// normalised undistorted camera plane (M_ray) -> OpenCV's rational lens model -> one sample from the raw frame.  8-bit and float32
// pixels, 1-4 channels, nearest and bilinear, BORDER_CONSTANT and BORDER_TRANSPARENT.  See DESIGN.md section 4.15.
//
// The frame -- item decoding, the row walk of the exact float64 chain, the rounding with the reference's NaN, a pixel's load and the
// store of a lane's 4 pixels -- is flat_frame.h; the lens step (float64, every operation rounded on its own: the definition in
// include/bevwarp.h, operation for operation) and the blend of four taps are lens_pixel.h, shared with the map builder; the sampler that
// guards each tap against the frame and a lane's work are lens_sample.h, shared with the fisheye warp (warp_fisheye.hip).  This unit adds
// the model's step to them, and the launcher.
// The lens and r2_max are kernel arguments: wave-uniform, they stay in scalar registers and cost no vector register.
#include "lens_sample.h"

namespace bevwarp {
namespace {

template <typename T, int C, int INTERP, bool TRANSPARENT>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_lens_kernel(const LensArgs a) {
#define BEVWARP_LENS_STEP lens_pixel
#include "lens_lane.inc"
#undef BEVWARP_LENS_STEP
}

template <typename T, int INTERP, bool TRANSPARENT>
void launch_c(const LensArgs& a, int channels, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    switch (channels) {
        case 1: hipLaunchKernelGGL((warp_lens_kernel<T, 1, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((warp_lens_kernel<T, 2, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((warp_lens_kernel<T, 3, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((warp_lens_kernel<T, 4, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
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

hipError_t launch_warp_lens(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    if (dtype == 0)
        (interp == kNearest ? launch_mode<uint8_t, kNearest> : launch_mode<uint8_t, kLinear>)(a, channels, transparent, grid, stream);
    else
        (interp == kNearest ? launch_mode<float, kNearest> : launch_mode<float, kLinear>)(a, channels, transparent, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
