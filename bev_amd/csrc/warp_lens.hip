// warp_lens.hip -- the perspective warp of frames as a distorted camera delivers them (bevwarp_warp_lens): destination pixel ->
// normalised undistorted camera plane (M_ray) -> OpenCV's rational lens model -> one sample from the raw frame.  8-bit and float32
// pixels, 1-4 channels, nearest and bilinear, BORDER_CONSTANT and BORDER_TRANSPARENT.  See DESIGN.md section 4.15.
//
// The frame -- item decoding, the row walk of the exact float64 chain, the rounding with the reference's NaN, a pixel's load and the
// store of a lane's 4 pixels -- is flat_frame.h; the lens step (float64, every operation rounded on its own: the definition in
// include/bevwarp.h, operation for operation) and the blend of four taps are lens_pixel.h, shared with the map builder; the sampler that
// guards each tap against the frame and a lane's work are lens_sample.h, shared with the fisheye warp (warp_fisheye.hip).  This unit adds
// the model's step to them, and names the instance to launch (launch_pick.h).
// The lens and r2_max are kernel arguments: wave-uniform, they stay in scalar registers and cost no vector register.
#include "lens_sample.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

template <typename T, int C, int INTERP, bool TRANSPARENT>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_lens_kernel(const LensArgs a) {
#define BEVWARP_LENS_STEP lens_pixel
#include "lens_lane.inc"
#undef BEVWARP_LENS_STEP
}

}  // namespace

hipError_t launch_warp_lens(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<kNearest, kLinear>(interp, [&](auto i) {
                pick::flag(transparent, [&](auto tr) {
                    pick::channels(channels, [&](auto c) { launch(warp_lens_kernel<typename decltype(t)::type, c(), i(), tr()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
