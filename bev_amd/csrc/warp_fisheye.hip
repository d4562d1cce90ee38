// warp_fisheye.hip -- bevwarp_warp_lens under BEVWARP_LENS_FISHEYE: the lens warp (warp_lens.hip) with the equidistant lens step where the
// rational one stood -- destination pixel -> ray in the camera's frame (M_ray, NOT divided by its depth: a ray at or beyond 90 degrees from
// the optical axis is a pixel like any other) -> angle -> raw pixel -> one sample.  The same formats, borders, frame (flat_frame.h),
// samplers and lane (lens_sample.h); the step is fisheye_pixel.h.  See DESIGN.md section 4.23.
// a.lens: fx, fy, cx, cy, k1..k4, four zeros; a.r2_max carries theta_max.  Wave-uniform, in scalar registers.
#include "lens_sample.h"
#include "fisheye_pixel.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

template <typename T, int C, int INTERP, bool TRANSPARENT>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_fisheye_kernel(const LensArgs a) {
#define BEVWARP_LENS_STEP fisheye_pixel
#include "lens_lane.inc"
#undef BEVWARP_LENS_STEP
}

}  // namespace

hipError_t launch_warp_fisheye(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<kNearest, kLinear>(interp, [&](auto i) {
                pick::flag(transparent, [&](auto tr) {
                    pick::channels(channels, [&](auto c) { launch(warp_fisheye_kernel<typename decltype(t)::type, c(), i(), tr()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
