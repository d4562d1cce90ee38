// warp_map_fisheye.hip -- bevwarp_build_map under BEVWARP_LENS_FISHEYE: the map builder (warp_map.hip) with the equidistant lens step where
// the rational one stood.  The maps' format is unchanged, so every sampler and stitch through maps serves a fisheye camera as it stands.
// The frame is flat_frame.h, the body and its stores map_build.inc, the step fisheye_pixel.h.  See DESIGN.md section 4.23.
// a.lens: fx, fy, cx, cy, k1..k4, four zeros; a.r2_max carries theta_max.  Wave-uniform, in scalar registers.
#include "warp_map.h"
#include "fisheye_pixel.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

template <int INTERP>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void build_map_fisheye_kernel(const MapBuildArgs a) {
#define BEVWARP_MAP_STEP const bool valid = fisheye_pixel<INTERP>(a, Xn, Yn, W, X, Y);
#include "map_build.inc"
#undef BEVWARP_MAP_STEP
}

}  // namespace

hipError_t launch_build_map_fisheye(const MapBuildArgs& a, int interp, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) { launch(build_map_fisheye_kernel<i()>); });
    });
}

}  // namespace bevwarp
