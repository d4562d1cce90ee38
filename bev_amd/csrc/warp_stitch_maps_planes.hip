// warp_stitch_maps_planes.hip -- several fixed cameras sampled through their warp maps into one BEV canvas that is written as normalised
// channel planes for a detector, in one launch (bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes):
// bevwarp_warp_nv12_planes' plane stage of bevwarp_stitch_maps' (bevwarp_stitch_maps_nv12's) 8-bit canvas under BORDER_CONSTANT, bit for
// bit, with the canvas never in memory.  It is stitch_maps_nv12_out_kernel's shape (warp_stitch_maps_nv12_out.hip): stitch_maps_body's
// camera loop and blends for 8-bit pixels of 3 channels, unchanged in meaning, every pixel starting as the border pixel and stored
// unconditionally, with plane_store.inc's store where the NV12 store stood.  No float64.
//
// One frame per item, the cameras are kernel arguments and the loop's camera number is wave-uniform, every sampled pixel is an inlier: all
// as warp_stitch_maps.hip describes.  The samplers are stitch_sample.h's, shared with that unit; the camera loop is stitch_maps_u8x3.inc,
// shared as text with warp_stitch_maps_nv12_out.hip.
//
// warp_stitch_gain_planes.hip is this text once more under BEVWARP_STITCH_GAIN_UNIT (warp_stitch_maps.h): the same kernel and launcher
// over Gained<> arguments, with which the camera loop applies the camera's gain to every tap.
#include "warp_stitch_maps_planes.h"
#include "stitch_sample.h"
#include "launch_pick.h"

#define UNIT_KERNEL BEVWARP_STITCH_UNIT(stitch_maps_planes_kernel, stitch_gain_planes_kernel)
#define UNIT_LAUNCH BEVWARP_STITCH_UNIT(launch_stitch_maps_planes, launch_stitch_gain_planes)

namespace bevwarp {
namespace {

using Args = UnitArgs<StitchMapsPlanesArgs>;

// NV12: the cameras' frames are NV12, converted to B, G, R (RGB = 0) or R, G, B (1); otherwise plane k is the frames' channel k (RGB is 0).
template <int INTERP, int BLEND, bool NV12, int RGB, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void UNIT_KERNEL(const Args a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kFeather = BLEND == kStitchFeather;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;

#include "stitch_maps_u8x3.inc"
    const uint32_t (&p)[PPL] = px;
#include "plane_store.inc"
}

}  // namespace

hipError_t UNIT_LAUNCH(const UnitArgs<StitchMapsPlanesArgs>& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream) {
    const int source = nv12_src ? (rgb_order ? 2 : 1) : 0;  // 0 = interleaved frames, 1 = NV12 frames as B, G, R, 2 = NV12 frames as R, G, B
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<kStitchFeather, kStitchOver>(blend, [&](auto bl) {
                pick::value<2, 1, 0>(source, [&](auto s) {
                    pick::flag(a.plane != kPlaneF32, [&](auto wide16) { launch(UNIT_KERNEL<i(), bl(), s() != 0, s() == 2, wide16()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
