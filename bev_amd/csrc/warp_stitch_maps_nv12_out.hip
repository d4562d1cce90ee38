// warp_stitch_maps_nv12_out.hip -- several fixed cameras sampled through their warp maps into one BEV canvas that is written as NV12 for a
// video encoder, in one launch (bevwarp_stitch_maps_to_nv12, bevwarp_stitch_maps_nv12_to_nv12): BGR -> NV12 of
// bevwarp_stitch_maps' (bevwarp_stitch_maps_nv12's) 8-bit canvas under BORDER_CONSTANT, bit for bit, with the canvas never in memory.  It
// is stitch_maps_body's camera loop and blends (warp_stitch_maps.hip) for 8-bit pixels of 3 channels, unchanged in meaning, with every
// uncovered pixel filled, and nv12_store.h's store in place of store_lane_pixels.  No float64.
//
// One frame per item, the cameras are kernel arguments and the loop's camera number is wave-uniform, every sampled pixel is an inlier: all
// as warp_stitch_maps.hip describes.  The samplers are stitch_sample.h's, shared with that unit; the camera loop is stitch_maps_u8x3.inc,
// shared as text with warp_stitch_maps_planes.hip.
//
// warp_stitch_gain_nv12_out.hip is this text once more under BEVWARP_STITCH_GAIN_UNIT (warp_stitch_maps.h): the same kernel and
// launcher over Gained<> arguments, with which the camera loop applies the camera's gain to every tap.
#include "warp_stitch_maps_nv12_out.h"
#include "stitch_sample.h"
#include "launch_pick.h"

#define UNIT_KERNEL BEVWARP_STITCH_UNIT(stitch_maps_nv12_out_kernel, stitch_gain_nv12_out_kernel)
#define UNIT_LAUNCH BEVWARP_STITCH_UNIT(launch_stitch_maps_nv12_out, launch_stitch_gain_nv12_out)

namespace bevwarp {
namespace {

using Args = UnitArgs<StitchMapsNv12OutArgs>;

// NV12: the cameras' frames are NV12, sampled as B, G, R (RGB is then 0); otherwise RGB names the frames' channel order.
template <int INTERP, int BLEND, bool NV12, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void UNIT_KERNEL(const Args a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kFeather = BLEND == kStitchFeather;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;

#include "stitch_maps_u8x3.inc"
    store_lane_nv12<RGB>(a, a, b, y, xs, px);
}

}  // namespace

hipError_t UNIT_LAUNCH(const UnitArgs<StitchMapsNv12OutArgs>& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream) {
    const int source = nv12_src ? 2 : (rgb_order ? 1 : 0);  // 0 = B, G, R frames, 1 = R, G, B frames, 2 = NV12 frames
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<kStitchFeather, kStitchOver>(blend, [&](auto bl) {
                pick::value<2, 1, 0>(source, [&](auto s) { launch(UNIT_KERNEL<i(), bl(), s() == 2, s() == 1>); });
            });
        });
    });
}

}  // namespace bevwarp
