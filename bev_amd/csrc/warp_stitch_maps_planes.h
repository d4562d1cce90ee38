// Internal interface of the multi-camera stitch through warp maps that writes channel planes (warp_stitch_maps_planes.hip:
// bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes): bevwarp_stitch_maps' (bevwarp_stitch_maps_nv12's) 8-bit canvas pixel put
// through bevwarp_warp_nv12_planes' plane stage.  Every canvas pixel is written: what no camera covers is the border pixel.  The launch
// geometry is the border kernel's, one frame per item.  Not installed.
#pragma once
#include "warp_stitch_maps.h"

namespace bevwarp {

// StitchMapsArgs' cameras, grid and feather width; dst: plane 0 of frame 0; dst_vec_ok: base and the three destination strides admit
// 4-element stores; fill and bv_f are unused.  Plane k takes channel k of the canvas pixel (NV12 frames: in the order the kernel converts
// to).  bv_u8: the 8-bit border pixel, byte k = channel k.
struct StitchMapsPlanesArgs : StitchMapsArgs {
    int64_t ch_off[3];            // bytes from a frame's base to plane k
    float pscale[3], pbias[3];    // of channel k
    int plane;                    // kPlaneF32, kPlaneF16, kPlaneBF16 (warp_kernels.h)
};
static_assert(sizeof(StitchMapsPlanesArgs) <= 4096, "eight cameras fit the kernel-argument block");

// nv12_src: the cameras' frames are (src = y, uv), converted to B, G, R (rgb_order 0) or R, G, B (1); otherwise src, whose channel k is plane k
hipError_t launch_stitch_maps_planes(const StitchMapsPlanesArgs& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream);
// ... and under BEVWARP_STITCH_GAIN (warp_stitch_gain_planes.hip)
hipError_t launch_stitch_gain_planes(const Gained<StitchMapsPlanesArgs>& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream);

}  // namespace bevwarp
