// Internal interface of the multi-camera stitch through warp maps that writes NV12 (warp_stitch_maps_nv12_out.hip:
// bevwarp_stitch_maps_to_nv12, bevwarp_stitch_maps_nv12_to_nv12): bevwarp_stitch_maps' (bevwarp_stitch_maps_nv12's) 8-bit canvas pixel,
// stored as a Y byte and -- at even columns of even rows -- a (U, V) pair.  Every canvas pixel is written: what no camera covers is the
// border pixel.  The launch geometry is the border kernel's, one frame per item.  Not installed.
#pragma once
#include "nv12_store.h"
#include "warp_stitch_maps.h"

namespace bevwarp {

// StitchMapsArgs' cameras, grid and feather width; its destination (dst, dst_fs, dst_rs, dst_vec_ok) is the Y plane; fill and bv_f are
// unused.  bv_u8: the border PIXEL packed in the sampled pixel's channel order; converted like any other.
struct StitchMapsNv12OutArgs : StitchMapsArgs, Nv12DstUv {};
static_assert(sizeof(StitchMapsNv12OutArgs) <= 4096, "eight cameras fit the kernel-argument block");

// nv12_src: the cameras' frames are (src = y, uv), sampled as B, G, R (rgb_order is then 0); otherwise src, B, G, R (rgb_order 0) or R, G, B (1)
hipError_t launch_stitch_maps_nv12_out(const StitchMapsNv12OutArgs& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream);
// ... and under BEVWARP_STITCH_GAIN (warp_stitch_gain_nv12_out.hip)
hipError_t launch_stitch_gain_nv12_out(const Gained<StitchMapsNv12OutArgs>& a, int nv12_src, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream);

}  // namespace bevwarp
