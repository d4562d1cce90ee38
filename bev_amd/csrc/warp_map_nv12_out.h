// Internal interface of the map samplers that write NV12 (warp_map_nv12_out.hip; bevwarp_remap_to_nv12, bevwarp_remap_nv12_to_nv12): an
// 8-bit BGR / RGB frame or a decoder's NV12 planes are sampled through the fixed-point maps of bevwarp_build_map as bevwarp_remap /
// bevwarp_remap_nv12 sample them, and every sampled pixel is stored as a Y byte and -- at even columns of even rows -- a (U, V) pair.
// The five border modes that write every pixel, nearest and bilinear, no float64.  The launch geometry is bevwarp_remap's: plan_remap's
// items of frames_per_item frames.  Not installed.
#pragma once
#include "nv12_store.h"
#include "warp_map_nv12.h"

namespace bevwarp {

// RemapNv12Args' maps, index remap and grid; its destination (dst, dst_fs, dst_rs, dst_vec_ok) is the Y plane.  The frames are src (8-bit,
// 3 channels) or the two planes y, uv.  bv_u8: the border PIXEL packed in the sampled pixel's channel order; converted like any other.
struct RemapNv12OutArgs : RemapNv12Args, Nv12DstUv {};

// nv12_src: the source is (y, uv), sampled as B, G, R (rgb_order is then 0); otherwise src, whose pixels are B, G, R (rgb_order 0) or R, G, B (1)
hipError_t launch_remap_nv12_out(const RemapNv12OutArgs& a, int nv12_src, int interp, int mode, int rgb_order, int64_t items, hipStream_t stream);

}  // namespace bevwarp
