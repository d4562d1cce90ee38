// Internal interface of the map sampler that writes channel planes from interleaved frames (warp_map_planes.hip; bevwarp_remap_planes):
// 8-bit frames of 3 channels are sampled through the fixed-point maps of bevwarp_build_map as bevwarp_remap samples them, and every sampled
// pixel goes through bevwarp_warp_nv12_planes' plane stage into normalised float32 / float16 / bfloat16 planes.  The five border modes that
// write every pixel, nearest and bilinear, no float64.  The launch geometry is bevwarp_remap's: plan_remap's items of frames_per_item
// frames.  Not installed.
#pragma once
#include "warp_map.h"

namespace bevwarp {

// RemapArgs' frames, maps, index remap and grid.  dst: plane 0 of frame 0; dst_vec_ok: base and the three destination strides admit
// 4-element stores.  Plane k takes sampled channel k: there is no channel swap.  bv_u8: the 8-bit border pixel, byte k = channel k.
struct RemapPlanesArgs : RemapArgs {
    int64_t ch_off[3];            // bytes from a frame's base to plane k
    float pscale[3], pbias[3];    // of channel k
    int plane;                    // kPlaneF32, kPlaneF16, kPlaneBF16 (warp_kernels.h)
};

hipError_t launch_remap_planes(const RemapPlanesArgs& a, int interp, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
