// Internal interface of the NV12 warps: a Y plane and a half-resolution plane of (U, V) pairs are sampled and converted tap by tap into an
// 8-bit BGR / RGB destination (warp_nv12.hip, bevwarp_warp_nv12) or into normalised float32 / float16 / bfloat16 channel planes
// (warp_nv12_planes.hip, bevwarp_warp_nv12_planes).  Constant border, nearest and bilinear.  Not installed.
#pragma once
#include "flat_frame.h"

namespace bevwarp {

// The launch geometry, the destination (3 bytes per pixel) and the matrices are the shared frame's (flat_frame.h).
struct Nv12Args : FrameArgs {
    const uint8_t* y;             // src_h rows of src_w bytes
    const uint8_t* uv;            // src_h / 2 rows of src_w / 2 (U, V) pairs; base and strides even
    int64_t y_fs, y_rs;           // bytes
    int64_t uv_fs, uv_rs;
    int src_h, src_w;
    uint32_t border;              // the border value packed in the destination's channel order (byte k = channel k)
};

hipError_t launch_warp_nv12(const Nv12Args& a, int interp, int rgb_order, int64_t items, hipStream_t stream);

// The plane kernel samples in ONE channel order -- B, G, R in bytes 0, 1, 2 of a pixel -- and knows no other: the destination's order is
// where the host points each sampled channel (plane offset, scale, bias and border byte k belong to sampled channel k).
// (dst: plane 0 of frame 0; dst_vec_ok: base and the three destination strides admit 4-element stores, 16 bytes float32, 8 bytes
// 16-bit; border: byte k = the border value of sampled channel k)
struct Nv12PlanesArgs : Nv12Args {
    int64_t ch_off[3];            // bytes from a frame's base to the plane sampled channel k (B, G, R) is written to
    float pscale[3], pbias[3];    // of sampled channel k
    int plane;                    // kPlaneF32, kPlaneF16, kPlaneBF16 (warp_kernels.h)
};

hipError_t launch_warp_nv12_planes(const Nv12PlanesArgs& a, int interp, int64_t items, hipStream_t stream);

}  // namespace bevwarp
