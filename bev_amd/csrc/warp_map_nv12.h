// Internal interface of the NV12 map sampler (warp_map_nv12.hip): bevwarp_remap_nv12 samples a video decoder's NV12 frames through
// the fixed-point maps of bevwarp_build_map into 8-bit BGR / RGB pixels, bevwarp_remap_nv12_planes into normalised float32 / float16 /
// bfloat16 channel planes -- every tap converted before the blend, all six border modes (the planes: the five that write every pixel),
// no float64.  The launch geometry is bevwarp_remap's: plan_remap's items of frames_per_item frames.  Not installed.
#pragma once
#include "warp_map.h"

#ifndef BEVWARP_REMAP_NV12_WINDOWS
#define BEVWARP_REMAP_NV12_WINDOWS 1  // 0: every tap loaded on its own (tools/time_remap_nv12.py's yardstick for the window loads)
#endif

namespace bevwarp {

// RemapArgs' destination, maps, index remap (of src_w, src_h) and grid; the frames are the two planes here (src, src_fs, src_rs,
// src_vec_ok and bv_f are unused).  bv_u8: the border value in the order the kernel samples in (byte k = sampled channel k).
struct RemapNv12Args : RemapArgs {
    const uint8_t* y;             // src_h rows of src_w bytes
    const uint8_t* uv;            // src_h / 2 rows of src_w / 2 (U, V) pairs; base and strides even
    int64_t y_fs, y_rs;           // bytes
    int64_t uv_fs, uv_rs;
};

hipError_t launch_remap_nv12(const RemapNv12Args& a, int interp, int mode, int rgb_order, int64_t items, hipStream_t stream);

// The plane kernel samples B, G, R and knows no other order (Nv12PlanesArgs' rule, warp_nv12.h): plane offset, scale, bias and border byte
// k belong to sampled channel k.  dst: plane 0 of frame 0; dst_vec_ok: base and the three destination strides admit 4-element stores.
struct RemapNv12PlanesArgs : RemapNv12Args {
    int64_t ch_off[3];            // bytes from a frame's base to the plane sampled channel k is written to
    float pscale[3], pbias[3];    // of sampled channel k
    int plane;                    // kPlaneF32, kPlaneF16, kPlaneBF16 (warp_kernels.h)
};

hipError_t launch_remap_nv12_planes(const RemapNv12PlanesArgs& a, int interp, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
