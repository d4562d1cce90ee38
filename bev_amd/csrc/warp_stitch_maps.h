// Internal interface of the multi-camera stitch through warp maps (warp_stitch_maps.hip: bevwarp_stitch_maps, bevwarp_stitch_maps_nv12):
// up to 8 cameras, each with frames, sizes, strides and maps of its own, sampled into one canvas in one launch with bevwarp_warp_stitch's
// two blend rules and no float64.  The launch geometry is the border kernel's, one frame per item.  Not installed.
#pragma once
#include "warp_stitch.h"

namespace bevwarp {

// 112 bytes; the kernel indexes the array with the loop's camera number, from scalar registers.  Interleaved frames: src; NV12 frames: src
// is the Y plane and uv the plane of (U, V) pairs (base and strides even).  A shared map has frame strides of 0.
struct StitchMapCamera {
    const uint8_t* src;
    const uint8_t* uv;
    const uint8_t* xy;            // int16 pairs (sx, sy)
    const uint8_t* frac;          // uint16 (fy << 5) | fx; bilinear only
    int64_t src_fs, src_rs;       // bytes
    int64_t uv_fs, uv_rs;
    int64_t xy_fs, xy_rs, frac_fs, frac_rs;
    int src_h, src_w;
    int src_vec_ok;               // 8-bit, 2 / 4 channels: every pixel of THIS source is 2- / 4-byte aligned (one load per tap)
    int map_vec_ok;               // both planes of THIS camera admit a lane's 16-byte / 8-byte load
};

struct StitchMapsArgs : FrameArgs {  // (the destination and the grid: flat_frame.h; minv, m_stride and bw0 are unused)
    StitchMapCamera cams[kStitchMaxCameras];
    int n_cams;
    int feather;                  // F of BEVWARP_STITCH_FEATHER, 1..4096
    int fill;                     // pixels no camera covers: 1 = store the border pixel (BORDER_CONSTANT), 0 = leave them alone (TRANSPARENT)
    uint32_t bv_u8;               // the border pixel, 8-bit, packed: byte k = channel k (NV12: in the destination's order)
    float bv_f[4];                // ... and float32
};
static_assert(sizeof(StitchMapsArgs) <= 4096, "eight cameras fit the kernel-argument block");

// A gained launch's arguments (BEVWARP_STITCH_GAIN): the plain launch's, and behind them every camera's gain word
// G0 | G1 << 10 | G2 << 20 (Q8).  Only the gained kernels see them: StitchMapCamera and the plain kernels' arguments are what they were.
template <class Args>
struct Gained : Args {
    uint32_t gains[kStitchMaxCameras];
};
static_assert(sizeof(Gained<StitchMapsArgs>) <= 4096, "eight cameras and their gains fit the kernel-argument block");

// The gained units -- warp_stitch_gain.hip, warp_stitch_gain_nv12_out.hip, warp_stitch_gain_planes.hip -- are the text of the unit each
// shadows, compiled once more with BEVWARP_STITCH_GAIN_UNIT defined: the same kernel bodies and launchers over Gained<> arguments,
// under names of their own.  (8-bit pixels of 3 channels only: warp_stitch_maps.hip leaves its other formats out.)
#ifdef BEVWARP_STITCH_GAIN_UNIT
#define BEVWARP_STITCH_UNIT(plain, gained) gained
template <class Args>
using UnitArgs = Gained<Args>;
#else
#define BEVWARP_STITCH_UNIT(plain, gained) plain
template <class Args>
using UnitArgs = Args;
#endif

hipError_t launch_stitch_maps(const StitchMapsArgs& a, int dtype, int channels, int interp, int blend, int64_t items, hipStream_t stream);
hipError_t launch_stitch_gain(const Gained<StitchMapsArgs>& a, int dtype, int channels, int interp, int blend, int64_t items, hipStream_t stream);  // (8-bit, 3 channels)
hipError_t launch_stitch_gain_nv12(const Gained<StitchMapsArgs>& a, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream);
hipError_t launch_stitch_maps_nv12(const StitchMapsArgs& a, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream);

}  // namespace bevwarp
