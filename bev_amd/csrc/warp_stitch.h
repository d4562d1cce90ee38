// Internal interface of the multi-camera warp (warp_stitch.hip, bevwarp_warp_stitch): up to 8 cameras, each with frames, sizes, strides
// and matrices of its own, sampled into one canvas in one launch.  The launch geometry is the border kernel's.  Not installed.
#pragma once
#include "flat_frame.h"

namespace bevwarp {

constexpr int kStitchMaxCameras = 8;  // BEVWARP_STITCH_MAX_CAMERAS
constexpr int kStitchOver = 0;        // BEVWARP_STITCH_OVER
constexpr int kStitchFeather = 1;     // BEVWARP_STITCH_FEATHER

struct StitchCamera {  // 48 bytes; the kernel indexes the array with the loop's camera number, from scalar registers
    const uint8_t* src;
    const double* minv;           // device, inverse matrices: canvas px -> this camera's px
    int64_t src_fs, src_rs;       // bytes
    int src_h, src_w;
    int m_stride;                 // 9 (one matrix per frame) or 0 (shared)
    int src_vec_ok;               // 8-bit, 2 / 4 channels: every pixel of THIS source is 2- / 4-byte aligned (one load per tap)
};

struct StitchArgs : FrameArgs {   // (the destination and the grid: flat_frame.h; minv and m_stride are unused, each camera has its own)
    StitchCamera cams[kStitchMaxCameras];
    int n_cams;
    int feather;                  // F of BEVWARP_STITCH_FEATHER, 1..4096
    int fill;                     // pixels no camera covers: 1 = store the border pixel (BORDER_CONSTANT), 0 = leave them alone (TRANSPARENT)
    uint32_t bv_u8;               // the border pixel, 8-bit, packed: byte k = channel k
    float bv_f[4];                // ... and float32
};

hipError_t launch_warp_stitch(const StitchArgs& a, int dtype, int channels, int interp, int blend, int64_t items, hipStream_t stream);

}  // namespace bevwarp
