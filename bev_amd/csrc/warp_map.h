// Internal interface of the fixed-camera warp maps (warp_map.hip, warp_map_cubic.hip): bevwarp_build_map writes the coordinate chain's result as OpenCV's
// fixed-point maps (CV_16SC2 + CV_16UC1, include/bevwarp.h), bevwarp_remap samples frames through such maps with no float64 at all.
// The launch geometry is the border kernel's flat grid; a remap item covers one tile of several consecutive frames.  Not installed.
#pragma once
#include "warp_border.h"

// the most frames a remap item walks with its map entries held in registers (plan_remap chooses up to it; 1: one frame per item, the
// map re-read per frame through the caches).  Measured at 1, 2, 4 and 8 (tools/time_remap.py, profiles/remap_timing.txt): 2 and 4 gain
// 7.5 % on a footprint of inliers, every value above 1 loses on the Brno-like BEV, the more the fewer and fatter the items -- 2.7 % at 2,
// 14.6 % at 8.  2 is the fastest over both footprints; DESIGN.md section 4.18.
#ifndef BEVWARP_REMAP_MAX_FPI
#define BEVWARP_REMAP_MAX_FPI 2
#endif

namespace bevwarp {

constexpr int kRemapMaxFramesPerItem = BEVWARP_REMAP_MAX_FPI;

// the builder: FrameArgs' destination is the xy plane (dst, dst_fs, dst_rs: int16 pairs), minv the m_count matrices (m_stride 9)
struct MapBuildArgs : FrameArgs {
    uint8_t* frac;              // uint16 plane (bilinear; unused for nearest)
    int64_t frac_fs, frac_rs;   // bytes
    double lens[12];            // fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 (with a lens: minv holds M_ray)
    double r2_max;
};

// the sampler: BorderArgs' frames, index remap and grid; the grid's "frame" is a group of frames_per_item consecutive frames
struct RemapArgs : BorderArgs {
    const uint8_t* xy;          // int16 pairs (sx, sy)
    const uint8_t* frac;        // uint16 (fy << 5) | fx; bilinear only
    int64_t xy_fs, xy_rs, frac_fs, frac_rs;  // bytes; the frame strides are 0 for a shared map
    int batch, frames_per_item;
    int map_vec_ok;             // both planes admit a lane's 16-byte / 8-byte load
    float bv_f[4];              // the border value per channel, float32 pixels
    uint32_t bv_u8;             // ... and saturate_cast<uchar> of it, packed: byte k = channel k
    // (the same border value per channel, as cubic_sample.h's sampler takes it: BORDER_CONSTANT's, 0 for every other mode)
    __device__ __forceinline__ int cv_int(int k) const { return (int)((bv_u8 >> (8 * k)) & 0xffu); }
    __device__ __forceinline__ float cv_float(int k) const { return bv_f[k]; }
};

hipError_t launch_build_map(const MapBuildArgs& a, int interp, bool lens, int64_t items, hipStream_t stream);
// ... under BEVWARP_LENS_FISHEYE (warp_map_fisheye.hip): lens holds fx, fy, cx, cy, k1, k2, k3, k4 and four zeros, r2_max holds theta_max
hipError_t launch_build_map_fisheye(const MapBuildArgs& a, int interp, int64_t items, hipStream_t stream);
hipError_t launch_remap(const RemapArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream);
// ... under BEVWARP_MAP_BICUBIC (warp_map_cubic.hip): a bilinear map's entries sampled by the bicubic sampler; per_*, off_*, mag_* are
// cubic::window_period's for every mode (the 4-tap window reaches one index further than a saturated one)
hipError_t launch_remap_cubic(const RemapArgs& a, int dtype, int channels, int mode, int64_t items, hipStream_t stream);

}  // namespace bevwarp
