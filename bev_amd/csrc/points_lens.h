// Internal interface of the lens point projection (points_lens.hip, bevwarp_project_points_lens): points through the lens model of
// bevwarp_warp_lens, plane -> raw pixel and raw pixel -> plane.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevwarp {

// One pass of the grid-stride loop covers at most kPointsLensMaxBlocks * kPointsLensBlock lanes: two float32 points per lane (one on
// the 8-byte path), one float64 point.
constexpr int kPointsLensBlock = 256;
constexpr int kPointsLensMaxBlocks = 256 * 8;

struct PointsLensArgs {  // by value: wave-uniform, in scalar registers
    double H[9];         // DISTORT: points -> normalised undistorted camera plane; UNDISTORT: that plane -> the target
    double lens[12];     // fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 (OpenCV's order)
    double r2_max;
    double tol_px;       // UNDISTORT only, like iters
    int iters;
};

// in, out: n x 2 values of dtype (BEVWARP_F32 | BEVWARP_F64), aligned to a point; residual: n values or NULL (UNDISTORT only).
hipError_t launch_points_lens(const void* in, void* out, void* residual, int64_t n, const PointsLensArgs& a, int direction, int dtype, hipStream_t stream);
// ... under BEVWARP_LENS_FISHEYE (points_fisheye.hip): lens holds fx, fy, cx, cy, k1, k2, k3, k4 and four zeros, r2_max holds theta_max
hipError_t launch_points_fisheye(const void* in, void* out, void* residual, int64_t n, const PointsLensArgs& a, int direction, int dtype, hipStream_t stream);

}  // namespace bevwarp
