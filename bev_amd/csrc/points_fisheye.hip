// points_fisheye.hip -- bevwarp_project_points_lens under BEVWARP_LENS_FISHEYE: point projection through the equidistant lens model, plane ->
// raw pixel (DISTORT) and raw pixel -> plane (UNDISTORT: a fixed number of Newton steps in s = tan(theta / 2), in which the ray is rational,
// and a verdict per point).  See DESIGN.md section 4.23.
//
// The memory pattern is points_stream.h, shared with the rational model's kernels (points_lens.hip); the lens step is fisheye_pixel.h,
// shared with the fisheye warp and map builder.  The arithmetic is the definition in include/bevwarp.h operation for operation: float64,
// every operation rounded on its own (the unit is built with -ffp-contract=off), IEEE division and square root, no library arctangent.
// H, the lens, theta_max (in r2_max), tol_px and iters are kernel arguments: wave-uniform, they stay in scalar registers, and the iteration
// loop is a scalar loop.
#include "points_stream.h"
#include "fisheye_pixel.h"

namespace bevwarp {
namespace {

// H (x, y, z) in the operand order of plane(x, y) of the header (z = 1 there: the same bits), NOT divided
__device__ __forceinline__ void ray_of(const PointsLensArgs& a, double x, double y, double z, double& X, double& Y, double& W) {
    X = (a.H[1] * y + a.H[2] * z) + a.H[0] * x;
    Y = (a.H[4] * y + a.H[5] * z) + a.H[3] * x;
    W = (a.H[7] * y + a.H[8] * z) + a.H[6] * x;
}

// One point.  e: the reprojection error (UNDISTORT; untouched by DISTORT).
template <int DIR>
__device__ __forceinline__ void fisheye_point(const PointsLensArgs& a, double px, double py, double& ox, double& oy, double& e) {
    const double nan = __builtin_nan("");
    if constexpr (DIR == BEVWARP_LENS_DISTORT) {
        double X, Y, W, u, v, theta;
        ray_of(a, px, py, 1.0, X, Y, W);
        fisheye_steps(a, X, Y, W, u, v, theta);
        const bool valid = theta <= a.r2_max;  // (false for NaN)
        ox = valid ? u : nan, oy = valid ? v : nan;
    } else {
        const double fx = a.lens[0], fy = a.lens[1], cx = a.lens[2], cy = a.lens[3], k1 = a.lens[4], k2 = a.lens[5], k3 = a.lens[6], k4 = a.lens[7];
        const double d1 = 3.0 * k1, d2 = 5.0 * k2, d3 = 7.0 * k3, d4 = 9.0 * k4;
        const double xd = (px - cx) / fx, yd = (py - cy) / fy;
        const double thd = __builtin_sqrt(xd * xd + yd * yd);
        double s = thd / 2.0;
        for (int it = 0; it < a.iters; it++) {  // wave-uniform, no early exit: the count is part of the definition
            const double theta = 2.0 * fisheye_atan_pos(s);
            const double th2 = theta * theta;
            const double poly = 1.0 + (((k4 * th2 + k3) * th2 + k2) * th2 + k1) * th2;
            const double f = theta * poly - thd;
            const double D = 1.0 + (((d4 * th2 + d3) * th2 + d2) * th2 + d1) * th2;
            s = s - (f * (1.0 + s * s)) / (2.0 * D);
            s = (s < 0.0) ? 0.0 : s;
        }
        const bool off = thd != 0.0;
        const double s2 = 2.0 * s;
        const double rx = off ? s2 * (xd / thd) : 0.0, ry = off ? s2 * (yd / thd) : 0.0, rz = off ? 1.0 - s * s : 1.0;
        double u, v, theta;
        fisheye_steps(a, rx, ry, rz, u, v, theta);
        const double du = fabs(u - px), dv = fabs(v - py);
        e = (du > dv || du != du) ? du : dv;  // numpy.maximum: NaN if either is
        const bool valid = (theta <= a.r2_max) && (e <= a.tol_px);
        double X, Y, W;
        ray_of(a, rx, ry, rz, X, Y, W);
        const double Wr = (W != 0.0) ? (1.0 / W) : 0.0;  // IEEE division
        ox = valid ? X * Wr : nan, oy = valid ? Y * Wr : nan;
    }
}

template <typename T, int DIR>
__global__ __launch_bounds__(kPointsLensBlock) void points_fisheye_kernel(const T* in, T* out, T* residual, int64_t n, const PointsLensArgs a, int vec16) {
#define BEVWARP_POINT fisheye_point
#include "points_stream.inc"
#undef BEVWARP_POINT
}

template <typename T>
void launch_dir(const void* in, void* out, void* residual, int64_t n, const PointsLensArgs& a, int direction, int vec16, int grid, hipStream_t stream) {
    const dim3 g(grid), b(kPointsLensBlock);
    if (direction == BEVWARP_LENS_DISTORT)
        hipLaunchKernelGGL((points_fisheye_kernel<T, BEVWARP_LENS_DISTORT>), g, b, 0, stream, (const T*)in, (T*)out, (T*)nullptr, n, a, vec16);
    else
        hipLaunchKernelGGL((points_fisheye_kernel<T, BEVWARP_LENS_UNDISTORT>), g, b, 0, stream, (const T*)in, (T*)out, (T*)residual, n, a, vec16);
}

}  // namespace

hipError_t launch_points_fisheye(const void* in, void* out, void* residual, int64_t n, const PointsLensArgs& a, int direction, int dtype, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const bool f32 = dtype == BEVWARP_F32;
    int vec16;
    const int grid = points_grid(in, out, residual, n, f32, vec16);
    if (f32)
        launch_dir<float>(in, out, residual, n, a, direction, vec16, grid, stream);
    else
        launch_dir<double>(in, out, residual, n, a, direction, vec16, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
