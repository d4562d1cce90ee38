// points_lens.hip -- point projection through the lens model of bevwarp_warp_lens (bevwarp_project_points_lens): plane -> raw pixel
// (DISTORT) and raw pixel -> plane (UNDISTORT, a fixed number of fixed-point steps and a verdict per point).  See DESIGN.md section 4.17.
//
// The memory pattern is project_points_kernel's (geom_kernels.hip), in points_stream.h, shared with the fisheye model's kernels
// (points_fisheye.hip).  The arithmetic is the definition in include/bevwarp.h operation for operation: float64, every operation
// rounded on its own (the unit is built with -ffp-contract=off), IEEE division -- no fused multiply-add and no approximate reciprocal,
// which is what separates it from project_points_kernel.  H, the lens, r2_max, tol_px and iters are kernel arguments: wave-uniform,
// they stay in scalar registers, and the iteration loop is a scalar loop.
#include "points_stream.h"

namespace bevwarp {
namespace {

// plane(x, y) of the header: the homography in the operand order of the lens warp's first evaluation block
__device__ __forceinline__ void plane(const PointsLensArgs& a, double x, double y, double& xo, double& yo) {
    const double X = (a.H[1] * y + a.H[2]) + a.H[0] * x;
    const double Y = (a.H[4] * y + a.H[5]) + a.H[3] * x;
    const double W = (a.H[7] * y + a.H[8]) + a.H[6] * x;
    const double Wr = (W != 0.0) ? (1.0 / W) : 0.0;  // IEEE division
    xo = X * Wr, yo = Y * Wr;
}

// the lens steps of bevwarp_warp_lens (warp_lens.hip, lens_pixel), restated: (xn, yn) -> (u, v, r2)
__device__ __forceinline__ void lens_steps(const PointsLensArgs& a, double xn, double yn, double& u, double& v, double& r2) {
    const double fx = a.lens[0], fy = a.lens[1], cx = a.lens[2], cy = a.lens[3], k1 = a.lens[4], k2 = a.lens[5], p1 = a.lens[6], p2 = a.lens[7],
                 k3 = a.lens[8], k4 = a.lens[9], k5 = a.lens[10], k6 = a.lens[11];
    const double x2 = xn * xn, y2 = yn * yn, xy2 = 2.0 * (xn * yn);
    r2 = x2 + y2;
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double kr = num / den;
    const double xd = (xn * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (yn * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    u = fx * xd + cx, v = fy * yd + cy;
}

// One point.  e: the reprojection error (UNDISTORT; untouched by DISTORT).
template <int DIR>
__device__ __forceinline__ void lens_point(const PointsLensArgs& a, double px, double py, double& ox, double& oy, double& e) {
    const double nan = __builtin_nan("");
    if constexpr (DIR == BEVWARP_LENS_DISTORT) {
        double xn, yn, u, v, r2;
        plane(a, px, py, xn, yn);
        lens_steps(a, xn, yn, u, v, r2);
        const bool valid = r2 <= a.r2_max;  // (false for NaN)
        ox = valid ? u : nan, oy = valid ? v : nan;
    } else {
        const double fx = a.lens[0], fy = a.lens[1], cx = a.lens[2], cy = a.lens[3], k1 = a.lens[4], k2 = a.lens[5], p1 = a.lens[6], p2 = a.lens[7],
                     k3 = a.lens[8], k4 = a.lens[9], k5 = a.lens[10], k6 = a.lens[11];
        const double xd = (px - cx) / fx, yd = (py - cy) / fy;
        double x = xd, y = yd;
        for (int it = 0; it < a.iters; it++) {  // wave-uniform, no early exit: the count is part of the definition
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
            const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
            const double ic = den / num;
            const double dx = p1 * xy2 + p2 * (r2 + 2.0 * x2);
            const double dy = p1 * (r2 + 2.0 * y2) + p2 * xy2;
            x = (xd - dx) * ic, y = (yd - dy) * ic;
        }
        double u, v, r2;
        lens_steps(a, x, y, u, v, r2);
        const double du = fabs(u - px), dv = fabs(v - py);
        e = (du > dv || du != du) ? du : dv;  // numpy.maximum: NaN if either is
        const bool valid = (r2 <= a.r2_max) && (e <= a.tol_px);
        double wx, wy;
        plane(a, x, y, wx, wy);
        ox = valid ? wx : nan, oy = valid ? wy : nan;
    }
}

template <typename T, int DIR>
__global__ __launch_bounds__(kPointsLensBlock) void points_lens_kernel(const T* in, T* out, T* residual, int64_t n, const PointsLensArgs a, int vec16) {
#define BEVWARP_POINT lens_point
#include "points_stream.inc"
#undef BEVWARP_POINT
}

template <typename T>
void launch_dir(const void* in, void* out, void* residual, int64_t n, const PointsLensArgs& a, int direction, int vec16, int grid, hipStream_t stream) {
    const dim3 g(grid), b(kPointsLensBlock);
    if (direction == BEVWARP_LENS_DISTORT)
        hipLaunchKernelGGL((points_lens_kernel<T, BEVWARP_LENS_DISTORT>), g, b, 0, stream, (const T*)in, (T*)out, (T*)nullptr, n, a, vec16);
    else
        hipLaunchKernelGGL((points_lens_kernel<T, BEVWARP_LENS_UNDISTORT>), g, b, 0, stream, (const T*)in, (T*)out, (T*)residual, n, a, vec16);
}

}  // namespace

hipError_t launch_points_lens(const void* in, void* out, void* residual, int64_t n, const PointsLensArgs& a, int direction, int dtype, hipStream_t stream) {
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
