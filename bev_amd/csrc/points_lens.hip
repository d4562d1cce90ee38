// points_lens.hip -- point projection through the lens model of bevwarp_warp_lens (bevwarp_project_points_lens): plane -> raw pixel
// (DISTORT) and raw pixel -> plane (UNDISTORT, a fixed number of fixed-point steps and a verdict per point).  See DESIGN.md section 4.17.
//
// The memory pattern is project_points_kernel's (geom_kernels.hip): 16 bytes per lane and step -- two float32 points or one float64
// point --, non-temporal loads, plain stores, a grid-stride loop, the odd last point, and one point per step for float32 buffers that
// are only 8-byte aligned.  The arithmetic is the definition in include/bevwarp.h operation for operation: float64, every operation
// rounded on its own (the unit is built with -ffp-contract=off), IEEE division -- no fused multiply-add and no approximate reciprocal,
// which is what separates it from project_points_kernel.  H, the lens, r2_max, tol_px and iters are kernel arguments: wave-uniform,
// they stay in scalar registers, and the iteration loop is a scalar loop.
#include "points_lens.h"

#include "bevwarp.h"

namespace bevwarp {
namespace {

typedef float plf32x4 __attribute__((ext_vector_type(4)));
typedef double plf64x2 __attribute__((ext_vector_type(2)));

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

// (`out` may be `in`: every lane reads its own points before it writes them, and no pointer is __restrict__.  residual is NULL under
// DISTORT, and may be under UNDISTORT.)
template <typename T, int DIR>
__global__ __launch_bounds__(kPointsLensBlock) void points_lens_kernel(const T* in, T* out, T* residual, int64_t n, const PointsLensArgs a, int vec16) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool res = DIR == BEVWARP_LENS_UNDISTORT && residual != nullptr;
    if constexpr (sizeof(T) == 4) {
        if (!vec16) {  // buffers that are only 8-byte aligned (a view starting at an odd point), or a residual that is only 4-byte aligned
            for (int64_t i = t0; i < n; i += stride) {
                const float2 p = reinterpret_cast<const float2*>(in)[i];
                double ox, oy, e = 0.0;
                lens_point<DIR>(a, (double)p.x, (double)p.y, ox, oy, e);
                reinterpret_cast<float2*>(out)[i] = make_float2((float)ox, (float)oy);
                if (res) residual[i] = (float)e;
            }
            return;
        }
        const int64_t pairs = n >> 1;
        for (int64_t i = t0; i < pairs; i += stride) {
            const plf32x4 p = __builtin_nontemporal_load(reinterpret_cast<const plf32x4*>(in) + i);
            double ax, ay, bx, by, ea = 0.0, eb = 0.0;
            lens_point<DIR>(a, (double)p.x, (double)p.y, ax, ay, ea);
            lens_point<DIR>(a, (double)p.z, (double)p.w, bx, by, eb);
            const plf32x4 o = {(float)ax, (float)ay, (float)bx, (float)by};
            reinterpret_cast<plf32x4*>(out)[i] = o;
            if (res) reinterpret_cast<float2*>(residual)[i] = make_float2((float)ea, (float)eb);
        }
        if ((n & 1) && t0 == 0) {  // the odd last point
            double ox, oy, e = 0.0;
            lens_point<DIR>(a, (double)in[2 * (n - 1)], (double)in[2 * (n - 1) + 1], ox, oy, e);
            out[2 * (n - 1)] = (float)ox;
            out[2 * (n - 1) + 1] = (float)oy;
            if (res) residual[n - 1] = (float)e;
        }
    } else {
        for (int64_t i = t0; i < n; i += stride) {
            const plf64x2 p = __builtin_nontemporal_load(reinterpret_cast<const plf64x2*>(in) + i);
            double ox, oy, e = 0.0;
            lens_point<DIR>(a, p.x, p.y, ox, oy, e);
            const plf64x2 o = {ox, oy};
            reinterpret_cast<plf64x2*>(out)[i] = o;
            if (res) residual[i] = e;
        }
    }
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
    // two float32 points per lane and step where both buffers are 16-byte aligned (and the residual's pairs 8-byte aligned)
    const int vec16 = f32 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0 && ((uintptr_t)residual & 7) == 0;
    const int64_t lanes = (f32 && vec16) ? (n + 1) / 2 : n;
    const int64_t want = (lanes + kPointsLensBlock - 1) / kPointsLensBlock;
    // 8 workgroups per CU and a grid-stride loop above, for either type: unlike project_points_kernel<double> this kernel is bound by its
    // float64 arithmetic, not by the stream
    const int grid = (int)(want < kPointsLensMaxBlocks ? want : kPointsLensMaxBlocks);
    if (f32)
        launch_dir<float>(in, out, residual, n, a, direction, vec16, grid, stream);
    else
        launch_dir<double>(in, out, residual, n, a, direction, vec16, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
