// fisheye_pixel.h -- the equidistant (fisheye) lens step of the coordinate chain (include/bevwarp.h, BEVWARP_LENS_FISHEYE: float64, every
// operation rounded on its own, operation for operation), shared by the fisheye warp (warp_fisheye.hip), the fisheye map builder
// (warp_map_fisheye.hip) and the fisheye point projection (points_fisheye.hip).  Args: any kernel-argument struct with `double lens[12]`
// (fx, fy, cx, cy, k1, k2, k3, k4, 0, 0, 0, 0) and `double r2_max`, which carries theta_max (wave-uniform: scalar registers).
// No library arctangent: two libraries do not agree on the last bit, so the definition brings its own (atan_pos), and the square root
// and the divisions are the correctly rounded IEEE operations.  No pointer but the caller's arguments is touched.
#pragma once
#include "flat_frame.h"

namespace bevwarp {
namespace {

// the doubles nearest to pi / 2 and pi, and nearest to what they leave of them
constexpr double kPio2Hi = 0x1.921fb54442d18p+0, kPio2Lo = 0x1.1a62633145c07p-54;
constexpr double kPiHi = 0x1.921fb54442d18p+1, kPiLo = 0x1.1a62633145c07p-53;

// A[i]: the double nearest to atan(i / 8), i = 0..8 (i is clamped).  A select chain: the index differs from lane to lane, and a table
// in memory would be a load per pixel (in LDS, a resource the kernels of the flat frame do not have).
__device__ __forceinline__ double fisheye_atan_eighth(int i) {
    double a = 0x0.0p+0;
    a = i >= 1 ? 0x1.fd5ba9aac2f6ep-4 : a;
    a = i >= 2 ? 0x1.f5b75f92c80ddp-3 : a;
    a = i >= 3 ? 0x1.6f61941e4def1p-2 : a;
    a = i >= 4 ? 0x1.dac670561bb4fp-2 : a;
    a = i >= 5 ? 0x1.1e00babdefeb4p-1 : a;
    a = i >= 6 ? 0x1.4978fa3269ee1p-1 : a;
    a = i >= 7 ? 0x1.700a7c5784634p-1 : a;
    a = i >= 8 ? 0x1.921fb54442d18p-1 : a;
    return a;
}

// atan(t) for t >= 0 (+inf: kPio2Hi; NaN: NaN): the argument reduced to [0, 1] by 1 / t, then to |z| <= 1 / 16 around the nearest
// eighth by atan(r) = atan(c) + atan((r - c) / (1 + r c)), then the odd series to z^15 with the coefficients 1 / (2 n + 1).
__device__ __forceinline__ double fisheye_atan_pos(double t) {
    constexpr double c3 = 1.0 / 3.0, c5 = 1.0 / 5.0, c7 = 1.0 / 7.0, c9 = 1.0 / 9.0, c11 = 1.0 / 11.0, c13 = 1.0 / 13.0, c15 = 1.0 / 15.0;
    const bool big = t > 1.0;
    const double r = big ? 1.0 / t : t;  // IEEE division
    const double i = __builtin_rint(8.0 * r);  // (half to even; 8 r is exact)
    const double c = i / 8.0;
    const double z = (r - c) / (1.0 + r * c);
    const double z2 = z * z;
    double p = c15;
    p = c13 - z2 * p;
    p = c11 - z2 * p;
    p = c9 - z2 * p;
    p = c7 - z2 * p;
    p = c5 - z2 * p;
    p = c3 - z2 * p;
    // (minNum: a NaN index is 8 here, and the NaN arrives through z)
    const double a = fisheye_atan_eighth((int)fmax(fmin(i, 8.0), 0.0)) + (z - (z * z2) * p);
    return big ? (kPio2Hi - a) + kPio2Lo : a;
}

// The fisheye steps on a ray (Xn, Yn, W), undivided: (u, v) in pixels and the angle theta to the optical axis.  A ray at or beyond 90
// degrees (W <= 0) is a ray like any other.
template <class Args>
__device__ __forceinline__ void fisheye_steps(const Args& a, double Xn, double Yn, double W, double& u, double& v, double& theta) {
    const double fx = a.lens[0], fy = a.lens[1], cx = a.lens[2], cy = a.lens[3], k1 = a.lens[4], k2 = a.lens[5], k3 = a.lens[6], k4 = a.lens[7];
    const double q = Xn * Xn + Yn * Yn;
    const double rho = __builtin_sqrt(q);  // (llvm.sqrt.f64 without fast-math flags: the correctly rounded IEEE square root)
    const double t = rho / fabs(W);        // (W == 0, rho > 0: +inf; 0 / 0: NaN)
    const double at = fisheye_atan_pos(t);
    theta = (W < 0.0) ? (kPiHi - at) + kPiLo : at;
    const double th2 = theta * theta;
    const double poly = 1.0 + (((k4 * th2 + k3) * th2 + k2) * th2 + k1) * th2;
    const double thd = theta * poly;
    const double g = (rho != 0.0) ? thd / rho : 0.0;
    const double xd = Xn * g, yd = Yn * g;
    u = fx * xd + cx, v = fy * yd + cy;
}

// (Xn, Yn, W) of the row walk -> the distorted image point in the units of the maps (pixels; 1 / 32 px for bilinear), as lens_pixel
// (lens_pixel.h) gives it for the rational model.  False: theta is beyond theta_max, or NaN -- the pixel is outside whatever (X, Y) say.
template <int INTERP, class Args>
__device__ __forceinline__ bool fisheye_pixel(const Args& a, double Xn, double Yn, double W, int& X, int& Y) {
    double u, v, theta;
    fisheye_steps(a, Xn, Yn, W, u, v, theta);
    X = round_sat_nan_max(INTERP == kLinear ? u * 32.0 : u);
    Y = round_sat_nan_max(INTERP == kLinear ? v * 32.0 : v);
    return theta <= a.r2_max;
}

}  // namespace
}  // namespace bevwarp
