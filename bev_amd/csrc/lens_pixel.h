// lens_pixel.h -- the lens step of the coordinate chain (include/bevwarp.h, bevwarp_warp_lens: float64, every operation rounded on its
// own, operation for operation), shared by the lens warp (warp_lens.hip), which samples with it, and the map builder (warp_map.hip), which
// stores what it gives.  Args: any kernel-argument struct with `double lens[12]` and `double r2_max` (wave-uniform: scalar registers).
#pragma once
#include "flat_frame.h"

namespace bevwarp {
namespace {

// (Xn, Yn, W) of the row walk -> the distorted image point in the units of the maps (pixels; 1/32 px for bilinear).  False: r^2 is
// beyond r2_max, or NaN -- the pixel is outside whatever (X, Y) say.
template <int INTERP, class Args>
__device__ __forceinline__ bool lens_pixel(const Args& a, double Xn, double Yn, double W, int& X, int& Y) {
    const double fx = a.lens[0], fy = a.lens[1], cx = a.lens[2], cy = a.lens[3], k1 = a.lens[4], k2 = a.lens[5], p1 = a.lens[6], p2 = a.lens[7],
                 k3 = a.lens[8], k4 = a.lens[9], k5 = a.lens[10], k6 = a.lens[11];
    const double Wr = (W != 0.0) ? (1.0 / W) : 0.0;  // IEEE division
    const double xn = Xn * Wr, yn = Yn * Wr;
    const double x2 = xn * xn, y2 = yn * yn, r2 = x2 + y2, xy2 = 2.0 * (xn * yn);
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double kr = num / den;  // (a pole needs no special case: +-inf and NaN round to INT_MAX / INT_MIN, outside every source)
    const double xd = (xn * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (yn * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    const double u = fx * xd + cx, v = fy * yd + cy;
    X = round_sat_nan_max(INTERP == kLinear ? u * 32.0 : u);
    Y = round_sat_nan_max(INTERP == kLinear ? v * 32.0 : v);
    return r2 <= a.r2_max;
}

// the blend of a pixel's four taps: 8-bit in 15-bit fixed point, float32 with float weights, as bevwarp_warp blends them
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> blend_taps(const Pixel<T, C>& p00, const Pixel<T, C>& p01, const Pixel<T, C>& p10, const Pixel<T, C>& p11, int fx, int fy) {
    Pixel<T, C> out;
    if constexpr (sizeof(T) == 1) {
        out.packed = blend_u8_packed<C>(p00.packed, p01.packed, p10.packed, p11.packed, (uint32_t)fx, (uint32_t)fy);
    } else {
        float w00, w01, w10, w11;
        weights_f32(fx, fy, w00, w01, w10, w11);
#pragma unroll
        for (int k = 0; k < C; k++) out.v[k] = blend_f32(p00.v[k], p01.v[k], p10.v[k], p11.v[k], w00, w01, w10, w11);
    }
    return out;
}

}  // namespace
}  // namespace bevwarp
