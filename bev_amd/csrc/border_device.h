// border_device.h -- the parts of the border kernel's frame that the bicubic kernel (warp_cubic.hip) takes over as they are: the
// reference's coordinate rounding with its NaN, the int16 saturation of the maps, a source pixel's load, and the store of a
// lane's row segment.  warp_border.hip keeps its own text of them: moving it here changed the register allocation of its 80
// kernels, and their code objects are not this header's to change.  An edit to either copy belongs in both.  See DESIGN.md
// sections 4.9 and 4.10.
#pragma once
#include "sample.h"
#include "warp_border.h"

namespace bevwarp {
namespace {

// round_sat with the reference's NaN: std::min(INT_MAX, NaN) is INT_MAX.  (coords.h's round_sat sends NaN to INT_MIN, which
// only the constant border cannot tell apart: REPLICATE or WRAP of INT_MIN and of INT_MAX are different pixels.)  A NaN comes
// from 0 * (32 / W) where W is denormal and the division overflows.
__device__ __forceinline__ int round_sat_nan_max(double v) {
    v = fmax(fmin(v, 2147483647.0), -2147483648.0);  // (minNum: fmin(NaN, c) == c)
    return (int)rint(v);
}

template <int INTERP>
__device__ __forceinline__ void map_pixel_exact_nan_max(double Xn, double Yn, double W, int& X, int& Y) {
    W = (W != 0.0) ? ((INTERP == kLinear ? 32.0 : 1.0) / W) : 0.0;  // IEEE division
    X = round_sat_nan_max(Xn * W);
    Y = round_sat_nan_max(Yn * W);
}

// the maps are int16: an index saturates BEFORE borderInterpolate (WRAP of 32767 is not WRAP of 40000)
__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// One source pixel at column x of a row: exactly its C * sizeof(T) bytes are read (never a wider word over its end).
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> load_pixel(const uint8_t* __restrict__ row, int x, bool vec) {
    Pixel<T, C> p;
    if constexpr (sizeof(T) == 1) {
        const uint8_t* q = row + (uint32_t)(x * C);
        if (C == 4 && vec) {
            p.packed = *reinterpret_cast<const uint32_t*>(q);
        } else if (C == 2 && vec) {
            p.packed = *reinterpret_cast<const uint16_t*>(q);
        } else {
            p.packed = 0;
#pragma unroll
            for (int k = 0; k < C; k++) p.packed |= (uint32_t)q[k] << (8 * k);
        }
    } else {
        const float* q = reinterpret_cast<const float*>(row) + (uint32_t)(x * C);
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = q[k];
    }
    return p;
}

// A lane's kBorderPPL consecutive pixels of one destination row, first pixel xs: wide stores (the layout rule of bevwarp_warp's
// dst_vec_ok) for a lane whose pixels are all written; per pixel otherwise.  PREDICATED: some pixels may be unwritten for a
// reason other than the row's end (TRANSPARENT), and their registers hold nothing.
template <typename T, int C, bool PREDICATED>
__device__ __forceinline__ void store_lane_pixels(uint8_t* __restrict__ drow, int xs, const Pixel<T, C> (&px)[kBorderPPL], const bool (&wr)[kBorderPPL],
                                                  int dst_vec_ok) {
    constexpr int PPL = kBorderPPL;
    bool all = true;
#pragma unroll
    for (int j = 0; j < PPL; j++) all = all && wr[j];
    if constexpr (sizeof(T) == 1) {
        uint8_t* d = drow + (int64_t)xs * C;
        uint32_t p[PPL];
#pragma unroll
        for (int j = 0; j < PPL; j++) p[j] = PREDICATED && !wr[j] ? 0u : px[j].packed;
        if (dst_vec_ok && all) {
            if constexpr (C == 1) {
                *reinterpret_cast<uint32_t*>(d) = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
            } else if constexpr (C == 2) {
                u32x2 o = {p[0] | (p[1] << 16), p[2] | (p[3] << 16)};
                *reinterpret_cast<u32x2*>(d) = o;
            } else if constexpr (C == 3) {
                u32x3 o = {__builtin_amdgcn_perm(p[1], p[0], 0x04020100u), __builtin_amdgcn_perm(p[2], p[1], 0x05040201u), __builtin_amdgcn_perm(p[3], p[2], 0x06050402u)};
                wide_store(reinterpret_cast<u32x3*>(d), o);
            } else {
                u32x4 o = {p[0], p[1], p[2], p[3]};
                wide_store(reinterpret_cast<u32x4*>(d), o);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++)
                if (wr[j])
#pragma unroll
                    for (int k = 0; k < C; k++) d[j * C + k] = (uint8_t)(p[j] >> (8 * k));
        }
    } else {
        float* d = reinterpret_cast<float*>(drow) + (int64_t)xs * C;
        if (dst_vec_ok && all) {  // the lane's 4 C floats as C 16-byte stores
#pragma unroll
            for (int i = 0; i < C; i++) {
                f32x4 o = {px[(4 * i) / C].v[(4 * i) % C], px[(4 * i + 1) / C].v[(4 * i + 1) % C], px[(4 * i + 2) / C].v[(4 * i + 2) % C],
                           px[(4 * i + 3) / C].v[(4 * i + 3) % C]};
                wide_store(reinterpret_cast<f32x4*>(d) + i, o);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++)
                if (wr[j])
#pragma unroll
                    for (int k = 0; k < C; k++) d[j * C + k] = px[j].v[k];
        }
    }
}

}  // namespace
}  // namespace bevwarp
