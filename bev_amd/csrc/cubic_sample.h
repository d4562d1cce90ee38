// cubic_sample.h -- the bicubic sampler (device code, gfx950), shared by the matrix kernel (warp_cubic.hip: BEVWARP_CUBIC through
// bevwarp_warp / bevwarp_warp_border) and the map kernel (warp_map_cubic.hip: BEVWARP_MAP_BICUBIC through bevwarp_remap): the tables'
// __device__ definitions, a pixel's 16 weights, and the two paths from (the window's first tap, the weights) to the pixel.  An INLIER
// (all 16 taps inside the source) loads each of its four tap rows as ONE window of exactly 4 C values and sums them row by row.  Every
// other written pixel takes the general path: eight index remaps, sixteen per-pixel loads, one tap at a time around the border value.
// The definition is in include/bevwarp.h and DESIGN.md section 4.10, the tables in cubic_tab.h.  An args struct serves the general path
// with src_w / src_h, src_rs, the period plan of cubic::window_period, src_vec_ok and the border value as cv_int(k) / cv_float(k)
// (BORDER_CONSTANT; 0 for every other mode).  Not installed.
#pragma once
#include <type_traits>

#include "cubic_tab.h"
#include "warp_border.h"

namespace bevwarp {
namespace {

// Emitted by constant evaluation of cubic_tab.h's own functions (a dynamic initialiser of a __device__ variable does not compile):
// 32 KB of fixed-point entries, one entry = 32 contiguous bytes = two 16-byte loads; float weights are formed in registers from the
// 512-byte coefficient table (the same float32 products as cubic::entry_f32).  Read-only: no state, nothing to allocate.  (One copy
// per unit that includes this header.)
alignas(32) __device__ const cubic::FixedTable kFixedTab = cubic::make_fixed_table();
alignas(16) __device__ const cubic::CoeffTable kCoeffTab = cubic::make_coeff_table();

typedef short s16x2 __attribute__((ext_vector_type(2)));

// the 16 weights of a pixel in registers: W[4 i + j], i the row
template <typename T>
struct Weights {
    float cy[4], cx[4];  // the float32 product is formed where it is used: 8 live registers instead of 16 (4 channels would spill)
    __device__ __forceinline__ float at(int k) const { return cy[k >> 2] * cx[k & 3]; }
};
template <>
struct Weights<uint8_t> {
    uint32_t wd[8];  // int16 pairs as the table holds them: W[2 q] in the low half of wd[q]
    __device__ __forceinline__ int at(int k) const { return (k & 1) ? ((int)wd[k >> 1] >> 16) : (int)(short)(wd[k >> 1] & 0xffffu); }
};

template <typename T>
__device__ __forceinline__ Weights<T> load_weights(int fy, int fx) {
    Weights<T> W;
    if constexpr (sizeof(T) == 1) {
        const u32x4* e = reinterpret_cast<const u32x4*>(&kFixedTab.w[fy * cubic::kTabSize + fx][0]);
        const u32x4 lo = e[0], hi = e[1];
#pragma unroll
        for (int q = 0; q < 4; q++) W.wd[q] = lo[q], W.wd[4 + q] = hi[q];
    } else {
        const f32x4 cy = *reinterpret_cast<const f32x4*>(&kCoeffTab.c[fy][0]), cx = *reinterpret_cast<const f32x4*>(&kCoeffTab.c[fx][0]);
#pragma unroll
        for (int i = 0; i < 4; i++) W.cy[i] = cy[i], W.cx[i] = cx[i];
    }
    return W;
}

// clamp((sum + 16384) >> 15, 0, 255), clamped BEFORE the shift (the same value: the shift is monotonic and |sum| < 2^24).  Written as
// shift-then-clamp, two channels were selected as one v_ashr_pk_u8_i32 in six of the 8-bit kernels, and the one of them that has run
// on a device (4 channels, CONSTANT) missed parity by up to 128 where its siblings without the instruction met it: DESIGN.md 4.10.
__device__ __forceinline__ uint32_t clamp_u8(int sum) { return (uint32_t)min(max(sum + (cubic::kOne >> 1), 0), 256 * cubic::kOne - 1) >> 15; }

// Bytes b0 < b1 <= b0 + 4 of a window of dwords as the halves of a 16-bit pair: one v_perm_b32 (selectors 0-3 address the second
// operand, 4-7 the first, 0x0c gives 0).
__device__ __forceinline__ s16x2 byte_pair(const uint32_t* d, int b0, int b1) {
    const uint32_t sel = (uint32_t)(b0 & 3) | 0x0c00u | ((4u + (uint32_t)(b1 & 3)) << 16) | 0x0c000000u;
    return __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(d[b1 >> 2], d[b0 >> 2], sel));
}

// (The two paths are sample_cubic_inlier and sample_cubic_general -- warp_cubic.hip's sample_inlier and sample_general, renamed with the
// move: the map samplers' own sample_inlier is stitch_sample.h's, a header a unit may include next to this one.)
// An inlier: row i's four taps are the 4 C values at `p + i * rs`, read as one window of exactly those bytes (a load of its own
// size at the taps' own address: nothing beside them is touched, whatever the alignment).
//   sum = ((r_0 + r_1) + r_2) + r_3,  r_i = ((S_i0 W[4i] + S_i1 W[4i+1]) + S_i2 W[4i+2]) + S_i3 W[4i+3]
// 8-bit: integers, so the order is free -- two v_dot2_i32_i16 per row and channel on (tap, tap + 1) pairs against the weight pairs.
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> sample_cubic_inlier(const uint8_t* __restrict__ p, int64_t rs, const Weights<T>& W) {
    Pixel<T, C> out;
    if constexpr (sizeof(T) == 1) {
        int acc[C];
#pragma unroll
        for (int k = 0; k < C; k++) acc[k] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t d[C];
            __builtin_memcpy(d, p + i * rs, 4 * C);
#pragma unroll
            for (int k = 0; k < C; k++) {
                acc[k] = __builtin_amdgcn_sdot2(byte_pair(d, k, C + k), __builtin_bit_cast(s16x2, W.wd[2 * i]), acc[k], false);
                acc[k] = __builtin_amdgcn_sdot2(byte_pair(d, 2 * C + k, 3 * C + k), __builtin_bit_cast(s16x2, W.wd[2 * i + 1]), acc[k], false);
            }
        }
        out.packed = 0;
#pragma unroll
        for (int k = 0; k < C; k++) out.packed |= clamp_u8(acc[k]) << (8 * k);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float v[4 * C];
            __builtin_memcpy(v, reinterpret_cast<const float*>(p + i * rs), 16 * C);
#pragma unroll
            for (int k = 0; k < C; k++) {
                const float r = ((v[k] * W.at(4 * i) + v[C + k] * W.at(4 * i + 1)) + v[2 * C + k] * W.at(4 * i + 2)) + v[3 * C + k] * W.at(4 * i + 3);
                out.v[k] = i == 0 ? r : out.v[k] + r;
            }
        }
    }
    return out;
}

// the border value itself, as a pixel
template <typename T, int C, class Args>
__device__ __forceinline__ Pixel<T, C> cubic_border_pixel(const Args& a) {
    Pixel<T, C> out;
    if constexpr (sizeof(T) == 1) {
        out.packed = 0;
#pragma unroll
        for (int k = 0; k < C; k++) out.packed |= (uint32_t)a.cv_int(k) << (8 * k);
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) out.v[k] = a.cv_float(k);
    }
    return out;
}

// Every other written pixel: x_j = borderInterpolate(sx + j), y_i = borderInterpolate(sy + i) (-1 = outside, BORDER_CONSTANT only),
//   sum = cv * ONE;  for i, for j:  sum = sum + (S[y_i][x_j] - cv) * W[4i + j]   (taps with a negative index skipped)
// in exactly this order for float32.  MODE is the remap's mode: REFLECT_101 for BORDER_TRANSPARENT.  Loads go to a clamped index
// (always a source pixel) and a skipped tap's sum is kept by a select, so the 16 loads issue together.  (sx, sy): the window's first tap.
template <typename T, int C, int MODE, class Args>
__device__ __forceinline__ Pixel<T, C> sample_cubic_general(const Args& a, const uint8_t* __restrict__ frame, int sx, int sy, const Weights<T>& W) {
    if (MODE == BEVWARP_BORDER_CONSTANT && (sx >= a.src_w || sx + 4 <= 0 || sy >= a.src_h || sy + 4 <= 0)) return cubic_border_pixel<T, C>(a);
    int xi[4], yi[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        xi[j] = cubic::window_index(MODE, sx + j, a.src_w, a.per_x, a.off_x, a.mag_x);
        yi[j] = cubic::window_index(MODE, sy + j, a.src_h, a.per_y, a.off_y, a.mag_y);
    }
    using Acc = std::conditional_t<sizeof(T) == 1, int, float>;
    Acc cv[C], acc[C];
#pragma unroll
    for (int k = 0; k < C; k++) {
        if constexpr (sizeof(T) == 1)
            cv[k] = a.cv_int(k), acc[k] = cv[k] * cubic::kOne;
        else
            cv[k] = a.cv_float(k), acc[k] = cv[k] * 1.f;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint8_t* row = frame + (int64_t)max(yi[i], 0) * a.src_rs;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = MODE != BEVWARP_BORDER_CONSTANT || (xi[j] >= 0 && yi[i] >= 0);
            const Pixel<T, C> t = load_pixel<T, C>(row, max(xi[j], 0), a.src_vec_ok);
#pragma unroll
            for (int k = 0; k < C; k++) {
                Acc s;
                if constexpr (sizeof(T) == 1)
                    s = (int)((t.packed >> (8 * k)) & 0xffu);
                else
                    s = t.v[k];
                const Acc next = acc[k] + (s - cv[k]) * W.at(4 * i + j);
                acc[k] = ok ? next : acc[k];
            }
        }
    }
    Pixel<T, C> out;
    if constexpr (sizeof(T) == 1) {
        out.packed = 0;
#pragma unroll
        for (int k = 0; k < C; k++) out.packed |= clamp_u8(acc[k]) << (8 * k);
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) out.v[k] = acc[k];
    }
    return out;
}

}  // namespace
}  // namespace bevwarp
