// warp_cubic.hip -- the bicubic perspective warp (BEVWARP_CUBIC = cv2.INTER_CUBIC): 8-bit and float32 pixels, 1-4 channels, all six
// border modes.  OpenCV 3.x-4.x's remapBicubic restated from memory (parity unpinned, like the rest of the warp); the definition is
// in include/bevwarp.h and DESIGN.md section 4.10, the tables in cubic_tab.h.
//
// The frame is flat_frame.h's, shared with the border and NV12 kernels: a flat grid, a lane owns 4 consecutive pixels of one destination
// row, the exact float64 coordinate chain per pixel, int16 saturation before anything else, wide stores for lanes that write all 4
// pixels.  This unit holds the sampler, in two paths.  An INLIER (all 16 taps inside the source) loads each of its four tap rows as ONE window
// of exactly 4 C values and sums them row by row.  Every other written pixel takes the general path: eight index remaps, sixteen
// per-pixel loads, one tap at a time around the border value.  A wave diverges where a row segment crosses the frame's edge.
#include "cubic_tab.h"
#include "warp_cubic.h"

namespace bevwarp {
namespace {

// Emitted by constant evaluation of cubic_tab.h's own functions (a dynamic initialiser of a __device__ variable does not compile):
// 32 KB of fixed-point entries, one entry = 32 contiguous bytes = two 16-byte loads; float weights are formed in registers from the
// 512-byte coefficient table (the same float32 products as cubic::entry_f32).  Read-only: no state, nothing to allocate.
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

// An inlier: row i's four taps are the 4 C values at `p + i * rs`, read as one window of exactly those bytes (a load of its own
// size at the taps' own address: nothing beside them is touched, whatever the alignment).
//   sum = ((r_0 + r_1) + r_2) + r_3,  r_i = ((S_i0 W[4i] + S_i1 W[4i+1]) + S_i2 W[4i+2]) + S_i3 W[4i+3]
// 8-bit: integers, so the order is free -- two v_dot2_i32_i16 per row and channel on (tap, tap + 1) pairs against the weight pairs.
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> sample_inlier(const uint8_t* __restrict__ p, int64_t rs, const Weights<T>& W) {
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

template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> border_pixel(const CubicArgs& a) {
    Pixel<T, C> out;
    if constexpr (sizeof(T) == 1) {
        out.packed = 0;
#pragma unroll
        for (int k = 0; k < C; k++) out.packed |= (uint32_t)a.cv_u8[k] << (8 * k);
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) out.v[k] = a.cv_f[k];
    }
    return out;
}

// Every other written pixel: x_j = borderInterpolate(sx + j), y_i = borderInterpolate(sy + i) (-1 = outside, BORDER_CONSTANT only),
//   sum = cv * ONE;  for i, for j:  sum = sum + (S[y_i][x_j] - cv) * W[4i + j]   (taps with a negative index skipped)
// in exactly this order for float32.  MODE is the remap's mode: REFLECT_101 for BORDER_TRANSPARENT.  Loads go to a clamped index
// (always a source pixel) and a skipped tap's sum is kept by a select, so the 16 loads issue together.
template <typename T, int C, int MODE>
__device__ __forceinline__ Pixel<T, C> sample_general(const CubicArgs& a, const uint8_t* __restrict__ frame, int sx, int sy, const Weights<T>& W) {
    if (MODE == BEVWARP_BORDER_CONSTANT && (sx >= a.src_w || sx + 4 <= 0 || sy >= a.src_h || sy + 4 <= 0)) return border_pixel<T, C>(a);
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
            cv[k] = a.cv_u8[k], acc[k] = cv[k] * cubic::kOne;
        else
            cv[k] = a.cv_f[k], acc[k] = cv[k] * 1.f;
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

template <typename T, int C, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_cubic_kernel(const CubicArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = MODE == BEVWARP_BORDER_TRANSPARENT;
    constexpr int kRemap = kTransparent ? BEVWARP_BORDER_REFLECT_101 : MODE;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);
    const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
    // all 16 taps inside: 0 <= sx < max(w - 3, 0) and 0 <= sy < max(h - 3, 0)
    const unsigned in_w = (unsigned)max(a.src_w - 3, 0), in_h = (unsigned)max(a.src_h - 3, 0);

    Pixel<T, C> px[PPL];
    bool wr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int x = xs + j;
        double Xn, Yn, Wn;
        walk.pixel(a, x, Xn, Yn, Wn);
        int X, Y;
        map_pixel_exact_nan_max<kLinear>(Xn, Yn, Wn, X, Y);  // the bilinear warp's maps
        // the window starts one pixel before the map's position, AFTER its int16 saturation
        const int sx = sat16(X >> kInterBits) - 1, sy = sat16(Y >> kInterBits) - 1;
        const bool inl = (unsigned)sx < in_w && (unsigned)sy < in_h;
        // TRANSPARENT writes the pixels whose integer position (sx + 1, sy + 1) lies in the source (inliers are among them)
        wr[j] = x < a.dst_w && (!kTransparent || inl || ((unsigned)(sx + 1) < (unsigned)a.src_w && (unsigned)(sy + 1) < (unsigned)a.src_h));
        if constexpr (sizeof(T) == 1) px[j].packed = 0;
        if (!wr[j]) continue;  // neither read nor written
        const Weights<T> W = load_weights<T>(Y & 31, X & 31);
        if (inl)
            px[j] = sample_inlier<T, C>(frame + (int64_t)sy * a.src_rs + (uint32_t)(sx * C * (int)sizeof(T)), a.src_rs, W);
        else
            px[j] = sample_general<T, C, kRemap>(a, frame, sx, sy, W);
    }
    store_lane_pixels<T, C, true>(a, b, y, xs, px, wr);
}

template <typename T, int MODE>
void launch_c(const CubicArgs& a, int channels, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    switch (channels) {
        case 1: hipLaunchKernelGGL((warp_cubic_kernel<T, 1, MODE>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((warp_cubic_kernel<T, 2, MODE>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((warp_cubic_kernel<T, 3, MODE>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((warp_cubic_kernel<T, 4, MODE>), grid, block, 0, stream, a); break;
    }
}

template <typename T>
void launch_mode(const CubicArgs& a, int channels, int mode, dim3 grid, hipStream_t stream) {
    switch (mode) {
        case BEVWARP_BORDER_CONSTANT: launch_c<T, BEVWARP_BORDER_CONSTANT>(a, channels, grid, stream); break;
        case BEVWARP_BORDER_REPLICATE: launch_c<T, BEVWARP_BORDER_REPLICATE>(a, channels, grid, stream); break;
        case BEVWARP_BORDER_REFLECT: launch_c<T, BEVWARP_BORDER_REFLECT>(a, channels, grid, stream); break;
        case BEVWARP_BORDER_WRAP: launch_c<T, BEVWARP_BORDER_WRAP>(a, channels, grid, stream); break;
        case BEVWARP_BORDER_REFLECT_101: launch_c<T, BEVWARP_BORDER_REFLECT_101>(a, channels, grid, stream); break;
        default: launch_c<T, BEVWARP_BORDER_TRANSPARENT>(a, channels, grid, stream); break;
    }
}

}  // namespace

hipError_t launch_warp_cubic(const CubicArgs& a, int dtype, int channels, int mode, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    if (dtype == 0)
        launch_mode<uint8_t>(a, channels, mode, grid, stream);
    else
        launch_mode<float>(a, channels, mode, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
