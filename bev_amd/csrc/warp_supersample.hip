// warp_supersample.hip -- the supersampled perspective warp (bevwarp_warp_border under BEVWARP_SUPERSAMPLE_2 / _4 / _8): a destination
// pixel is the average of the k x k pixels that bevwarp_warp_border writes at (k x + i, k y + j) of a k times finer destination, whose
// inverse matrix F maps the fine pixels' centres.  One pass: the k^2 fine pixels are sampled and reduced in registers, no fine frame is
// ever in memory.  8-bit and float32 pixels, 1-4 channels, nearest and bilinear, the five borders that write every pixel.  See DESIGN.md
// section 4.26.
//
// The frame is flat_frame.h on the DESTINATION grid (a wave per row, 4 pixels per lane, store_lane_pixels); the coordinate walk is RowWalk
// over the fine rows k y + j with the fine matrix, and FrameArgs::bw0 is the FINE grid's evaluation block width -- no multiple of k in
// general, so a destination pixel's sub-columns may straddle two blocks and the block origin is found per sub-sample (RowWalk::pixel).
// The index remap is warp_border.h's, the taps and their blend sample_taps, the constant border the guarded sampler of lens_sample.h.
// k is a loop bound, not a template parameter: 80 instances, as many as warp_border.hip.
#include "warp_supersample.h"
#include "lens_sample.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// the pixel bevwarp_warp_border writes at column x of the fine row `walk` stands on
template <typename T, int C, int INTERP, int MODE>
__device__ __forceinline__ Pixel<T, C> fine_pixel(const SupersampleArgs& a, RowWalk& walk, const uint8_t* __restrict__ frame, int x, bool vec) {
    double Xn, Yn, W;
    walk.pixel(a, x, Xn, Yn, W);
    int X, Y;
    map_pixel_exact_nan_max<INTERP>(Xn, Yn, W, X, Y);
    const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
    const int fx = INTERP == kLinear ? (X & 31) : 0, fy = INTERP == kLinear ? (Y & 31) : 0;
    if constexpr (MODE == kBorderConstant) {
        return sample_guarded<T, C, INTERP>(a, frame, sx, sy, fx, fy, true, vec);
    } else {
        const int cx0 = border_index<MODE>(sx, a.src_w, a.per_x, a.off_x, a.mag_x);
        const int cy0 = border_index<MODE>(sy, a.src_h, a.per_y, a.off_y, a.mag_y);
        const int cx1 = INTERP == kLinear ? border_index<MODE>(sx + 1, a.src_w, a.per_x, a.off_x, a.mag_x) : cx0;
        const int cy1 = INTERP == kLinear ? border_index<MODE>(sy + 1, a.src_h, a.per_y, a.off_y, a.mag_y) : cy0;
        return sample_taps<T, C, INTERP>(frame, a.src_rs, cx0, cx1, cy0, cy1, fx, fy, vec);
    }
}

// The running reduce of one destination pixel.  8-bit: the channel sums (at most 64 * 255) as 16-bit halves of two dwords, channels 0 and
// 2 in one, 1 and 3 in the other; (sum + k^2 / 2) >> 2 log2 k.  float32: acc = acc + s in the order the sub-samples come, every addition
// rounded to float32, then one multiply by 1 / k^2.  The accumulator starts as -0, the one float that leaves every first sample as it is
// (-0 + s == s for every s, +0 and -0 included), so the first sub-sample needs no branch.
template <typename T, int C>
struct Reduce {
    float acc[C];
    __device__ __forceinline__ Reduce() {
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = -0.0f;
    }
    __device__ __forceinline__ void add(const Pixel<T, C>& s) {
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = acc[c] + s.v[c];
    }
    __device__ __forceinline__ Pixel<T, C> result(int log2k) const {
        const float inv = __builtin_bit_cast(float, (uint32_t)(127 - 2 * log2k) << 23);  // 1 / k^2
        Pixel<T, C> p;
#pragma unroll
        for (int c = 0; c < C; c++) p.v[c] = acc[c] * inv;
        return p;
    }
};
template <int C>
struct Reduce<uint8_t, C> {
    uint32_t s02 = 0, s13 = 0;
    __device__ __forceinline__ void add(const Pixel<uint8_t, C>& s) {
        s02 += s.packed & 0x00ff00ffu;
        if (C > 1) s13 += (s.packed >> 8) & 0x00ff00ffu;
    }
    __device__ __forceinline__ Pixel<uint8_t, C> result(int log2k) const {
        const uint32_t half = 0x00010001u << (2 * log2k - 1);  // k^2 / 2 in both halves: no half's sum carries into the other
        Pixel<uint8_t, C> p;
        p.packed = ((s02 + half) >> (2 * log2k)) & 0x00ff00ffu;
        if (C > 1) p.packed |= (((s13 + half) >> (2 * log2k)) & 0x00ff00ffu) << 8;
        return p;
    }
};

template <typename T, int C, int INTERP, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_supersample_kernel(const SupersampleArgs a) {
    constexpr int PPL = kBorderPPL;
    uint32_t b;
    int y, xs;  // frame, destination row, the lane's first destination pixel
    if (!lane_position(a, b, y, xs)) return;
    const int log2k = a.log2k, k = 1 << log2k;

    // The fine matrix (include/bevwarp.h): the centre of fine pixel (x', y') is the destination coordinate ((x' + 0.5) / k - 0.5, ...).
    // Wave-uniform; M * (1 / k) is M / k to the bit (a power of two), every other operation is rounded on its own.
    const double* __restrict__ M = a.minv + (int64_t)b * a.m_stride;
    double F[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double m0 = M[3 * r], m1 = M[3 * r + 1];
        F[3 * r] = m0 * a.inv_k, F[3 * r + 1] = m1 * a.inv_k;
        F[3 * r + 2] = (m0 * a.centre + m1 * a.centre) + M[3 * r + 2];
    }
    RowWalk walk(F, k * y);
    const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
    const bool vec = a.src_vec_ok;

    // Fine rows outermost, then the lane's destination pixels, then a pixel's sub-columns: every pixel sees its sub-samples rows outermost,
    // and the walk crosses the fine row's columns k xs .. k (xs + 4) - 1 in order (row_terms only where the evaluation block changes).
    // Pixels past the row's end are computed like any other (their taps are source pixels, or clamped) and not stored.
    Reduce<T, C> sum[PPL];
#pragma unroll 1
    for (int j = 0; j < k; j++) {
        walk.y = k * y + j, walk.bx = -1;
#pragma unroll
        for (int p = 0; p < PPL; p++) {
            const int x0 = (xs + p) << log2k;
#pragma unroll 1
            for (int i = 0; i < k; i += 2) {  // (k is even: two sub-samples' gathers in flight)
                const Pixel<T, C> s0 = fine_pixel<T, C, INTERP, MODE>(a, walk, frame, x0 + i, vec);
                const Pixel<T, C> s1 = fine_pixel<T, C, INTERP, MODE>(a, walk, frame, x0 + i + 1, vec);
                sum[p].add(s0);
                sum[p].add(s1);
            }
        }
    }

    Pixel<T, C> px[PPL];
    bool wr[PPL];
#pragma unroll
    for (int p = 0; p < PPL; p++) px[p] = sum[p].result(log2k), wr[p] = xs + p < a.dst_w;
    store_lane_pixels<T, C, false>(a, b, y, xs, px, wr);
}

}  // namespace

hipError_t launch_warp_supersample(const SupersampleArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<kNearest, kLinear>(interp, [&](auto i) {
                pick::value<kBorderConstant, kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101>(mode, [&](auto m) {
                    pick::channels(channels, [&](auto c) { launch(warp_supersample_kernel<typename decltype(t)::type, c(), i(), m()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
