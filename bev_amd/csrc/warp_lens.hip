// warp_lens.hip -- the perspective warp of frames as a distorted camera delivers them (bevwarp_warp_lens): destination pixel ->
// normalised undistorted camera plane (M_ray) -> OpenCV's rational lens model -> one sample from the raw frame.  8-bit and float32
// pixels, 1-4 channels, nearest and bilinear, BORDER_CONSTANT and BORDER_TRANSPARENT.  See DESIGN.md section 4.15.
//
// The frame -- item decoding, the row walk of the exact float64 chain, the rounding with the reference's NaN, a pixel's load and the
// store of a lane's 4 pixels -- is flat_frame.h; the lens step (float64, every operation rounded on its own: the definition in
// include/bevwarp.h, operation for operation) and the blend of four taps are lens_pixel.h, shared with the map builder.  This unit adds
// a sampler that guards each tap against the frame, and the launcher.
// The lens and r2_max are kernel arguments: wave-uniform, they stay in scalar registers and cost no vector register.
#include "warp_lens.h"
#include "lens_pixel.h"

namespace bevwarp {
namespace {

template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> border_pixel(const LensArgs& a) {
    Pixel<T, C> p;
    if constexpr (sizeof(T) == 1) {
        p.packed = a.bv_u8;
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = a.bv_f[k];
    }
    return p;
}

// an inlier's taps: all four are source pixels
template <typename T, int C, int INTERP>
__device__ __forceinline__ Pixel<T, C> sample_inside(const uint8_t* __restrict__ frame, int64_t rs, int sx, int sy, int fx, int fy, bool vec) {
    const uint8_t* r0 = frame + (int64_t)sy * rs;
    if (INTERP == kNearest) return load_pixel<T, C>(r0, sx, vec);
    const uint8_t* r1 = r0 + rs;
    return blend_taps<T, C>(load_pixel<T, C>(r0, sx, vec), load_pixel<T, C>(r0, sx + 1, vec), load_pixel<T, C>(r1, sx, vec), load_pixel<T, C>(r1, sx + 1, vec), fx, fy);
}

// The constant border: a tap inside the frame is its pixel, a tap outside -- every tap of an invalid pixel -- the border pixel; a pixel
// whose four taps are all outside is the border value itself.  Every tap is loaded from the CLAMPED position (always a source pixel, also
// for the lanes past the row's end) and replaced afterwards, so the loads are unconditional and all issue before the first wait.
template <typename T, int C, int INTERP>
__device__ __forceinline__ Pixel<T, C> sample_guarded(const LensArgs& a, const uint8_t* __restrict__ frame, int sx, int sy, int fx, int fy, bool valid, bool vec) {
    const Pixel<T, C> b = border_pixel<T, C>(a);
    const int w = a.src_w, h = a.src_h;
    const bool xin0 = (unsigned)sx < (unsigned)w, yin0 = (unsigned)sy < (unsigned)h;
    const int cx0 = min(max(sx, 0), w - 1), cy0 = min(max(sy, 0), h - 1);
    const uint8_t* r0 = frame + (int64_t)cy0 * a.src_rs;
    if (INTERP == kNearest) {
        const Pixel<T, C> p = load_pixel<T, C>(r0, cx0, vec);
        return (valid && xin0 && yin0) ? p : b;
    }
    const bool xin1 = (unsigned)(sx + 1) < (unsigned)w, yin1 = (unsigned)(sy + 1) < (unsigned)h;
    const int cx1 = min(max(sx + 1, 0), w - 1), cy1 = min(max(sy + 1, 0), h - 1);
    const uint8_t* r1 = frame + (int64_t)cy1 * a.src_rs;
    const Pixel<T, C> t00 = load_pixel<T, C>(r0, cx0, vec), t01 = load_pixel<T, C>(r0, cx1, vec);
    const Pixel<T, C> t10 = load_pixel<T, C>(r1, cx0, vec), t11 = load_pixel<T, C>(r1, cx1, vec);
    const Pixel<T, C> out = blend_taps<T, C>((valid && xin0 && yin0) ? t00 : b, (valid && xin1 && yin0) ? t01 : b, (valid && xin0 && yin1) ? t10 : b,
                                             (valid && xin1 && yin1) ? t11 : b, fx, fy);
    // (8-bit pixels: the blend of four border pixels is the border pixel)
    const bool all_out = !valid || !(xin0 || xin1) || !(yin0 || yin1);
    return (sizeof(T) == 4 && all_out) ? b : out;
}

template <typename T, int C, int INTERP, bool TRANSPARENT>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_lens_kernel(const LensArgs a) {
    constexpr int PPL = kBorderPPL;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);
    const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
    const bool vec = a.src_vec_ok;

    Pixel<T, C> px[PPL];
    bool wr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other and not stored
        const int x = xs + j;
        double Xn, Yn, W;
        walk.pixel(a, x, Xn, Yn, W);
        int X, Y;
        const bool valid = lens_pixel<INTERP>(a, Xn, Yn, W, X, Y);
        const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
        const int fx = INTERP == kLinear ? (X & 31) : 0, fy = INTERP == kLinear ? (Y & 31) : 0;
        if constexpr (TRANSPARENT) {
            // valid inliers only (bevwarp_warp_border's test); every other pixel is neither read nor written
            const bool in = x < a.dst_w && valid &&
                            (INTERP == kLinear ? ((unsigned)sx < (unsigned)(a.src_w - 1) && (unsigned)sy < (unsigned)(a.src_h - 1))
                                               : ((unsigned)sx < (unsigned)a.src_w && (unsigned)sy < (unsigned)a.src_h));
            wr[j] = in;
            if (in) px[j] = sample_inside<T, C, INTERP>(frame, a.src_rs, sx, sy, fx, fy, vec);
        } else {
            wr[j] = x < a.dst_w;
            px[j] = sample_guarded<T, C, INTERP>(a, frame, sx, sy, fx, fy, valid, vec);
        }
    }

    store_lane_pixels<T, C, TRANSPARENT>(a, b, y, xs, px, wr);
}

template <typename T, int INTERP, bool TRANSPARENT>
void launch_c(const LensArgs& a, int channels, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    switch (channels) {
        case 1: hipLaunchKernelGGL((warp_lens_kernel<T, 1, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((warp_lens_kernel<T, 2, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((warp_lens_kernel<T, 3, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((warp_lens_kernel<T, 4, INTERP, TRANSPARENT>), grid, block, 0, stream, a); break;
    }
}

template <typename T, int INTERP>
void launch_mode(const LensArgs& a, int channels, bool transparent, dim3 grid, hipStream_t stream) {
    if (transparent)
        launch_c<T, INTERP, true>(a, channels, grid, stream);
    else
        launch_c<T, INTERP, false>(a, channels, grid, stream);
}

}  // namespace

hipError_t launch_warp_lens(const LensArgs& a, int dtype, int channels, int interp, bool transparent, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    if (dtype == 0)
        (interp == kNearest ? launch_mode<uint8_t, kNearest> : launch_mode<uint8_t, kLinear>)(a, channels, transparent, grid, stream);
    else
        (interp == kNearest ? launch_mode<float, kNearest> : launch_mode<float, kLinear>)(a, channels, transparent, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
