// warp_border.hip -- the perspective warp with OpenCV's other borders (bevwarp_warp_border): REPLICATE, REFLECT, WRAP and
// REFLECT_101 read a source pixel for every tap, TRANSPARENT writes inliers only.  8-bit and float32 pixels, 1-4 channels,
// nearest and bilinear.  See DESIGN.md section 4.9.
//
// A kernel of its own, not a mode of warp_rows: that kernel's tile classes assume the constant border (its outside tiles store
// the constant without computing a coordinate, its edge tiles guard taps against the frame), its register budget is what
// bounds it, and bench.py times it.  Here every tap index goes through borderInterpolate first, after which it IS a source
// pixel: interior and exterior pixels run the same straight-line code (index remap, gathers, blend, store) -- no tile
// classification, no guarded reads.  The coordinates are the reference's exact float64 chain, pixel by pixel.
//
// The frame -- item decoding, the coordinate walk, the rounding with the reference's NaN, a pixel's load and the store of a lane's 4
// pixels, the taps of a pixel and their blend -- is flat_frame.h, shared with the bicubic, NV12 and stitch kernels; the index remap is
// warp_border.h (the remap kernel takes it too); this unit holds the kernel body.
#include "warp_border.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

template <typename T, int C, int INTERP, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_border_kernel(const BorderArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = MODE == kBorderTransparent;
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
        // pixels past the row's end are computed like any other (their taps are source pixels too) and not stored
        const int x = xs + j;
        double Xn, Yn, W;
        walk.pixel(a, x, Xn, Yn, W);
        int X, Y;
        map_pixel_exact_nan_max<INTERP>(Xn, Yn, W, X, Y);
        const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
        const int fx = INTERP == kLinear ? (X & 31) : 0, fy = INTERP == kLinear ? (Y & 31) : 0;
        if constexpr (kTransparent) {
            // inliers only (remapBilinear's (unsigned)sx < width - 1: an identity warp leaves the last column and row alone)
            const bool in = x < a.dst_w && (INTERP == kLinear ? ((unsigned)sx < (unsigned)(a.src_w - 1) && (unsigned)sy < (unsigned)(a.src_h - 1))
                                                             : ((unsigned)sx < (unsigned)a.src_w && (unsigned)sy < (unsigned)a.src_h));
            wr[j] = in;
            if (in) px[j] = sample_taps<T, C, INTERP>(frame, a.src_rs, sx, sx + 1, sy, sy + 1, fx, fy, vec);
        } else {
            wr[j] = x < a.dst_w;
            const int cx0 = border_index<MODE>(sx, a.src_w, a.per_x, a.off_x, a.mag_x);
            const int cy0 = border_index<MODE>(sy, a.src_h, a.per_y, a.off_y, a.mag_y);
            const int cx1 = INTERP == kLinear ? border_index<MODE>(sx + 1, a.src_w, a.per_x, a.off_x, a.mag_x) : cx0;
            const int cy1 = INTERP == kLinear ? border_index<MODE>(sy + 1, a.src_h, a.per_y, a.off_y, a.mag_y) : cy0;
            px[j] = sample_taps<T, C, INTERP>(frame, a.src_rs, cx0, cx1, cy0, cy1, fx, fy, vec);
        }
    }

    store_lane_pixels<T, C, kTransparent>(a, b, y, xs, px, wr);
}

}  // namespace

hipError_t launch_warp_border(const BorderArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<kNearest, kLinear>(interp, [&](auto i) {
                pick::value<kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101, kBorderTransparent>(mode, [&](auto m) {
                    pick::channels(channels, [&](auto c) { launch(warp_border_kernel<typename decltype(t)::type, c(), i(), m()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
