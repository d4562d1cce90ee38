// warp_cubic.hip -- the bicubic perspective warp (BEVWARP_CUBIC = cv2.INTER_CUBIC): 8-bit and float32 pixels, 1-4 channels, all six
// border modes.  OpenCV 3.x-4.x's remapBicubic restated from memory (parity unpinned, like the rest of the warp); the definition is
// in include/bevwarp.h and DESIGN.md section 4.10, the tables in cubic_tab.h.
//
// The frame is flat_frame.h's, shared with the border and NV12 kernels: a flat grid, a lane owns 4 consecutive pixels of one destination
// row, the exact float64 coordinate chain per pixel, int16 saturation before anything else, wide stores for lanes that write all 4
// pixels.  The sampler is cubic_sample.h's, shared with the map kernel (warp_map_cubic.hip), in two paths: inliers (all 16 taps inside the
// source) by row windows, every other written pixel tap by tap.  A wave diverges where a row segment crosses the frame's edge.
#include "cubic_sample.h"
#include "warp_cubic.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

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
            px[j] = sample_cubic_inlier<T, C>(frame + (int64_t)sy * a.src_rs + (uint32_t)(sx * C * (int)sizeof(T)), a.src_rs, W);
        else
            px[j] = sample_cubic_general<T, C, kRemap>(a, frame, sx, sy, W);
    }
    store_lane_pixels<T, C, true>(a, b, y, xs, px, wr);
}

}  // namespace

hipError_t launch_warp_cubic(const CubicArgs& a, int dtype, int channels, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<BEVWARP_BORDER_CONSTANT, BEVWARP_BORDER_REPLICATE, BEVWARP_BORDER_REFLECT, BEVWARP_BORDER_WRAP, BEVWARP_BORDER_REFLECT_101,
                        BEVWARP_BORDER_TRANSPARENT>(mode, [&](auto m) {
                pick::channels(channels, [&](auto c) { launch(warp_cubic_kernel<typename decltype(t)::type, c(), m()>); });
            });
        });
    });
}

}  // namespace bevwarp
