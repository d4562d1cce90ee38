// warp_nv12.hip -- the perspective warp of NV12 frames into 8-bit BGR / RGB (bevwarp_warp_nv12): every tap is converted with OpenCV's
// 8-bit YUV420sp -> RGB fixed point before the blend, so the result is bevwarp_warp of the converted frame, bit for bit, and the
// converted frame never exists.  Constant border, nearest and bilinear.  See DESIGN.md section 4.12.
//
// The frame is flat_frame.h's, shared with the border and bicubic kernels: a lane owns 4 consecutive destination pixels of one row, the
// coordinates are the reference's exact float64 chain, and every pixel runs the same straight-line code, stored as 8-bit, 3-channel
// pixels by store_lane_pixels.  Each tap is loaded from the CLAMPED coordinate -- always an address inside the two planes -- and
// replaced by the border value afterwards (sample_global's rule), so all loads of a pixel issue before the first wait.
#include "nv12_sample.h"
#include "warp_nv12.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// (the sampler -- chroma_terms, convert, load_pair, sample_nv12 -- is nv12_sample.h: warp_nv12_planes.hip takes the same taps)
template <int INTERP, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_nv12_kernel(const Nv12Args a) {
    constexpr int PPL = kBorderPPL;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);
    const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
    const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;

    Pixel<uint8_t, 3> px[PPL];
    bool wr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other (their taps are clamped into the planes too) and not stored
        const int x = xs + j;
        double Xn, Yn, W;
        walk.pixel(a, x, Xn, Yn, W);
        int X, Y;
        // (a NaN coordinate lands on INT_MIN: outside, as the reference's INT_MAX is under the constant border)
        map_pixel_exact<INTERP>(Xn, Yn, W, X, Y);
        px[j].packed = sample_nv12<INTERP, RGB>(yf, uvf, a.y_rs, a.uv_rs, a.src_w, a.src_h, a.border, X, Y);
        wr[j] = x < a.dst_w;
    }
    store_lane_pixels<uint8_t, 3, false>(a, b, y, xs, px, wr);
}

}  // namespace

hipError_t launch_warp_nv12(const Nv12Args& a, int interp, int rgb_order, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) { pick::flag(rgb_order, [&](auto rgb) { launch(warp_nv12_kernel<i(), rgb()>); }); });
    });
}

}  // namespace bevwarp
