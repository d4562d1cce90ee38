// warp_nv12_out.hip -- the perspective warps that write NV12 frames for a video encoder (bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12):
// the warped 8-bit pixel -- bevwarp_warp's of a BGR / RGB frame, or bevwarp_warp_nv12's of a decoder's planes -- is converted with
// OpenCV's 8-bit RGB -> YUV 4:2:0 fixed point in registers and stored as a Y byte and, at even columns of even rows, a (U, V) pair: the
// result is BGR -> NV12 of the warped frame, bit for bit, and the warped frame never exists.  Constant border, nearest and bilinear.
// See DESIGN.md section 4.14.
//
// The frame is flat_frame.h's: a wave per destination row, a lane owns 4 consecutive pixels, the coordinates are the reference's exact
// float64 chain, every tap is loaded from the clamped coordinate (sample_global, sample_nv12).  Only the store stage is this unit's: no
// destination row depends on another (a pair is taken from ONE pixel, there is no averaging), so rows need not meet in a workgroup.
#include "nv12_out.h"
#include "nv12_sample.h"
#include "warp_nv12_out.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

template <int NV12_SRC, int INTERP, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_nv12_out_kernel(const Nv12OutArgs a) {
    constexpr int PPL = kBorderPPL;
    static_assert(PPL == 4, "the store stage packs 4 Y bytes and 2 pairs per lane");
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);
    const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
    const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;
    const SrcView view = {a.src + (int64_t)b * a.src_fs, a.src_rs, a.src_w, a.src_h, {0.f, 0.f, 0.f, 0.f}, a.border, false};

    uint32_t px[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other (their taps are clamped into the source too) and not stored
        double Xn, Yn, W;
        walk.pixel(a, xs + j, Xn, Yn, W);
        int X, Y;
        map_pixel_exact<INTERP>(Xn, Yn, W, X, Y);
        if constexpr (NV12_SRC)
            px[j] = sample_nv12<INTERP, 0>(yf, uvf, a.y_rs, a.uv_rs, a.src_w, a.src_h, a.border, X, Y);
        else
            px[j] = sample_global<uint8_t, 3, INTERP>(view, X, Y).packed;
    }
    // dst_w is even and xs a multiple of 4: the lane writes all 4 pixels, or -- the last lane of a row of 4 k + 2 pixels -- the first 2
    const bool all = xs + PPL <= a.dst_w;
    const Yuv601<RGB> p0(px[0]), p1(px[1]), p2(px[2]), p3(px[3]);
    const uint32_t y01 = p0.luma() | (p1.luma() << 8), y23 = p2.luma() | (p3.luma() << 8);
    uint8_t* dy = dst_row(a, b, y) + xs;
    if (a.dst_vec_ok) {  // base and strides are multiples of 4, and so is dy
        if (all)
            *reinterpret_cast<uint32_t*>(dy) = y01 | (y23 << 16);
        else
            *reinterpret_cast<uint16_t*>(dy) = (uint16_t)y01;
    } else {
        dy[0] = (uint8_t)y01, dy[1] = (uint8_t)(y01 >> 8);
        if (all) dy[2] = (uint8_t)y23, dy[3] = (uint8_t)(y23 >> 8);
    }
    // chroma: the pixel at the even column of an even row gives its 2 x 2 block's pair.  Wave-uniform: a wave is one row.
    if (y & 1) return;
    uint8_t* duv = a.dst_uv + (int64_t)b * a.duv_fs + (int64_t)(y >> 1) * a.duv_rs + xs;  // pair x / 2 lies at byte x; 2-byte aligned by contract
    const uint32_t c0 = p0.pair(), c2 = p2.pair();
    if (all && a.uv_vec_ok) {
        *reinterpret_cast<uint32_t*>(duv) = c0 | (c2 << 16);
    } else {
        *reinterpret_cast<uint16_t*>(duv) = (uint16_t)c0;
        if (all) *reinterpret_cast<uint16_t*>(duv + 2) = (uint16_t)c2;
    }
}

}  // namespace

hipError_t launch_warp_nv12_out(const Nv12OutArgs& a, int nv12_src, int interp, int rgb_order, int64_t items, hipStream_t stream) {
    const int source = nv12_src ? 2 : (rgb_order ? 1 : 0);  // 0 = B, G, R frames, 1 = R, G, B frames, 2 = NV12 frames (sampled as B, G, R)
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<2, 1, 0>(source, [&](auto s) { launch(warp_nv12_out_kernel<s() == 2, i(), s() == 1>); });
        });
    });
}

}  // namespace bevwarp
