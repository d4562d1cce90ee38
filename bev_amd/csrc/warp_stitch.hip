// warp_stitch.hip -- several cameras warped into one BEV canvas in one launch (bevwarp_warp_stitch): every destination pixel runs through
// the cameras, each with frames, sizes, strides and matrices of its own; a camera covers the pixel where BORDER_TRANSPARENT's inlier test
// holds, and the covering cameras are combined by one of two rules -- OVER (the last one wins: what one bevwarp_warp_border call per camera
// leaves on a canvas) and FEATHER (integer weights that fall off towards each frame's edge).  8-bit and float32 pixels, 1-4 channels,
// nearest and bilinear.  See DESIGN.md section 4.16.
//
// The frame -- item decoding, the row walk of the exact float64 chain, the rounding with the reference's NaN, the taps of a pixel and the
// store of a lane's 4 pixels -- is flat_frame.h.  This unit adds the camera loop and the two rules; its launch is launch_pick.h's.  The cameras are kernel
// arguments and the loop's camera number is wave-uniform: a camera's fields and its matrix of the workgroup's frame are scalar loads and
// cost no vector register.  The lane's 4 pixels are walked inside the loop, so one matrix serves all four.  FEATHER's division of 8-bit
// sums, div_byte_mean, is stitch_sample.h's, shared with the stitches through warp maps.
#include "warp_stitch.h"
#include "stitch_sample.h"
#include "launch_pick.h"

#include <type_traits>

namespace bevwarp {
namespace {

template <typename T, int C, int INTERP, int BLEND>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_stitch_kernel(const StitchArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kFeather = BLEND == kStitchFeather, kU8 = sizeof(T) == 1;
    using Acc = std::conditional_t<kU8, int, float>;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;

    // Per pixel.  OVER: px is the pixel, todo says that no camera has covered it yet.  FEATHER: the weighted sums and the sum of weights;
    // float32 keeps the cover count and the first covering camera's value as well (a single cover stores that value itself; 8-bit pixels
    // need neither: (w p + (w >> 1)) / w is p).
    Pixel<T, C> px[PPL];
    bool wr[PPL], todo[PPL];
    Acc acc[PPL][C];
    int wsum[PPL], cnt[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        todo[j] = xs + j < a.dst_w;  // pixels past the row's end are neither computed nor stored
        wr[j] = false;
        wsum[j] = cnt[j] = 0;
#pragma unroll
        for (int c = 0; c < C; c++) acc[j][c] = 0;
    }

    // OVER runs from the last camera to the first and leaves a pixel alone once it is decided: every pixel is sampled once at most, and
    // the loop ends when the lane's four are.  FEATHER runs in ascending order, the order of its float32 sums.
    const int n = a.n_cams;
    for (int i = 0; i < n; i++) {
        if (!kFeather && !(todo[0] || todo[1] || todo[2] || todo[3])) break;
        const StitchCamera& cam = a.cams[kFeather ? i : n - 1 - i];
        RowWalk walk(cam.minv + (int64_t)b * cam.m_stride, y);
        const uint8_t* frame = cam.src + (int64_t)b * cam.src_fs;
        const int64_t rs = cam.src_rs;
        const int sw = cam.src_w, sh = cam.src_h;
        const bool vec = cam.src_vec_ok;
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (!todo[j]) continue;
            double Xn, Yn, W;
            walk.pixel(a, xs + j, Xn, Yn, W);
            int X, Y;
            map_pixel_exact_nan_max<INTERP>(Xn, Yn, W, X, Y);
            const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
            const int fx = INTERP == kLinear ? (X & 31) : 0, fy = INTERP == kLinear ? (Y & 31) : 0;
            // bevwarp_warp_border's TRANSPARENT inlier test against THIS camera's frame: every tap read below is a source pixel
            const bool in = INTERP == kLinear ? ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1))
                                              : ((unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh);
            if (!in) continue;
            const Pixel<T, C> p = sample_taps<T, C, INTERP>(frame, rs, sx, sx + 1, sy, sy + 1, fx, fy, vec);
            wr[j] = true;
            if constexpr (!kFeather) {
                px[j] = p;
                todo[j] = false;
            } else {
                // whole source pixels to the nearest frame edge (>= 1 for an inlier), cut off at F
                const int w = min(min(min(sx + 1, sw - sx), min(sy + 1, sh - sy)), a.feather);
                wsum[j] += w;
                if constexpr (kU8) {
#pragma unroll
                    for (int c = 0; c < C; c++) acc[j][c] += (int)((p.packed >> (8 * c)) & 0xffu) * w;  // (the sums stay below 2^23)
                } else {
                    if (cnt[j] == 0) px[j] = p;
                    cnt[j]++;
                    const float wf = (float)w;
#pragma unroll
                    for (int c = 0; c < C; c++) acc[j][c] = acc[j][c] + wf * p.v[c];  // (each rounded to float32: no FMA in this unit)
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < PPL; j++) {
        if constexpr (kFeather) {
            if (wr[j]) {
                if constexpr (kU8) {
                    uint32_t out = 0;
#pragma unroll
                    for (int c = 0; c < C; c++) out |= (uint32_t)div_byte_mean(acc[j][c] + (wsum[j] >> 1), wsum[j]) << (8 * c);
                    px[j].packed = out;
                } else if (cnt[j] > 1) {
                    const float wf = (float)wsum[j];
#pragma unroll
                    for (int c = 0; c < C; c++) px[j].v[c] = __fdiv_rn(acc[j][c], wf);  // one correctly rounded division
                }
            }
        }
        if (!wr[j] && a.fill && xs + j < a.dst_w) {  // no camera covers the pixel: the border pixel, or nothing
            wr[j] = true;
            if constexpr (kU8) {
                px[j].packed = a.bv_u8;
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) px[j].v[c] = a.bv_f[c];
            }
        }
    }

    store_lane_pixels<T, C, true>(a, b, y, xs, px, wr);
}

}  // namespace

hipError_t launch_warp_stitch(const StitchArgs& a, int dtype, int channels, int interp, int blend, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<kNearest, kLinear>(interp, [&](auto i) {
                pick::value<kStitchFeather, kStitchOver>(blend, [&](auto bl) {
                    pick::channels(channels, [&](auto c) { launch(warp_stitch_kernel<typename decltype(t)::type, c(), i(), bl()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
