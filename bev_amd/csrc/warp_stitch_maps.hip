// warp_stitch_maps.hip -- several fixed cameras sampled through their warp maps into one BEV canvas in one launch (bevwarp_stitch_maps,
// bevwarp_stitch_maps_nv12).  It is bevwarp_warp_stitch's camera loop and blend rules (warp_stitch.hip) over
// bevwarp_remap's map entries (warp_map.hip): per camera the lane's 4 entries replace the float64 chain, a camera covers a pixel where its
// entry passes BORDER_TRANSPARENT's inlier test against that camera's own frame, and the covering cameras are combined by OVER or FEATHER.
// The maps carry the lens, so there is no float64 here.  The NV12 instances convert every tap before the blend (nv12_sample.h), as
// bevwarp_remap_nv12 does.
//
// The frame -- item decoding and the store of a lane's 4 pixels -- is flat_frame.h; one frame per item: a lane cannot keep 8 cameras'
// entries in registers, and a shared map is re-read through the caches.  The cameras are kernel arguments and the loop's camera number is
// wave-uniform, so a camera's fields are scalar loads; whether a camera's planes admit the lane-wide map loads is one of them, and a launch
// may mix cameras that do and cameras that do not.
//
// Every sampled pixel is an inlier: bilinear taps are columns sx, sx + 1 and rows sy, sy + 1 of the source, never clamped or remapped.  So
// the 6-byte pair loads (8-bit, 3 channels) and the NV12 windows apply to every covered pixel with no per-lane decision; warp_map.hip and
// warp_map_nv12.hip, where an edge lane falls back to loads tap by tap, describe both.  A camera's entries, the inlier samplers and
// FEATHER's division are stitch_sample.h, shared with warp_stitch_maps_nv12_out.hip and warp_stitch_maps_planes.hip.
//
// warp_stitch_gain.hip is this text once more under BEVWARP_STITCH_GAIN_UNIT (warp_stitch_maps.h): the same body and launchers over
// Gained<> arguments, for 8-bit pixels of 3 channels only, every tap put through its camera's gain (stitch_sample.h: TapGain).
#include "warp_stitch_maps.h"
#include "stitch_sample.h"
#include "launch_pick.h"

#include <type_traits>

#define UNIT_KERNEL BEVWARP_STITCH_UNIT(stitch_maps_kernel, stitch_gain_kernel)
#define UNIT_KERNEL_NV12 BEVWARP_STITCH_UNIT(stitch_maps_nv12_kernel, stitch_gain_nv12_kernel)
#define UNIT_LAUNCH BEVWARP_STITCH_UNIT(launch_stitch_maps, launch_stitch_gain)
#define UNIT_LAUNCH_NV12 BEVWARP_STITCH_UNIT(launch_stitch_maps_nv12, launch_stitch_gain_nv12)

namespace bevwarp {
namespace {

using Args = UnitArgs<StitchMapsArgs>;

// The kernels' common body.  NV12: T = uint8_t, C = 3, and RGB is the destination's channel order.
template <typename T, int C, int INTERP, int BLEND, bool NV12, int RGB>
__device__ __forceinline__ void stitch_maps_body(const Args& a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kFeather = BLEND == kStitchFeather, kU8 = sizeof(T) == 1, kGained = !std::is_same_v<Args, StitchMapsArgs>;
    using Acc = std::conditional_t<kU8, int, float>;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;

    // per pixel, as in warp_stitch_kernel: OVER keeps the pixel and whether it is still undecided; FEATHER the weighted sums and the sum
    // of weights, float32 the cover count and the first covering camera's value as well
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

    // OVER runs from the last camera to the first and stops when the lane's four pixels are decided; FEATHER runs in ascending order, the
    // order of its float32 sums
    const int n = a.n_cams;
    for (int i = 0; i < n; i++) {
        if (!kFeather && !(todo[0] || todo[1] || todo[2] || todo[3])) break;
        const int k = kFeather ? i : n - 1 - i;
        const StitchMapCamera& cam = a.cams[k];
        const auto tap = camera_tap(a, k);  // (a gained launch: the camera's gain on every tap; otherwise nothing)
        uint32_t e[PPL], fr[PPL];
        load_camera_entries<INTERP>(cam, b, y, xs, a.dst_w, e, fr);
        const uint8_t* frame = cam.src + (int64_t)b * cam.src_fs;
        const uint8_t* uvf = NV12 ? cam.uv + (int64_t)b * cam.uv_fs : nullptr;
        const uint32_t rs = (uint32_t)cam.src_rs, uv_rs = (uint32_t)cam.uv_rs;  // (below 2^24: the source limits)
        const int sw = cam.src_w, sh = cam.src_h;
        const bool vec = cam.src_vec_ok, window = sw >= 4;
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (!todo[j]) continue;
            const int sx = (int)(short)(e[j] & 0xffffu), sy = (int)e[j] >> 16;
            const int fx = INTERP == kLinear ? (int)(fr[j] & 31u) : 0, fy = INTERP == kLinear ? (int)((fr[j] >> 5) & 31u) : 0;  // (higher bits are ignored)
            // bevwarp_remap's TRANSPARENT inlier test against THIS camera's frame: every tap read below is a source pixel
            const bool in = INTERP == kLinear ? ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1))
                                              : ((unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh);
            if (!in) continue;
            Pixel<T, C> p;
            if constexpr (NV12)
                p.packed = sample_inlier_nv12<INTERP, RGB>(frame, uvf, rs, uv_rs, sw, window, sx, sy, fx, fy, tap);
            else if constexpr (kGained)
                p.packed = sample_inlier<INTERP>(frame, rs, sx, sy, fx, fy, tap);  // (the packed sampler: the same pixel, by bits)
            else
                p = sample_inlier<T, C, INTERP>(frame, rs, sx, sy, fx, fy, vec);
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

template <typename T, int C, int INTERP, int BLEND>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void UNIT_KERNEL(const Args a) {
    stitch_maps_body<T, C, INTERP, BLEND, false, 0>(a);
}

template <int INTERP, int BLEND, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void UNIT_KERNEL_NV12(const Args a) {
    stitch_maps_body<uint8_t, 3, INTERP, BLEND, true, RGB>(a);
}

}  // namespace

hipError_t UNIT_LAUNCH(const UnitArgs<StitchMapsArgs>& a, int dtype, int channels, int interp, int blend, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<kStitchFeather, kStitchOver>(blend, [&](auto bl) {
#ifdef BEVWARP_STITCH_GAIN_UNIT  // (the host checks admit 8-bit pixels of 3 channels only under the flag)
                launch(UNIT_KERNEL<uint8_t, 3, i(), bl()>);
#else
                pick::pixel(dtype, [&](auto t) {
                    pick::channels(channels, [&](auto c) { launch(UNIT_KERNEL<typename decltype(t)::type, c(), i(), bl()>); });
                });
#endif
            });
        });
    });
}

hipError_t UNIT_LAUNCH_NV12(const UnitArgs<StitchMapsArgs>& a, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<kStitchFeather, kStitchOver>(blend, [&](auto bl) {
                pick::flag(rgb_order, [&](auto rgb) { launch(UNIT_KERNEL_NV12<i(), bl(), rgb()>); });
            });
        });
    });
}

}  // namespace bevwarp
