// warp_map_nv12_out.hip -- frames sampled through a fixed camera's warp map and written as NV12 for a video encoder (bevwarp_remap_to_nv12,
// bevwarp_remap_nv12_to_nv12): BGR -> NV12 of bevwarp_remap's (bevwarp_remap_nv12's) 8-bit pixel, bit for bit, with
// the sampled BGR frame never in memory.  The map carries the lens, so there is no float64 here.  The structure is remap_kernel's
// (warp_map.hip) and remap_nv12_body's (warp_map_nv12.hip): a workgroup loads its tile's map entries once, derives what does not depend on
// the frame -- the taps' byte offsets, the weights, the inside mask (BORDER_CONSTANT) -- and walks frames_per_item frames with that in
// registers.  The five border modes that write every pixel; BORDER_TRANSPARENT has no instance.
//
// The frame is flat_frame.h; the map loads (map_entry.h) and the index stage (map_entry_taps.inc) are shared with those two units; the
// conversion of NV12 taps and the blend are nv12_sample.h and sample.h; the store is nv12_store.h, shared with
// warp_stitch_maps_nv12_out.hip.  The samplers are shared too: remap_sample_u8x3.h (BGR sources, the 6-byte pair loads; with
// warp_map_planes.hip) and remap_sample_nv12.h (NV12 sources, the 2-byte Y and 4-byte pair windows, convert_packed; with warp_map_nv12.hip).
#include "warp_map_nv12_out.h"
#include "map_entry.h"
#include "remap_sample_nv12.h"
#include "remap_sample_u8x3.h"
#include "warp_kernels.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// ---- 8-bit BGR / RGB frames (remap_sample_u8x3.h) ---------------------------------------------------------------------------------------------
template <int INTERP, int MODE, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_to_nv12_kernel(const RemapNv12OutArgs a) {
    static_assert(MODE != kBorderTransparent, "the NV12 store writes every pixel");
#include "remap_taps_u8x3.inc"
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
        uint32_t p[PPL];
#include "remap_frame_u8x3.inc"
        store_lane_nv12<RGB>(a, a, b, y, xs, p);
    }
}

// ---- NV12 frames, sampled as B, G, R (remap_sample_nv12.h) -------------------------------------------------------------------------------
template <int INTERP, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_nv12_to_nv12_kernel(const RemapNv12OutArgs a) {
    static_assert(MODE != kBorderTransparent, "the NV12 store writes every pixel");
#include "remap_taps_nv12.inc"
    (void)wr;  // (every pixel of the row is written: the row's end is the store's to judge)
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
        const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;
        uint32_t p[PPL];
        if constexpr (kWindows) {
            if (window) {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry_nv12<INTERP, MODE, 0, true>(yf, uvf, tap[j], border);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry_nv12<INTERP, MODE, 0, false>(yf, uvf, tap[j], border);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) p[j] = sample_entry_nv12<INTERP, MODE, 0, false>(yf, uvf, tap[j], border);
        }
        store_lane_nv12<0>(a, a, b, y, xs, p);
    }
}

}  // namespace

hipError_t launch_remap_nv12_out(const RemapNv12OutArgs& a, int nv12_src, int interp, int mode, int rgb_order, int64_t items, hipStream_t stream) {
    const int source = nv12_src ? 2 : (rgb_order ? 1 : 0);  // 0 = B, G, R frames, 1 = R, G, B frames, 2 = NV12 frames
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<0, kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101>(mode, [&](auto m) {
                pick::value<2, 1, 0>(source, [&](auto s) {
                    if constexpr (s() == 2)
                        launch(remap_nv12_to_nv12_kernel<i(), m()>);
                    else
                        launch(remap_to_nv12_kernel<i(), m(), s()>);
                });
            });
        });
    });
}

}  // namespace bevwarp
