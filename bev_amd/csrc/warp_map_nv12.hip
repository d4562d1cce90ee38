// warp_map_nv12.hip -- NV12 frames sampled through a fixed camera's warp map (bevwarp_remap_nv12, bevwarp_remap_nv12_planes; DESIGN.md
// section 4.19): bevwarp_remap of the converted frame, bit for bit, with every tap converted before the blend (OpenCV's 8-bit
// YUV420sp -> RGB fixed point, nv12_sample.h) and the converted frame never in memory.  The map carries the lens, so there is no float64
// here either.  The structure is remap_kernel's (warp_map.hip): a workgroup loads its tile's map entries once, derives what does not
// depend on the frame -- per pixel the byte offsets of the taps in the Y plane and in the plane of (U, V) pairs, the weights, and the
// inside mask (BORDER_CONSTANT) or the write mask (BORDER_TRANSPARENT) -- and walks frames_per_item frames with that in registers.
//
// The frame is flat_frame.h; the map loads (map_entry.h) and the index stage (map_entry_taps.inc) are shared with remap_kernel; what a
// lane keeps of an entry and one pixel from it are remap_sample_nv12.h, shared with warp_map_nv12_out.hip; conversion and blend are
// nv12_sample.h; the BGR store is store_lane_pixels and the plane store plane_store.inc, shared with warp_nv12_planes.hip.
//
// The tap gathers bind this kernel as they bind remap_kernel: tap by tap a bilinear pixel takes 8 loads per
// frame, 4 bytes of Y and 4 pairs.  Where the two taps of a row are adjacent columns c and c + 1 they are the two bytes of ONE 2-byte
// window of the Y row, and their pairs -- the same pair or two adjacent ones -- lie in ONE 4-byte window of the row of pairs that starts
// at pair min(c >> 1, src_w / 2 - 2): 4 loads.  Which form a lane takes is frame-invariant and decided once per item, as remap_kernel
// decides `pair`: a lane whose 4 pixels all have adjacent columns -- every inlier, every interior pixel -- takes the windows; a lane with
// a clamped or remapped edge tap, and every lane of a source 2 px wide, takes the loads tap by tap.  Neither form reads a byte outside
// the first src_w bytes of a plane row.
#include "warp_map_nv12.h"
#include "map_entry.h"
#include "remap_sample_nv12.h"
#include "warp_kernels.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// a lane's 4 pixels of one frame
template <int INTERP, int MODE, int RGB, bool WINDOW>
__device__ __forceinline__ void frame_pixels_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, const NvTaps (&tap)[kBorderPPL],
                                                  const bool (&wr)[kBorderPPL], uint32_t border, uint32_t (&p)[kBorderPPL]) {
#pragma unroll
    for (int j = 0; j < kBorderPPL; j++) {
        if constexpr (MODE == kBorderTransparent) {
            if (wr[j]) p[j] = sample_entry_nv12<INTERP, MODE, RGB, WINDOW>(yf, uvf, tap[j], border);
        } else {
            p[j] = sample_entry_nv12<INTERP, MODE, RGB, WINDOW>(yf, uvf, tap[j], border);
        }
    }
}

// The kernels' common body; store(b, y, xs, p, wr) writes a lane's 4 pixels of frame b.
template <int INTERP, int MODE, int RGB, class Store>
__device__ __forceinline__ void remap_nv12_body(const RemapNv12Args& a, Store store) {
#include "remap_taps_nv12.inc"
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
        const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;
        uint32_t p[PPL];
        if constexpr (kWindows) {
            if (window)
                frame_pixels_nv12<INTERP, MODE, RGB, true>(yf, uvf, tap, wr, border, p);
            else
                frame_pixels_nv12<INTERP, MODE, RGB, false>(yf, uvf, tap, wr, border, p);
        } else {
            frame_pixels_nv12<INTERP, MODE, RGB, false>(yf, uvf, tap, wr, border, p);
        }
        store(b, y, xs, p, wr);
    }
}

// 8-bit pixels of 3 channels, B, G, R or R, G, B
template <int INTERP, int MODE, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_nv12_kernel(const RemapNv12Args a) {
    remap_nv12_body<INTERP, MODE, RGB>(a, [&](uint32_t b, int y, int xs, const uint32_t (&p)[kBorderPPL], const bool (&wr)[kBorderPPL]) __attribute__((always_inline)) {
        Pixel<uint8_t, 3> px[kBorderPPL];
#pragma unroll
        for (int j = 0; j < kBorderPPL; j++) px[j].packed = p[j];
        store_lane_pixels<uint8_t, 3, MODE == kBorderTransparent>(a, b, y, xs, px, wr);
    });
}

// channel planes: the kernel samples B, G, R (the host's table points each sampled channel at its plane); every pixel is written
template <int INTERP, int MODE, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_nv12_planes_kernel(const RemapNv12PlanesArgs a) {
    static_assert(MODE != kBorderTransparent, "the plane stage writes every pixel");
    remap_nv12_body<INTERP, MODE, 0>(a, [&](uint32_t b, int y, int xs, const uint32_t (&p)[kBorderPPL], const bool (&)[kBorderPPL]) __attribute__((always_inline)) {
        constexpr int PPL = kBorderPPL;
#include "plane_store.inc"
    });
}

}  // namespace

hipError_t launch_remap_nv12(const RemapNv12Args& a, int interp, int mode, int rgb_order, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<0, kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101, kBorderTransparent>(mode, [&](auto m) {
                pick::flag(rgb_order, [&](auto rgb) { launch(remap_nv12_kernel<i(), m(), rgb()>); });
            });
        });
    });
}

// (the plane stage writes every pixel: no transparent instance)
hipError_t launch_remap_nv12_planes(const RemapNv12PlanesArgs& a, int interp, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<0, kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101>(mode, [&](auto m) {
                pick::flag(a.plane != kPlaneF32, [&](auto wide16) { launch(remap_nv12_planes_kernel<i(), m(), wide16()>); });
            });
        });
    });
}

}  // namespace bevwarp
