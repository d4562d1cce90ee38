// map_entry.h -- what the map samplers do with a map before they touch a frame (device code, gfx950), shared by warp_map.hip's
// remap_kernel (interleaved frames) and warp_map_nv12.hip (NV12 frames): a lane's 4 entries loaded once here, and per entry the index
// stage -- (sx, sy) -> the four taps' source columns and rows under the border mode, which taps lie inside (BORDER_CONSTANT) and whether
// the pixel is written (BORDER_TRANSPARENT) -- in map_entry_taps.inc, text both kernels include in their per-pixel loop, the way the row
// kernel's rows_*.inc are shared: as a function the stage changed remap_kernel's machine code, as text it does not.  Everything here is
// frame-invariant under a shared map.  See DESIGN.md sections 4.18, 4.19.  Not installed.
#pragma once
#include "warp_map.h"

namespace bevwarp {
namespace {

// The lane's map entries of row y, first pixel xs, map of frame b0: wide loads where all 4 pixels lie in the row and the planes' layout
// admits them; no entry past the row's end is read (such a lane's entry is 0: the source's first pixel, never stored).  fr: bilinear only.
template <int INTERP>
__device__ __forceinline__ void load_entries(const RemapArgs& a, int b0, int y, int xs, uint32_t (&e)[kBorderPPL], uint32_t (&fr)[kBorderPPL]) {
    constexpr int PPL = kBorderPPL;
    const bool whole = xs + PPL <= a.dst_w;
    const uint8_t* xrow = a.xy + (int64_t)b0 * a.xy_fs + (int64_t)y * a.xy_rs + (int64_t)xs * 4;
    if (a.map_vec_ok && whole) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xrow);
        e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < PPL; j++) e[j] = (xs + j < a.dst_w) ? reinterpret_cast<const uint32_t*>(xrow)[j] : 0u;
    }
    if constexpr (INTERP == kLinear) {
        const uint8_t* frow = a.frac + (int64_t)b0 * a.frac_fs + (int64_t)y * a.frac_rs + (int64_t)xs * 2;
        if (a.map_vec_ok && whole) {
            const u32x2 v = *reinterpret_cast<const u32x2*>(frow);
            fr[0] = v.x & 0xffffu, fr[1] = v.x >> 16, fr[2] = v.y & 0xffffu, fr[3] = v.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) fr[j] = (xs + j < a.dst_w) ? (uint32_t)reinterpret_cast<const uint16_t*>(frow)[j] : 0u;
        }
    }
}

}  // namespace
}  // namespace bevwarp
