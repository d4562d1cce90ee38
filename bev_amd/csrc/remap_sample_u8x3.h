// remap_sample_u8x3.h -- the sampler of the remap kernels that know only 8-bit frames of 3 channels (device code, gfx950):
// remap_planes_kernel (warp_map_planes.hip) and remap_to_nv12_kernel (warp_map_nv12_out.hip).  It is warp_map.hip's sampler for
// uint8_t x 3 with the pixel packed in a uint32_t: what a lane keeps of a map entry, and one destination pixel from it.  The loads are
// tap_load.h's.  See DESIGN.md sections 4.21 and 4.22.  Not installed.
#pragma once
#include "tap_load.h"

namespace bevwarp {
namespace {

// What a lane keeps of one map entry for every frame it walks: the byte offsets of its four taps in a frame (source pixels: remapped or
// clamped; a frame is below 2 GiB), the weights, and for the constant border which of the four taps lie inside.
struct Taps {
    uint32_t a00, a01, a10, a11;
    uint32_t w;  // fx | fy << 5 | in << 10; in: map_entry_taps.inc's
    __device__ __forceinline__ uint32_t fx() const { return w & 31u; }
    __device__ __forceinline__ uint32_t fy() const { return (w >> 5) & 31u; }
    __device__ __forceinline__ uint32_t in() const { return w >> 10; }
};

// One destination pixel of one frame, packed: byte k = the source's channel k.  PAIR: both rows' taps are adjacent columns.
template <int INTERP, int MODE, bool PAIR>
__device__ __forceinline__ uint32_t sample_entry(const uint8_t* __restrict__ frame, const Taps& t, uint32_t border) {
    if constexpr (INTERP == kNearest) {
        const uint32_t p = load_at(frame, t.a00);
        return (MODE != 0 || (t.in() & 1u)) ? p : border;
    } else {
        // every load is of a source pixel (the constant border: of the CLAMPED position) and issues before the first wait
        uint32_t p00, p01, p10, p11;
        if constexpr (PAIR) {
            load_pair(frame, t.a00, p00, p01);
            load_pair(frame, t.a10, p10, p11);
        } else {
            p00 = load_at(frame, t.a00), p01 = load_at(frame, t.a01), p10 = load_at(frame, t.a10), p11 = load_at(frame, t.a11);
        }
        if constexpr (MODE == 0) {  // a tap outside is the border pixel (all four outside: the blend of four border pixels is the border pixel)
            const uint32_t in = t.in();
            p00 = (in & 1u) ? p00 : border, p01 = (in & 2u) ? p01 : border, p10 = (in & 4u) ? p10 : border, p11 = (in & 8u) ? p11 : border;
        }
        return blend_u8_packed<3>(p00, p01, p10, p11, t.fx(), t.fy());
    }
}

}  // namespace
}  // namespace bevwarp
