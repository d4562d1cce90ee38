// remap_sample_nv12.h -- the sampler of the remap kernels that read NV12 frames (device code, gfx950): remap_nv12_body
// (warp_map_nv12.hip) and remap_nv12_to_nv12_kernel (warp_map_nv12_out.hip).  What a lane keeps of a map entry, and one destination pixel
// from it, every tap converted before the blend (nv12_sample.h's convert_packed).  How a lane comes to take the window loads is
// warp_map_nv12.hip's account.  See DESIGN.md section 4.19.  Not installed.
#pragma once
#include "nv12_sample.h"

namespace bevwarp {
namespace {

// What a lane keeps of one map entry for every frame it walks.  All offsets are of source pixels (remapped, an inlier's, or clamped);
// a plane is below 2 GiB, so 32 bits hold them and a load is the plane's wave-uniform base plus one register.
struct NvTaps {
    uint32_t y00, y01, y10, y11;  // bytes into the Y plane; a window lane loads 2 bytes at y00 and at y10
    uint32_t u00, u01, u10, u11;  // bytes into the plane of pairs (even); a window lane loads 4 bytes at u00 and at u10 (the windows' starts)
    uint32_t w;  // fx | fy << 5 | in << 10 | s0 << 14 | s1 << 15; in: map_entry_taps.inc's; s0, s1: window lanes, which pair of the window column c0 / c1 takes
    __device__ __forceinline__ uint32_t fx() const { return w & 31u; }
    __device__ __forceinline__ uint32_t fy() const { return (w >> 5) & 31u; }
    __device__ __forceinline__ uint32_t in() const { return (w >> 10) & 15u; }
};

// a (U, V) pair at an even byte offset of a plane whose base and strides are even
__device__ __forceinline__ uint32_t pair_at(const uint8_t* __restrict__ uvf, uint32_t off) { return *reinterpret_cast<const uint16_t*>(uvf + off); }

// One destination pixel of one frame, packed in the order convert<RGB> gives.  WINDOW: the lane's pixels all have adjacent columns.
template <int INTERP, int MODE, int RGB, bool WINDOW>
__device__ __forceinline__ uint32_t sample_entry_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, const NvTaps& t, uint32_t border) {
    if constexpr (INTERP == kNearest) {
        const uint32_t p = convert_packed<RGB>(yf[t.y00], chroma_terms(pair_at(uvf, t.u00)));
        return (MODE != 0 || (t.in() & 1u)) ? p : border;
    } else {
        // every load is of a source pixel (the constant border: of the CLAMPED position) and issues before the first wait
        uint32_t Y00, Y01, Y10, Y11, q00, q01, q10, q11;
        if constexpr (WINDOW) {
            uint16_t w0, w1;
            uint32_t v0, v1;
            __builtin_memcpy(&w0, yf + t.y00, 2);  // (unaligned, like sample_nv12's windows)
            __builtin_memcpy(&w1, yf + t.y10, 2);
            __builtin_memcpy(&v0, uvf + t.u00, 4);  // (2-byte aligned)
            __builtin_memcpy(&v1, uvf + t.u10, 4);
            const uint32_t s0 = (t.w >> 10) & 16u, s1 = (t.w >> 11) & 16u;  // 16 * (bit 14), 16 * (bit 15)
            Y00 = w0 & 0xffu, Y01 = (uint32_t)w0 >> 8, Y10 = w1 & 0xffu, Y11 = (uint32_t)w1 >> 8;
            q00 = (v0 >> s0) & 0xffffu, q01 = (v0 >> s1) & 0xffffu, q10 = (v1 >> s0) & 0xffffu, q11 = (v1 >> s1) & 0xffffu;
        } else {
            Y00 = yf[t.y00], Y01 = yf[t.y01], Y10 = yf[t.y10], Y11 = yf[t.y11];
            q00 = pair_at(uvf, t.u00), q01 = pair_at(uvf, t.u01), q10 = pair_at(uvf, t.u10), q11 = pair_at(uvf, t.u11);
        }
        uint32_t p00 = convert_packed<RGB>(Y00, chroma_terms(q00)), p01 = convert_packed<RGB>(Y01, chroma_terms(q01));
        uint32_t p10 = convert_packed<RGB>(Y10, chroma_terms(q10)), p11 = convert_packed<RGB>(Y11, chroma_terms(q11));
        if constexpr (MODE == 0) {
            // a tap outside is the border value, in the destination's order and not converted (all four outside: the blend of four
            // border pixels is the border pixel)
            const uint32_t in = t.in();
            p00 = (in & 1u) ? p00 : border, p01 = (in & 2u) ? p01 : border, p10 = (in & 4u) ? p10 : border, p11 = (in & 8u) ? p11 : border;
        }
        return blend_u8_packed<3>(p00, p01, p10, p11, t.fx(), t.fy());
    }
}

}  // namespace
}  // namespace bevwarp
