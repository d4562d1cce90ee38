// nv12_sample.h -- the sampler of the NV12 warps (device code, gfx950): one destination pixel from a Y plane and a plane of (U, V) pairs,
// every tap converted with OpenCV's 8-bit YUV420sp -> RGB fixed point before the blend.  Shared by warp_nv12.hip (8-bit BGR / RGB
// destinations) and warp_nv12_planes.hip (normalised channel planes); the conversion, by the samplers through warp maps as well
// (remap_sample_nv12.h, stitch_sample.h).  See DESIGN.md sections 4.12, 4.13 and 4.19.  Not installed.
#pragma once
#include "sample.h"

namespace bevwarp {
namespace {

// cvtYUV420sp2RGB, 8 bits (BT.601, limited range, 20-bit fixed point; restated from OpenCV's colour conversion, parity unpinned):
//   yy = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128
//   R = clamp((yy + 524288 + 1673527 v) >> 20), G = clamp((yy + 524288 - 852492 v - 409993 u) >> 20), B = clamp((yy + 524288 + 2116026 u) >> 20)
// in int32 (no sum leaves it: -270,327,040 ... 560,969,128 over all (Y, U, V)), >> arithmetic.
// The part of each sum that depends on the (U, V) pair alone, rounding constant included.  Computed once per LOADED pair: a bilinear pixel
// loads four (one per tap), and where its taps share one or two pairs the same terms are computed again -- which taps coincide differs
// from lane to lane, so computing them once per DISTINCT pair would take selects or divergent branches in otherwise straight-line code.
struct Chroma {
    int r, g, b;
};
__device__ __forceinline__ Chroma chroma_terms(uint32_t pair) {  // byte 0 = U, byte 1 = V
    const int u = (int)(pair & 0xffu) - 128, v = (int)(pair >> 8) - 128;
    Chroma c;
    c.r = 524288 + 1673527 * v;
    c.g = 524288 - 852492 * v - 409993 * u;
    c.b = 524288 + 2116026 * u;
    return c;
}
// the three channels of one converted pixel
__device__ __forceinline__ void convert_channels(uint32_t Y, const Chroma& c, uint32_t& r, uint32_t& g, uint32_t& b) {
    const int yy = max(0, (int)Y - 16) * 1220542;
    r = (uint32_t)min(max((yy + c.r) >> 20, 0), 255);  // (min(max()): v_med3_i32)
    g = (uint32_t)min(max((yy + c.g) >> 20, 0), 255);
    b = (uint32_t)min(max((yy + c.b) >> 20, 0), 255);
}
// one converted pixel, packed in the destination's channel order (RGB = 0: B, G, R in bytes 0, 1, 2; 1: R, G, B)
// (The compiler may fuse two channels' >> 20 and clamp with this packing into v_ashr_pk_u8_i32; the one kernel in which it did gave wrong
// pixels on the MI355X -- convert_packed below, DESIGN.md section 4.19.  A kernel that uses convert and fails its bit-exact test: look for
// that instruction in its code first.)
template <int RGB>
__device__ __forceinline__ uint32_t convert(uint32_t Y, const Chroma& c) {
    uint32_t r, g, b;
    convert_channels(Y, c, r, g, b);
    return RGB ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
}
// convert<RGB> with the middle channel behind a value barrier: what every sampler through warp maps converts with (remap_sample_nv12.h,
// stitch_sample.h).  Without the barrier the compiler fuses two channels' shift and clamp of one instance of the bilinear R, G, B kernel
// of warp_map_nv12.hip into v_ashr_pk_u8_i32, and on the MI355X that instance -- the only one of the unit's kernels with the instruction
// -- gave pixels up to 128 off the definition (2.6 % of a frame; every other instance was exact).  The barrier costs no instruction: each
// channel keeps its own v_ashrrev_i32 and v_med3_i32, as in every other kernel of the library.  This is the only copy: a new sampler of
// NV12 taps calls it and restates nothing.
template <int RGB>
__device__ __forceinline__ uint32_t convert_packed(uint32_t Y, const Chroma& c) {
    uint32_t r, g, b;
    convert_channels(Y, c, r, g, b);
    asm("" : "+v"(g));
    return RGB ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
}

// a (U, V) pair: 2-byte aligned by contract (even base, even strides)
__device__ __forceinline__ uint32_t load_pair(const uint8_t* __restrict__ row, int x) {
    return *reinterpret_cast<const uint16_t*>(row + (uint32_t)(x >> 1) * 2u);
}

// One destination pixel from the two planes (frame = this frame's planes).  X, Y: the map (1/32 px for bilinear).
template <int INTERP, int RGB>
__device__ __forceinline__ uint32_t sample_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, int64_t y_rs, int64_t uv_rs, int w, int h,
                                                uint32_t border, int X, int Y) {
    if (INTERP == kNearest) {
        const bool in = (unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h;
        const int cx = min(max(X, 0), w - 1), cy = min(max(Y, 0), h - 1);
        const uint32_t yv = yf[(int64_t)cy * y_rs + cx];
        const uint32_t pair = load_pair(uvf + (int64_t)(cy >> 1) * uv_rs, cx);
        return in ? convert<RGB>(yv, chroma_terms(pair)) : border;
    }
    const int sx = X >> kInterBits, sy = Y >> kInterBits, fx = X & 31, fy = Y & 31;
    const bool xin0 = (unsigned)sx < (unsigned)w, xin1 = (unsigned)(sx + 1) < (unsigned)w;
    const bool yin0 = (unsigned)sy < (unsigned)h, yin1 = (unsigned)(sy + 1) < (unsigned)h;
    const int cx0 = min(max(sx, 0), w - 1), cx1 = min(max(sx + 1, 0), w - 1);
    const int cy0 = min(max(sy, 0), h - 1), cy1 = min(max(sy + 1, 0), h - 1);
    // Y: the two taps of a row are the bytes of ONE 2-byte window starting at column c <= w - 2 (w is even, so >= 2): cx0 and cx1 are
    // c or c + 1, and the window ends inside the row.  Unaligned, like the resize kernel's windows.
    const int c = min(cx0, w - 2);
    const uint8_t* y0 = yf + (int64_t)cy0 * y_rs + c;
    const uint8_t* y1 = yf + (int64_t)cy1 * y_rs + c;
    uint16_t w0, w1;
    __builtin_memcpy(&w0, y0, 2);
    __builtin_memcpy(&w1, y1, 2);
    // UV: a tap's pair is (row >> 1, column >> 1); the four taps read one, two or four distinct pairs
    const uint8_t* uv0 = uvf + (int64_t)(cy0 >> 1) * uv_rs;
    const uint8_t* uv1 = uvf + (int64_t)(cy1 >> 1) * uv_rs;
    const uint32_t q00 = load_pair(uv0, cx0), q01 = load_pair(uv0, cx1);
    const uint32_t q10 = load_pair(uv1, cx0), q11 = load_pair(uv1, cx1);

    const uint32_t s0 = 8u * (uint32_t)(cx0 - c), s1 = 8u * (uint32_t)(cx1 - c);  // the taps' bytes in the windows
    const uint32_t p00 = convert<RGB>(((uint32_t)w0 >> s0) & 0xffu, chroma_terms(q00));
    const uint32_t p01 = convert<RGB>(((uint32_t)w0 >> s1) & 0xffu, chroma_terms(q01));
    const uint32_t p10 = convert<RGB>(((uint32_t)w1 >> s0) & 0xffu, chroma_terms(q10));
    const uint32_t p11 = convert<RGB>(((uint32_t)w1 >> s1) & 0xffu, chroma_terms(q11));
    // (all four taps outside: the blend of four border values is the border value)
    return blend_u8_packed<3>((xin0 && yin0) ? p00 : border, (xin1 && yin0) ? p01 : border, (xin0 && yin1) ? p10 : border, (xin1 && yin1) ? p11 : border,
                              (uint32_t)fx, (uint32_t)fy);
}

}  // namespace
}  // namespace bevwarp
