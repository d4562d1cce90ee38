// nv12_store.h -- the store stage of the map samplers that write NV12 (warp_map_nv12_out.hip, warp_stitch_maps_nv12_out.hip): a lane's 4
// sampled 8-bit pixels of one destination row -> 4 Y bytes and, on even rows, the (U, V) pairs of pixels 0 and 2.  It is
// warp_nv12_out_kernel's store (warp_nv12_out.hip), restated as a function for kernels that sample through maps; the conversion is
// nv12_out.h's.  No destination row depends on another: a pair is taken from ONE pixel, there is no averaging.  See DESIGN.md sections
// 4.14 and 4.21.  Not installed.
#pragma once
#include "flat_frame.h"
#include "nv12_out.h"

namespace bevwarp {

// The second plane of an NV12 destination, next to FrameArgs' first (dst, dst_fs, dst_rs, dst_vec_ok: the Y plane, dst_h rows of dst_w
// bytes, both even).
struct Nv12DstUv {
    uint8_t* dst_uv;              // dst_h / 2 rows of dst_w / 2 (U, V) pairs; base and strides even
    int64_t duv_fs, duv_rs;       // bytes
    int uv_vec_ok;                // the UV plane's base and strides are multiples of 4: a lane's two pairs go out as one dword
};

namespace {

// px: the lane's pixels xs .. xs + 3 of row y of frame b, packed, channel k in byte k (RGB = 0: B, G, R; 1: R, G, B).  dst_w is even and
// xs a multiple of 4: the lane writes all 4 pixels, or -- the last lane of a row of 4 k + 2 pixels -- the first 2 (px[2], px[3] are then
// converted and dropped).  uv: the args' Nv12DstUv part.
template <int RGB>
__device__ __forceinline__ void store_lane_nv12(const FrameArgs& a, const Nv12DstUv& uv, uint32_t b, int y, int xs, const uint32_t (&px)[kBorderPPL]) {
    static_assert(kBorderPPL == 4, "the store stage packs 4 Y bytes and 2 pairs per lane");
    const bool all = xs + kBorderPPL <= a.dst_w;
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
    uint8_t* duv = uv.dst_uv + (int64_t)b * uv.duv_fs + (int64_t)(y >> 1) * uv.duv_rs + xs;  // pair x / 2 lies at byte x; 2-byte aligned by contract
    const uint32_t c0 = p0.pair(), c2 = p2.pair();
    if (all && uv.uv_vec_ok) {
        *reinterpret_cast<uint32_t*>(duv) = c0 | (c2 << 16);
    } else {
        *reinterpret_cast<uint16_t*>(duv) = (uint16_t)c0;
        if (all) *reinterpret_cast<uint16_t*>(duv + 2) = (uint16_t)c2;
    }
}

}  // namespace
}  // namespace bevwarp
