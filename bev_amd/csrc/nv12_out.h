// nv12_out.h -- the store-side conversion of the warps that write NV12 (warp_nv12_out.hip): one warped 8-bit pixel -> its Y byte and its
// (U, V) pair, OpenCV's 8-bit RGB -> YUV 4:2:0 fixed point (BT.601, limited range, 20 bits; restated from OpenCV's colour conversion,
// parity unpinned).  See include/bevwarp.h, bevwarp_warp_to_nv12, and DESIGN.md section 4.14.  Not installed.
//   Y = ( 269484 R + 528482 G + 102760 B + (16  << 20) + (1 << 19)) >> 20
//   U = (-155188 R - 305135 G + 460324 B + (128 << 20) + (1 << 19)) >> 20
//   V = ( 460324 R - 385875 G -  74448 B + (128 << 20) + (1 << 19)) >> 20
// in int32.  Over all 2^24 pixels the sums span 17,301,504 ... 246,986,634 (Y) and 17,359,651 ... 252,124,636 (U, V): no sum leaves
// int32 or goes negative, Y spans 16 ... 235 and U, V span 16 ... 240, so there is no clamp (tests/test_nv12_out_cpu.py counts them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevwarp {
namespace {

// A pixel travels packed, channel k in byte k; RGB = 0: the channels are B, G, R; 1: R, G, B.
template <int RGB>
struct Yuv601 {
    int r, g, b;
    __device__ __forceinline__ explicit Yuv601(uint32_t p) : r((int)((RGB ? p : p >> 16) & 0xffu)), g((int)((p >> 8) & 0xffu)), b((int)((RGB ? p >> 16 : p) & 0xffu)) {}
    __device__ __forceinline__ uint32_t luma() const { return (uint32_t)((269484 * r + 528482 * g + 102760 * b + (16 << 20) + (1 << 19)) >> 20); }
    // byte 0 = U, byte 1 = V: the pair as it lies in memory
    __device__ __forceinline__ uint32_t pair() const {
        const uint32_t u = (uint32_t)((-155188 * r - 305135 * g + 460324 * b + (128 << 20) + (1 << 19)) >> 20);
        const uint32_t v = (uint32_t)((460324 * r - 385875 * g - 74448 * b + (128 << 20) + (1 << 19)) >> 20);
        return u | (v << 8);
    }
};

}  // namespace
}  // namespace bevwarp
