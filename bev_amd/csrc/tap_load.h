// tap_load.h -- a source pixel, or the two adjacent pixels of a row, at a byte offset of a frame (device code, gfx950): the loads of every
// sampler that keeps tap offsets in 32 bits -- the remap kernels (warp_map.hip, remap_sample_u8x3.h) and the map stitches
// (stitch_sample.h).  Two forms side by side: Pixel<T, C> for the kernels of every pixel type, and a packed uint32_t for the kernels that
// know only 8-bit pixels of 3 channels.  The tap loads are what binds these kernels.  Not installed.
#pragma once
#include "sample.h"

namespace bevwarp {
namespace {

// One source pixel at a byte offset of the frame: exactly its C * sizeof(T) bytes are read (flat_frame.h's load_pixel, by offset).
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> load_at(const uint8_t* __restrict__ frame, uint32_t off, bool vec) {
    Pixel<T, C> p;
    const uint8_t* q = frame + off;
    if constexpr (sizeof(T) == 1) {
        if (C == 4 && vec) {
            p.packed = *reinterpret_cast<const uint32_t*>(q);
        } else if (C == 2 && vec) {
            p.packed = *reinterpret_cast<const uint16_t*>(q);
        } else {
            p.packed = 0;
#pragma unroll
            for (int k = 0; k < C; k++) p.packed |= (uint32_t)q[k] << (8 * k);
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = reinterpret_cast<const float*>(q)[k];
    }
    return p;
}

// one 8-bit pixel of 3 channels, packed: exactly its 3 bytes are read
__device__ __forceinline__ uint32_t load_at(const uint8_t* __restrict__ frame, uint32_t off) {
    const uint8_t* q = frame + off;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

// The two taps of a row of 8-bit 3-channel pixels whose columns are adjacent are 6 contiguous bytes: one dword and one short load
// (unaligned, as the byte pairs the compiler forms on its own already are) instead of two shorts and two bytes, and never a byte beyond the
// six.
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ frame, uint32_t off, uint32_t& p0, uint32_t& p1) {
    uint32_t lo;
    uint16_t hi;
    __builtin_memcpy(&lo, frame + off, 4);
    __builtin_memcpy(&hi, frame + off + 4, 2);
    p0 = lo & 0xffffffu;
    p1 = __builtin_amdgcn_alignbit((uint32_t)hi, lo, 24);  // bytes 3, 4, 5
}
__device__ __forceinline__ void load_pair_u8x3(const uint8_t* __restrict__ frame, uint32_t off, Pixel<uint8_t, 3>& p0, Pixel<uint8_t, 3>& p1) {
    load_pair(frame, off, p0.packed, p1.packed);
}

}  // namespace
}  // namespace bevwarp
