// warp_map_planes.hip -- 8-bit frames of 3 channels sampled through a fixed camera's warp map and written as normalised channel planes for a
// detector (bevwarp_remap_planes): bevwarp_warp_nv12_planes' plane stage of bevwarp_remap's 8-bit pixel, bit for
// bit, with the sampled BEV frame never in memory.  The map carries the lens, so there is no float64 here.  The structure is remap_kernel's
// (warp_map.hip) for uint8_t x 3: a workgroup loads its tile's map entries once, derives what does not depend on the frame -- the taps'
// byte offsets, the weights, the inside mask (BORDER_CONSTANT), whether the lane takes the 6-byte pair loads -- and walks frames_per_item
// frames with that in registers.  The five border modes that write every pixel; BORDER_TRANSPARENT has no instance.
//
// The frame is flat_frame.h; the map loads (map_entry.h) and the index stage (map_entry_taps.inc) are shared with the other map samplers;
// the blend is sample.h's; the store is plane_store.inc, shared as text with warp_nv12_planes.hip and warp_map_nv12.hip.  The sampler's
// helpers -- the 3-byte tap load and the 6-byte pair load -- are restated from warp_map.hip rather than moved into a header: that unit's
// machine code stays what it was.
#include "warp_map_planes.h"
#include "map_entry.h"
#include "warp_kernels.h"

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

// one source pixel at a byte offset of the frame: exactly its 3 bytes are read
__device__ __forceinline__ uint32_t load_at(const uint8_t* __restrict__ frame, uint32_t off) {
    const uint8_t* q = frame + off;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

// the two adjacent taps of a row: 6 contiguous bytes, never a byte beyond them (warp_map.hip's load_pair_u8x3)
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ frame, uint32_t off, uint32_t& p0, uint32_t& p1) {
    uint32_t lo;
    uint16_t hi;
    __builtin_memcpy(&lo, frame + off, 4);
    __builtin_memcpy(&hi, frame + off + 4, 2);
    p0 = lo & 0xffffffu;
    p1 = __builtin_amdgcn_alignbit((uint32_t)hi, lo, 24);  // bytes 3, 4, 5
}

// One destination pixel of one frame, packed: byte k = channel k.  PAIR: both rows' taps are adjacent columns.
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

template <int INTERP, int MODE, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_planes_kernel(const RemapPlanesArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = false;
    static_assert(MODE != kBorderTransparent, "the plane stage writes every pixel");
    uint32_t g;
    int y, xs;  // group of frames, row, the lane's first pixel
    if (!lane_position(a, g, y, xs)) return;
    const int b0 = (int)g * a.frames_per_item;
    const int nb = min(a.frames_per_item, a.batch - b0);

    uint32_t e[PPL], fr[PPL];
    load_entries<INTERP>(a, b0, y, xs, e, fr);

    Taps tap[PPL];
    bool wr[PPL];
    // a lane whose pixels all have their two columns side by side -- every inlier, every interior pixel -- takes the pair loads; a lane with
    // a pixel at a clamped or remapped edge takes the loads tap by tap
    bool pair = INTERP == kLinear;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        Taps& t = tap[j];
#include "map_entry_taps.inc"
        t.w = f | (in << 10);
        const uint32_t o0 = (uint32_t)cy0 * (uint32_t)a.src_rs, o1 = (uint32_t)cy1 * (uint32_t)a.src_rs;
        const uint32_t x0 = (uint32_t)c0 * 3u, x1 = (uint32_t)c1 * 3u;
        t.a00 = o0 + x0, t.a01 = o0 + x1, t.a10 = o1 + x0, t.a11 = o1 + x1;
        pair = pair && c1 == c0 + 1;
    }
    (void)wr;  // (every pixel of the row is written: the row's end is the store's to judge)

    const uint32_t border = a.bv_u8;
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
        uint32_t p[PPL];
        if constexpr (INTERP == kLinear) {
            if (pair) {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, true>(frame, tap[j], border);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, false>(frame, tap[j], border);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, false>(frame, tap[j], border);
        }
        {
#include "plane_store.inc"
        }
    }
}

template <int INTERP, int MODE>
void launch_format(const RemapPlanesArgs& a, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (a.plane == kPlaneF32)
        hipLaunchKernelGGL((remap_planes_kernel<INTERP, MODE, false>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((remap_planes_kernel<INTERP, MODE, true>), grid, block, 0, stream, a);
}

template <int INTERP>
void launch_mode(const RemapPlanesArgs& a, int mode, dim3 grid, hipStream_t stream) {
    switch (mode) {
        case 0: launch_format<INTERP, 0>(a, grid, stream); break;
        case kBorderReplicate: launch_format<INTERP, kBorderReplicate>(a, grid, stream); break;
        case kBorderReflect: launch_format<INTERP, kBorderReflect>(a, grid, stream); break;
        case kBorderWrap: launch_format<INTERP, kBorderWrap>(a, grid, stream); break;
        default: launch_format<INTERP, kBorderReflect101>(a, grid, stream); break;
    }
}

}  // namespace

hipError_t launch_remap_planes(const RemapPlanesArgs& a, int interp, int mode, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    (interp == kNearest ? launch_mode<kNearest> : launch_mode<kLinear>)(a, mode, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
