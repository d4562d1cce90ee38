// warp_map_planes.hip -- 8-bit frames of 3 channels sampled through a fixed camera's warp map and written as normalised channel planes for a
// detector (bevwarp_remap_planes): bevwarp_warp_nv12_planes' plane stage of bevwarp_remap's 8-bit pixel, bit for
// bit, with the sampled BEV frame never in memory.  The map carries the lens, so there is no float64 here.  The structure is remap_kernel's
// (warp_map.hip) for uint8_t x 3: a workgroup loads its tile's map entries once, derives what does not depend on the frame -- the taps'
// byte offsets, the weights, the inside mask (BORDER_CONSTANT), whether the lane takes the 6-byte pair loads -- and walks frames_per_item
// frames with that in registers.  The five border modes that write every pixel; BORDER_TRANSPARENT has no instance.
//
// The frame is flat_frame.h; the map loads (map_entry.h) and the index stage (map_entry_taps.inc) are shared with the other map samplers;
// the blend is sample.h's; the store is plane_store.inc, shared as text with warp_nv12_planes.hip and warp_map_nv12.hip.  The sampler's
// taps and one pixel from them are remap_sample_u8x3.h, shared with warp_map_nv12_out.hip; its 3-byte tap load and 6-byte pair load are
// tap_load.h's.
#include "warp_map_planes.h"
#include "map_entry.h"
#include "remap_sample_u8x3.h"
#include "warp_kernels.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

template <int INTERP, int MODE, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_planes_kernel(const RemapPlanesArgs a) {
    static_assert(MODE != kBorderTransparent, "the plane stage writes every pixel");
#include "remap_taps_u8x3.inc"
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
        uint32_t p[PPL];
#include "remap_frame_u8x3.inc"
        {
#include "plane_store.inc"
        }
    }
}

}  // namespace

hipError_t launch_remap_planes(const RemapPlanesArgs& a, int interp, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) {
            pick::value<0, kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101>(mode, [&](auto m) {
                pick::flag(a.plane != kPlaneF32, [&](auto wide16) { launch(remap_planes_kernel<i(), m(), wide16()>); });
            });
        });
    });
}

}  // namespace bevwarp
