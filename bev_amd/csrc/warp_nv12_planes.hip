// warp_nv12_planes.hip -- the perspective warp of NV12 frames into normalised float32 / float16 / bfloat16 channel planes
// (bevwarp_warp_nv12_planes): what bevwarp_warp_nv12 followed by the plane stage of bevwarp_warp_planes gives, bit for bit, in one pass --
// neither the converted frame nor the 8-bit BEV frame exists.  Constant border, nearest and bilinear.  See DESIGN.md section 4.13.
//
// The frame is flat_frame.h's and the sampler warp_nv12_kernel's (nv12_sample.h); the store stage, which has no twin in the frame, is
// the plane stage of the row kernel's 8-bit sources (rows_store.inc): per channel the lane converts its 4 values and writes them with
// one 16-byte (float32) or 8-byte (16-bit) store into that channel's plane row, so a wave writes 1024 / 512 contiguous bytes per
// instruction (plane_store.inc, text shared with warp_map_nv12.hip).  The kernel samples B, G, R and never learns the destination's channel order: the host hands it a plane offset, scale,
// bias and border byte per SAMPLED channel.
#include "nv12_sample.h"
#include "warp_kernels.h"
#include "warp_nv12.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// WIDE16: 2-byte planes (a.plane = kPlaneF16 | kPlaneBF16, wave-uniform, as in warp_rows_planes16); otherwise float32 planes
template <int INTERP, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void nv12_planes_kernel(const Nv12PlanesArgs a) {
    constexpr int PPL = kBorderPPL;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);
    const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
    const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;

    uint32_t p[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other (their taps are clamped into the planes too) and not stored
        double Xn, Yn, W;
        walk.pixel(a, xs + j, Xn, Yn, W);
        int X, Y;
        map_pixel_exact<INTERP>(Xn, Yn, W, X, Y);
        p[j] = sample_nv12<INTERP, 0>(yf, uvf, a.y_rs, a.uv_rs, a.src_w, a.src_h, a.border, X, Y);
    }

#include "plane_store.inc"
}

}  // namespace

hipError_t launch_warp_nv12_planes(const Nv12PlanesArgs& a, int interp, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) { pick::flag(a.plane != kPlaneF32, [&](auto wide16) { launch(nv12_planes_kernel<i(), wide16()>); }); });
    });
}

}  // namespace bevwarp
