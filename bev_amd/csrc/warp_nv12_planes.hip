// warp_nv12_planes.hip -- the perspective warp of NV12 frames into normalised float32 / float16 / bfloat16 channel planes
// (bevwarp_warp_nv12_planes): what bevwarp_warp_nv12 followed by the plane stage of bevwarp_warp_planes gives, bit for bit, in one pass --
// neither the converted frame nor the 8-bit BEV frame exists.  Constant border, nearest and bilinear.  See DESIGN.md section 4.13.
//
// The frame is flat_frame.h's and the sampler warp_nv12_kernel's (nv12_sample.h); the store stage, which has no twin in the frame, is
// the plane stage of the row kernel's 8-bit sources (rows_store.inc): per channel the lane converts its 4 values and writes them with
// one 16-byte (float32) or 8-byte (16-bit) store into that channel's plane row, so a wave writes 1024 / 512 contiguous bytes per
// instruction.  The kernel samples B, G, R and never learns the destination's channel order: the host hands it a plane offset, scale,
// bias and border byte per SAMPLED channel.
#include "nv12_sample.h"
#include "warp_kernels.h"
#include "warp_nv12.h"

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

    // the plane stores: per sampled channel the 8-bit value as float32, times scale, plus bias (each rounded), converted; 4 elements of
    // a plane row in one store for a lane whose 4 pixels lie in the row, element stores otherwise
    constexpr int ELEM = WIDE16 ? 2 : 4;
    uint8_t* d = dst_row(a, b, y) + (int64_t)xs * ELEM;
    const int lane_px = min(PPL, a.dst_w - xs);
    const bool lane_vec = a.dst_vec_ok && lane_px == PPL;
    if constexpr (WIDE16) {
        auto planes = [&](auto as) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float sc = a.pscale[k], bi = a.pbias[k];
                const uint32_t h[4] = {as((float)((p[0] >> (8 * k)) & 0xffu) * sc + bi), as((float)((p[1] >> (8 * k)) & 0xffu) * sc + bi),
                                       as((float)((p[2] >> (8 * k)) & 0xffu) * sc + bi), as((float)((p[3] >> (8 * k)) & 0xffu) * sc + bi)};
                uint16_t* dk = reinterpret_cast<uint16_t*>(d + a.ch_off[k]);
                if (__builtin_expect(lane_vec, 1)) {
                    u32x2 o = {h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
                    wide_store(reinterpret_cast<u32x2*>(dk), o);
                } else {
#pragma unroll
                    for (int i = 0; i < PPL; i++)
                        if (i < lane_px) dk[i] = (uint16_t)h[i];
                }
            }
        };
        if (a.plane == kPlaneBF16)  // (wave-uniform)
            planes(BitsBF16{});
        else
            planes(BitsF16{});
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float sc = a.pscale[k], bi = a.pbias[k];
            f32x4 o = {(float)((p[0] >> (8 * k)) & 0xffu) * sc + bi, (float)((p[1] >> (8 * k)) & 0xffu) * sc + bi,
                       (float)((p[2] >> (8 * k)) & 0xffu) * sc + bi, (float)((p[3] >> (8 * k)) & 0xffu) * sc + bi};
            float* dk = reinterpret_cast<float*>(d + a.ch_off[k]);
            if (__builtin_expect(lane_vec, 1)) {
                wide_store(reinterpret_cast<f32x4*>(dk), o);
            } else {
#pragma unroll
                for (int i = 0; i < PPL; i++)
                    if (i < lane_px) dk[i] = o[i];
            }
        }
    }
}

template <int INTERP>
void launch_format(const Nv12PlanesArgs& a, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (a.plane == kPlaneF32)
        hipLaunchKernelGGL((nv12_planes_kernel<INTERP, false>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((nv12_planes_kernel<INTERP, true>), grid, block, 0, stream, a);
}

}  // namespace

hipError_t launch_warp_nv12_planes(const Nv12PlanesArgs& a, int interp, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    (interp == kNearest ? launch_format<kNearest> : launch_format<kLinear>)(a, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
