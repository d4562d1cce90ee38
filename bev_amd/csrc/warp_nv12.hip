// warp_nv12.hip -- the perspective warp of NV12 frames into 8-bit BGR / RGB (bevwarp_warp_nv12): every tap is converted with OpenCV's
// 8-bit YUV420sp -> RGB fixed point before the blend, so the result is bevwarp_warp of the converted frame, bit for bit, and the
// converted frame never exists.  Constant border, nearest and bilinear.  See DESIGN.md section 4.12.
//
// A kernel of its own with the border kernel's structure (warp_border.hip): a lane owns 4 consecutive destination pixels of one row,
// the coordinates are the reference's exact float64 chain, and every pixel runs the same straight-line code.  Each tap is loaded from
// the CLAMPED coordinate -- always an address inside the two planes -- and replaced by the border value afterwards (sample_global's
// rule), so all loads of a pixel issue before the first wait.
#include "nv12_sample.h"
#include "warp_border.h"
#include "warp_nv12.h"

namespace bevwarp {
namespace {

// (the sampler -- chroma_terms, convert, load_pair, sample_nv12 -- is nv12_sample.h: warp_nv12_planes.hip takes the same taps)
template <int INTERP, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_nv12_kernel(const Nv12Args a) {
    constexpr int PPL = kBorderPPL;
    const uint32_t t = blockIdx.x;
    const uint32_t b = fast_div(t, a.tpf_magic, (uint32_t)a.tiles_per_frame);
    const uint32_t r = t - b * (uint32_t)a.tiles_per_frame;
    const uint32_t ty = fast_div(r, a.tx_magic, (uint32_t)a.tiles_x);
    const uint32_t tx = r - ty * (uint32_t)a.tiles_x;
    const int y = (int)ty * kBorderTileH + (int)(threadIdx.x >> 6);
    const int xs = (int)tx * kBorderTileW + (int)(threadIdx.x & 63) * PPL;  // the lane's first pixel
    if (y >= a.dst_h || xs >= a.dst_w) return;
    const double* M = a.minv + (int64_t)b * a.m_stride;
    double Mr[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Mr[i] = M[i];
    const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
    const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;

    uint32_t p[PPL];
    int bx = -1;
    double X0 = 0.0, Y0 = 0.0, W0 = 0.0;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other (their taps are clamped into the planes too) and not stored
        const int x = xs + j;
        const int bxj = (int)fast_div((uint32_t)x, a.bw0_magic, (uint32_t)a.bw0) * a.bw0;
        if (bxj != bx) {  // (the lane's 4 pixels share an evaluation block unless its width is not a multiple of 4)
            bx = bxj;
            row_terms(Mr, bx, y, X0, Y0, W0);
        }
        const double x1 = (double)(x - bx);
        int X, Y;
        // (a NaN coordinate lands on INT_MIN: outside, as the reference's INT_MAX is under the constant border)
        map_pixel_exact<INTERP>(X0 + Mr[0] * x1, Y0 + Mr[3] * x1, W0 + Mr[6] * x1, X, Y);
        p[j] = sample_nv12<INTERP, RGB>(yf, uvf, a.y_rs, a.uv_rs, a.src_w, a.src_h, a.border, X, Y);
    }

    // the border kernel's 8-bit, 3-channel stores: three dwords for a lane whose 4 pixels lie in the row, per pixel otherwise
    uint8_t* d = a.dst + (int64_t)b * a.dst_fs + (int64_t)y * a.dst_rs + (int64_t)xs * 3;
    if (a.dst_vec_ok && xs + PPL <= a.dst_w) {
        u32x3 o = {__builtin_amdgcn_perm(p[1], p[0], 0x04020100u), __builtin_amdgcn_perm(p[2], p[1], 0x05040201u), __builtin_amdgcn_perm(p[3], p[2], 0x06050402u)};
        wide_store(reinterpret_cast<u32x3*>(d), o);
    } else {
#pragma unroll
        for (int j = 0; j < PPL; j++)
            if (xs + j < a.dst_w)
#pragma unroll
                for (int k = 0; k < 3; k++) d[j * 3 + k] = (uint8_t)(p[j] >> (8 * k));
    }
}

template <int INTERP>
void launch_order(const Nv12Args& a, int rgb_order, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (rgb_order)
        hipLaunchKernelGGL((warp_nv12_kernel<INTERP, 1>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((warp_nv12_kernel<INTERP, 0>), grid, block, 0, stream, a);
}

}  // namespace

hipError_t launch_warp_nv12(const Nv12Args& a, int interp, int rgb_order, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    (interp == kNearest ? launch_order<kNearest> : launch_order<kLinear>)(a, rgb_order, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
