// Internal interface of the NV12 warps: a Y plane and a half-resolution plane of (U, V) pairs are sampled and converted tap by tap into an
// 8-bit BGR / RGB destination (warp_nv12.hip, bevwarp_warp_nv12) or into normalised float32 / float16 / bfloat16 channel planes
// (warp_nv12_planes.hip, bevwarp_warp_nv12_planes).  Constant border, nearest and bilinear.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bevwarp {

// The launch geometry is the border kernel's (warp_border.h: 4 pixels per lane, a wave per row, 4 rows per workgroup, flat grid).
struct Nv12Args {
    const uint8_t* y;             // src_h rows of src_w bytes
    const uint8_t* uv;            // src_h / 2 rows of src_w / 2 (U, V) pairs; base and strides even
    uint8_t* dst;                 // 3 bytes per pixel
    const double* minv;           // device, inverse matrices
    int64_t y_fs, y_rs;           // bytes
    int64_t uv_fs, uv_rs;
    int64_t dst_fs, dst_rs;
    int src_h, src_w, dst_h, dst_w;
    int m_stride;                 // 9 (one matrix per frame) or 0 (shared)
    int bw0;                      // evaluation block width of the reference algorithm
    int tiles_x, tiles_per_frame;
    uint32_t bw0_magic, tx_magic, tpf_magic;  // fast_div magics (0 = divide)
    int dst_vec_ok;               // destination layout admits the wide stores (the rule of bevwarp_warp)
    uint32_t border;              // the border value packed in the destination's channel order (byte k = channel k)
};

hipError_t launch_warp_nv12(const Nv12Args& a, int interp, int rgb_order, int64_t items, hipStream_t stream);

// The plane kernel samples in ONE channel order -- B, G, R in bytes 0, 1, 2 of a pixel -- and knows no other: the destination's order is
// where the host points each sampled channel (plane offset, scale, bias and border byte k belong to sampled channel k).
struct Nv12PlanesArgs {
    const uint8_t* y;             // as Nv12Args
    const uint8_t* uv;
    uint8_t* dst;                 // plane 0 of frame 0
    const double* minv;
    int64_t y_fs, y_rs;           // bytes
    int64_t uv_fs, uv_rs;
    int64_t dst_fs, dst_rs;
    int64_t ch_off[3];            // bytes from a frame's base to the plane sampled channel k (B, G, R) is written to
    float pscale[3], pbias[3];    // of sampled channel k
    int src_h, src_w, dst_h, dst_w;
    int m_stride;
    int bw0;
    int tiles_x, tiles_per_frame;
    uint32_t bw0_magic, tx_magic, tpf_magic;
    int dst_vec_ok;               // base and the three destination strides admit 4-element stores (16 bytes float32, 8 bytes 16-bit)
    uint32_t border;              // byte k = the border value of sampled channel k
    int plane;                    // kPlaneF32, kPlaneF16, kPlaneBF16 (warp_kernels.h)
};

hipError_t launch_warp_nv12_planes(const Nv12PlanesArgs& a, int interp, int64_t items, hipStream_t stream);

}  // namespace bevwarp
