// Internal interface of the warps that write NV12 (warp_nv12_out.hip; bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12): an 8-bit BGR / RGB
// frame or a decoder's NV12 planes are sampled as bevwarp_warp / bevwarp_warp_nv12 sample them, and every warped pixel is stored as a Y
// byte and -- at even columns of even rows -- a (U, V) pair.  Constant border, nearest and bilinear.  Not installed.
#pragma once
#include "flat_frame.h"

namespace bevwarp {

// The launch geometry and the matrices are the shared frame's (flat_frame.h); its destination (dst, dst_fs, dst_rs, dst_vec_ok) is the Y
// plane: dst_h rows of dst_w bytes, dst_h and dst_w even.
struct Nv12OutArgs : FrameArgs {
    uint8_t* dst_uv;              // dst_h / 2 rows of dst_w / 2 (U, V) pairs; base and strides even
    int64_t duv_fs, duv_rs;       // bytes
    int uv_vec_ok;                // the UV plane's base and strides are multiples of 4: a lane's two pairs go out as one dword
    const uint8_t* src;           // the BGR / RGB source: src_h rows of src_w 3-byte pixels ...
    int64_t src_fs, src_rs;
    const uint8_t* y;             // ... or the NV12 source, as Nv12Args holds it (warp_nv12.h)
    const uint8_t* uv;
    int64_t y_fs, y_rs;
    int64_t uv_fs, uv_rs;
    int src_h, src_w;
    uint32_t border;              // the border PIXEL packed in the warped pixel's channel order (byte k = channel k); converted like any other
};

// nv12_src: the source is (y, uv), sampled as B, G, R (rgb_order is then 0); otherwise src, whose pixels are B, G, R (rgb_order 0) or R, G, B (1)
hipError_t launch_warp_nv12_out(const Nv12OutArgs& a, int nv12_src, int interp, int rgb_order, int64_t items, hipStream_t stream);

}  // namespace bevwarp
