// warp_nv12.hip -- the perspective warp of NV12 frames into 8-bit BGR / RGB (bevwarp_warp_nv12): every tap is converted with OpenCV's
// 8-bit YUV420sp -> RGB fixed point before the blend, so the result is bevwarp_warp of the converted frame, bit for bit, and the
// converted frame never exists.  Constant border, nearest and bilinear.  See DESIGN.md section 4.12.
//
// A kernel of its own with the border kernel's structure (warp_border.hip): a lane owns 4 consecutive destination pixels of one row,
// the coordinates are the reference's exact float64 chain, and every pixel runs the same straight-line code.  Each tap is loaded from
// the CLAMPED coordinate -- always an address inside the two planes -- and replaced by the border value afterwards (sample_global's
// rule), so all loads of a pixel issue before the first wait.
#include "sample.h"
#include "warp_border.h"
#include "warp_nv12.h"

namespace bevwarp {
namespace {

// cvtYUV420sp2RGB, 8 bits (BT.601, limited range, 20-bit fixed point; restated from OpenCV's colour conversion, parity unpinned):
//   yy = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128
//   R = clamp((yy + 524288 + 1673527 v) >> 20), G = clamp((yy + 524288 - 852492 v - 409993 u) >> 20), B = clamp((yy + 524288 + 2116026 u) >> 20)
// in int32 (no sum leaves it: -270,327,040 ... 560,969,128 over all (Y, U, V)), >> arithmetic.
// The part of each sum that depends on the (U, V) pair alone, rounding constant included.  Computed once per LOADED pair: a bilinear pixel
// loads four (one per tap), and where its taps share one or two pairs the same terms are computed again -- which taps coincide differs
// from lane to lane, so computing them once per DISTINCT pair would take selects or divergent branches in otherwise straight-line code.
struct Chroma {
    int r, g, b;
};
__device__ __forceinline__ Chroma chroma_terms(uint32_t pair) {  // byte 0 = U, byte 1 = V
    const int u = (int)(pair & 0xffu) - 128, v = (int)(pair >> 8) - 128;
    Chroma c;
    c.r = 524288 + 1673527 * v;
    c.g = 524288 - 852492 * v - 409993 * u;
    c.b = 524288 + 2116026 * u;
    return c;
}
// one converted pixel, packed in the destination's channel order (RGB = 0: B, G, R in bytes 0, 1, 2; 1: R, G, B)
template <int RGB>
__device__ __forceinline__ uint32_t convert(uint32_t Y, const Chroma& c) {
    const int yy = max(0, (int)Y - 16) * 1220542;
    const uint32_t r = (uint32_t)min(max((yy + c.r) >> 20, 0), 255);  // (min(max()): v_med3_i32)
    const uint32_t g = (uint32_t)min(max((yy + c.g) >> 20, 0), 255);
    const uint32_t b = (uint32_t)min(max((yy + c.b) >> 20, 0), 255);
    return RGB ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
}

// a (U, V) pair: 2-byte aligned by contract (even base, even strides)
__device__ __forceinline__ uint32_t load_pair(const uint8_t* __restrict__ row, int x) {
    return *reinterpret_cast<const uint16_t*>(row + (uint32_t)(x >> 1) * 2u);
}

// One destination pixel from the two planes (frame = this frame's planes).  X, Y: the map (1/32 px for bilinear).
template <int INTERP, int RGB>
__device__ __forceinline__ uint32_t sample_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, int64_t y_rs, int64_t uv_rs, int w, int h,
                                                uint32_t border, int X, int Y) {
    if (INTERP == kNearest) {
        const bool in = (unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h;
        const int cx = min(max(X, 0), w - 1), cy = min(max(Y, 0), h - 1);
        const uint32_t yv = yf[(int64_t)cy * y_rs + cx];
        const uint32_t pair = load_pair(uvf + (int64_t)(cy >> 1) * uv_rs, cx);
        return in ? convert<RGB>(yv, chroma_terms(pair)) : border;
    }
    const int sx = X >> kInterBits, sy = Y >> kInterBits, fx = X & 31, fy = Y & 31;
    const bool xin0 = (unsigned)sx < (unsigned)w, xin1 = (unsigned)(sx + 1) < (unsigned)w;
    const bool yin0 = (unsigned)sy < (unsigned)h, yin1 = (unsigned)(sy + 1) < (unsigned)h;
    const int cx0 = min(max(sx, 0), w - 1), cx1 = min(max(sx + 1, 0), w - 1);
    const int cy0 = min(max(sy, 0), h - 1), cy1 = min(max(sy + 1, 0), h - 1);
    // Y: the two taps of a row are the bytes of ONE 2-byte window starting at column c <= w - 2 (w is even, so >= 2): cx0 and cx1 are
    // c or c + 1, and the window ends inside the row.  Unaligned, like the resize kernel's windows.
    const int c = min(cx0, w - 2);
    const uint8_t* y0 = yf + (int64_t)cy0 * y_rs + c;
    const uint8_t* y1 = yf + (int64_t)cy1 * y_rs + c;
    uint16_t w0, w1;
    __builtin_memcpy(&w0, y0, 2);
    __builtin_memcpy(&w1, y1, 2);
    // UV: a tap's pair is (row >> 1, column >> 1); the four taps read one, two or four distinct pairs
    const uint8_t* uv0 = uvf + (int64_t)(cy0 >> 1) * uv_rs;
    const uint8_t* uv1 = uvf + (int64_t)(cy1 >> 1) * uv_rs;
    const uint32_t q00 = load_pair(uv0, cx0), q01 = load_pair(uv0, cx1);
    const uint32_t q10 = load_pair(uv1, cx0), q11 = load_pair(uv1, cx1);

    const uint32_t s0 = 8u * (uint32_t)(cx0 - c), s1 = 8u * (uint32_t)(cx1 - c);  // the taps' bytes in the windows
    const uint32_t p00 = convert<RGB>(((uint32_t)w0 >> s0) & 0xffu, chroma_terms(q00));
    const uint32_t p01 = convert<RGB>(((uint32_t)w0 >> s1) & 0xffu, chroma_terms(q01));
    const uint32_t p10 = convert<RGB>(((uint32_t)w1 >> s0) & 0xffu, chroma_terms(q10));
    const uint32_t p11 = convert<RGB>(((uint32_t)w1 >> s1) & 0xffu, chroma_terms(q11));
    // (all four taps outside: the blend of four border values is the border value)
    return blend_u8_packed<3>((xin0 && yin0) ? p00 : border, (xin1 && yin0) ? p01 : border, (xin0 && yin1) ? p10 : border, (xin1 && yin1) ? p11 : border,
                              (uint32_t)fx, (uint32_t)fy);
}

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
