// warp_border.hip -- the perspective warp with OpenCV's other borders (bevwarp_warp_border): REPLICATE, REFLECT, WRAP and
// REFLECT_101 read a source pixel for every tap, TRANSPARENT writes inliers only.  8-bit and float32 pixels, 1-4 channels,
// nearest and bilinear.  See DESIGN.md section 4.9.
//
// A kernel of its own, not a mode of warp_rows: that kernel's tile classes assume the constant border (its outside tiles store
// the constant without computing a coordinate, its edge tiles guard taps against the frame), its register budget is what
// bounds it, and bench.py times it.  Here every tap index goes through borderInterpolate first, after which it IS a source
// pixel: interior and exterior pixels run the same straight-line code (index remap, gathers, blend, store) -- no tile
// classification, no guarded reads.  The coordinates are the reference's exact float64 chain, pixel by pixel.
#include "sample.h"
#include "warp_border.h"

namespace bevwarp {
namespace {

// round_sat with the reference's NaN: std::min(INT_MAX, NaN) is INT_MAX.  (coords.h's round_sat sends NaN to INT_MIN, which
// only the constant border cannot tell apart: REPLICATE or WRAP of INT_MIN and of INT_MAX are different pixels.)  A NaN comes
// from 0 * (32 / W) where W is denormal and the division overflows.
__device__ __forceinline__ int round_sat_nan_max(double v) {
    v = fmax(fmin(v, 2147483647.0), -2147483648.0);  // (minNum: fmin(NaN, c) == c)
    return (int)rint(v);
}

template <int INTERP>
__device__ __forceinline__ void map_pixel_exact_nan_max(double Xn, double Yn, double W, int& X, int& Y) {
    W = (W != 0.0) ? ((INTERP == kLinear ? 32.0 : 1.0) / W) : 0.0;  // IEEE division
    X = round_sat_nan_max(Xn * W);
    Y = round_sat_nan_max(Yn * W);
}

// the maps are int16: an index saturates BEFORE borderInterpolate (WRAP of 32767 is not WRAP of 40000)
__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// borderInterpolate(p, n, MODE) in closed form for p in [-32768, 32768] (a saturated index, or one past it):
//   REPLICATE clamp; WRAP p mod n; REFLECT q = p mod 2n, q < n ? q : 2n-1-q; REFLECT_101 q = p mod (2n-2), q < n ? q : 2n-2-q.
// per = the period (n, 2n, 2n - 2; 1 for REFLECT_101 of n == 1, which maps everything to 0), off = a multiple of it that makes
// p + off non-negative, mag = fast_div's magic of per for p + off <= off + 32768.
template <int MODE>
__device__ __forceinline__ int border_index(int p, int n, uint32_t per, uint32_t off, uint32_t mag) {
    if (MODE == kBorderReplicate) return min(max(p, 0), n - 1);
    const uint32_t u = (uint32_t)(p + (int)off);
    const int q = (int)(u - fast_div(u, mag, per) * per);
    if (MODE == kBorderWrap) return q;
    if (MODE == kBorderReflect) return q < n ? q : (int)per - 1 - q;
    return q < n ? q : (int)per - q;  // REFLECT_101
}

// One source pixel at column x of a row: exactly its C * sizeof(T) bytes are read (never a wider word over its end).
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> load_pixel(const uint8_t* __restrict__ row, int x, bool vec) {
    Pixel<T, C> p;
    if constexpr (sizeof(T) == 1) {
        const uint8_t* q = row + (uint32_t)(x * C);
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
        const float* q = reinterpret_cast<const float*>(row) + (uint32_t)(x * C);
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = q[k];
    }
    return p;
}

// the taps (source pixels, already remapped) and the blend of the constant-border kernel
template <typename T, int C, int INTERP>
__device__ __forceinline__ Pixel<T, C> sample_taps(const uint8_t* __restrict__ frame, int64_t rs, int x0, int x1, int y0, int y1, int fx, int fy,
                                                   bool vec) {
    const uint8_t* r0 = frame + (int64_t)y0 * rs;
    if (INTERP == kNearest) return load_pixel<T, C>(r0, x0, vec);
    const uint8_t* r1 = frame + (int64_t)y1 * rs;
    const Pixel<T, C> p00 = load_pixel<T, C>(r0, x0, vec), p01 = load_pixel<T, C>(r0, x1, vec);
    const Pixel<T, C> p10 = load_pixel<T, C>(r1, x0, vec), p11 = load_pixel<T, C>(r1, x1, vec);
    Pixel<T, C> out;
    if constexpr (sizeof(T) == 1) {
        out.packed = blend_u8_packed<C>(p00.packed, p01.packed, p10.packed, p11.packed, (uint32_t)fx, (uint32_t)fy);
    } else {
        float w00, w01, w10, w11;
        weights_f32(fx, fy, w00, w01, w10, w11);
#pragma unroll
        for (int k = 0; k < C; k++) out.v[k] = blend_f32(p00.v[k], p01.v[k], p10.v[k], p11.v[k], w00, w01, w10, w11);
    }
    return out;
}

template <typename T, int C, int INTERP, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void warp_border_kernel(const BorderArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = MODE == kBorderTransparent;
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
    const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
    const bool vec = a.src_vec_ok;

    Pixel<T, C> px[PPL];
    bool wr[PPL];
    int bx = -1;
    double X0 = 0.0, Y0 = 0.0, W0 = 0.0;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other (their taps are source pixels too) and not stored
        const int x = xs + j;
        const int bxj = (int)fast_div((uint32_t)x, a.bw0_magic, (uint32_t)a.bw0) * a.bw0;
        if (bxj != bx) {  // (the lane's 4 pixels share an evaluation block unless its width is not a multiple of 4)
            bx = bxj;
            row_terms(Mr, bx, y, X0, Y0, W0);
        }
        const double x1 = (double)(x - bx);
        int X, Y;
        map_pixel_exact_nan_max<INTERP>(X0 + Mr[0] * x1, Y0 + Mr[3] * x1, W0 + Mr[6] * x1, X, Y);
        const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
        const int fx = INTERP == kLinear ? (X & 31) : 0, fy = INTERP == kLinear ? (Y & 31) : 0;
        if constexpr (kTransparent) {
            // inliers only (remapBilinear's (unsigned)sx < width - 1: an identity warp leaves the last column and row alone)
            const bool in = x < a.dst_w && (INTERP == kLinear ? ((unsigned)sx < (unsigned)(a.src_w - 1) && (unsigned)sy < (unsigned)(a.src_h - 1))
                                                             : ((unsigned)sx < (unsigned)a.src_w && (unsigned)sy < (unsigned)a.src_h));
            wr[j] = in;
            if (in) px[j] = sample_taps<T, C, INTERP>(frame, a.src_rs, sx, sx + 1, sy, sy + 1, fx, fy, vec);
        } else {
            wr[j] = x < a.dst_w;
            const int cx0 = border_index<MODE>(sx, a.src_w, a.per_x, a.off_x, a.mag_x);
            const int cy0 = border_index<MODE>(sy, a.src_h, a.per_y, a.off_y, a.mag_y);
            const int cx1 = INTERP == kLinear ? border_index<MODE>(sx + 1, a.src_w, a.per_x, a.off_x, a.mag_x) : cx0;
            const int cy1 = INTERP == kLinear ? border_index<MODE>(sy + 1, a.src_h, a.per_y, a.off_y, a.mag_y) : cy0;
            px[j] = sample_taps<T, C, INTERP>(frame, a.src_rs, cx0, cx1, cy0, cy1, fx, fy, vec);
        }
    }

    uint8_t* drow = a.dst + (int64_t)b * a.dst_fs + (int64_t)y * a.dst_rs;
    bool all = true;
#pragma unroll
    for (int j = 0; j < PPL; j++) all = all && wr[j];
    // wide stores (the layout rule of bevwarp_warp's dst_vec_ok) for a lane whose 4 pixels are all written; per pixel otherwise
    if constexpr (sizeof(T) == 1) {
        uint8_t* d = drow + (int64_t)xs * C;
        uint32_t p[PPL];
#pragma unroll
        for (int j = 0; j < PPL; j++) p[j] = kTransparent && !wr[j] ? 0u : px[j].packed;
        if (a.dst_vec_ok && all) {
            if constexpr (C == 1) {
                *reinterpret_cast<uint32_t*>(d) = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
            } else if constexpr (C == 2) {
                u32x2 o = {p[0] | (p[1] << 16), p[2] | (p[3] << 16)};
                *reinterpret_cast<u32x2*>(d) = o;
            } else if constexpr (C == 3) {
                u32x3 o = {__builtin_amdgcn_perm(p[1], p[0], 0x04020100u), __builtin_amdgcn_perm(p[2], p[1], 0x05040201u), __builtin_amdgcn_perm(p[3], p[2], 0x06050402u)};
                wide_store(reinterpret_cast<u32x3*>(d), o);
            } else {
                u32x4 o = {p[0], p[1], p[2], p[3]};
                wide_store(reinterpret_cast<u32x4*>(d), o);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++)
                if (wr[j])
#pragma unroll
                    for (int k = 0; k < C; k++) d[j * C + k] = (uint8_t)(p[j] >> (8 * k));
        }
    } else {
        float* d = reinterpret_cast<float*>(drow) + (int64_t)xs * C;
        if (a.dst_vec_ok && all) {  // the lane's 4 C floats as C 16-byte stores
#pragma unroll
            for (int i = 0; i < C; i++) {
                f32x4 o = {px[(4 * i) / C].v[(4 * i) % C], px[(4 * i + 1) / C].v[(4 * i + 1) % C], px[(4 * i + 2) / C].v[(4 * i + 2) % C],
                           px[(4 * i + 3) / C].v[(4 * i + 3) % C]};
                wide_store(reinterpret_cast<f32x4*>(d) + i, o);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++)
                if (wr[j])
#pragma unroll
                    for (int k = 0; k < C; k++) d[j * C + k] = px[j].v[k];
        }
    }
}

template <typename T, int INTERP, int MODE>
void launch_c(const BorderArgs& a, int channels, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    switch (channels) {
        case 1: hipLaunchKernelGGL((warp_border_kernel<T, 1, INTERP, MODE>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((warp_border_kernel<T, 2, INTERP, MODE>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((warp_border_kernel<T, 3, INTERP, MODE>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((warp_border_kernel<T, 4, INTERP, MODE>), grid, block, 0, stream, a); break;
    }
}

template <typename T, int INTERP>
void launch_mode(const BorderArgs& a, int channels, int mode, dim3 grid, hipStream_t stream) {
    switch (mode) {
        case kBorderReplicate: launch_c<T, INTERP, kBorderReplicate>(a, channels, grid, stream); break;
        case kBorderReflect: launch_c<T, INTERP, kBorderReflect>(a, channels, grid, stream); break;
        case kBorderWrap: launch_c<T, INTERP, kBorderWrap>(a, channels, grid, stream); break;
        case kBorderReflect101: launch_c<T, INTERP, kBorderReflect101>(a, channels, grid, stream); break;
        default: launch_c<T, INTERP, kBorderTransparent>(a, channels, grid, stream); break;
    }
}

}  // namespace

hipError_t launch_warp_border(const BorderArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    if (dtype == 0)
        (interp == kNearest ? launch_mode<uint8_t, kNearest> : launch_mode<uint8_t, kLinear>)(a, channels, mode, grid, stream);
    else
        (interp == kNearest ? launch_mode<float, kNearest> : launch_mode<float, kLinear>)(a, channels, mode, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
