// flat_frame.h -- the frame that the border, bicubic, NV12, lens and stitch warps share (warp_border.hip, warp_cubic.hip, warp_nv12.hip,
// warp_nv12_planes.hip, warp_nv12_out.hip, warp_lens.hip, warp_stitch.hip): a flat grid, item -> frame / tile row / tile column by
// fast_div, one wave per destination row, 4 consecutive pixels per lane, the reference's exact float64 coordinate chain pixel by pixel,
// wide stores for lanes that write all 4 pixels.  What a unit adds is its sampler, its kernel body from "for each of my 4 pixels" on, and
// its launcher.  See DESIGN.md section 4.9.
#pragma once
#include "sample.h"

namespace bevwarp {

// One destination row segment of 4 pixels per lane, a wave per row, four rows per workgroup; the grid is flat:
// item t -> frame t / tiles_per_frame, tile (t mod tiles_per_frame) -> (tile row, tile column).
constexpr int kBorderPPL = 4;
constexpr int kBorderTileW = 64 * kBorderPPL;
constexpr int kBorderTileH = 4;

// What every kernel of the frame takes: the destination, the matrices and the grid (the host fills it in one place, fill_frame)
struct FrameArgs {
    uint8_t* dst;
    const double* minv;           // device, inverse matrices
    int64_t dst_fs, dst_rs;       // bytes
    int dst_h, dst_w;
    int m_stride;                 // 9 (one matrix per frame) or 0 (shared)
    int bw0;                      // evaluation block width of the reference algorithm
    int tiles_x, tiles_per_frame;
    uint32_t bw0_magic, tx_magic, tpf_magic;  // fast_div magics (0 = divide)
    int dst_vec_ok;               // destination layout admits the wide stores (each entry point's own rule)
};

namespace {

// Item and lane -> frame b, destination row y and the lane's first pixel xs.  False: the lane lies outside the destination.
__device__ __forceinline__ bool lane_position(const FrameArgs& a, uint32_t& b, int& y, int& xs) {
    const uint32_t t = blockIdx.x;
    b = fast_div(t, a.tpf_magic, (uint32_t)a.tiles_per_frame);
    const uint32_t r = t - b * (uint32_t)a.tiles_per_frame;
    const uint32_t ty = fast_div(r, a.tx_magic, (uint32_t)a.tiles_x);
    const uint32_t tx = r - ty * (uint32_t)a.tiles_x;
    y = (int)ty * kBorderTileH + (int)(threadIdx.x >> 6);
    xs = (int)tx * kBorderTileW + (int)(threadIdx.x & 63) * kBorderPPL;
    return y < a.dst_h && xs < a.dst_w;
}

__device__ __forceinline__ uint8_t* dst_row(const FrameArgs& a, uint32_t b, int y) { return a.dst + (int64_t)b * a.dst_fs + (int64_t)y * a.dst_rs; }

// The exact chain's numerators along a row: row_terms once per evaluation block, then (Xn, Yn, W) of one pixel at a time.  Pixels past
// the row's end are computed like any other.
struct RowWalk {
    double Mr[9];
    double X0 = 0.0, Y0 = 0.0, W0 = 0.0;
    int y, bx = -1;

    __device__ __forceinline__ RowWalk(const FrameArgs& a, uint32_t b, int row) : y(row) {
        const double* M = a.minv + (int64_t)b * a.m_stride;
#pragma unroll
        for (int i = 0; i < 9; i++) Mr[i] = M[i];
    }
    // ... from the matrix itself: a kernel with several sources, each with matrices of its own (warp_stitch.hip)
    __device__ __forceinline__ RowWalk(const double* __restrict__ M, int row) : y(row) {
#pragma unroll
        for (int i = 0; i < 9; i++) Mr[i] = M[i];
    }
    __device__ __forceinline__ void pixel(const FrameArgs& a, int x, double& Xn, double& Yn, double& W) {
        const int bxj = (int)fast_div((uint32_t)x, a.bw0_magic, (uint32_t)a.bw0) * a.bw0;
        if (bxj != bx) {  // (the lane's 4 pixels share an evaluation block unless its width is not a multiple of 4)
            bx = bxj;
            row_terms(Mr, bx, y, X0, Y0, W0);
        }
        const double x1 = (double)(x - bx);
        Xn = X0 + Mr[0] * x1, Yn = Y0 + Mr[3] * x1, W = W0 + Mr[6] * x1;
    }
};

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

// The taps of one pixel (source pixels: indices already remapped, or an inlier's) and the blend of the constant-border kernel: the border
// and the stitch kernels sample with it.
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

// A lane's kBorderPPL consecutive pixels of row y of frame b, first pixel xs: wide stores (the layout rule of bevwarp_warp's
// dst_vec_ok) for a lane whose pixels are all written; per pixel otherwise.  PREDICATED: some pixels may be unwritten for a
// reason other than the row's end (TRANSPARENT), and their registers hold nothing.
template <typename T, int C, bool PREDICATED>
__device__ __forceinline__ void store_lane_pixels(const FrameArgs& a, uint32_t b, int y, int xs, const Pixel<T, C> (&px)[kBorderPPL],
                                                  const bool (&wr)[kBorderPPL]) {
    constexpr int PPL = kBorderPPL;
    uint8_t* drow = dst_row(a, b, y);
    bool all = wr[PPL - 1];  // (unpredicated: only the row's end leaves pixels unwritten, the last one first)
    if constexpr (PREDICATED) {
#pragma unroll
        for (int j = 0; j < PPL - 1; j++) all = all && wr[j];
    }
    if constexpr (sizeof(T) == 1) {
        uint8_t* d = drow + (int64_t)xs * C;
        uint32_t p[PPL];
#pragma unroll
        for (int j = 0; j < PPL; j++) p[j] = PREDICATED && !wr[j] ? 0u : px[j].packed;
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

}  // namespace
}  // namespace bevwarp
