// stitch_sample.h -- what the stitches through warp maps do per camera and pixel (device code, gfx950), shared by warp_stitch_maps.hip,
// warp_stitch_maps_nv12_out.hip and warp_stitch_maps_planes.hip: a camera's map entries for a lane, an inlier sampled from interleaved or
// NV12 frames, and FEATHER's division, which warp_stitch.hip uses too.  Every sampled pixel is an inlier: bilinear taps are columns
// sx, sx + 1 and rows sy, sy + 1 of the source, never clamped or remapped, so the 6-byte pair loads (tap_load.h) and the NV12 windows
// apply to every covered pixel with no per-lane decision.  The gained units (BEVWARP_STITCH_GAIN_UNIT, warp_stitch_maps.h) are those three
// units' text with the samplers' tap operation set to the camera's gain.  See DESIGN.md sections 4.16, 4.20 and 4.24.  Not installed.
#pragma once
#include "warp_stitch_maps.h"
#include "lens_pixel.h"
#include "nv12_sample.h"
#include "tap_load.h"

namespace bevwarp {
namespace {

// floor(n / d) for 0 <= n < 2^23 and 1 <= d < 2^16 with a quotient of at most 255 (the rounded mean of bytes): n and d are floats
// exactly, v_rcp_f32 is within one ulp and the product rounds once more, so the estimate is within 256 * 2^-22 of n / d and its
// truncation within one of the quotient; one step either way makes it exact.
__device__ __forceinline__ int div_byte_mean(int n, int d) {
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int r = n - q * d;
    q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
    return q;
}

// What a sampler does to each packed tap before the blend (nearest: to its one tap).  The plain stitches keep the tap ...
struct TapKeep {
    __device__ __forceinline__ uint32_t operator()(uint32_t p) const { return p; }
};
// ... and the gained ones (BEVWARP_STITCH_GAIN) replace each of its 3 channels by min(255, (p * Gc + 128) >> 8), Gc the
// camera's Q8 gain of that channel: g is the camera's gain word G0 | G1 << 10 | G2 << 20, wave-uniform, so its fields are scalar.  p * Gc
// reaches 255 * 1023: a 24-bit multiply-add holds it, a packed 16-bit one would not.
struct TapGain {
    uint32_t g;
    __device__ __forceinline__ uint32_t operator()(uint32_t p) const {
        const uint32_t c0 = min(255u, ((p & 0xffu) * (g & 1023u) + 128u) >> 8);
        const uint32_t c1 = min(255u, (((p >> 8) & 0xffu) * ((g >> 10) & 1023u) + 128u) >> 8);
        const uint32_t c2 = min(255u, (((p >> 16) & 0xffu) * ((g >> 20) & 1023u) + 128u) >> 8);
        return c0 | (c1 << 8) | (c2 << 16);
    }
};
// the tap operation of camera k of a launch, by the type of the launch's arguments
template <class Args>
__device__ __forceinline__ TapKeep camera_tap(const Args&, int) {
    return {};
}
template <class Args>
__device__ __forceinline__ TapGain camera_tap(const Gained<Args>& a, int k) {
    return {a.gains[k]};
}

// An inlier of interleaved frames: a frame is below 2 GiB (the source limits), so 32 bits hold the offsets.
template <typename T, int C, int INTERP>
__device__ __forceinline__ Pixel<T, C> sample_inlier(const uint8_t* __restrict__ frame, uint32_t rs, int sx, int sy, int fx, int fy, bool vec) {
    const uint32_t o00 = (uint32_t)sy * rs + (uint32_t)sx * (uint32_t)(C * sizeof(T));
    if constexpr (INTERP == kNearest) {
        return load_at<T, C>(frame, o00, vec);
    } else {
        const uint32_t o10 = o00 + rs;
        Pixel<T, C> p00, p01, p10, p11;
        if constexpr (sizeof(T) == 1 && C == 3) {
            load_pair_u8x3(frame, o00, p00, p01);
            load_pair_u8x3(frame, o10, p10, p11);
        } else {
            constexpr uint32_t kPx = C * sizeof(T);
            p00 = load_at<T, C>(frame, o00, vec), p01 = load_at<T, C>(frame, o00 + kPx, vec);
            p10 = load_at<T, C>(frame, o10, vec), p11 = load_at<T, C>(frame, o10 + kPx, vec);
        }
        return blend_taps<T, C>(p00, p01, p10, p11, fx, fy);
    }
}

// an inlier of interleaved 8-bit pixels of 3 channels, packed
template <int INTERP, class Tap = TapKeep>
__device__ __forceinline__ uint32_t sample_inlier(const uint8_t* __restrict__ frame, uint32_t rs, int sx, int sy, int fx, int fy, Tap tap = Tap()) {
    const uint32_t o00 = (uint32_t)sy * rs + (uint32_t)sx * 3u;
    if constexpr (INTERP == kNearest) {
        return tap(load_at(frame, o00));
    } else {
        uint32_t p00, p01, p10, p11;
        load_pair(frame, o00, p00, p01);
        load_pair(frame, o00 + rs, p10, p11);
        return blend_u8_packed<3>(tap(p00), tap(p01), tap(p10), tap(p11), (uint32_t)fx, (uint32_t)fy);
    }
}

// An inlier of NV12 frames, packed in the order convert<RGB> gives.  A tap at pixel (c, r) reads Y[r][c] and the pair (r >> 1, c >> 1).
// Bilinear: the two taps of a row are ONE 2-byte window of the Y row, and where a row of pairs holds two of them (src_w >= 4: `window`,
// uniform over the camera) their pairs lie in ONE 4-byte window starting at pair min(sx >> 1, src_w / 2 - 2); a source 2 px wide has one
// pair per row, which both taps share.  No byte outside the first src_w bytes of a plane row is read.  `tap` sees every converted tap.
template <int INTERP, int RGB, class Tap = TapKeep>
__device__ __forceinline__ uint32_t sample_inlier_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, uint32_t y_rs, uint32_t uv_rs, int src_w,
                                                       bool window, int sx, int sy, int fx, int fy, Tap tap = Tap()) {
    const uint32_t yo0 = (uint32_t)sy * y_rs + (uint32_t)sx, uo0 = (uint32_t)(sy >> 1) * uv_rs;
    const int p0 = sx >> 1;
    if constexpr (INTERP == kNearest) {
        const uint32_t q = *reinterpret_cast<const uint16_t*>(uvf + uo0 + 2u * (uint32_t)p0);
        return tap(convert_packed<RGB>(yf[yo0], chroma_terms(q)));
    } else {
        const uint32_t yo1 = yo0 + y_rs, uo1 = (uint32_t)((sy + 1) >> 1) * uv_rs;
        uint16_t w0, w1;
        __builtin_memcpy(&w0, yf + yo0, 2);  // (unaligned)
        __builtin_memcpy(&w1, yf + yo1, 2);
        uint32_t q00, q01, q10, q11;
        if (window) {
            const int p1 = (sx + 1) >> 1, ps = min(p0, (src_w >> 1) - 2);
            const uint32_t s0 = 16u * (uint32_t)(p0 - ps), s1 = 16u * (uint32_t)(p1 - ps);  // (p1 - ps is 0 or 1: p0 passes ps only at sx = src_w - 2)
            uint32_t v0, v1;
            __builtin_memcpy(&v0, uvf + uo0 + 2u * (uint32_t)ps, 4);  // (2-byte aligned)
            __builtin_memcpy(&v1, uvf + uo1 + 2u * (uint32_t)ps, 4);
            q00 = (v0 >> s0) & 0xffffu, q01 = (v0 >> s1) & 0xffffu, q10 = (v1 >> s0) & 0xffffu, q11 = (v1 >> s1) & 0xffffu;
        } else {
            q00 = q01 = *reinterpret_cast<const uint16_t*>(uvf + uo0);  // src_w == 2: sx is 0
            q10 = q11 = *reinterpret_cast<const uint16_t*>(uvf + uo1);
        }
        const uint32_t p00 = convert_packed<RGB>(w0 & 0xffu, chroma_terms(q00)), p01 = convert_packed<RGB>((uint32_t)w0 >> 8, chroma_terms(q01));
        const uint32_t p10 = convert_packed<RGB>(w1 & 0xffu, chroma_terms(q10)), p11 = convert_packed<RGB>((uint32_t)w1 >> 8, chroma_terms(q11));
        return blend_u8_packed<3>(tap(p00), tap(p01), tap(p10), tap(p11), (uint32_t)fx, (uint32_t)fy);
    }
}

// The lane's 4 entries of camera `cam`, map of frame b (a shared map: frame strides of 0), row y, first pixel xs: map_entry.h's loads with
// the camera's own planes.  No entry past the row's end is read (such an entry is the sentinel: it covers nothing).
template <int INTERP>
__device__ __forceinline__ void load_camera_entries(const StitchMapCamera& cam, uint32_t b, int y, int xs, int dst_w, uint32_t (&e)[kBorderPPL], uint32_t (&fr)[kBorderPPL]) {
    constexpr int PPL = kBorderPPL;
    const bool wide = cam.map_vec_ok && xs + PPL <= dst_w;
    const uint8_t* xrow = cam.xy + (int64_t)b * cam.xy_fs + (int64_t)y * cam.xy_rs + (int64_t)xs * 4;
    if (wide) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xrow);
        e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < PPL; j++) e[j] = (xs + j < dst_w) ? reinterpret_cast<const uint32_t*>(xrow)[j] : 0x80008000u;
    }
    if constexpr (INTERP == kLinear) {
        const uint8_t* frow = cam.frac + (int64_t)b * cam.frac_fs + (int64_t)y * cam.frac_rs + (int64_t)xs * 2;
        if (wide) {
            const u32x2 v = *reinterpret_cast<const u32x2*>(frow);
            fr[0] = v.x & 0xffffu, fr[1] = v.x >> 16, fr[2] = v.y & 0xffffu, fr[3] = v.y >> 16;
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) fr[j] = (xs + j < dst_w) ? (uint32_t)reinterpret_cast<const uint16_t*>(frow)[j] : 0u;
        }
    }
}

}  // namespace
}  // namespace bevwarp
