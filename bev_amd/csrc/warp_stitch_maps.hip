// warp_stitch_maps.hip -- several fixed cameras sampled through their warp maps into one BEV canvas in one launch (bevwarp_stitch_maps,
// bevwarp_stitch_maps_nv12).  It is bevwarp_warp_stitch's camera loop and blend rules (warp_stitch.hip) over
// bevwarp_remap's map entries (warp_map.hip): per camera the lane's 4 entries replace the float64 chain, a camera covers a pixel where its
// entry passes BORDER_TRANSPARENT's inlier test against that camera's own frame, and the covering cameras are combined by OVER or FEATHER.
// The maps carry the lens, so there is no float64 here.  The NV12 instances convert every tap before the blend (nv12_sample.h), as
// bevwarp_remap_nv12 does.
//
// The frame -- item decoding and the store of a lane's 4 pixels -- is flat_frame.h; one frame per item: a lane cannot keep 8 cameras'
// entries in registers, and a shared map is re-read through the caches.  The cameras are kernel arguments and the loop's camera number is
// wave-uniform, so a camera's fields are scalar loads; whether a camera's planes admit the lane-wide map loads is one of them, and a launch
// may mix cameras that do and cameras that do not.
//
// Every sampled pixel is an inlier: bilinear taps are columns sx, sx + 1 and rows sy, sy + 1 of the source, never clamped or remapped.  So
// the 6-byte pair loads (8-bit, 3 channels) and the NV12 windows apply to every covered pixel with no per-lane decision; warp_map.hip and
// warp_map_nv12.hip, where an edge lane falls back to loads tap by tap, describe both.  The helpers are restated here rather than moved
// into a header: those units' machine code stays what it was.
#include "warp_stitch_maps.h"
#include "lens_pixel.h"
#include "nv12_sample.h"

#include <type_traits>

namespace bevwarp {
namespace {

// floor(n / d) for 0 <= n < 2^23 and 1 <= d < 2^16 with a quotient of at most 255 (warp_stitch.hip's, which has the argument)
__device__ __forceinline__ int div_byte_mean(int n, int d) {
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int r = n - q * d;
    q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
    return q;
}

// One source pixel at a byte offset of the frame: exactly its C * sizeof(T) bytes are read (warp_map.hip's load_at).
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> load_at(const uint8_t* __restrict__ frame, uint32_t off, bool vec) {
    Pixel<T, C> p;
    const uint8_t* q = frame + off;
    if constexpr (sizeof(T) == 1) {
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
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = reinterpret_cast<const float*>(q)[k];
    }
    return p;
}

// the two adjacent taps of a row of 8-bit 3-channel pixels: 6 contiguous bytes, never a byte beyond them (warp_map.hip's load_pair_u8x3)
__device__ __forceinline__ void load_pair_u8x3(const uint8_t* __restrict__ frame, uint32_t off, Pixel<uint8_t, 3>& p0, Pixel<uint8_t, 3>& p1) {
    uint32_t lo;
    uint16_t hi;
    __builtin_memcpy(&lo, frame + off, 4);
    __builtin_memcpy(&hi, frame + off + 4, 2);
    p0.packed = lo & 0xffffffu;
    p1.packed = __builtin_amdgcn_alignbit((uint32_t)hi, lo, 24);  // bytes 3, 4, 5
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

// convert<RGB> (nv12_sample.h) with the middle channel behind a value barrier: warp_map_nv12.hip's convert_packed, which records why --
// fused into v_ashr_pk_u8_i32, two channels' shift and clamp gave wrong pixels on the MI355X in one instance of that unit.  The barrier
// costs no instruction.
template <int RGB>
__device__ __forceinline__ uint32_t convert_packed(uint32_t Y, const Chroma& c) {
    uint32_t r, g, b;
    convert_channels(Y, c, r, g, b);
    asm("" : "+v"(g));
    return RGB ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
}

// An inlier of NV12 frames, packed in the destination's order.  A tap at pixel (c, r) reads Y[r][c] and the pair (r >> 1, c >> 1).
// Bilinear: the two taps of a row are ONE 2-byte window of the Y row, and where a row of pairs holds two of them (src_w >= 4: `window`,
// uniform over the camera) their pairs lie in ONE 4-byte window starting at pair min(sx >> 1, src_w / 2 - 2); a source 2 px wide has one
// pair per row, which both taps share.  No byte outside the first src_w bytes of a plane row is read.
template <int INTERP, int RGB>
__device__ __forceinline__ uint32_t sample_inlier_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, uint32_t y_rs, uint32_t uv_rs, int src_w,
                                                       bool window, int sx, int sy, int fx, int fy) {
    const uint32_t yo0 = (uint32_t)sy * y_rs + (uint32_t)sx, uo0 = (uint32_t)(sy >> 1) * uv_rs;
    const int p0 = sx >> 1;
    if constexpr (INTERP == kNearest) {
        const uint32_t q = *reinterpret_cast<const uint16_t*>(uvf + uo0 + 2u * (uint32_t)p0);
        return convert_packed<RGB>(yf[yo0], chroma_terms(q));
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
        return blend_u8_packed<3>(p00, p01, p10, p11, (uint32_t)fx, (uint32_t)fy);
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

// The kernels' common body.  NV12: T = uint8_t, C = 3, and RGB is the destination's channel order.
template <typename T, int C, int INTERP, int BLEND, bool NV12, int RGB>
__device__ __forceinline__ void stitch_maps_body(const StitchMapsArgs& a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kFeather = BLEND == kStitchFeather, kU8 = sizeof(T) == 1;
    using Acc = std::conditional_t<kU8, int, float>;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;

    // per pixel, as in warp_stitch_kernel: OVER keeps the pixel and whether it is still undecided; FEATHER the weighted sums and the sum
    // of weights, float32 the cover count and the first covering camera's value as well
    Pixel<T, C> px[PPL];
    bool wr[PPL], todo[PPL];
    Acc acc[PPL][C];
    int wsum[PPL], cnt[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        todo[j] = xs + j < a.dst_w;  // pixels past the row's end are neither computed nor stored
        wr[j] = false;
        wsum[j] = cnt[j] = 0;
#pragma unroll
        for (int c = 0; c < C; c++) acc[j][c] = 0;
    }

    // OVER runs from the last camera to the first and stops when the lane's four pixels are decided; FEATHER runs in ascending order, the
    // order of its float32 sums
    const int n = a.n_cams;
    for (int i = 0; i < n; i++) {
        if (!kFeather && !(todo[0] || todo[1] || todo[2] || todo[3])) break;
        const StitchMapCamera& cam = a.cams[kFeather ? i : n - 1 - i];
        uint32_t e[PPL], fr[PPL];
        load_camera_entries<INTERP>(cam, b, y, xs, a.dst_w, e, fr);
        const uint8_t* frame = cam.src + (int64_t)b * cam.src_fs;
        const uint8_t* uvf = NV12 ? cam.uv + (int64_t)b * cam.uv_fs : nullptr;
        const uint32_t rs = (uint32_t)cam.src_rs, uv_rs = (uint32_t)cam.uv_rs;  // (below 2^24: the source limits)
        const int sw = cam.src_w, sh = cam.src_h;
        const bool vec = cam.src_vec_ok, window = sw >= 4;
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (!todo[j]) continue;
            const int sx = (int)(short)(e[j] & 0xffffu), sy = (int)e[j] >> 16;
            const int fx = INTERP == kLinear ? (int)(fr[j] & 31u) : 0, fy = INTERP == kLinear ? (int)((fr[j] >> 5) & 31u) : 0;  // (higher bits are ignored)
            // bevwarp_remap's TRANSPARENT inlier test against THIS camera's frame: every tap read below is a source pixel
            const bool in = INTERP == kLinear ? ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1))
                                              : ((unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh);
            if (!in) continue;
            Pixel<T, C> p;
            if constexpr (NV12)
                p.packed = sample_inlier_nv12<INTERP, RGB>(frame, uvf, rs, uv_rs, sw, window, sx, sy, fx, fy);
            else
                p = sample_inlier<T, C, INTERP>(frame, rs, sx, sy, fx, fy, vec);
            wr[j] = true;
            if constexpr (!kFeather) {
                px[j] = p;
                todo[j] = false;
            } else {
                // whole source pixels to the nearest frame edge (>= 1 for an inlier), cut off at F
                const int w = min(min(min(sx + 1, sw - sx), min(sy + 1, sh - sy)), a.feather);
                wsum[j] += w;
                if constexpr (kU8) {
#pragma unroll
                    for (int c = 0; c < C; c++) acc[j][c] += (int)((p.packed >> (8 * c)) & 0xffu) * w;  // (the sums stay below 2^23)
                } else {
                    if (cnt[j] == 0) px[j] = p;
                    cnt[j]++;
                    const float wf = (float)w;
#pragma unroll
                    for (int c = 0; c < C; c++) acc[j][c] = acc[j][c] + wf * p.v[c];  // (each rounded to float32: no FMA in this unit)
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < PPL; j++) {
        if constexpr (kFeather) {
            if (wr[j]) {
                if constexpr (kU8) {
                    uint32_t out = 0;
#pragma unroll
                    for (int c = 0; c < C; c++) out |= (uint32_t)div_byte_mean(acc[j][c] + (wsum[j] >> 1), wsum[j]) << (8 * c);
                    px[j].packed = out;
                } else if (cnt[j] > 1) {
                    const float wf = (float)wsum[j];
#pragma unroll
                    for (int c = 0; c < C; c++) px[j].v[c] = __fdiv_rn(acc[j][c], wf);  // one correctly rounded division
                }
            }
        }
        if (!wr[j] && a.fill && xs + j < a.dst_w) {  // no camera covers the pixel: the border pixel, or nothing
            wr[j] = true;
            if constexpr (kU8) {
                px[j].packed = a.bv_u8;
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) px[j].v[c] = a.bv_f[c];
            }
        }
    }

    store_lane_pixels<T, C, true>(a, b, y, xs, px, wr);
}

template <typename T, int C, int INTERP, int BLEND>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void stitch_maps_kernel(const StitchMapsArgs a) {
    stitch_maps_body<T, C, INTERP, BLEND, false, 0>(a);
}

template <int INTERP, int BLEND, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void stitch_maps_nv12_kernel(const StitchMapsArgs a) {
    stitch_maps_body<uint8_t, 3, INTERP, BLEND, true, RGB>(a);
}

template <typename T, int INTERP, int BLEND>
void launch_c(const StitchMapsArgs& a, int channels, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    switch (channels) {
        case 1: hipLaunchKernelGGL((stitch_maps_kernel<T, 1, INTERP, BLEND>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((stitch_maps_kernel<T, 2, INTERP, BLEND>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((stitch_maps_kernel<T, 3, INTERP, BLEND>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((stitch_maps_kernel<T, 4, INTERP, BLEND>), grid, block, 0, stream, a); break;
    }
}

template <typename T, int INTERP>
void launch_blend(const StitchMapsArgs& a, int channels, int blend, dim3 grid, hipStream_t stream) {
    if (blend == kStitchFeather)
        launch_c<T, INTERP, kStitchFeather>(a, channels, grid, stream);
    else
        launch_c<T, INTERP, kStitchOver>(a, channels, grid, stream);
}

template <int INTERP, int BLEND>
void launch_order(const StitchMapsArgs& a, int rgb_order, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (rgb_order)
        hipLaunchKernelGGL((stitch_maps_nv12_kernel<INTERP, BLEND, 1>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((stitch_maps_nv12_kernel<INTERP, BLEND, 0>), grid, block, 0, stream, a);
}

template <int INTERP>
void launch_nv12_blend(const StitchMapsArgs& a, int blend, int rgb_order, dim3 grid, hipStream_t stream) {
    if (blend == kStitchFeather)
        launch_order<INTERP, kStitchFeather>(a, rgb_order, grid, stream);
    else
        launch_order<INTERP, kStitchOver>(a, rgb_order, grid, stream);
}

}  // namespace

hipError_t launch_stitch_maps(const StitchMapsArgs& a, int dtype, int channels, int interp, int blend, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    if (dtype == 0)
        (interp == kNearest ? launch_blend<uint8_t, kNearest> : launch_blend<uint8_t, kLinear>)(a, channels, blend, grid, stream);
    else
        (interp == kNearest ? launch_blend<float, kNearest> : launch_blend<float, kLinear>)(a, channels, blend, grid, stream);
    return hipGetLastError();
}

hipError_t launch_stitch_maps_nv12(const StitchMapsArgs& a, int interp, int blend, int rgb_order, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    (interp == kNearest ? launch_nv12_blend<kNearest> : launch_nv12_blend<kLinear>)(a, blend, rgb_order, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
