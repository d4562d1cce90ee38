// warp_map_nv12.hip -- NV12 frames sampled through a fixed camera's warp map (bevwarp_remap_nv12, bevwarp_remap_nv12_planes; DESIGN.md
// section 4.19): bevwarp_remap of the converted frame, bit for bit, with every tap converted before the blend (OpenCV's 8-bit
// YUV420sp -> RGB fixed point, nv12_sample.h) and the converted frame never in memory.  The map carries the lens, so there is no float64
// here either.  The structure is remap_kernel's (warp_map.hip): a workgroup loads its tile's map entries once, derives what does not
// depend on the frame -- per pixel the byte offsets of the taps in the Y plane and in the plane of (U, V) pairs, the weights, and the
// inside mask (BORDER_CONSTANT) or the write mask (BORDER_TRANSPARENT) -- and walks frames_per_item frames with that in registers.
//
// The frame is flat_frame.h; the map loads (map_entry.h) and the index stage (map_entry_taps.inc) are shared with remap_kernel; conversion and blend are
// nv12_sample.h; the BGR store is store_lane_pixels and the plane store plane_store.inc, shared with warp_nv12_planes.hip.
//
// The tap gathers bind this kernel as they bind remap_kernel: tap by tap a bilinear pixel takes 8 loads per
// frame, 4 bytes of Y and 4 pairs.  Where the two taps of a row are adjacent columns c and c + 1 they are the two bytes of ONE 2-byte
// window of the Y row, and their pairs -- the same pair or two adjacent ones -- lie in ONE 4-byte window of the row of pairs that starts
// at pair min(c >> 1, src_w / 2 - 2): 4 loads.  Which form a lane takes is frame-invariant and decided once per item, as remap_kernel
// decides `pair`: a lane whose 4 pixels all have adjacent columns -- every inlier, every interior pixel -- takes the windows; a lane with
// a clamped or remapped edge tap, and every lane of a source 2 px wide, takes the loads tap by tap.  Neither form reads a byte outside
// the first src_w bytes of a plane row.
#include "warp_map_nv12.h"
#include "map_entry.h"
#include "nv12_sample.h"
#include "warp_kernels.h"

namespace bevwarp {
namespace {

// What a lane keeps of one map entry for every frame it walks.  All offsets are of source pixels (remapped, an inlier's, or clamped);
// a plane is below 2 GiB, so 32 bits hold them and a load is the plane's wave-uniform base plus one register.
struct NvTaps {
    uint32_t y00, y01, y10, y11;  // bytes into the Y plane; a window lane loads 2 bytes at y00 and at y10
    uint32_t u00, u01, u10, u11;  // bytes into the plane of pairs (even); a window lane loads 4 bytes at u00 and at u10 (the windows' starts)
    uint32_t w;  // fx | fy << 5 | in << 10 | s0 << 14 | s1 << 15; in: map_entry_taps.inc's; s0, s1: window lanes, which pair of the window column c0 / c1 takes
    __device__ __forceinline__ uint32_t fx() const { return w & 31u; }
    __device__ __forceinline__ uint32_t fy() const { return (w >> 5) & 31u; }
    __device__ __forceinline__ uint32_t in() const { return (w >> 10) & 15u; }
};

// a (U, V) pair at an even byte offset of a plane whose base and strides are even
__device__ __forceinline__ uint32_t pair_at(const uint8_t* __restrict__ uvf, uint32_t off) { return *reinterpret_cast<const uint16_t*>(uvf + off); }

// convert<RGB> (nv12_sample.h) with the middle channel behind a value barrier.  Without it the compiler fuses two channels' shift and
// clamp of one instance of the bilinear R, G, B kernel into v_ashr_pk_u8_i32, and on the MI355X that instance -- the only one of the
// unit's kernels with the instruction -- gave pixels up to 128 off the definition (2.6 % of a frame; every other instance was exact).
// The barrier costs no instruction: each channel keeps its own v_ashrrev_i32 and v_med3_i32, as in every other kernel of the library.
template <int RGB>
__device__ __forceinline__ uint32_t convert_packed(uint32_t Y, const Chroma& c) {
    uint32_t r, g, b;
    convert_channels(Y, c, r, g, b);
    asm("" : "+v"(g));
    return RGB ? (r | (g << 8) | (b << 16)) : (b | (g << 8) | (r << 16));
}

// One destination pixel of one frame, packed in the order convert<RGB> gives.  WINDOW: the lane's pixels all have adjacent columns.
template <int INTERP, int MODE, int RGB, bool WINDOW>
__device__ __forceinline__ uint32_t sample_entry_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, const NvTaps& t, uint32_t border) {
    if constexpr (INTERP == kNearest) {
        const uint32_t p = convert_packed<RGB>(yf[t.y00], chroma_terms(pair_at(uvf, t.u00)));
        return (MODE != 0 || (t.in() & 1u)) ? p : border;
    } else {
        // every load is of a source pixel (the constant border: of the CLAMPED position) and issues before the first wait
        uint32_t Y00, Y01, Y10, Y11, q00, q01, q10, q11;
        if constexpr (WINDOW) {
            uint16_t w0, w1;
            uint32_t v0, v1;
            __builtin_memcpy(&w0, yf + t.y00, 2);  // (unaligned, like sample_nv12's windows)
            __builtin_memcpy(&w1, yf + t.y10, 2);
            __builtin_memcpy(&v0, uvf + t.u00, 4);  // (2-byte aligned)
            __builtin_memcpy(&v1, uvf + t.u10, 4);
            const uint32_t s0 = (t.w >> 10) & 16u, s1 = (t.w >> 11) & 16u;  // 16 * (bit 14), 16 * (bit 15)
            Y00 = w0 & 0xffu, Y01 = (uint32_t)w0 >> 8, Y10 = w1 & 0xffu, Y11 = (uint32_t)w1 >> 8;
            q00 = (v0 >> s0) & 0xffffu, q01 = (v0 >> s1) & 0xffffu, q10 = (v1 >> s0) & 0xffffu, q11 = (v1 >> s1) & 0xffffu;
        } else {
            Y00 = yf[t.y00], Y01 = yf[t.y01], Y10 = yf[t.y10], Y11 = yf[t.y11];
            q00 = pair_at(uvf, t.u00), q01 = pair_at(uvf, t.u01), q10 = pair_at(uvf, t.u10), q11 = pair_at(uvf, t.u11);
        }
        uint32_t p00 = convert_packed<RGB>(Y00, chroma_terms(q00)), p01 = convert_packed<RGB>(Y01, chroma_terms(q01));
        uint32_t p10 = convert_packed<RGB>(Y10, chroma_terms(q10)), p11 = convert_packed<RGB>(Y11, chroma_terms(q11));
        if constexpr (MODE == 0) {
            // a tap outside is the border value, in the destination's order and not converted (all four outside: the blend of four
            // border pixels is the border pixel)
            const uint32_t in = t.in();
            p00 = (in & 1u) ? p00 : border, p01 = (in & 2u) ? p01 : border, p10 = (in & 4u) ? p10 : border, p11 = (in & 8u) ? p11 : border;
        }
        return blend_u8_packed<3>(p00, p01, p10, p11, t.fx(), t.fy());
    }
}

// a lane's 4 pixels of one frame
template <int INTERP, int MODE, int RGB, bool WINDOW>
__device__ __forceinline__ void frame_pixels_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, const NvTaps (&tap)[kBorderPPL],
                                                  const bool (&wr)[kBorderPPL], uint32_t border, uint32_t (&p)[kBorderPPL]) {
#pragma unroll
    for (int j = 0; j < kBorderPPL; j++) {
        if constexpr (MODE == kBorderTransparent) {
            if (wr[j]) p[j] = sample_entry_nv12<INTERP, MODE, RGB, WINDOW>(yf, uvf, tap[j], border);
        } else {
            p[j] = sample_entry_nv12<INTERP, MODE, RGB, WINDOW>(yf, uvf, tap[j], border);
        }
    }
}

// The kernels' common body; store(b, y, xs, p, wr) writes a lane's 4 pixels of frame b.
template <int INTERP, int MODE, int RGB, class Store>
__device__ __forceinline__ void remap_nv12_body(const RemapNv12Args& a, Store store) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = MODE == kBorderTransparent;
    constexpr bool kWindows = INTERP == kLinear && BEVWARP_REMAP_NV12_WINDOWS != 0;
    uint32_t g;
    int y, xs;  // group of frames, row, the lane's first pixel
    if (!lane_position(a, g, y, xs)) return;
    const int b0 = (int)g * a.frames_per_item;
    const int nb = min(a.frames_per_item, a.batch - b0);

    uint32_t e[PPL], fr[PPL];
    load_entries<INTERP>(a, b0, y, xs, e, fr);

    NvTaps tap[PPL];
    bool wr[PPL];
    // the windows: a row of pairs holds at least two of them (src_w >= 4), and every (loaded) pixel of the lane has its two columns side
    // by side
    bool window = kWindows && a.src_w >= 4;
    const int last_start = (a.src_w >> 1) - 2;  // the last pair a 4-byte window may start at
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        NvTaps& t = tap[j];
#include "map_entry_taps.inc"
        // a tap at pixel (c, r) reads Y[r][c] and the pair (r >> 1, c >> 1)
        const uint32_t yo0 = (uint32_t)cy0 * (uint32_t)a.y_rs, yo1 = (uint32_t)cy1 * (uint32_t)a.y_rs;
        const uint32_t uo0 = (uint32_t)(cy0 >> 1) * (uint32_t)a.uv_rs, uo1 = (uint32_t)(cy1 >> 1) * (uint32_t)a.uv_rs;
        const int p0 = c0 >> 1, p1 = c1 >> 1;
        t.y00 = yo0 + (uint32_t)c0, t.y01 = yo0 + (uint32_t)c1, t.y10 = yo1 + (uint32_t)c0, t.y11 = yo1 + (uint32_t)c1;
        t.u00 = uo0 + 2u * (uint32_t)p0, t.u01 = uo0 + 2u * (uint32_t)p1, t.u10 = uo1 + 2u * (uint32_t)p0, t.u11 = uo1 + 2u * (uint32_t)p1;
        // with adjacent columns the window starting at pair min(p0, last_start) holds both taps' pairs: p1 is p0 or p0 + 1, and p0 is
        // past last_start only for c0 = src_w - 2, whose two taps share the row's last pair
        const int ps = min(p0, last_start);
        t.w = f | (in << 10) | ((uint32_t)((p0 - ps) & 1) << 14) | ((uint32_t)((p1 - ps) & 1) << 15);
        if constexpr (kWindows) window = window && ((kTransparent && !wr[j]) || c1 == c0 + 1);
    }
    if constexpr (kWindows) {
        if (window) {
#pragma unroll
            for (int j = 0; j < PPL; j++) {
                const uint32_t back = (tap[j].w >> 13) & 2u;  // 2 bytes where the window starts one pair before c0's
                tap[j].u00 -= back, tap[j].u10 -= back;
            }
        }
    }

    const uint32_t border = a.bv_u8;
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* yf = a.y + (int64_t)b * a.y_fs;
        const uint8_t* uvf = a.uv + (int64_t)b * a.uv_fs;
        uint32_t p[PPL];
        if constexpr (kWindows) {
            if (window)
                frame_pixels_nv12<INTERP, MODE, RGB, true>(yf, uvf, tap, wr, border, p);
            else
                frame_pixels_nv12<INTERP, MODE, RGB, false>(yf, uvf, tap, wr, border, p);
        } else {
            frame_pixels_nv12<INTERP, MODE, RGB, false>(yf, uvf, tap, wr, border, p);
        }
        store(b, y, xs, p, wr);
    }
}

// 8-bit pixels of 3 channels, B, G, R or R, G, B
template <int INTERP, int MODE, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_nv12_kernel(const RemapNv12Args a) {
    remap_nv12_body<INTERP, MODE, RGB>(a, [&](uint32_t b, int y, int xs, const uint32_t (&p)[kBorderPPL], const bool (&wr)[kBorderPPL]) __attribute__((always_inline)) {
        Pixel<uint8_t, 3> px[kBorderPPL];
#pragma unroll
        for (int j = 0; j < kBorderPPL; j++) px[j].packed = p[j];
        store_lane_pixels<uint8_t, 3, MODE == kBorderTransparent>(a, b, y, xs, px, wr);
    });
}

// channel planes: the kernel samples B, G, R (the host's table points each sampled channel at its plane); every pixel is written
template <int INTERP, int MODE, bool WIDE16>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_nv12_planes_kernel(const RemapNv12PlanesArgs a) {
    static_assert(MODE != kBorderTransparent, "the plane stage writes every pixel");
    remap_nv12_body<INTERP, MODE, 0>(a, [&](uint32_t b, int y, int xs, const uint32_t (&p)[kBorderPPL], const bool (&)[kBorderPPL]) __attribute__((always_inline)) {
        constexpr int PPL = kBorderPPL;
#include "plane_store.inc"
    });
}

template <int INTERP, int MODE>
void launch_order(const RemapNv12Args& a, int rgb_order, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (rgb_order)
        hipLaunchKernelGGL((remap_nv12_kernel<INTERP, MODE, 1>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((remap_nv12_kernel<INTERP, MODE, 0>), grid, block, 0, stream, a);
}

template <int INTERP>
void launch_mode(const RemapNv12Args& a, int mode, int rgb_order, dim3 grid, hipStream_t stream) {
    switch (mode) {
        case 0: launch_order<INTERP, 0>(a, rgb_order, grid, stream); break;
        case kBorderReplicate: launch_order<INTERP, kBorderReplicate>(a, rgb_order, grid, stream); break;
        case kBorderReflect: launch_order<INTERP, kBorderReflect>(a, rgb_order, grid, stream); break;
        case kBorderWrap: launch_order<INTERP, kBorderWrap>(a, rgb_order, grid, stream); break;
        case kBorderReflect101: launch_order<INTERP, kBorderReflect101>(a, rgb_order, grid, stream); break;
        default: launch_order<INTERP, kBorderTransparent>(a, rgb_order, grid, stream); break;
    }
}

template <int INTERP, int MODE>
void launch_format(const RemapNv12PlanesArgs& a, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (a.plane == kPlaneF32)
        hipLaunchKernelGGL((remap_nv12_planes_kernel<INTERP, MODE, false>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((remap_nv12_planes_kernel<INTERP, MODE, true>), grid, block, 0, stream, a);
}

template <int INTERP>
void launch_planes_mode(const RemapNv12PlanesArgs& a, int mode, dim3 grid, hipStream_t stream) {
    switch (mode) {
        case 0: launch_format<INTERP, 0>(a, grid, stream); break;
        case kBorderReplicate: launch_format<INTERP, kBorderReplicate>(a, grid, stream); break;
        case kBorderReflect: launch_format<INTERP, kBorderReflect>(a, grid, stream); break;
        case kBorderWrap: launch_format<INTERP, kBorderWrap>(a, grid, stream); break;
        default: launch_format<INTERP, kBorderReflect101>(a, grid, stream); break;
    }
}

}  // namespace

hipError_t launch_remap_nv12(const RemapNv12Args& a, int interp, int mode, int rgb_order, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    (interp == kNearest ? launch_mode<kNearest> : launch_mode<kLinear>)(a, mode, rgb_order, grid, stream);
    return hipGetLastError();
}

hipError_t launch_remap_nv12_planes(const RemapNv12PlanesArgs& a, int interp, int mode, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    (interp == kNearest ? launch_planes_mode<kNearest> : launch_planes_mode<kLinear>)(a, mode, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
