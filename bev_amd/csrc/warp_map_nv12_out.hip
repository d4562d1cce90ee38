// warp_map_nv12_out.hip -- frames sampled through a fixed camera's warp map and written as NV12 for a video encoder (bevwarp_remap_to_nv12,
// bevwarp_remap_nv12_to_nv12): BGR -> NV12 of bevwarp_remap's (bevwarp_remap_nv12's) 8-bit pixel, bit for bit, with
// the sampled BGR frame never in memory.  The map carries the lens, so there is no float64 here.  The structure is remap_kernel's
// (warp_map.hip) and remap_nv12_body's (warp_map_nv12.hip): a workgroup loads its tile's map entries once, derives what does not depend on
// the frame -- the taps' byte offsets, the weights, the inside mask (BORDER_CONSTANT) -- and walks frames_per_item frames with that in
// registers.  The five border modes that write every pixel; BORDER_TRANSPARENT has no instance.
//
// The frame is flat_frame.h; the map loads (map_entry.h) and the index stage (map_entry_taps.inc) are shared with those two units; the
// conversion of NV12 taps and the blend are nv12_sample.h and sample.h; the store is nv12_store.h, shared with
// warp_stitch_maps_nv12_out.hip.  The samplers' helpers -- the 6-byte pair loads of BGR sources, the 2-byte Y and 4-byte pair windows of NV12
// sources, convert_packed -- are restated from those units rather than moved into a header: their machine code stays what it was.
#include "warp_map_nv12_out.h"
#include "map_entry.h"
#include "nv12_sample.h"
#include "warp_kernels.h"

namespace bevwarp {
namespace {

// ---- 8-bit BGR / RGB frames (warp_map.hip's sampler for uint8_t, 3 channels) ------------------------------------------------------------------
// What a lane keeps of one map entry for every frame it walks: the byte offsets of its four taps in a frame (source pixels: remapped or
// clamped; a frame is below 2 GiB), the weights, and for the constant border which of the four taps lie inside.
struct Taps {
    uint32_t a00, a01, a10, a11;
    uint32_t w;  // fx | fy << 5 | in << 10; in: map_entry_taps.inc's
    __device__ __forceinline__ uint32_t fx() const { return w & 31u; }
    __device__ __forceinline__ uint32_t fy() const { return (w >> 5) & 31u; }
    __device__ __forceinline__ uint32_t in() const { return w >> 10; }
};

// one source pixel at a byte offset of the frame: exactly its 3 bytes are read
__device__ __forceinline__ uint32_t load_at(const uint8_t* __restrict__ frame, uint32_t off) {
    const uint8_t* q = frame + off;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

// the two adjacent taps of a row: 6 contiguous bytes, never a byte beyond them (warp_map.hip's load_pair_u8x3)
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ frame, uint32_t off, uint32_t& p0, uint32_t& p1) {
    uint32_t lo;
    uint16_t hi;
    __builtin_memcpy(&lo, frame + off, 4);
    __builtin_memcpy(&hi, frame + off + 4, 2);
    p0 = lo & 0xffffffu;
    p1 = __builtin_amdgcn_alignbit((uint32_t)hi, lo, 24);  // bytes 3, 4, 5
}

// One destination pixel of one frame, packed in the source's channel order.  PAIR: both rows' taps are adjacent columns.
template <int INTERP, int MODE, bool PAIR>
__device__ __forceinline__ uint32_t sample_entry(const uint8_t* __restrict__ frame, const Taps& t, uint32_t border) {
    if constexpr (INTERP == kNearest) {
        const uint32_t p = load_at(frame, t.a00);
        return (MODE != 0 || (t.in() & 1u)) ? p : border;
    } else {
        // every load is of a source pixel (the constant border: of the CLAMPED position) and issues before the first wait
        uint32_t p00, p01, p10, p11;
        if constexpr (PAIR) {
            load_pair(frame, t.a00, p00, p01);
            load_pair(frame, t.a10, p10, p11);
        } else {
            p00 = load_at(frame, t.a00), p01 = load_at(frame, t.a01), p10 = load_at(frame, t.a10), p11 = load_at(frame, t.a11);
        }
        if constexpr (MODE == 0) {  // a tap outside is the border pixel (all four outside: the blend of four border pixels is the border pixel)
            const uint32_t in = t.in();
            p00 = (in & 1u) ? p00 : border, p01 = (in & 2u) ? p01 : border, p10 = (in & 4u) ? p10 : border, p11 = (in & 8u) ? p11 : border;
        }
        return blend_u8_packed<3>(p00, p01, p10, p11, t.fx(), t.fy());
    }
}

template <int INTERP, int MODE, int RGB>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_to_nv12_kernel(const RemapNv12OutArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = false;
    static_assert(MODE != kBorderTransparent, "the NV12 store writes every pixel");
    uint32_t g;
    int y, xs;  // group of frames, row, the lane's first pixel
    if (!lane_position(a, g, y, xs)) return;
    const int b0 = (int)g * a.frames_per_item;
    const int nb = min(a.frames_per_item, a.batch - b0);

    uint32_t e[PPL], fr[PPL];
    load_entries<INTERP>(a, b0, y, xs, e, fr);

    Taps tap[PPL];
    bool wr[PPL];
    // a lane whose pixels all have their two columns side by side -- every inlier, every interior pixel -- takes the pair loads; a lane with
    // a pixel at a clamped or remapped edge takes the loads tap by tap
    bool pair = INTERP == kLinear;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        Taps& t = tap[j];
#include "map_entry_taps.inc"
        t.w = f | (in << 10);
        const uint32_t o0 = (uint32_t)cy0 * (uint32_t)a.src_rs, o1 = (uint32_t)cy1 * (uint32_t)a.src_rs;
        const uint32_t x0 = (uint32_t)c0 * 3u, x1 = (uint32_t)c1 * 3u;
        t.a00 = o0 + x0, t.a01 = o0 + x1, t.a10 = o1 + x0, t.a11 = o1 + x1;
        pair = pair && c1 == c0 + 1;
    }
    (void)wr;  // (every pixel of the row is written: the row's end is the store's to judge)

    const uint32_t border = a.bv_u8;
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
        uint32_t p[PPL];
        if constexpr (INTERP == kLinear) {
            if (pair) {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, true>(frame, tap[j], border);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, false>(frame, tap[j], border);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, false>(frame, tap[j], border);
        }
        store_lane_nv12<RGB>(a, a, b, y, xs, p);
    }
}

// ---- NV12 frames (warp_map_nv12.hip's sampler, B, G, R) -----------------------------------------------------------------------------------
// All offsets are of source pixels (remapped or clamped); a plane is below 2 GiB.
struct NvTaps {
    uint32_t y00, y01, y10, y11;  // bytes into the Y plane; a window lane loads 2 bytes at y00 and at y10
    uint32_t u00, u01, u10, u11;  // bytes into the plane of pairs (even); a window lane loads 4 bytes at u00 and at u10 (the windows' starts)
    uint32_t w;  // fx | fy << 5 | in << 10 | s0 << 14 | s1 << 15; s0, s1: window lanes, which pair of the window column c0 / c1 takes
    __device__ __forceinline__ uint32_t fx() const { return w & 31u; }
    __device__ __forceinline__ uint32_t fy() const { return (w >> 5) & 31u; }
    __device__ __forceinline__ uint32_t in() const { return (w >> 10) & 15u; }
};

// a (U, V) pair at an even byte offset of a plane whose base and strides are even
__device__ __forceinline__ uint32_t pair_at(const uint8_t* __restrict__ uvf, uint32_t off) { return *reinterpret_cast<const uint16_t*>(uvf + off); }

// convert<0> (nv12_sample.h) with the middle channel behind a value barrier: warp_map_nv12.hip's convert_packed, which records why -- fused
// into v_ashr_pk_u8_i32, two channels' shift and clamp gave wrong pixels on the MI355X in one instance of that unit.  The barrier costs no
// instruction.
__device__ __forceinline__ uint32_t convert_packed(uint32_t Y, const Chroma& c) {
    uint32_t r, g, b;
    convert_channels(Y, c, r, g, b);
    asm("" : "+v"(g));
    return b | (g << 8) | (r << 16);
}

// One destination pixel of one frame as B, G, R.  WINDOW: the lane's pixels all have adjacent columns.
template <int INTERP, int MODE, bool WINDOW>
__device__ __forceinline__ uint32_t sample_entry_nv12(const uint8_t* __restrict__ yf, const uint8_t* __restrict__ uvf, const NvTaps& t, uint32_t border) {
    if constexpr (INTERP == kNearest) {
        const uint32_t p = convert_packed(yf[t.y00], chroma_terms(pair_at(uvf, t.u00)));
        return (MODE != 0 || (t.in() & 1u)) ? p : border;
    } else {
        uint32_t Y00, Y01, Y10, Y11, q00, q01, q10, q11;
        if constexpr (WINDOW) {
            uint16_t w0, w1;
            uint32_t v0, v1;
            __builtin_memcpy(&w0, yf + t.y00, 2);  // (unaligned)
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
        uint32_t p00 = convert_packed(Y00, chroma_terms(q00)), p01 = convert_packed(Y01, chroma_terms(q01));
        uint32_t p10 = convert_packed(Y10, chroma_terms(q10)), p11 = convert_packed(Y11, chroma_terms(q11));
        if constexpr (MODE == 0) {  // a tap outside is the border pixel, B, G, R, not converted on the way in
            const uint32_t in = t.in();
            p00 = (in & 1u) ? p00 : border, p01 = (in & 2u) ? p01 : border, p10 = (in & 4u) ? p10 : border, p11 = (in & 8u) ? p11 : border;
        }
        return blend_u8_packed<3>(p00, p01, p10, p11, t.fx(), t.fy());
    }
}

template <int INTERP, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_nv12_to_nv12_kernel(const RemapNv12OutArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = false;
    static_assert(MODE != kBorderTransparent, "the NV12 store writes every pixel");
    uint32_t g;
    int y, xs;  // group of frames, row, the lane's first pixel
    if (!lane_position(a, g, y, xs)) return;
    const int b0 = (int)g * a.frames_per_item;
    const int nb = min(a.frames_per_item, a.batch - b0);

    uint32_t e[PPL], fr[PPL];
    load_entries<INTERP>(a, b0, y, xs, e, fr);

    NvTaps tap[PPL];
    bool wr[PPL];
    // the windows: a row of pairs holds at least two of them (src_w >= 4), and every pixel of the lane has its two columns side by side
    bool window = INTERP == kLinear && a.src_w >= 4;
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
        window = window && c1 == c0 + 1;
    }
    (void)wr;
    if constexpr (INTERP == kLinear) {
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
        if constexpr (INTERP == kLinear) {
            if (window) {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry_nv12<INTERP, MODE, true>(yf, uvf, tap[j], border);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry_nv12<INTERP, MODE, false>(yf, uvf, tap[j], border);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) p[j] = sample_entry_nv12<INTERP, MODE, false>(yf, uvf, tap[j], border);
        }
        store_lane_nv12<0>(a, a, b, y, xs, p);
    }
}

// source: 0 = B, G, R frames, 1 = R, G, B frames, 2 = NV12 frames
template <int INTERP, int MODE>
void launch_source(const RemapNv12OutArgs& a, int source, dim3 grid, hipStream_t stream) {
    const dim3 block(kWG);
    if (source == 2)
        hipLaunchKernelGGL((remap_nv12_to_nv12_kernel<INTERP, MODE>), grid, block, 0, stream, a);
    else if (source == 1)
        hipLaunchKernelGGL((remap_to_nv12_kernel<INTERP, MODE, 1>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((remap_to_nv12_kernel<INTERP, MODE, 0>), grid, block, 0, stream, a);
}

template <int INTERP>
void launch_mode(const RemapNv12OutArgs& a, int mode, int source, dim3 grid, hipStream_t stream) {
    switch (mode) {
        case 0: launch_source<INTERP, 0>(a, source, grid, stream); break;
        case kBorderReplicate: launch_source<INTERP, kBorderReplicate>(a, source, grid, stream); break;
        case kBorderReflect: launch_source<INTERP, kBorderReflect>(a, source, grid, stream); break;
        case kBorderWrap: launch_source<INTERP, kBorderWrap>(a, source, grid, stream); break;
        default: launch_source<INTERP, kBorderReflect101>(a, source, grid, stream); break;
    }
}

}  // namespace

hipError_t launch_remap_nv12_out(const RemapNv12OutArgs& a, int nv12_src, int interp, int mode, int rgb_order, int64_t items, hipStream_t stream) {
    (void)hipGetLastError();  // a stale error left by the host framework is not this call's
    const dim3 grid((unsigned)items);
    const int source = nv12_src ? 2 : (rgb_order ? 1 : 0);
    (interp == kNearest ? launch_mode<kNearest> : launch_mode<kLinear>)(a, mode, source, grid, stream);
    return hipGetLastError();
}

}  // namespace bevwarp
