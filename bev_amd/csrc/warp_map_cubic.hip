// warp_map_cubic.hip -- bicubic sampling through a bilinear warp map (bevwarp_remap | BEVWARP_MAP_BICUBIC): 8-bit and
// float32 pixels, 1-4 channels, all six border modes.  OpenCV's bicubic is defined on the bilinear map: an entry (sx, sy, fx, fy) is the
// window's first tap (sx - 1, sy - 1) and the table index (fy, fx), so from the entry on a pixel is the matrix kernel's (warp_cubic.hip) with
// no float64 at all -- the sampler is cubic_sample.h's, the one both units include.
//
// The frame is remap_kernel's (warp_map.hip): flat_frame.h's flat grid, a lane owns 4 consecutive pixels of one destination row, its 4 map
// entries loaded once (map_entry.h), an item walks frames_per_item frames.  What an entry gives -- inlier, written, the window's byte
// offset in a frame, the table index -- is computed once and kept in registers across the frames; the 16 weights are loaded per frame
// from the table (32 KB, cache-resident): 4 pixels' weights held across the loop are 32 registers the float32 4-channel instances do
// not have.  A pixel that is no inlier remaps its eight indices per frame: it is the rare path, at the frame's edge.
#include "cubic_sample.h"
#include "map_entry.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// What a lane keeps of one map entry for every frame it walks
struct CubicEntry {
    uint32_t e;    // the entry as the map holds it: (sx, sy), for the pixels that are no inliers
    uint32_t off;  // inliers: the byte offset of the window's first tap in a frame (a frame is below 2 GiB)
    uint32_t w;    // fx | fy << 5 (the table index) | inlier << 10
    __device__ __forceinline__ int wx() const { return (int)(short)(e & 0xffffu) - 1; }
    __device__ __forceinline__ int wy() const { return ((int)e >> 16) - 1; }
    __device__ __forceinline__ int fx() const { return (int)(w & 31u); }
    __device__ __forceinline__ int fy() const { return (int)((w >> 5) & 31u); }
    __device__ __forceinline__ bool inlier() const { return (w >> 10) != 0u; }
};

// the byte offset of an inlier's first tap in a frame (a frame is below 2 GiB: 32 bits hold it)
template <typename T, int C>
__device__ __forceinline__ uint32_t window_offset(const RemapArgs& a, int wx, int wy) {
    return (uint32_t)wy * (uint32_t)a.src_rs + (uint32_t)wx * (uint32_t)(C * sizeof(T));
}

// store_lane_pixels<float, 4> (flat_frame.h) one pixel at a time: pixel x of row y of frame b -- its 16-byte store where the layout admits
// the wide stores and the lane writes all its pixels (`all`), else its four values if it is written
__device__ __forceinline__ void store_pixel_f32x4(const FrameArgs& a, uint32_t b, int y, int x, const Pixel<float, 4>& p, bool written, bool all) {
    float* d = reinterpret_cast<float*>(dst_row(a, b, y)) + (int64_t)x * 4;
    if (a.dst_vec_ok && all) {
        f32x4 o = {p.v[0], p.v[1], p.v[2], p.v[3]};
        wide_store(reinterpret_cast<f32x4*>(d), o);
    } else if (written) {
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = p.v[k];
    }
}

template <typename T, int C, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_cubic_kernel(const RemapArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = MODE == BEVWARP_BORDER_TRANSPARENT;
    constexpr int kRemap = kTransparent ? BEVWARP_BORDER_REFLECT_101 : MODE;
    // float32 pixels of 4 channels have no registers for the lane's finished pixels beside the next one's taps (the general path's 16 taps
    // are 64 of the 128): such a pixel is one 16-byte store of store_lane_pixels' own, which it gets as soon as it is computed ...
    constexpr bool kStorePerPixel = sizeof(T) == 4 && C == 4;
    // ... nor for the 4 offsets (REPLICATE spills 4 registers with them): two multiplies and an add per inlier and frame instead
    constexpr bool kKeepOffset = !(sizeof(T) == 4 && C == 4);
    uint32_t g;
    int y, xs;  // group of frames, row, the lane's first pixel
    if (!lane_position(a, g, y, xs)) return;
    const int b0 = (int)g * a.frames_per_item;
    const int nb = min(a.frames_per_item, a.batch - b0);

    uint32_t e[PPL], fr[PPL];
    load_entries<kLinear>(a, b0, y, xs, e, fr);

    // all 16 taps inside: 0 <= wx < max(w - 3, 0) and 0 <= wy < max(h - 3, 0)
    const unsigned in_w = (unsigned)max(a.src_w - 3, 0), in_h = (unsigned)max(a.src_h - 3, 0);
    CubicEntry ent[PPL];
    bool wr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        CubicEntry& t = ent[j];
        t.e = e[j];
        // the window starts one pixel before the entry's position (int32: -32768 - 1 does not wrap)
        const int wx = t.wx(), wy = t.wy();
        const bool inl = (unsigned)wx < in_w && (unsigned)wy < in_h;
        // TRANSPARENT writes the pixels whose integer position (sx, sy) lies in the source (inliers are among them)
        wr[j] = xs + j < a.dst_w && (!kTransparent || inl || ((unsigned)(wx + 1) < (unsigned)a.src_w && (unsigned)(wy + 1) < (unsigned)a.src_h));
        t.w = (fr[j] & 1023u) | ((uint32_t)inl << 10);  // (higher bits of frac are ignored)
        t.off = (kKeepOffset && inl) ? window_offset<T, C>(a, wx, wy) : 0u;
    }

    const bool all = wr[0] && wr[1] && wr[2] && wr[3];  // (the lane writes its 4 pixels: store_lane_pixels' condition for the wide stores)
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
        Pixel<T, C> px[PPL];
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if constexpr (sizeof(T) == 1) {
                px[j].packed = 0;
            } else {
#pragma unroll
                for (int k = 0; k < C; k++) px[j].v[k] = 0.f;
            }
            if (!wr[j]) continue;  // neither read nor written
            // What the sampler derives from the entry -- a table entry's 8 registers, the general path's 8 indices -- is frame-invariant
            // as well, and the compiler would hoist all of it for all 4 pixels out of the frame loop and spill: the entry is handed to
            // each frame's pass as a value it cannot see through (no instruction is emitted).
            CubicEntry t = ent[j];
            asm volatile("" : "+v"(t.e), "+v"(t.w));
            const Weights<T> W = load_weights<T>(t.fy(), t.fx());
            if (t.inlier())
                px[j] = sample_cubic_inlier<T, C>(frame + (kKeepOffset ? t.off : window_offset<T, C>(a, t.wx(), t.wy())), a.src_rs, W);
            else
                px[j] = sample_cubic_general<T, C, kRemap>(a, frame, t.wx(), t.wy(), W);
            if constexpr (kStorePerPixel) store_pixel_f32x4(a, b, y, xs + j, px[j], wr[j], all);
        }
        if constexpr (!kStorePerPixel) store_lane_pixels<T, C, kTransparent>(a, b, y, xs, px, wr);
    }
}

}  // namespace

hipError_t launch_remap_cubic(const RemapArgs& a, int dtype, int channels, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<BEVWARP_BORDER_CONSTANT, BEVWARP_BORDER_REPLICATE, BEVWARP_BORDER_REFLECT, BEVWARP_BORDER_WRAP, BEVWARP_BORDER_REFLECT_101,
                        BEVWARP_BORDER_TRANSPARENT>(mode, [&](auto m) {
                pick::channels(channels, [&](auto c) { launch(remap_cubic_kernel<typename decltype(t)::type, c(), m()>); });
            });
        });
    });
}

}  // namespace bevwarp
