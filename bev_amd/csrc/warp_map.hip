// warp_map.hip -- the warp of a fixed camera in two steps (bevwarp_build_map, bevwarp_remap).  The builder runs the
// exact float64 coordinate chain -- the border kernel's, or with a lens the lens kernel's, operation for operation -- once per camera and
// geometry and stores what it gives in OpenCV's fixed-point map format: int16 pairs (sx, sy) and, for bilinear, uint16 (fy << 5) | fx.
// The remap kernel samples frames through such maps: from (sx, sy, fx, fy) on it is the lens kernel's guarded sampler (BORDER_CONSTANT)
// and the border kernel's body (the other five modes), with no float64 at all.  A lane's 4 map entries are frame-invariant under a shared
// map: a workgroup loads its tile's entries once, derives tap offsets and the inside masks, and walks frames_per_item frames with them in
// registers.
//
// The frame -- item decoding, the row walk, the rounding, a pixel's load and the store of a lane's 4 pixels -- is flat_frame.h; the lens
// step and the blend are lens_pixel.h; the builder's body is map_build.inc, shared with the fisheye builder
// (warp_map_fisheye.hip); the index remap is warp_border.h; the sampler's map loads and index stage are map_entry.h, shared with the NV12
// sampler (warp_map_nv12.hip); a tap's load by byte offset and the 6-byte pair load are tap_load.h, shared with the stitches through maps.
#include "warp_map.h"
#include "lens_pixel.h"
#include "map_entry.h"
#include "tap_load.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// ---- the builder ---------------------------------------------------------------------------------------------------------------------------
#define BEVWARP_MAP_STEP                                   \
    bool valid = true;                                     \
    if constexpr (LENS)                                    \
        valid = lens_pixel<INTERP>(a, Xn, Yn, W, X, Y);    \
    else                                                   \
        map_pixel_exact_nan_max<INTERP>(Xn, Yn, W, X, Y);
template <int INTERP, bool LENS>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void build_map_kernel(const MapBuildArgs a) {
#include "map_build.inc"
}
#undef BEVWARP_MAP_STEP

// ---- the sampler ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int C>
__device__ __forceinline__ Pixel<T, C> border_pixel(const RemapArgs& a) {
    Pixel<T, C> p;
    if constexpr (sizeof(T) == 1) {
        p.packed = a.bv_u8;
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) p.v[k] = a.bv_f[k];
    }
    return p;
}

// What a lane keeps of one map entry for every frame it walks: the byte offsets of its four taps in a frame (all four are source pixels:
// remapped, an inlier's, or clamped; a frame is below 2 GiB, so 32 bits hold them and a load is the frame's wave-uniform base plus one
// register), the weights, and for the constant border which of the four taps lie inside.
struct Taps {
    uint32_t a00, a01, a10, a11;
    uint32_t w;  // fx | fy << 5 | in << 10; in: bit 0 = tap (row 0, col 0), 1 = (0, 1), 2 = (1, 0), 3 = (1, 1)
    __device__ __forceinline__ int fx() const { return (int)(w & 31u); }
    __device__ __forceinline__ int fy() const { return (int)((w >> 5) & 31u); }
    __device__ __forceinline__ uint32_t in() const { return w >> 10; }
};

// the four taps of an entry; PAIR: both rows' taps are adjacent columns of 8-bit 3-channel pixels
template <typename T, int C, bool PAIR>
__device__ __forceinline__ void load_taps(const uint8_t* __restrict__ frame, const Taps& t, bool vec, Pixel<T, C>& p00, Pixel<T, C>& p01, Pixel<T, C>& p10, Pixel<T, C>& p11) {
    if constexpr (PAIR) {
        load_pair_u8x3(frame, t.a00, p00, p01);
        load_pair_u8x3(frame, t.a10, p10, p11);
    } else {
        p00 = load_at<T, C>(frame, t.a00, vec), p01 = load_at<T, C>(frame, t.a01, vec);
        p10 = load_at<T, C>(frame, t.a10, vec), p11 = load_at<T, C>(frame, t.a11, vec);
    }
}

template <typename T, int C, int INTERP, int MODE, bool PAIR>
__device__ __forceinline__ Pixel<T, C> sample_entry(const RemapArgs& a, const uint8_t* __restrict__ frame, const Taps& t, bool vec) {
    if constexpr (MODE != 0) {  // every tap is a source pixel
        if (INTERP == kNearest) return load_at<T, C>(frame, t.a00, vec);
        Pixel<T, C> p00, p01, p10, p11;
        load_taps<T, C, PAIR>(frame, t, vec, p00, p01, p10, p11);
        return blend_taps<T, C>(p00, p01, p10, p11, t.fx(), t.fy());
    } else {
        // The constant border: every tap is loaded from the CLAMPED position (unconditional loads, all issued before the first wait) and
        // replaced by the border pixel where its true position is outside; all four outside: the border value itself.
        const Pixel<T, C> b = border_pixel<T, C>(a);
        if (INTERP == kNearest) {
            const Pixel<T, C> p = load_at<T, C>(frame, t.a00, vec);
            return (t.in() & 1u) ? p : b;
        }
        Pixel<T, C> t00, t01, t10, t11;
        load_taps<T, C, PAIR>(frame, t, vec, t00, t01, t10, t11);
        const Pixel<T, C> out = blend_taps<T, C>((t.in() & 1u) ? t00 : b, (t.in() & 2u) ? t01 : b, (t.in() & 4u) ? t10 : b, (t.in() & 8u) ? t11 : b, t.fx(), t.fy());
        // (8-bit pixels: the blend of four border pixels is the border pixel)
        return (sizeof(T) == 4 && t.in() == 0u) ? b : out;
    }
}

// a lane's 4 pixels of one frame
template <typename T, int C, int INTERP, int MODE, bool PAIR>
__device__ __forceinline__ void frame_pixels(const RemapArgs& a, const uint8_t* __restrict__ frame, const Taps (&tap)[kBorderPPL], const bool (&wr)[kBorderPPL], bool vec,
                                             Pixel<T, C> (&px)[kBorderPPL]) {
#pragma unroll
    for (int j = 0; j < kBorderPPL; j++) {
        if constexpr (MODE == kBorderTransparent) {
            if (wr[j]) px[j] = sample_entry<T, C, INTERP, MODE, PAIR>(a, frame, tap[j], vec);
        } else {
            px[j] = sample_entry<T, C, INTERP, MODE, PAIR>(a, frame, tap[j], vec);
        }
        // float32 pixels of 3 / 4 channels, bilinear: the taps of two pixels are 24 / 32 registers -- the loads of the lane's second pair
        // wait for the first pair's blends, or the kernel passes the 128 registers its occupancy is planned for
        if (sizeof(T) == 4 && C >= 3 && INTERP == kLinear && j == 1) __builtin_amdgcn_sched_barrier(0);
    }
}

template <typename T, int C, int INTERP, int MODE>
__global__ __launch_bounds__(kWG) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd, 8))) void remap_kernel(const RemapArgs a) {
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = MODE == kBorderTransparent;
    uint32_t g;
    int y, xs;  // group of frames, row, the lane's first pixel
    if (!lane_position(a, g, y, xs)) return;
    const int b0 = (int)g * a.frames_per_item;
    const int nb = min(a.frames_per_item, a.batch - b0);

    // the lane's map entries (map_entry.h) and, per entry, the taps' indices under the border mode (map_entry_taps.inc)
    uint32_t e[PPL], fr[PPL];
    load_entries<INTERP>(a, b0, y, xs, e, fr);

    Taps tap[PPL];
    bool wr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        Taps& t = tap[j];
#include "map_entry_taps.inc"
        t.w = f | (in << 10);
        const uint32_t o0 = (uint32_t)cy0 * (uint32_t)a.src_rs, o1 = (uint32_t)cy1 * (uint32_t)a.src_rs;
        const uint32_t x0 = (uint32_t)c0 * (uint32_t)(C * sizeof(T)), x1 = (uint32_t)c1 * (uint32_t)(C * sizeof(T));
        t.a00 = o0 + x0, t.a01 = o0 + x1, t.a10 = o1 + x0, t.a11 = o1 + x1;
    }

    // 8-bit 3-channel bilinear: a lane whose (loaded) pixels all have their two columns side by side -- every inlier, every interior pixel --
    // takes the pair loads; a lane with a pixel at a clamped or remapped edge takes the loads tap by tap
    bool pair = sizeof(T) == 1 && C == 3 && INTERP == kLinear;
    if constexpr (sizeof(T) == 1 && C == 3 && INTERP == kLinear) {
#pragma unroll
        for (int j = 0; j < PPL; j++) pair = pair && ((kTransparent && !wr[j]) || tap[j].a01 == tap[j].a00 + 3u);
    }

    const bool vec = a.src_vec_ok;
#pragma unroll 1
    for (int f = 0; f < nb; f++) {
        const uint32_t b = (uint32_t)(b0 + f);
        const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
        Pixel<T, C> px[PPL];
        if constexpr (sizeof(T) == 1 && C == 3 && INTERP == kLinear) {
            if (pair)
                frame_pixels<T, C, INTERP, MODE, true>(a, frame, tap, wr, vec, px);
            else
                frame_pixels<T, C, INTERP, MODE, false>(a, frame, tap, wr, vec, px);
        } else {
            frame_pixels<T, C, INTERP, MODE, false>(a, frame, tap, wr, vec, px);
        }
        store_lane_pixels<T, C, kTransparent>(a, b, y, xs, px, wr);
    }
}

}  // namespace

hipError_t launch_build_map(const MapBuildArgs& a, int interp, bool lens, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::value<kNearest, kLinear>(interp, [&](auto i) { pick::flag(lens, [&](auto l) { launch(build_map_kernel<i(), l()>); }); });
    });
}

hipError_t launch_remap(const RemapArgs& a, int dtype, int channels, int interp, int mode, int64_t items, hipStream_t stream) {
    return launch_items(a, items, kWG, stream, [&](auto launch) {
        pick::pixel(dtype, [&](auto t) {
            pick::value<kNearest, kLinear>(interp, [&](auto i) {
                pick::value<0, kBorderReplicate, kBorderReflect, kBorderWrap, kBorderReflect101, kBorderTransparent>(mode, [&](auto m) {
                    pick::channels(channels, [&](auto c) { launch(remap_kernel<typename decltype(t)::type, c(), i(), m()>); });
                });
            });
        });
    });
}

}  // namespace bevwarp
