// warp_rows.h -- batched BEV homography warp for MI355X (gfx950, wave64).  See DESIGN.md section 4.
//
// Replaces the per-frame cv2.warpPerspective call of the reference (vis_homo.py:89,91; bev/tool/compo.py:38,46,47).
//
// ONE kernel, warp_rows.  A workgroup of 4 waves owns a tile of TW x tile_h destination pixels (TW = 256 for 8-bit,
// 128 for float pixels); a wave owns whole TW-pixel row segments (rows dealt round-robin to the 4 waves) and pixel j of
// lane l is x0 + 64 j + l, so every load instruction covers 64 consecutive destination pixels.  Each row segment is
// classified from its two end pixels, in scalar registers:
//     FAST  both ends sample inside the frame by a margin, W keeps its sign  -> every pixel does: unguarded tap loads
//           (aligned 12-byte windows + funnel shift for 8-bit RGB), no per-pixel range or sign test at all
//     OUT   both ends beyond the same frame edge                             -> the border value
//     EDGE  the frame's edge crosses the segment                             -> fast coordinates, guarded taps
//     SLOW  W changes sign / is tiny, or coordinates leave the fixed-point range -> exact chain per pixel
// Passes are software-pipelined (full-height tiles: straight-line code with two tap sets in flight); a pass's pixels are
// transposed through a wave-private LDS row and the wave writes all its rows, with contiguous plain stores, after its last
// pass.  No workgroup barrier.
//
// Layout of the sources: coords.h (coordinate arithmetic), sample.h (blending, guarded sampler), this file (the kernel: its
// two entries here, its body in rows_body.inc: the prologue, then the stages in the fragments rows_coords.inc / rows_sample.inc /
// rows_store.inc / rows_tiles.inc, how a tile is run in rows_run.inc; included in that order), and one translation unit per
// pixel type and interpolation (warp_u8_linear.hip, ...; their _p16 twins hold the 16-bit-plane instances) so that the formats
// compile side by side.
//
// Coordinates are float64.  The reference rounds fX = (X0 + M0 x1) * (32 / W) half-to-even; the fast chain (one
// v_rcp_f64 + Newton step shared by the lane's pixels, FMAs, row terms evaluated once per row) lands within 2^-40
// relative of it and rounds through the float64 mantissa:  t = fX' * 2^27 + (1.5 * 2^52 + 2^26 + 2^8)  leaves
// floor(X / 32) in the HIGH dword (X = the rounded 1/32-px coordinate), X & 31 in bits 27..31 of the low dword and the
// distance to the nearest rounding boundary below.  A pixel whose low bits lie within 2^-19 unit of a boundary -- the
// only place the two chains can disagree -- re-runs the reference chain operation for operation (exact_px).
// 8-bit blending is exact integer arithmetic on v_dot4_u32_u8 / v_dot2_u32_u16; float blending keeps the reference's
// operation order (FMA contraction off).
//
// No MFMA: this is a gather.  The float kernel is bound by HBM; the 8-bit kernels by vector-ALU issue (float64
// coordinate chain + blending) and the texture path's cost per gather instruction.
#pragma once
#include "sample.h"
#include "launch_pick.h"

namespace bevwarp {
namespace {

// ===================================================================================================
// warp_rows<T, C, INTERP, RS4, PLANAR>
//   RS4     8-bit RGB bilinear only: the source row stride is a multiple of 4 bytes (both tap rows of a pixel then share
//           one window alignment and one funnel-shift amount)
//   PLANAR  the destination is C float32 planes, dst[c][y][x] = float(pixel) * pscale[c] + pbias[c] (the layout a detector takes)
// warp_rows_planes16<T, C, INTERP, RS4>: the same planes converted to float16 / bfloat16 on the way out (rows_store.inc)
// Register budget: 4 waves per SIMD -- what the FAST row loop needs; the rare row classes may spill.
// ===================================================================================================
// Diagnostic build only (-DBEVWARP_CLOCK, tools/clock.py, bench.py's sclk_mhz): wave 0 of every workgroup adds the shader-clock
// ticks (s_memtime) and the 100 MHz reference ticks (s_memrealtime) it lived for; their ratio is the clock the chip held.  The
// kernels of that build are named warp_rows_clockbuild, so that a kernel trace of bench.py does not mix them with the product's.
#ifdef BEVWARP_CLOCK
#define warp_rows warp_rows_clockbuild
#define warp_rows_planes16 warp_rows_planes16_clockbuild
// One record of kClkWords counters per workgroup (blockIdx mod kClkRecords), ACCUMULATED with plain read-modify-writes by one lane of the
// workgroup -- no atomics: thousands of workgroups adding to a handful of shared words serialise in the L2's atomic unit and slow the
// very kernel that is being timed several-fold.  Words: [0] shader ticks the workgroup lived, [1] 100-MHz ticks, [2] workgroups.
constexpr int kClkWords = 4, kClkRecords = 8192;  // (three words in use; four keep a record's address a shift)
static __device__ unsigned long long g_clk[kClkRecords * kClkWords];
__device__ __forceinline__ void clk_add(int word, unsigned long long v) { g_clk[(blockIdx.x & (kClkRecords - 1)) * kClkWords + word] += v; }
#endif
// NSRC = 3 is warp_composite (bev/tool/compo.py:26-49) in one launch: a workgroup of 12 waves, four per source -- waves 0-3
// warp the background, 4-7 the foreground, 8-11 its mask, each group exactly as a workgroup of the plain kernel would, every
// group through its own homography and its own tile classification -- into an LDS copy of the tile instead of memory; after one
// barrier all twelve blend the three LDS tiles and store the composite.  The three warped images never exist in memory and
// every pixel is, by construction, what three bevwarp_warp calls produce.
constexpr int kCompositeRows = 16;  // tallest tile of the composite (its three LDS copies: 48 KB)
// The destination format of an instance (PFMT): interleaved pixels of the source type, float32 planes, or 16-bit planes (float16 or
// bfloat16 by the wave-uniform WarpArgs::planar).  warp_rows spells it as its bool PLANAR, as it always has -- the kernels' names, and
// with them every byte of the instances that existed before the 16-bit planes, stay what they were (profiles/planes16_isa_identity.txt)
// -- and warp_rows_planes16 is the same body with PFMT = kPlanes16.
constexpr int kInterleaved = 0, kPlanesF32 = 1, kPlanes16 = 2;
#define BEVWARP_ROWS_KERNEL(NSRC) __global__ __launch_bounds__(kWG * NSRC) __attribute__((amdgpu_waves_per_eu(NSRC > 1 ? 3 : kWavesPerSimd, 8)))
template <typename T, int C, int INTERP, bool RS4, bool PLANAR, int NSRC = 1>
BEVWARP_ROWS_KERNEL(NSRC) void warp_rows(const WarpArgs a) {
    constexpr int PFMT = PLANAR ? kPlanesF32 : kInterleaved;
#include "rows_body.inc"
}
template <typename T, int C, int INTERP, bool RS4>
BEVWARP_ROWS_KERNEL(1) void warp_rows_planes16(const WarpArgs a) {
    constexpr bool PLANAR = true;
    constexpr int NSRC = 1, PFMT = kPlanes16;
#include "rows_body.inc"
}

template <typename T, int C, int INTERP>
void launch_tci(const WarpArgs& a, dim3 grid, hipStream_t stream) {
    constexpr bool kRgb8Lin = sizeof(T) == 1 && C == 3 && INTERP == kLinear;
    if (a.planar) {
        if (kRgb8Lin && a.src_rs % 4 == 0)
            hipLaunchKernelGGL((warp_rows<T, C, INTERP, kRgb8Lin, true>), grid, dim3(kWG), 0, stream, a);
        else
            hipLaunchKernelGGL((warp_rows<T, C, INTERP, false, true>), grid, dim3(kWG), 0, stream, a);
        return;
    }
    if (kRgb8Lin && a.src_rs % 4 == 0)
        hipLaunchKernelGGL((warp_rows<T, C, INTERP, kRgb8Lin, false>), grid, dim3(kWG), 0, stream, a);
    else
        hipLaunchKernelGGL((warp_rows<T, C, INTERP, false, false>), grid, dim3(kWG), 0, stream, a);
}

// the 16-bit-plane instances (a.planar = kPlaneF16 | kPlaneBF16): translation units of their own (warp_u8_linear_p16.hip, ...)
template <typename T, int C, int INTERP>
void launch_tci_planes16(const WarpArgs& a, dim3 grid, hipStream_t stream) {
    constexpr bool kRgb8Lin = sizeof(T) == 1 && C == 3 && INTERP == kLinear;
    if (kRgb8Lin && a.src_rs % 4 == 0)
        hipLaunchKernelGGL((warp_rows_planes16<T, C, INTERP, kRgb8Lin>), grid, dim3(kWG), 0, stream, a);
    else
        hipLaunchKernelGGL((warp_rows_planes16<T, C, INTERP, false>), grid, dim3(kWG), 0, stream, a);
}
template <typename T, int INTERP>
void launch_channels_planes16(const WarpArgs& a, int channels, dim3 grid, hipStream_t stream) {
    pick::channels(channels, [&](auto c) { launch_tci_planes16<T, c(), INTERP>(a, grid, stream); });
}

// every channel count of one pixel type and interpolation: what one translation unit instantiates (warp_u8_linear.hip, ...)
template <typename T, int INTERP>
void launch_channels(const WarpArgs& a, int channels, dim3 grid, hipStream_t stream) {
    pick::channels(channels, [&](auto c) { launch_tci<T, c(), INTERP>(a, grid, stream); });
}

#ifdef BEVWARP_CLOCK
inline hipError_t read_clock_of_this_unit(unsigned long long* out16, int reset) {  // out16[0..2] += this translation unit's counters
    static unsigned long long v[kClkRecords * kClkWords];  // (256 KB: not on the stack; the diagnostic build is single-threaded)
    hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_clk), sizeof(v));
    if (e != hipSuccess) return e;
    for (int r = 0; r < kClkRecords; r++)
        for (int i = 0; i < 3; i++) out16[i] += v[r * kClkWords + i];
    if (reset) {
        void* p = nullptr;
        e = hipGetSymbolAddress(&p, HIP_SYMBOL(g_clk));
        if (e == hipSuccess) e = hipMemset(p, 0, sizeof(v));
    }
    return e;
}
#endif

}  // namespace
}  // namespace bevwarp
