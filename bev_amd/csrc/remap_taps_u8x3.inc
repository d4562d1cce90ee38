// remap_taps_u8x3.inc -- what a lane of the 8-bit 3-channel remap kernels that write every pixel derives once per item, before it walks
// the item's frames (remap_planes_kernel, warp_map_planes.hip; remap_to_nv12_kernel, warp_map_nv12_out.hip), included at the top of the
// kernel's body.  Shared as text, the way map_entry_taps.inc is: as a function the body changed both units' machine code
// (profiles/map_samplers_identity.txt).  In scope: a (RemapArgs), INTERP, MODE (not BORDER_TRANSPARENT).  Returns for a lane outside the
// grid.  Defines PPL, y, xs, the item's first frame b0 and its frame count nb, tap[PPL] (remap_sample_u8x3.h's Taps), `pair` -- the lane
// takes the 6-byte pair loads -- and `border`, the border pixel.
    constexpr int PPL = kBorderPPL;
    constexpr bool kTransparent = false;
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
