// remap_taps_nv12.inc -- what a lane of the remap kernels that read NV12 frames derives once per item, before it walks the item's frames
// (remap_nv12_body, warp_map_nv12.hip; remap_nv12_to_nv12_kernel, warp_map_nv12_out.hip), included at the top of the body.  Shared as
// text, the way map_entry_taps.inc is: as a function it changed both units' machine code (profiles/map_samplers_identity.txt).  In scope:
// a (RemapNv12Args), INTERP, MODE.  Returns for a lane outside the grid.  Defines PPL, kTransparent, kWindows (bilinear, and the build
// has the window loads: BEVWARP_REMAP_NV12_WINDOWS), y, xs, the item's first frame b0 and its frame count nb, tap[PPL]
// (remap_sample_nv12.h's NvTaps), wr[PPL] -- the pixel is written -- `window` -- the lane takes the window loads -- and `border`.
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
