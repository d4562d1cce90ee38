// map_entry_taps.inc -- the index stage of the map samplers (remap_kernel, warp_map.hip; remap_taps_u8x3.inc; remap_taps_nv12.inc), included
// inside their loop over the lane's pixels j.  In scope: a (RemapArgs: src_w, src_h, dst_w and the index remap), INTERP, MODE,
// kTransparent, xs, j, e[j], fr[j], wr[].  Defines, for entry e[j] = (sx, sy): f (the weights: fx | fy << 5), the taps' columns c0, c1 and
// rows cy0, cy1, `in` (BORDER_CONSTANT: bit 0 = tap (row 0, col 0) inside, 1 = (0, 1), 2 = (1, 0), 3 = (1, 1); else 0), and sets wr[j]:
// the pixel is written.  CONSTANT clamps every tap into the source; the four remapping modes go through border_index (warp_border.h);
// TRANSPARENT keeps (sx, sy) as they are.
        const int sx = (int)(short)(e[j] & 0xffffu), sy = (int)e[j] >> 16;
        const uint32_t f = INTERP == kLinear ? (fr[j] & 1023u) : 0u;  // (higher bits are ignored)
        int c0, c1, cy0, cy1;
        uint32_t in = 0u;
        if constexpr (kTransparent) {
            // inliers only (remapBilinear's (unsigned)sx < width - 1); the others' taps are never used
            wr[j] = xs + j < a.dst_w && (INTERP == kLinear ? ((unsigned)sx < (unsigned)(a.src_w - 1) && (unsigned)sy < (unsigned)(a.src_h - 1))
                                                            : ((unsigned)sx < (unsigned)a.src_w && (unsigned)sy < (unsigned)a.src_h));
            c0 = sx, c1 = sx + 1, cy0 = sy, cy1 = sy + 1;
        } else if constexpr (MODE == 0) {
            wr[j] = xs + j < a.dst_w;
            const int w = a.src_w, h = a.src_h;
            const bool xin0 = (unsigned)sx < (unsigned)w, yin0 = (unsigned)sy < (unsigned)h;
            const bool xin1 = INTERP == kLinear && (unsigned)(sx + 1) < (unsigned)w, yin1 = INTERP == kLinear && (unsigned)(sy + 1) < (unsigned)h;
            c0 = min(max(sx, 0), w - 1), c1 = min(max(sx + 1, 0), w - 1), cy0 = min(max(sy, 0), h - 1), cy1 = min(max(sy + 1, 0), h - 1);
            in = (uint32_t)(xin0 && yin0) | ((uint32_t)(xin1 && yin0) << 1) | ((uint32_t)(xin0 && yin1) << 2) | ((uint32_t)(xin1 && yin1) << 3);
        } else {
            wr[j] = xs + j < a.dst_w;
            c0 = border_index<MODE>(sx, a.src_w, a.per_x, a.off_x, a.mag_x);
            cy0 = border_index<MODE>(sy, a.src_h, a.per_y, a.off_y, a.mag_y);
            c1 = INTERP == kLinear ? border_index<MODE>(sx + 1, a.src_w, a.per_x, a.off_x, a.mag_x) : c0;
            cy1 = INTERP == kLinear ? border_index<MODE>(sy + 1, a.src_h, a.per_y, a.off_y, a.mag_y) : cy0;
        }
