// rows_tiles.inc -- FRAGMENT of the body of warp_rows (warp_rows.h includes it inside the kernel; its lambdas capture the kernel's state by
// reference and are always inlined).  Not a header: row state, tile classification from the four corner pixels, the passes of a wave over a tile.
    // -- the row loop.  Rows of a tile are dealt to its waves round-robin: neighbouring rows share source lines and run
    // at the same time.
    uint32_t A0[PPL], A1[PPL], A2[PPL], B0[PPL], B1[PPL], B2[PPL];  // row state: current / next
    Bytes<WINB> u0[PPL], u1[PPL];
    uint4 out[NQ];
    // -- interior tiles.  When the tile's four corner pixels sample inside the frame by the FAST margin with W of one sign,
    // the tile maps into the convex quadrilateral of their images: every row is FAST and the loop needs no row classes --
    // no end-pixel read-out, no scalar decisions, row terms advanced by one addition each.
    // -- the tile's four corner pixels decide how it is processed
    bool tile_in, tile_slanted, tile_out, tile_affine;
    bool tile_pair = false;  // row-affine tile whose taps advance by 0 .. 2 source pixels per destination pixel: pixel pairs share a 16-byte window
    // A caller that warps many batches through the same matrices and geometry (a camera loop) may hand in the verdicts of an earlier
    // fill launch (bevwarp_warp_classes): the tile's set-up below -- a tenth of the 8-bit kernel's vector instructions -- is then one
    // scalar load.  The table is indexed by workgroup, so it is only valid for the launch geometry it was filled with (the host checks).
    bool have_class = false;
    if constexpr (NSRC == 1) {
        if (a.tile_class) {
            const uint32_t f = a.tile_class[cls_idx];
            have_class = (f >> 31) != 0;
            tile_in = f & 1u, tile_out = (f >> 1) & 1u, tile_slanted = (f >> 2) & 1u, tile_affine = (f >> 3) & 1u, tile_pair = (f >> 4) & 1u;
        }
    }
    if (!have_class) {
        const int ck = lane & 3;
        const double cdx = (ck & 1) ? (double)(TW - 1) : 0.0, cdy = (double)((ck & 2) ? y_last : y0);
        const double cW = __builtin_fma(RW, cdy, CW) + m6 * cdx;
        const double cr = rcp_newton(cW);
        const double ctx = __builtin_fma(__builtin_fma(RX, cdy, CX) + (m0 * kTwo32) * cdx, cr, F::kMagic);
        const double cty = __builtin_fma(__builtin_fma(RY, cdy, CY) + (m3 * kTwo32) * cdx, cr, F::kMagic);
        const uint32_t chx = (uint32_t)__double2hiint(ctx), chy = (uint32_t)__double2hiint(cty);
        const int csx = (int)(chx - kHiBias), csy = (int)(chy - kHiBias);
        const uint32_t cwh = (uint32_t)__double2hiint(cW);
        const bool c_w = ((cwh >> 20) & 0x7ffu) - 824u <= 398u;
        // (one pixel more than the rows' own margin: the exact chain may move a coordinate by a unit)
        const bool c_in = (uint32_t)(csx - kM - 1) <= (uint32_t)(sxw_lim - 2 * kM - 2) && (uint32_t)(csy - kM - 1) <= (uint32_t)(sy_lim - 2 * kM - 2) && c_w;
        const uint32_t in4 = (uint32_t)__ballot(c_in) & 0xFu, neg4 = (uint32_t)__ballot((cwh >> 31) != 0) & 0xFu;
        const bool one_sign = neg4 == 0u || neg4 == 0xFu;
        // interior: every pixel of the tile samples inside the frame (the tile maps into the convex quadrilateral of its
        // corners' images) -- no row classes at all
        tile_in = can_fast && sxw_lim >= 2 * kM + 2 && sy_lim >= 2 * kM + 2 && in4 == 0xFu && one_sign;
        // outside: all four corners beyond the same frame edge (coordinates representable, W sane) -- the border value
        const bool c_rep = c_w && (((chx ^ kHiExp) | (chy ^ kHiExp)) >> 20) == 0;
        auto all4 = [](bool v) { return ((uint32_t)__ballot(v) & 0xFu) == 0xFu; };
        tile_out = one_sign && all4(c_rep) && (all4(csx <= -3) || all4(csx > src_w) || all4(csy <= -3) || all4(csy > src_h));
        // Row-affine tiles.  Taking W and Y at a segment's first pixel for all TW of them leaves out m6 x in W and m3 x in Y: in
        // the fixed-point units of the chain (source pixels x 2^32) at most
        //     E = TW (|m3| 2^32 r + |m6| r^2 max(|X|, |Y|))        r = 1 / min |W|, X / Y the numerators, all over the tile's corners
        // (W of one sign is linear, so its extremes are at the corners; the numerators are affine too).  The tie window leaves
        // room: the chain itself is within 2^-21.9 output units of the reference for every coordinate the binade admits, the
        // window is 2^-19, so E <= 2^-21 units keeps every pixel outside a window on the reference's side of its rounding boundary.
        // Exactly zero for M3 = M6 = 0; ~1e-5 for a keystone whose matrix came out of a least-squares fit.
        {
            // (the four corners sit in the lanes of a quad: the reductions are two DPP quad permutes each -- no LDS round trips -- and
            // r = max |1 / W| reuses the corners' reciprocals: no division)
            auto quad_max = [](double v) {
                auto perm = [](double x, auto ctrl) {
                    constexpr int kCtrl = decltype(ctrl)::value;
                    return __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(x), kCtrl, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(__double2loint(x), kCtrl, 0xF, 0xF, true));
                };
                v = fmax(v, perm(v, std::integral_constant<int, 0xB1>{}));   // quad_perm [1, 0, 3, 2]
                return fmax(v, perm(v, std::integral_constant<int, 0x4E>{}));  // quad_perm [2, 3, 0, 1]
            };
            const double ax = fabs(__builtin_fma(RX, cdy, CX) + (m0 * kTwo32) * cdx), ay = fabs(__builtin_fma(RY, cdy, CY) + (m3 * kTwo32) * cdx);
            const double rr = quad_max(fabs(cr)) * 1.0000001, n_max = quad_max(fmax(ax, ay));  // (cr is 1 / W to 2^-48: the margin covers it a million times over)
            const double E = (double)TW * (fabs(m3) * kTwo32 * rr + fabs(m6) * rr * rr * n_max);
            constexpr double kUnit = INTERP == kLinear ? 134217728.0 /* 2^27 */ : kTwo32;
            tile_affine = __builtin_amdgcn_readfirstlane((int)(E <= kUnit * (1.0 / 2097152.0) /* 2^-21 */)) != 0;
        }
        // Turned footprints.  A row gather's 64 lanes lie on a source line that crosses dy source rows per 64 destination
        // pixels -- a cache line each once dy passes the lines the run would touch anyway -- and pixels sqrt(dx^2 + dy^2) / 64 apart;
        // a 16 x 4 patch of the same 64 pixels crosses a quarter of them.  Measured crossover (A/B over angles and
        // minifications, DESIGN.md section 6.4): 8-bit patches win when dy (dx^2 + dy^2) / 64^2 > ~15 (5 degrees at 1.4 x minification, 13
        // degrees at 1 x, 2.5 degrees at 2 x).  Both from the tile's top and bottom edges (corner images).
        auto edge_slant = [&](int l0, int l1) {
            const float dy = (float)abs(__builtin_amdgcn_readlane(csy, l1) - __builtin_amdgcn_readlane(csy, l0));
            const float dx = (float)abs(__builtin_amdgcn_readlane(csx, l1) - __builtin_amdgcn_readlane(csx, l0));
            return dy * (dx * dx + dy * dy);  // (over the tile's width = kStrips x 64 pixels: kStrips^3 times the per-64-pixel figure)
        };
        // The crossover scales with the bytes of a pixel (the lines a 64-pixel run touches anyway): 45 / bytes -- 15 for 8-bit
        // RGB, 11 for RGBA, 45 for grey, < 4 for float RGB (whose 32 x 2 patches cost an unturned footprint nothing).
        // (Single-channel float is the exception: its 32 x 2 patches lose to row segments up to ~20 degrees: 45.)
        constexpr float kSlantThr = sizeof(T) == 4 && C == 1 ? 45.0f : 45.0f / (float)PBs;
        // (a row-affine tile is never turned: its rows' images are source rows -- the test is skipped for them)
        tile_slanted = false;
        if (!tile_affine) tile_slanted = fmaxf(edge_slant(0, 1), edge_slant(2, 3)) > kSlantThr * 4096.0f * (float)(kStrips * kStrips * kStrips);
        if constexpr (kPairable) {
            // The left taps of neighbouring pixels of a row-affine tile are m0 / W source pixels apart, the same along a row and extreme at the
            // tile's top or bottom row (W of one sign is monotone in y): every corner within [0, 2 - 1/16] keeps the two left taps of a pair at
            // most 2 pixels apart whatever the rounding (a fast coordinate is a unit of 1/32 pixel off at worst).
            const double stp = m0 * cr;
            tile_pair = tile_affine && (((uint32_t)__ballot(stp >= 0.0 && stp <= 1.9375)) & 0xFu) == 0xFu;
        }
        if constexpr (NSRC == 1) {
            if (a.classify_out) {  // fill mode: the verdict, no pixels
                if (tid == 0)
                    a.classify_out[cls_idx] = 0x80000000u | (uint32_t)tile_in | (uint32_t)tile_out << 1 | (uint32_t)tile_slanted << 2 | (uint32_t)tile_affine << 3 | (uint32_t)tile_pair << 4;
                return;
            }
        }
    }
    // -- the passes of this wave over the tile, in order.
    //   row segments: rows y0 + w + 4 i (neighbouring rows share source lines and run at the same time)
    //   blocks:       strip after strip; inside a strip the four waves take neighbouring blocks (rotated by the strip index so
    //                 that a ragged tile height does not always short-change the same wave): together they walk a compact
    //                 64 x 4 BR patch of the destination at any time, which is what keeps a rotated footprint in L1
    struct Pass {
        int strip, y;
    };
    const int n_strips = (min(TW, a.dst_w - x0) + 63) >> 6;
    auto first_pass = [&](auto own, Pass& p) __attribute__((always_inline)) -> bool {
        constexpr bool kBlk = decltype(own)::blk;
        p.strip = 0;
        p.y = kBlk ? y0 + BR * wave : y0 + wave;
        if (!kBlk) return p.y <= y_last;
        while (p.y > y_last) {
            if (++p.strip >= n_strips) return false;
            p.y = y0 + BR * ((wave + p.strip) & (kWaves - 1));
        }
        return true;
    };
    auto next_pass = [&](auto own, Pass& p) __attribute__((always_inline)) -> bool {
        constexpr bool kBlk = decltype(own)::blk;
        p.y += kBlk ? BR * kWaves : kWaves;
        if (!kBlk) return p.y <= y_last;
        while (p.y > y_last) {
            if (++p.strip >= n_strips) return false;
            p.y = y0 + BR * ((wave + p.strip) & (kWaves - 1));
        }
        return true;
    };
    auto pass_x = [&](const Pass& p) { return x0 + 64 * p.strip; };

    {
        const bool patches = tile_slanted;  // (slanted tiles: interior and edge-cut alike)
        const bool pairs = kPairable && tile_in && !tile_slanted && tile_pair;  // (pair tiles: pixel 0 of lane l is pixel 2 l of the segment)
        const double lx = (double)(patches ? lane & (PWd - 1) : (pairs ? 2 * lane : lane)), ly = patches ? (double)(lane / PWd) : 0.0;
        cx0 = __builtin_fma(RX, ly, (m0 * kTwo32) * lx), cy0 = __builtin_fma(RY, ly, (m3 * kTwo32) * lx), cw0 = __builtin_fma(RW, ly, m6 * lx);
    }
