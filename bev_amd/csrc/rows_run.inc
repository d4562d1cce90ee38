// rows_run.inc -- FRAGMENT of the body of warp_rows (warp_rows.h includes it inside the kernel; its lambdas capture the kernel's state by
// reference and are always inlined).  Not a header: how a tile is processed -- outside tiles, the interior pipelines (straight-line, ring,
// loop), edge-cut tiles -- and the call that runs it.
    auto run_tile = [&]() __attribute__((always_inline)) {
    if (tile_out) {  // every pixel of the tile is the border value
        Pass p;
        if (!first_pass(BlkSeg{}, p)) return;
        fill_s();
        read_back(out);
        do store_s(BlkSeg{}, pass_x(p), p.y, out);
        while (next_pass(BlkSeg{}, p));
        return;
    }
    // -- interior tiles: no row classes; software-pipelined (the next pass's loads in flight, the pass after that getting its
    // coordinates, while the previous one is stored and the current one blended).
    // Pixels in a tie window are not fixed where they are found: the pass is blended from its fast coordinates (a unit off
    // at worst -- still inside the frame, the tile test keeps a pixel of margin for exactly this), a flag is shifted into a
    // scalar mask, and flagged passes (rare) are redone whole by the exact chain after the loop.  With the exact chain out
    // of the loop its state fits 128 VGPRs: four waves per SIMD instead of three (-12 %: DESIGN.md section 6.2).
    // ROW-AFFINE tiles (`row_affine` tag; row segments only).  When the source row and the perspective divide do not depend on the
    // destination column -- inverse matrix with M3 = M6 = 0: the rectification / inverse-perspective form, every keystone, every
    // scale + shift; judged per tile with the tolerance derived at `tile_affine` -- a row segment needs ONE reciprocal and ONE Y
    // coordinate per pass, the same in every lane: X = (UX + x M0) r is one add and one FMA per pixel, the tap row's byte offset is
    // a scalar, fy and the Y tie flag are wave-uniform.  18 float64 instructions per 256-pixel row instead of 38, 4 offset
    // instructions instead of 12.
    auto interior = [&](auto own, auto row_affine, auto pair_tag) __attribute__((always_inline)) {
        constexpr bool kBlk = decltype(own)::blk;
        constexpr bool kAff = decltype(row_affine)::value;
        constexpr bool kPair = decltype(pair_tag)::value;  // pixel pairs share a 16-byte tap window (rows_sample.inc: issue_p)
        static_assert(!kAff || !kBlk, "row-affine passes are row segments");
        static_assert(!kPair || (kAff && kPairable), "pair tiles are row-affine");
        auto issue_i = [&](const uint32_t (&S0)[PPL], Bytes<WINB> (&t0)[PPL], Bytes<WINB> (&t1)[PPL]) __attribute__((always_inline)) {
            if constexpr (kPair)
                issue_p(S0, t0, t1);
            else
                issue_s(kFast, S0, t0, t1);
        };
        auto finish_i = [&](const uint32_t (&S0)[PPL], const uint32_t (&S1)[PPL], const uint32_t (&S2)[PPL], const Bytes<WINB> (&t0)[PPL],
                            const Bytes<WINB> (&t1)[PPL]) __attribute__((always_inline)) {
            if constexpr (kPair)
                finish_p(S0, S1, S2, t0, t1);
            else
                finish_s(S0, S1, S2, t0, t1);
        };
        Pass p_cur, p_nxt;  // p_cur: the pass whose pixels sit in the LDS row; p_nxt: the pass whose coordinates are in the C state
        if (!first_pass(own, p_nxt)) return;
        // row terms of the pass the coordinate stage is at; a row segment's advance by one addition per pass
        double UX = 0, UY = 0, UW = 0;
        double DX1 = 0, DX2m1 = 0;  // (pair tiles: the steps between a lane's pixels)
        if constexpr (kPair) DX1 = uniform_f64(m0 * kTwo32), DX2m1 = uniform_f64(m0 * (127.0 * kTwo32));
        const double SX = uniform_f64(RX * (double)kWaves), SY = uniform_f64(RY * (double)kWaves), SW = uniform_f64(RW * (double)kWaves);
        if (!kBlk) UX = __builtin_fma(RX, (double)p_nxt.y, CX), UY = __builtin_fma(RY, (double)p_nxt.y, CY), UW = __builtin_fma(RW, (double)p_nxt.y, CW);
        auto coords_f = [&](const Pass& p, uint32_t (&S0)[PPL], uint32_t (&S1)[PPL], uint32_t (&S2)[PPL]) __attribute__((always_inline)) {
            uint32_t hx[PPL], lx[PPL], hy[PPL], ly[PPL], wf_, wl_;
            if constexpr (kAff) {
                // W, 1 / W and Y at the segment's first pixel stand for the whole segment (tile_affine bounds what that ignores)
                const double r = rcp_newton(UW);
                const double ty_ = __builtin_fma(UY, r, F::kMagic);
                const uint32_t hyu = (uint32_t)__builtin_amdgcn_readfirstlane(__double2hiint(ty_)), lyu = (uint32_t)__builtin_amdgcn_readfirstlane(__double2loint(ty_));
                const uint32_t row_off = (hyu & 0xffffffu) * rs32 + kOff;  // scalar; the low 24 bits like v_mul_u32_u24 (kOff carries their bias)
                double Xn = UX + cx0;
#pragma unroll
                for (int j = 0; j < PPL; j++) {
                    const double tx_ = __builtin_fma(Xn, r, F::kMagic);
                    S0[j] = __umul24((uint32_t)__double2hiint(tx_), (uint32_t)PBs) + row_off;
                    S1[j] = (uint32_t)__double2loint(tx_);
                    S2[j] = lyu;
                    if (j + 1 < PPL) Xn += kPair ? ((j & 1) ? DX2m1 : DX1) : DX;  // (pairs: pixels 2 l, 2 l + 1, 128 + 2 l, 128 + 2 l + 1 of the segment)
                }
                UX += SX;
                UY += SY;
                UW += SW;
                return;
            }
            if constexpr (kBlk) {
                set_strip(p.strip);
                chain(own, p.y, hx, lx, hy, ly, wf_, wl_);
            } else {
                chain_u(own, UX, UY, UW, hx, lx, hy, ly, wf_, wl_);
                UX += SX;
                UY += SY;
                UW += SW;
            }
#pragma unroll
            for (int j = 0; j < PPL; j++) {
                S0[j] = __umul24(hy[j], rs32) + (__umul24(hx[j], (uint32_t)PBs) + kOff);
                S1[j] = lx[j];
                S2[j] = ly[j];
            }
        };
        uint64_t tie_passes = 0;  // bit k: the pass blended k passes before the last one has a pixel in a tie window
        int n_blended = 0;        // (at most 64 passes per wave and tile: the host keeps tiles <= 64 rows)
        auto note_ties = [&](const uint32_t (&S1)[PPL], const uint32_t (&S2)[PPL]) __attribute__((always_inline)) {
            uint32_t tie = 0xffffffffu;
#pragma unroll
            for (int j = 0; j < PPL; j++) tie = min(tie, min(S1[j] & F::kTieMask, S2[j] & F::kTieMask));
            tie_passes = (tie_passes << 1) | (uint64_t)(__ballot(tie == 0) != 0ull);
            n_blended++;
        };
        bool more;
        int k_blend = 0;  // index of the pass being blended (its LDS row when stores are deferred)
        auto step = [&](uint32_t (&C0)[PPL], uint32_t (&C1)[PPL], uint32_t (&C2)[PPL], uint32_t (&N0)[PPL], uint32_t (&N1)[PPL], uint32_t (&N2)[PPL])
                        __attribute__((always_inline)) {
            if constexpr (!kDefer) read_back(out);  // p_cur's pixels (written a step ago: no LDS latency on the path)
            issue_i(C0, u0, u1);
            const Pass p_st = p_cur;
            p_cur = p_nxt;
            more = next_pass(own, p_nxt);
            if (more) coords_f(p_nxt, N0, N1, N2);
            if constexpr (!kDefer) store_s(own, pass_x(p_st), p_st.y, out);  // behind the loads: vmcnt retires in issue order
            lds_row(++k_blend);
            finish_i(C0, C1, C2, u0, u1);
            note_ties(C1, C2);
        };
        // Nearest neighbour: the taps of up to kDepth passes in flight -- a ring of pass slots; the loads of a pass are issued as soon
        // as the slot's previous pass has been put away, and with kDepth = 6 every pass of a wave over a 24-row tile has its loads out
        // before the first is consumed (a tap is one dword per pixel: 4 registers per slot).  A nearest pass has next to no arithmetic
        // to hide its loads behind, so the depth is what it runs at -- A/B on one box, 48 rounds, buffer sets drawn at random
        // (profiles/r03_late_ab.txt): depth 1 / 2 / 4 / 6 = 58.2 / 56.8 / 54.9 / 51.1 us per 32 frames (-12 %), a 25-degree
        // footprint 66.9 -> 63.2.  (Behind the ring's branches the compiler cannot count the loads issued after the ones a pass
        // consumes and waits for vmcnt(0): the ring only pays once everything is issued up front.  Full-height tiles take the
        // straight-line form below, whose counts are exact; the ring is what ragged tiles run.)
        constexpr bool kDeep = kDefer && INTERP == kNearest;
        // A wave with a full set of rows (kRowsLds passes: every wave of a full-height tile) runs them as STRAIGHT-LINE code.  Only
        // there does the compiler know how many loads were issued after the ones a pass is about to consume -- behind a loop's or the
        // ring's branches it has to assume none and waits for vmcnt(0), i.e. for every load in flight, the newest included.  Nearest:
        // all six passes' loads up front.  Bilinear: TWO tap sets, the loads of pass n + 2 issued right after pass n has been
        // blended and consumed after pass n + 1 has, under s_waitcnt vmcnt(13..8) -- a whole step in flight instead of the
        // coordinate stage of one: 8-bit row-affine tiles 80.1 -> 77.1 us per 32 frames (-3.7 %; A/B, profiles/r03_late_ab.txt),
        // float unchanged (191.5: it runs at the streaming rate either way).  The same two sets behind a loop's branches measured
        // nothing at all (80.1 -> 80.8): the waits, not the loads, were what did not overlap.  A third set does not fit 128
        // registers (the scheduler sinks its loads back to where two sets put them); the general chain spills with two.
        bool straight = false;
        if constexpr (kDefer && !kBlk && (INTERP == kNearest || kAff || sizeof(T) == 4)) {  // (8-bit bilinear, general chain: two tap sets spill)
            constexpr int kFull = kRowsLds;
            constexpr int kAhead = INTERP == kNearest ? kFull : 2;  // passes of taps in flight (bilinear: a third set does not fit 128 registers)
            if ((y_last - p_nxt.y) / kWaves + 1 == kFull) {
                straight = true;
                uint32_t R0[kAhead][PPL], R1[kAhead][PPL], R2[kAhead][PPL];
                Bytes<WINB> r0[kAhead][PPL], r1[kAhead][PPL];
                // (pair tiles: left alone, instruction selection floats the arithmetic of pass k -- and with it the wait for its taps -- above the
                // loads of pass k + 1: one set in flight, every wait a vmcnt(0).  `hold` is an empty asm that takes pass k's four tap windows
                // as read-write operands and clobbers memory: it cannot move above the loads issued before it, the blend cannot move above it,
                // and the wait the compiler puts in front of it is vmcnt(4) -- the other set stays in flight.)
                auto hold = [&](Bytes<WINB> (&t0)[PPL], Bytes<WINB> (&t1)[PPL]) __attribute__((always_inline)) {
                    if constexpr (kPair) {
                        // (the operands are the four 16-byte windows AS LOADED -- rebuilt from their components, which folds back to the loaded
                        // register tuples: sixteen separate 32-bit operands cost ~10 register copies per pass)
                        u32x4 a0 = {t0[0].w[0], t0[0].w[1], t0[0].w[2], t0[1].w[0]}, a1 = {t0[2].w[0], t0[2].w[1], t0[2].w[2], t0[3].w[0]};
                        u32x4 b0 = {t1[0].w[0], t1[0].w[1], t1[0].w[2], t1[1].w[0]}, b1 = {t1[2].w[0], t1[2].w[1], t1[2].w[2], t1[3].w[0]};
                        asm volatile("" : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1)::"memory");
#pragma unroll
                        for (int k = 0; k < 3; k++) t0[0].w[k] = a0[k], t0[2].w[k] = a1[k], t1[0].w[k] = b0[k], t1[2].w[k] = b1[k];
                        t0[1].w[0] = a0[3], t0[3].w[0] = a1[3], t1[1].w[0] = b0[3], t1[3].w[0] = b1[3];
                    }
                };
#pragma unroll
                for (int k = 0; k < kAhead; k++) {
                    coords_f(p_nxt, R0[k], R1[k], R2[k]);
                    note_ties(R1[k], R2[k]);
                    issue_i(R0[k], r0[k], r1[k]);
                }
#pragma unroll
                for (int k = 0; k < kFull; k++) {
                    constexpr int kA = kAhead;
                    const int d = k % kA;
                    lds_row(k);
                    hold(r0[d], r1[d]);
                    finish_i(R0[d], R1[d], R2[d], r0[d], r1[d]);
                    if (k + kA < kFull) {
                        coords_f(p_nxt, R0[d], R1[d], R2[d]);
                        note_ties(R1[d], R2[d]);
                        issue_i(R0[d], r0[d], r1[d]);
                    }
                }
            }
        }
        if (straight) {
        } else if constexpr (kDeep) {
            constexpr int kDepth = 6;  // passes in flight
            uint32_t R0[kDepth][PPL], R1[kDepth][PPL], R2[kDepth][PPL];  // ring of pass states (nearest: dead once the loads are out)
            Bytes<WINB> r0[kDepth][PPL], r1[kDepth][PPL];
            bool live[kDepth];
            bool any = true;  // passes are issued in order: the first slot that finds none ends the tile
#pragma unroll
            for (int d = 0; d < kDepth; d++) {
                live[d] = any && (d == 0 || next_pass(own, p_nxt));
                any = live[d];
                if (live[d]) {
                    coords_f(p_nxt, R0[d], R1[d], R2[d]);
                    note_ties(R1[d], R2[d]);
                    issue_i(R0[d], r0[d], r1[d]);
                }
            }
            int kb = 0;
            for (bool done = false; !done;) {
#pragma unroll
                for (int d = 0; d < kDepth; d++) {
                    if (done || !live[d]) {
                        done = true;
                        continue;
                    }
                    lds_row(kb++);
                    finish_i(R0[d], R1[d], R2[d], r0[d], r1[d]);
                    any = any && next_pass(own, p_nxt);
                    live[d] = any;
                    if (any) {
                        coords_f(p_nxt, R0[d], R1[d], R2[d]);
                        note_ties(R1[d], R2[d]);
                        issue_i(R0[d], r0[d], r1[d]);
                    }
                }
            }
        } else {
        coords_f(p_nxt, A0, A1, A2);
        issue_i(A0, u0, u1);
        p_cur = p_nxt;
        more = next_pass(own, p_nxt);
        if (more) coords_f(p_nxt, B0, B1, B2);
        lds_row(0);
        finish_i(A0, A1, A2, u0, u1);
        note_ties(A1, A2);
        while (more) {  // (two steps per trip: the states swap roles instead of being copied)
            step(B0, B1, B2, A0, A1, A2);
            if (!more) break;
            step(A0, A1, A2, B0, B1, B2);
        }
        if constexpr (!kDefer) {
            read_back(out);
            store_s(own, pass_x(p_cur), p_cur.y, out);
        }
        }
        if (__builtin_expect(tie_passes != 0, 0)) {  // redo the flagged passes: every pixel by the exact chain and the generic sampler
            Pass p;
            first_pass(own, p);
            int k = n_blended - 1, kr = 0;
            do {
                if ((tie_passes >> k) & 1ull) {
                    lds_row(kr);
                    slow_s(own, InTail{}, pass_x(p), p.y);
                    if constexpr (!kDefer) {
                        read_back(out);
                        store_s(own, pass_x(p), p.y, out);
                    }
                }
                k--, kr++;
            } while (next_pass(own, p));
        }
        if constexpr (kDefer) {  // every pass of this wave, LDS -> memory: the stores trail the tile's last load
            Pass p;
            first_pass(own, p);
            int kr = 0;
            do {
                lds_row(kr++);
                read_back(out);
                store_s(own, pass_x(p), p.y, out);
            } while (next_pass(own, p));
        }
    };
    // (the branch hints keep the common path -- interior tile, row segments -- the fall-through: with the patch code in the
    // kernel its layout otherwise costs unturned footprints 3 %)
    if (__builtin_expect(tile_in, 1)) {
        if (__builtin_expect(!tile_slanted, 1)) {
            if (tile_affine) {
                if constexpr (kPairable) {
                    if (tile_pair) {
                        interior(RowSeg{}, std::true_type{}, std::true_type{});
                        return;
                    }
                }
                interior(RowSeg{}, std::true_type{}, std::false_type{});
            } else {
                interior(RowSeg{}, std::false_type{}, std::false_type{});
            }
        } else {
            interior(PatSeg{}, std::false_type{}, std::false_type{});
        }
        return;
    }
    // -- the frame's edge crosses the tile (or W changes sign in it): blocks with a class each, the same pipeline
    auto edge_tile = [&](auto own) __attribute__((always_inline)) {
        Pass p_cur, p_nxt;
        if (!first_pass(own, p_nxt)) return;
        int k_blend = 0;
        int cls_c = coords_s(own, p_nxt.strip, p_nxt.y, A0, A1, A2), cls_n = kSlow;
        issue_s(cls_c, A0, u0, u1);
        p_cur = p_nxt;
        bool more = next_pass(own, p_nxt);
        if (more) cls_n = coords_s(own, p_nxt.strip, p_nxt.y, B0, B1, B2);
        lds_row(0);
        finish_any(own, cls_c, pass_x(p_cur), p_cur.y, A0, A1, A2, u0, u1);
        while (more) {
#pragma unroll
            for (int j = 0; j < PPL; j++) {
                A0[j] = B0[j];
                A1[j] = B1[j];
                A2[j] = B2[j];
            }
            cls_c = cls_n;
            if constexpr (!kDefer) read_back(out);
            issue_s(cls_c, A0, u0, u1);
            const Pass p_st = p_cur;
            p_cur = p_nxt;
            more = next_pass(own, p_nxt);
            if (more) cls_n = coords_s(own, p_nxt.strip, p_nxt.y, B0, B1, B2);  // overlaps with the loads in flight
            if constexpr (!kDefer) store_s(own, pass_x(p_st), p_st.y, out);
            lds_row(++k_blend);
            finish_any(own, cls_c, pass_x(p_cur), p_cur.y, A0, A1, A2, u0, u1);
        }
        if constexpr (!kDefer) {
            read_back(out);
            store_s(own, pass_x(p_cur), p_cur.y, out);
        } else {
            Pass p;
            first_pass(own, p);
            int kr = 0;
            do {
                lds_row(kr++);
                read_back(out);
                store_s(own, pass_x(p), p.y, out);
            } while (next_pass(own, p));
        }
    };
    if (tile_slanted)
        edge_tile(PatSeg{});
    else
        edge_tile(BlkSeg{});
    };  // run_tile
    run_tile();
