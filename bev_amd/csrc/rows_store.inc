// rows_store.inc -- FRAGMENT of the body of warp_rows (warp_rows.h includes it inside the kernel; its lambdas capture the kernel's state by
// reference and are always inlined).  Not a header: the store stage: LDS row -> registers in store order -> memory (wide stores, element stores for ragged lanes, float32 and 16-bit planes, the composite's LDS tiles).
    // -- LDS row -> registers in store order (u8: pixels 4 l .. 4 l + 3 of the segment; float: 16-byte unit u * 64 + l)
    constexpr int kVec = sizeof(T) == 1 ? 64 : TRW / 4;  // 16-byte units in the wave's row segment
    constexpr int NQ = (kVec + 63) / 64;
    static_assert(NQ * 4 >= PPL * C || sizeof(T) == 1, "the planar float path keeps a lane's PPL pixels in the same registers");
    auto read_back = [&](uint4 (&out)[NQ]) __attribute__((always_inline)) {
        asm volatile("" ::: "memory");  // compiler fence: one wave's LDS operations execute in program order
        if constexpr (PLANAR && sizeof(T) == 4) {  // float planes: the lane's own PPL pixels, channel by channel (pixel 64 j + lane)
            uint32_t* o = reinterpret_cast<uint32_t*>(&out[0]);
#pragma unroll
            for (int j = 0; j < PPL; j++)
#pragma unroll
                for (int k = 0; k < C; k++) o[j * C + k] = wtr[(64 * j + lane) * C + k];
            asm volatile("" ::: "memory");
            return;
        }
#pragma unroll
        for (int u = 0; u < NQ; u++) {
            const int q = u * 64 + lane;
            if (q < kVec) out[u] = reinterpret_cast<const uint4*>(wtr)[q];
        }
        asm volatile("" ::: "memory");  // (the next row's LDS writes cannot pass these reads)
    };
    auto finish_any = [&](auto own, int cls, int xs, int y, const uint32_t (&S0)[PPL], const uint32_t (&S1)[PPL], const uint32_t (&S2)[PPL], const Bytes<WINB> (&t0)[PPL],
                          const Bytes<WINB> (&t1)[PPL]) __attribute__((always_inline)) {
        if (__builtin_expect(cls == kFast, 1)) {
            finish_s(S0, S1, S2, t0, t1);
        } else {
            if (cls == kOut)
                fill_s();
            else if (cls == kEdge)
                edge_s(S1, S2);
            else
                slow_s(own, InLoop{}, xs, y);
        }
    };

    // -- stores.  Plain (default-policy) wide stores: the destination is written once and never read back by this kernel, but
    // non-temporal stores -- round 2's choice -- measure SLOWER on every format here (A/B of four builds interleaved on one
    // box, profiles/r03_store_ab.txt: float32 keystone 192.8 -> 183.7 us, 8-bit bilinear 73.7 -> 72.2, nearest 58.3 -> 55.6).
    // Lanes of a ragged last tile (and every lane when the destination's layout does not admit the wide stores) fall back to
    // element stores.  (Also measured and not kept: the wide store as ONE unconditional buffer_store whose masked lanes get an
    // out-of-range offset, so that the compiler's vmcnt accounting sees it -- nearest -4 %, bilinear and float +4 %.)
    auto store_s = [&](auto own, int xs, int y, const uint4 (&out)[NQ]) __attribute__((always_inline)) {  // xs = first pixel of the segment / block
        constexpr bool kBlk = decltype(own)::blk;
        const int seg_px = min(kBlk ? 64 : TW, a.dst_w - xs);  // valid pixels of a row of the segment / block
        // 8-bit: a lane stores the 4 consecutive pixels of its 16-byte unit of the LDS row: pixels 4 l .. of the wave's row; row
        // l / 16 of its block, pixels 4 (l % 16) ..; or (patches: LDS index 64 j + 16 ly + lx) row (l / 4) % 4, pixels 16 (l / 16) + 4 (l % 4) ..
        constexpr bool kPat = decltype(own)::pat;
        const int st_row = kPat ? (lane >> 2) & 3 : kBlk ? lane >> 4 : 0;
        const int st_x = kPat ? xs + 16 * (lane >> 4) + 4 * (lane & 3) : kBlk ? xs + (lane & 15) * PPL : xs + lane * PPL;
        const int lane_px = max(0, min(PPL, a.dst_w - st_x));  // valid pixels of this lane's store unit
        const bool lane_vec = a.dst_vec_ok && lane_px == PPL;
        if constexpr (sizeof(T) == 1) {  // the lane's 4 pixels = 4 C contiguous bytes, one instruction
            const uint32_t p[4] = {out[0].x, out[0].y, out[0].z, out[0].w};
            if constexpr (PFMT == kPlanes16) {  // 16-bit planes: the float32 value of the float planes, converted; one 8-byte store per channel
                if (kBlk && y + st_row > y_last) return;
                uint8_t* dp = dframe + (int64_t)(y + st_row) * a.dst_rs + (int64_t)st_x * 2;
                auto planes = [&](auto as) __attribute__((always_inline)) {
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const float sc = a.pscale[k], bi = a.pbias[k];
                        const uint32_t h[4] = {as((float)((p[0] >> (8 * k)) & 0xffu) * sc + bi), as((float)((p[1] >> (8 * k)) & 0xffu) * sc + bi),
                                               as((float)((p[2] >> (8 * k)) & 0xffu) * sc + bi), as((float)((p[3] >> (8 * k)) & 0xffu) * sc + bi)};
                        uint16_t* dk = reinterpret_cast<uint16_t*>(dp + k * a.dst_ps);
                        if (__builtin_expect(lane_vec, 1)) {
                            u32x2 o = {h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
                            wide_store(reinterpret_cast<u32x2*>(dk), o);
                        } else {
                            for (int i = 0; i < lane_px; i++) dk[i] = (uint16_t)h[i];
                        }
                    }
                };
                if (a.planar == kPlaneBF16)  // (wave-uniform)
                    planes(BitsBF16{});
                else
                    planes(BitsF16{});
                return;
            }
            if constexpr (PLANAR) {  // float planes: one 16-byte store per channel
                if (kBlk && y + st_row > y_last) return;
                uint8_t* dp = dframe + (int64_t)(y + st_row) * a.dst_rs + (int64_t)st_x * 4;
#pragma unroll
                for (int k = 0; k < C; k++) {
                    const float sc = a.pscale[k], bi = a.pbias[k];
                    f32x4 o = {(float)((p[0] >> (8 * k)) & 0xffu) * sc + bi, (float)((p[1] >> (8 * k)) & 0xffu) * sc + bi,
                               (float)((p[2] >> (8 * k)) & 0xffu) * sc + bi, (float)((p[3] >> (8 * k)) & 0xffu) * sc + bi};
                    float* dk = reinterpret_cast<float*>(dp + k * a.dst_ps);
                    if (__builtin_expect(lane_vec, 1)) {
                        wide_store(reinterpret_cast<f32x4*>(dk), o);
                    } else {
                        for (int i = 0; i < lane_px; i++) dk[i] = o[i];
                    }
                }
                return;
            }
            if (kBlk && y + st_row > y_last) return;
            if constexpr (NSRC > 1) {  // composite: the lane's four packed pixels go to this source's LDS copy of the tile
                *reinterpret_cast<uint4*>(&s_tile[(sid * kCompositeRows + (y + st_row - y0)) * TW + (st_x - x0)]) = out[0];
                return;
            }
            uint8_t* d = dframe + (int64_t)(y + st_row) * a.dst_rs + (int64_t)st_x * C;
            if (__builtin_expect(lane_vec, 1)) {
                if constexpr (C == 1) {
                    *reinterpret_cast<uint32_t*>(d) = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
                } else if constexpr (C == 2) {
                    u32x2 o = {p[0] | (p[1] << 16), p[2] | (p[3] << 16)};
                    *reinterpret_cast<u32x2*>(d) = o;
                } else if constexpr (C == 3) {
                    // (four packed pixels -> twelve bytes: three byte permutes instead of eight shifts and ors)
                    u32x3 o = {__builtin_amdgcn_perm(p[1], p[0], 0x04020100u), __builtin_amdgcn_perm(p[2], p[1], 0x05040201u), __builtin_amdgcn_perm(p[3], p[2], 0x06050402u)};
                    wide_store(reinterpret_cast<u32x3*>(d), o);
                } else {
                    u32x4 o = {p[0], p[1], p[2], p[3]};
                    wide_store(reinterpret_cast<u32x4*>(d), o);
                }
            } else {
                for (int i = 0; i < lane_px; i++)
#pragma unroll
                    for (int k = 0; k < C; k++) d[i * C + k] = (uint8_t)(p[i] >> (8 * k));
            }
        } else if constexpr (PLANAR) {  // float source -> float planes: 64 consecutive floats of a plane row per instruction
            const float* o = reinterpret_cast<const float*>(&out[0]);
#pragma unroll
            for (int j = 0; j < PPL; j++) {
                const int px = kPat ? xs + PWd * j + (lane & (PWd - 1)) : kBlk ? xs + lane : xs + 64 * j + lane, py = kPat ? y + lane / PWd : kBlk ? y + j : y;
                if (px >= a.dst_w || py > y_last) continue;
#pragma unroll
                for (int k = 0; k < C; k++) {
                    if constexpr (PFMT == kPlanes16) {  // (2-byte stores, 64 consecutive elements of a plane row per instruction)
                        uint16_t* dk = reinterpret_cast<uint16_t*>(dframe + k * a.dst_ps + (int64_t)py * a.dst_rs) + px;
                        const float v = o[j * C + k] * a.pscale[k] + a.pbias[k];
                        *dk = (uint16_t)(a.planar == kPlaneBF16 ? BitsBF16{}(v) : BitsF16{}(v));
                        continue;
                    }
                    float* dk = reinterpret_cast<float*>(dframe + k * a.dst_ps + (int64_t)py * a.dst_rs) + px;
                    *dk = o[j * C + k] * a.pscale[k] + a.pbias[k];
                }
            }
        } else {
            const int nfl = seg_px * C;  // valid floats of a row of the segment / block
            // blocks: the LDS row holds the block's rows one after the other (runs of 64 pixels); patches: pixels in the order
            // 64 j + PWd ly + lx, i.e. runs of PWd pixels: run n is row n % BR of the block, pixels PWd (n / BR) ..
            constexpr int kRunUnits = (kPat ? PWd : 64) * C / 4;
            static_assert(sizeof(T) == 1 || (PWd * C) % 4 == 0, "a run of the patch is a whole number of 16-byte units");
#pragma unroll
            for (int u = 0; u < NQ; u++) {
                const int q = u * 64 + lane;
                if (q >= kVec) continue;
                const int run = kBlk ? q / kRunUnits : 0;
                const int r = kPat ? run % BR : run, qr = kBlk ? (kPat ? run / BR : 0) * kRunUnits + (q - run * kRunUnits) : q;  // row of the block, unit within the row
                if (kBlk && y + r > y_last) continue;
                float* drow = reinterpret_cast<float*>(dframe + (int64_t)(y + r) * a.dst_rs) + (int64_t)xs * C;
                if (__builtin_expect(a.dst_vec_ok && 4 * qr + 4 <= nfl, 1)) {
                    u32x4 o = {out[u].x, out[u].y, out[u].z, out[u].w};
                    wide_store(&reinterpret_cast<u32x4*>(drow)[qr], o);
                } else {
                    const uint32_t f[4] = {out[u].x, out[u].y, out[u].z, out[u].w};
                    for (int i = 0; i < 4 && 4 * qr + i < nfl; i++) reinterpret_cast<uint32_t*>(drow)[4 * qr + i] = f[i];
                }
            }
        }
    };

