// rows_body.inc -- FRAGMENT: the body of the warp kernel (warp_rows.h includes it inside warp_rows and inside warp_rows_planes16, which
// differ in the store stage alone).  Not a header.  Its surroundings define T, C, INTERP, RS4, PLANAR, NSRC, PFMT and the argument `a`.
    constexpr int PPL = pixels_per_lane<T>();
    constexpr int TW = 64 * PPL;                                 // tile width
    constexpr int kStrips = PPL;                                 // 64-pixel column strips of a tile (block ownership)
    constexpr int BR = PPL;                                      // rows of a block
    constexpr int PWd = 64 / PPL;                                // lanes per row of a block's patch (BlkSeg)
    constexpr int PBs = (int)sizeof(T) * C;                      // source bytes per pixel
    constexpr int TAPB = INTERP == kLinear ? 2 * PBs : PBs;      // bytes of one row's taps
    constexpr int LOADB = (TAPB + 3) & ~3;                       // loaded per row (whole dwords)
    constexpr int SH = INTERP == kLinear ? kInterBits : 0;
    using F = Fix<INTERP>;
    // 8-bit RGB bilinear: a tap pair (6 bytes at any byte address) is fetched as the ALIGNED 12-byte window around it and
    // funnel-shifted into place.  The texture path turns byte-unaligned 8-byte gathers that miss L1 into data at ~50
    // cycles per wave instruction and 4-byte-aligned 12-byte ones at ~18 (tools/ubench_stream.hip).
    constexpr bool kAligned = sizeof(T) == 1 && C == 3 && INTERP == kLinear;
    constexpr int WINB = kAligned ? 12 : LOADB;  // bytes a FAST row loads per tap row
    constexpr bool kPairable = kAligned && RS4 && NSRC == 1 && PPL == 4;  // (pair tiles: rows_sample.inc issue_p)
    constexpr int kM = kAligned ? 2 : 1;         // FAST: both ends inside by this many pixels (the aligned window starts
                                                 // up to 3 bytes early: never before its row)
    constexpr int TRW = 64 * PPL * (sizeof(T) == 1 ? 1 : C);  // dwords of a wave's transposition row
    static_assert(!RS4 || kAligned, "RS4 only qualifies the aligned-window variant");
    static_assert(NSRC == 1 || (NSRC == 3 && sizeof(T) == 1 && INTERP == kLinear && !PLANAR), "the composite is three 8-bit bilinear warps");
    // Deferred stores (plain kernel): a wave keeps the pixels of ALL its passes over the tile in LDS, one transposition row per
    // pass, and writes them to memory after its last pass.  vmcnt retires in issue order, loads and stores alike, so a store
    // issued in pass n sits in front of the loads of pass n + 1 and their s_waitcnt cannot be satisfied before the store has
    // been acknowledged by the memory system: with either kind of access alone the kernel runs at its ALU time, with both it
    // loses 13 us of 75 (ablations: profiles/r03_tables.txt).  Stored at the end of the tile, nothing waits behind them.
    // (composite: one row, its passes go to the LDS tiles at once.)
    constexpr int kRowsLds = NSRC > 1 ? 1 : (sizeof(T) == 1 ? 6 : 4);  // passes of a wave over the tallest tile (24 / 16 rows)
    __shared__ __attribute__((aligned(16))) uint32_t s_tr[kWaves * NSRC][kRowsLds][TRW];
    // (composite only) the warped tiles, one packed pixel per dword: [source][row of the tile][pixel]
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[NSRC > 1 ? NSRC * kCompositeRows * TW : 4];
    constexpr int NEED = LOADB / 4;  // dwords of a tap row the blend takes, starting AT the left tap
#ifdef BEVWARP_CLOCK
    struct ClockStamp {
        unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
        __device__ ~ClockStamp() {
            if (threadIdx.x == 0) {
                clk_add(0, __builtin_amdgcn_s_memtime() - t0);
                clk_add(1, __builtin_amdgcn_s_memrealtime() - r0);
                clk_add(2, 1ull);
            }
        }
    } clock_stamp;
#endif
    // block -> (frame, tile): one XCD (blockIdx & 7) works on one contiguous run of items
    // The last `tail_split` tiles an XCD dispatches are cut into an upper and a lower half, one workgroup each: the launch's
    // tail is then made of half-length workgroups.
    uint32_t seq = blockIdx.x >> 3;  // dispatch order within the XCD
    int half = -1;
    if (seq >= (uint32_t)(a.chunk - a.tail_split)) {
        const uint32_t j = seq - (uint32_t)(a.chunk - a.tail_split);
        seq = (uint32_t)(a.chunk - a.tail_split) + (j >> 1);
        half = (int)(j & 1u);
    }
    uint32_t in_run = seq + (blockIdx.x & 7u) * (uint32_t)a.stagger;  // (stagger * 7 < chunk: bevwarp_api.hip)
    if (in_run >= (uint32_t)a.chunk) in_run -= (uint32_t)a.chunk;
    const uint32_t item = (blockIdx.x & 7u) * (uint32_t)a.chunk + in_run;
    if (item >= (uint32_t)a.total_tiles) return;
    const uint32_t cls_idx = item * 3u + (uint32_t)(half + 1);  // this workgroup's entry of the verdict table (full tile, upper half, lower half)
    const uint32_t frame_idx = fast_div(item, a.tpf_magic, (uint32_t)a.tiles_per_frame);
    const uint32_t t = item - frame_idx * (uint32_t)a.tiles_per_frame;
    const uint32_t ty = fast_div(t, a.tx_magic, (uint32_t)a.tiles_x), tx = t - ty * (uint32_t)a.tiles_x;
    const int x0 = (int)tx * TW, y0 = (int)ty * a.tile_h + (half == 1 ? a.tile_h / 2 : 0);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform, in an SGPR
    const int wave = NSRC > 1 ? (wave_all & (kWaves - 1)) : wave_all, sid = NSRC > 1 ? (wave_all >> 2) : 0;  // wave of its group of four / source
    // this wave's source (composite: background, foreground or mask; frames of one launch otherwise)
    const uint8_t* src_base = a.src;
    const double* m_base = a.minv;
    int64_t src_rs = a.src_rs;
    int src_w = a.src_w, src_h = a.src_h;
    if constexpr (NSRC > 1) {
        if (sid > 0) {
            src_base = a.xsrc[sid - 1], m_base = a.xminv[sid - 1], src_rs = a.xsrc_rs[sid - 1];
            src_w = a.xsrc_w[sid - 1], src_h = a.xsrc_h[sid - 1];
        }
    }
    const uint8_t* __restrict__ frame = src_base + (int64_t)frame_idx * a.src_fs;
    uint8_t* __restrict__ dframe = a.dst + (int64_t)frame_idx * a.dst_fs;
    const double* __restrict__ M = m_base + (int64_t)frame_idx * a.m_stride;
    const int y_last = min(y0 + (half >= 0 ? a.tile_h / 2 : a.tile_h), a.dst_h) - 1;
    if (y0 > y_last) return;  // (the lower half of a ragged last tile may be empty)

    SrcView view;
    view.frame = frame;
    view.rs = src_rs;
    view.w = src_w;
    view.h = src_h;
    const bool gray_src = NSRC > 1 && sizeof(T) == 1 && C == 3 && sid == 1 && a.fg_gray != 0;  // (constant false in the plain kernel)
    view.gray = gray_src;
#pragma unroll
    for (int k = 0; k < 4; k++) view.bf[k] = a.bval_f[k];
    view.bu = (uint32_t)a.bval_u8[0] | ((uint32_t)a.bval_u8[1] << 8) | ((uint32_t)a.bval_u8[2] << 16) | ((uint32_t)a.bval_u8[3] << 24);

    // -- limits of unguarded loads
    const int sx_lim = (int)(((int64_t)src_w * PBs - LOADB) / PBs);   // largest sx with sx*PBs + LOADB <= w*PBs
    const int sxw_lim = (int)(((int64_t)src_w * PBs - WINB) / PBs);   // same for the FAST rows' windows
    const int sy_lim = src_h - (INTERP == kLinear ? 2 : 1);
    const bool any_unguarded = (int64_t)src_w * PBs >= LOADB && sy_lim >= 0;
    const uint32_t sx_max = any_unguarded ? (uint32_t)sx_lim : 0u, sy_max = any_unguarded ? (uint32_t)sy_lim : 0u;
    const bool can_fast = (int64_t)src_w * PBs >= 32 && sxw_lim >= 2 * kM && sy_lim >= 2 * kM;

#include "rows_coords.inc"
#include "rows_sample.inc"
#include "rows_store.inc"
#include "rows_tiles.inc"
#include "rows_run.inc"
    if constexpr (NSRC > 1) {
        // -- composite_reg_img (bev/tool/compo.py:16-23) on the three LDS tiles.  The reference evaluates
        //   round(fg * (m / 255) + bg * (1 - m / 255)) in float64 and clips to 255; with N = fg m + bg (255 - m) that value is N / 255
        // up to 2.3e-13, while N / 255 is never closer than 1 / 510 to a rounding boundary (2 N - 255 is odd), so the result is
        // exactly floor((N + 127) / 255), which never exceeds 255: integer arithmetic, no division ((x * 0x8081) >> 23 == x / 255
        // for x < 2^16).
        __syncthreads();
        const int rows = y_last - y0 + 1;
        for (int u = tid; u < rows * 64; u += kWG * NSRC) {
            const int r = u >> 6, x = x0 + 4 * (u & 63);
            if (x >= a.dst_w) continue;
            const uint4 pb = *reinterpret_cast<const uint4*>(&s_tile[(0 * kCompositeRows + r) * TW + (x - x0)]);
            const uint4 pf = *reinterpret_cast<const uint4*>(&s_tile[(1 * kCompositeRows + r) * TW + (x - x0)]);
            const uint4 pm = *reinterpret_cast<const uint4*>(&s_tile[(2 * kCompositeRows + r) * TW + (x - x0)]);
            const uint32_t b4[4] = {pb.x, pb.y, pb.z, pb.w}, f4[4] = {pf.x, pf.y, pf.z, pf.w}, m4[4] = {pm.x, pm.y, pm.z, pm.w};
            uint32_t p[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                p[i] = 0;
#pragma unroll
                for (int k = 0; k < C; k++) {
                    const uint32_t m = (m4[i] >> (8 * k)) & 0xffu, f = (f4[i] >> (8 * k)) & 0xffu, b = (b4[i] >> (8 * k)) & 0xffu;
                    const uint32_t n = __umul24(f, m) + __umul24(b, 255u - m) + 127u;
                    p[i] |= ((n * 0x8081u) >> 23) << (8 * k);
                }
            }
            uint8_t* d = dframe + (int64_t)(y0 + r) * a.dst_rs + (int64_t)x * C;
            const int lane_px = min(4, a.dst_w - x);
            if (__builtin_expect(a.dst_vec_ok && lane_px == 4, 1)) {
                if constexpr (C == 1) {
                    *reinterpret_cast<uint32_t*>(d) = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
                } else if constexpr (C == 2) {
                    u32x2 o = {p[0] | (p[1] << 16), p[2] | (p[3] << 16)};
                    *reinterpret_cast<u32x2*>(d) = o;
                } else if constexpr (C == 3) {
                    u32x3 o = {p[0] | (p[1] << 24), (p[1] >> 8) | (p[2] << 16), (p[2] >> 16) | (p[3] << 8)};
                    *reinterpret_cast<u32x3*>(d) = o;
                } else {
                    u32x4 o = {p[0], p[1], p[2], p[3]};
                    *reinterpret_cast<u32x4*>(d) = o;
                }
            } else {
                for (int i = 0; i < lane_px; i++)
#pragma unroll
                    for (int k = 0; k < C; k++) d[i * C + k] = (uint8_t)(p[i] >> (8 * k));
            }
        }
    }
