// stitch_maps_u8x3.inc -- the camera loop of the map stitches that keep an 8-bit pixel of 3 channels packed and store every pixel
// (stitch_maps_nv12_out_kernel, warp_stitch_maps_nv12_out.hip; stitch_maps_planes_kernel, warp_stitch_maps_planes.hip), included in the
// kernel's body after lane_position; the gained units (BEVWARP_STITCH_GAIN_UNIT, warp_stitch_maps.h) are these two units' text.  It is stitch_maps_body's loop and blends (warp_stitch_maps.hip), unchanged in meaning, with every
// pixel starting as the border pixel.  Shared as text, the way map_entry_taps.inc is: as a function template the loop changed both units'
// machine code (profiles/map_samplers_identity.txt).  In scope: a (StitchMapsArgs: dst_w, n_cams, cams, feather, bv_u8), INTERP, NV12 (the
// cameras' frames are NV12, converted in the order RGB), kFeather, PPL, b, y, xs.  Defines px[PPL], the lane's 4 pixels of row y of frame b
// (byte k = channel k), for the kernel's store; the samplers are stitch_sample.h's.
    // per pixel, as in stitch_maps_body: OVER keeps the pixel and whether it is still undecided; FEATHER the weighted sums and the sum of
    // weights.  A pixel starts as the border pixel: what no camera covers stays that.
    uint32_t px[PPL];
    bool wr[PPL], todo[PPL];
    int acc[PPL][3], wsum[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        px[j] = a.bv_u8;
        todo[j] = xs + j < a.dst_w;  // pixels past the row's end are neither computed nor stored
        wr[j] = false;
        wsum[j] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[j][c] = 0;
    }

    // OVER runs from the last camera to the first and stops when the lane's four pixels are decided; FEATHER runs in ascending order
    const int n = a.n_cams;
    for (int i = 0; i < n; i++) {
        if (!kFeather && !(todo[0] || todo[1] || todo[2] || todo[3])) break;
        const int k = kFeather ? i : n - 1 - i;
        const StitchMapCamera& cam = a.cams[k];
        const auto tap = camera_tap(a, k);  // (a gained launch: the camera's gain on every tap; otherwise nothing)
        uint32_t e[PPL], fr[PPL];
        load_camera_entries<INTERP>(cam, b, y, xs, a.dst_w, e, fr);
        const uint8_t* frame = cam.src + (int64_t)b * cam.src_fs;
        const uint8_t* uvf = NV12 ? cam.uv + (int64_t)b * cam.uv_fs : nullptr;
        const uint32_t rs = (uint32_t)cam.src_rs, uv_rs = (uint32_t)cam.uv_rs;  // (below 2^24: the source limits)
        const int sw = cam.src_w, sh = cam.src_h;
        const bool window = sw >= 4;
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (!todo[j]) continue;
            const int sx = (int)(short)(e[j] & 0xffffu), sy = (int)e[j] >> 16;
            const int fx = INTERP == kLinear ? (int)(fr[j] & 31u) : 0, fy = INTERP == kLinear ? (int)((fr[j] >> 5) & 31u) : 0;  // (higher bits are ignored)
            // bevwarp_remap's TRANSPARENT inlier test against THIS camera's frame: every tap read below is a source pixel
            const bool in = INTERP == kLinear ? ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1))
                                              : ((unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh);
            if (!in) continue;
            uint32_t p;
            if constexpr (NV12)
                p = sample_inlier_nv12<INTERP, RGB>(frame, uvf, rs, uv_rs, sw, window, sx, sy, fx, fy, tap);
            else
                p = sample_inlier<INTERP>(frame, rs, sx, sy, fx, fy, tap);
            wr[j] = true;
            if constexpr (!kFeather) {
                px[j] = p;
                todo[j] = false;
            } else {
                // whole source pixels to the nearest frame edge (>= 1 for an inlier), cut off at F
                const int w = min(min(min(sx + 1, sw - sx), min(sy + 1, sh - sy)), a.feather);
                wsum[j] += w;
#pragma unroll
                for (int c = 0; c < 3; c++) acc[j][c] += (int)((p >> (8 * c)) & 0xffu) * w;  // (the sums stay below 2^23)
            }
        }
    }

    if constexpr (kFeather) {
#pragma unroll
        for (int j = 0; j < PPL; j++) {
            if (wr[j]) {
                uint32_t out = 0;
#pragma unroll
                for (int c = 0; c < 3; c++) out |= (uint32_t)div_byte_mean(acc[j][c] + (wsum[j] >> 1), wsum[j]) << (8 * c);
                px[j] = out;
            }
        }
    }
