// map_build.inc -- the body of a map builder kernel `template <int INTERP, ...> (const MapBuildArgs a)`, included by warp_map.hip (the
// pinhole chain and OpenCV's rational lens model) and warp_map_fisheye.hip (the equidistant one): a lane's 4 pixels from the row walk
// through the chain's last step to OpenCV's fixed-point map format -- int16 pairs (sx, sy) and, for bilinear, uint16 (fy << 5) | fx -- and
// their stores.
// BEVWARP_MAP_STEP: the unit's statement(s) that define `bool valid` and set X, Y from (Xn, Yn, W); not valid: the pixel is outside
// whatever (X, Y) say.
    constexpr int PPL = kBorderPPL;
    uint32_t b;
    int y, xs;  // map, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);

    uint32_t e[PPL], fr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other and not stored
        double Xn, Yn, W;
        walk.pixel(a, xs + j, Xn, Yn, W);
        int X, Y;
        BEVWARP_MAP_STEP
        const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
        const uint32_t f = INTERP == kLinear ? (uint32_t)(((Y & 31) << 5) | (X & 31)) : 0u;
        // an invalid pixel: every tap of (-32768, -32768) lies outside every admissible source (include/bevwarp.h)
        e[j] = valid ? (((uint32_t)sx & 0xffffu) | ((uint32_t)sy << 16)) : 0x80008000u;
        fr[j] = valid ? f : 0u;
    }

    uint8_t* xrow = dst_row(a, b, y) + (int64_t)xs * 4;
    uint8_t* frow = a.frac + (int64_t)b * a.frac_fs + (int64_t)y * a.frac_rs + (int64_t)xs * 2;
    if (a.dst_vec_ok && xs + PPL <= a.dst_w) {  // the lane's 4 entries: one 16-byte and one 8-byte store
        const u32x4 o = {e[0], e[1], e[2], e[3]};
        wide_store(reinterpret_cast<u32x4*>(xrow), o);
        if constexpr (INTERP == kLinear) {
            const u32x2 q = {fr[0] | (fr[1] << 16), fr[2] | (fr[3] << 16)};
            *reinterpret_cast<u32x2*>(frow) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PPL; j++)
            if (xs + j < a.dst_w) {
                reinterpret_cast<uint32_t*>(xrow)[j] = e[j];
                if constexpr (INTERP == kLinear) reinterpret_cast<uint16_t*>(frow)[j] = (uint16_t)fr[j];
            }
    }
