// lens_lane.inc -- the body of a lens warp kernel `template <typename T, int C, int INTERP, bool TRANSPARENT> (const LensArgs a)`, included
// by warp_lens.hip and warp_fisheye.hip: a lane's 4 pixels from the row walk through the lens step to the store.
// BEVWARP_LENS_STEP: the unit's lens step, lens_pixel (lens_pixel.h) or fisheye_pixel (fisheye_pixel.h).
    constexpr int PPL = kBorderPPL;
    uint32_t b;
    int y, xs;  // frame, row, the lane's first pixel
    if (!lane_position(a, b, y, xs)) return;
    RowWalk walk(a, b, y);
    const uint8_t* frame = a.src + (int64_t)b * a.src_fs;
    const bool vec = a.src_vec_ok;

    Pixel<T, C> px[PPL];
    bool wr[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        // pixels past the row's end are computed like any other and not stored
        const int x = xs + j;
        double Xn, Yn, W;
        walk.pixel(a, x, Xn, Yn, W);
        int X, Y;
        const bool valid = BEVWARP_LENS_STEP<INTERP>(a, Xn, Yn, W, X, Y);
        const int sx = sat16(INTERP == kLinear ? (X >> kInterBits) : X), sy = sat16(INTERP == kLinear ? (Y >> kInterBits) : Y);
        const int fx = INTERP == kLinear ? (X & 31) : 0, fy = INTERP == kLinear ? (Y & 31) : 0;
        if constexpr (TRANSPARENT) {
            // valid inliers only (bevwarp_warp_border's test); every other pixel is neither read nor written
            const bool in = x < a.dst_w && valid &&
                            (INTERP == kLinear ? ((unsigned)sx < (unsigned)(a.src_w - 1) && (unsigned)sy < (unsigned)(a.src_h - 1))
                                               : ((unsigned)sx < (unsigned)a.src_w && (unsigned)sy < (unsigned)a.src_h));
            wr[j] = in;
            if (in) px[j] = sample_inside<T, C, INTERP>(frame, a.src_rs, sx, sy, fx, fy, vec);
        } else {
            wr[j] = x < a.dst_w;
            px[j] = sample_guarded<T, C, INTERP>(a, frame, sx, sy, fx, fy, valid, vec);
        }
    }

    store_lane_pixels<T, C, TRANSPARENT>(a, b, y, xs, px, wr);
