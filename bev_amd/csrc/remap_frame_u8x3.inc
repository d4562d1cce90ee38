// remap_frame_u8x3.inc -- a lane's 4 pixels of one frame, after remap_taps_u8x3.inc and inside the loop over the item's frames.  In scope:
// INTERP, MODE, PPL, frame (the frame's first byte), tap[PPL], pair, border.  Fills p[PPL].
        if constexpr (INTERP == kLinear) {
            if (pair) {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, true>(frame, tap[j], border);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, false>(frame, tap[j], border);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPL; j++) p[j] = sample_entry<INTERP, MODE, false>(frame, tap[j], border);
        }
