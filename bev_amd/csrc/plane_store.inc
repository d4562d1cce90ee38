// plane_store.inc -- the plane stage of the NV12 kernels that write normalised channel planes, included at the end of their bodies:
// nv12_planes_kernel (warp_nv12_planes.hip, bevwarp_warp_nv12_planes) and remap_nv12_planes_kernel (warp_map_nv12.hip,
// bevwarp_remap_nv12_planes).  Shared as text, the way the row kernel's rows_*.inc are: as a function the stage changed
// nv12_planes_kernel's machine code, as text it does not.  In scope: a (FrameArgs with ch_off[3], pscale[3], pbias[3] and plane:
// Nv12PlanesArgs' fields, warp_nv12.h), PPL, WIDE16 (2-byte planes; a.plane = kPlaneF16 | kPlaneBF16 is wave-uniform), b, y, xs and
// p[PPL] -- pixel xs + j of row y of frame b, byte k = sampled channel k.  See DESIGN.md section 4.13.
    // the plane stores: per sampled channel the 8-bit value as float32, times scale, plus bias (each rounded), converted; 4 elements of
    // a plane row in one store for a lane whose 4 pixels lie in the row, element stores otherwise
    constexpr int ELEM = WIDE16 ? 2 : 4;
    uint8_t* d = dst_row(a, b, y) + (int64_t)xs * ELEM;
    const int lane_px = min(PPL, a.dst_w - xs);
    const bool lane_vec = a.dst_vec_ok && lane_px == PPL;
    if constexpr (WIDE16) {
        auto planes = [&](auto as) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float sc = a.pscale[k], bi = a.pbias[k];
                const uint32_t h[4] = {as((float)((p[0] >> (8 * k)) & 0xffu) * sc + bi), as((float)((p[1] >> (8 * k)) & 0xffu) * sc + bi),
                                       as((float)((p[2] >> (8 * k)) & 0xffu) * sc + bi), as((float)((p[3] >> (8 * k)) & 0xffu) * sc + bi)};
                uint16_t* dk = reinterpret_cast<uint16_t*>(d + a.ch_off[k]);
                if (__builtin_expect(lane_vec, 1)) {
                    u32x2 o = {h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
                    wide_store(reinterpret_cast<u32x2*>(dk), o);
                } else {
#pragma unroll
                    for (int i = 0; i < PPL; i++)
                        if (i < lane_px) dk[i] = (uint16_t)h[i];
                }
            }
        };
        if (a.plane == kPlaneBF16)  // (wave-uniform)
            planes(BitsBF16{});
        else
            planes(BitsF16{});
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float sc = a.pscale[k], bi = a.pbias[k];
            f32x4 o = {(float)((p[0] >> (8 * k)) & 0xffu) * sc + bi, (float)((p[1] >> (8 * k)) & 0xffu) * sc + bi,
                       (float)((p[2] >> (8 * k)) & 0xffu) * sc + bi, (float)((p[3] >> (8 * k)) & 0xffu) * sc + bi};
            float* dk = reinterpret_cast<float*>(d + a.ch_off[k]);
            if (__builtin_expect(lane_vec, 1)) {
                wide_store(reinterpret_cast<f32x4*>(dk), o);
            } else {
#pragma unroll
                for (int i = 0; i < PPL; i++)
                    if (i < lane_px) dk[i] = o[i];
            }
        }
    }
