// stitch_gain_plan_driver.cpp -- the host side of the six stitches through maps under BEVWARP_STITCH_GAIN (bev_amd/csrc/host_plan.h:
// take_gain_flag, then stitch_check with the gain words over stitch_maps_call and its kin) from the command line, for
// tests/test_stitch_gain_cpu.py, which builds it with g++ under the address and undefined-behaviour sanitizers.  One case per line of stdin,
// one line of numbers per case on stdout.  The call is made as bevwarp_api.hip makes it (a base of 0 is a null pointer; no pointer is
// dereferenced but the camera array and the host values, which are HOST):
//   maps | nv12 | to_nv12 | nv12_to_nv12 | planes | nv12_planes
//          n_cams cams_null dst batch dst_h dst_w channels dst_fs dst_rs dtype interp blend feather rgb_order border_mode border
//          dst2 dst2_fs dst2_rs plane_dtype listed
//          then per described camera (`listed` of them, which may differ from n_cams):
//            src uv src_h src_w fs rs uv_fs uv_rs xy frac xy_fs xy_rs frac_fs frac_rs map_count reserved
//       blend: the word as the caller passes it, BEVWARP_STITCH_GAIN included or not.
//       dst2, dst2_fs, dst2_rs: the plane of pairs of an NV12 destination; dst2_fs is the plane stride of a destination of planes.
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last channel (channels of `maps`, otherwise 3)
//       -> the status, the plan's status and total_tiles (kBorderTileW x kBorderTileH) where the status is BEVWARP_OK (else 0 0), whether the
//          flag was set, and where it was and the status is BEVWARP_OK the n_cams gain words as they were checked
#include "plan_driver_io.h"

int main() {
    return run_cases([](const std::string& cmd, std::istream& in, const std::string& line) {
        const bool nv12 = cmd == "nv12" || cmd == "nv12_to_nv12" || cmd == "nv12_planes";
        const bool to_nv12 = cmd == "to_nv12" || cmd == "nv12_to_nv12", planes = cmd == "planes" || cmd == "nv12_planes";
        if (cmd != "maps" && !nv12 && !to_nv12 && !planes) return -1;
        bevwarp_map_camera cams[16] = {};
        uint64_t dst = 0, dst2 = 0;
        Frames d = {}, d2 = {};
        int n_cams, cams_null, batch, dst_h, dst_w, channels, dtype, interp, blend, feather, rgb, mode, border, plane_dtype, listed;
        in >> n_cams >> cams_null >> dst >> batch >> dst_h >> dst_w >> channels >> d.fs >> d.rs >> dtype >> interp >> blend >> feather >> rgb >> mode >> border >> dst2 >>
            d2.fs >> d2.rs >> plane_dtype >> listed;
        d.base = ptr(dst), d2.base = ptr(dst2);
        if (!in || listed < 0 || listed > 16) return malformed(line);
        for (int k = 0; k < listed; k++)
            if (!read_map_cameras(in, 1, &cams[k]) || !(in >> cams[k].reserved)) return malformed(line);
        double bv[4] = {1.0, 2.0, 3.0, 4.0};
        const int nb = cmd == "maps" ? channels : 3;
        if (border == 2 && nb >= 1 && nb <= 4) bv[nb - 1] = NAN;
        const bool gained = take_gain_flag(blend);  // (every check below sees the word without the flag)
        TilePlan p = {};
        Call calls[BEVWARP_STITCH_MAX_CAMERAS];
        uint32_t gains[BEVWARP_STITCH_MAX_CAMERAS] = {};
        const auto describe = [&](const bevwarp_map_camera& k) {
            if (to_nv12) return stitch_maps_nv12_out_call(nv12, k, d, d2, batch, dst_h, dst_w, interp, blend, nv12 ? 0 : rgb);
            if (planes) return stitch_maps_planes_call(nv12, k, d, d2.fs, batch, dst_h, dst_w, interp, blend, nv12 ? rgb : 0, plane_dtype);
            return nv12 ? stitch_maps_nv12_call(k, d, batch, dst_h, dst_w, interp, blend, rgb, mode)
                        : stitch_maps_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, mode, gained);
        };
        // (the entries with a border mode read the border value under the constant border only; the others always)
        const double* constant = (border && (to_nv12 || planes || mode == BEVWARP_BORDER_CONSTANT)) ? bv : nullptr;
        const int st = stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{constant, nb}}, batch, dst_h, dst_w, 256, 4, p, calls,
                                    gained ? gains : nullptr);
        printf("%d %d %" PRId64 " %d", st, st == BEVWARP_OK ? p.status : 0, st == BEVWARP_OK ? p.total_tiles : 0, (int)gained);
        for (int k = 0; gained && st == BEVWARP_OK && k < n_cams; k++) printf(" %" PRIu32, gains[k]);
        printf("\n");
        return 0;
    });
}
