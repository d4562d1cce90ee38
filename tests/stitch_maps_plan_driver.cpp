// stitch_maps_plan_driver.cpp -- the host side of bevwarp_stitch_maps and bevwarp_stitch_maps_nv12 (bev_amd/csrc/host_plan.h:
// stitch_check over stitch_maps_call, stitch_maps_nv12_call) from the command line, for tests/test_stitch_maps_cpu.py, which builds it with
// g++ under the address and undefined-behaviour sanitizers.  One case per line of stdin, one line of numbers per case on stdout.  The call is
// made as bevwarp_api.hip makes it (a base of 0 is a null pointer; no pointer is dereferenced but the camera array and the border value, which
// are HOST):
//   maps | nv12   n_cams cams_null dst batch dst_h dst_w channels dst_fs dst_rs dtype interp blend feather rgb_order border_mode border listed
//          then per described camera (`listed` of them, which may differ from n_cams):
//            src uv src_h src_w fs rs uv_fs uv_rs xy frac xy_fs xy_rs frac_fs frac_rs map_count
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last channel (nv12: of 3; channels, dtype are not looked at)
//       -> the status, then the plan's status and total_tiles (kBorderTileW x kBorderTileH) where the status is BEVWARP_OK, else 0 0
#include "plan_driver_io.h"

int main() {
    return run_cases([](const std::string& cmd, std::istream& in, const std::string& line) {
        if (cmd != "maps" && cmd != "nv12") return -1;
        const bool nv12 = cmd == "nv12";
        bevwarp_map_camera cams[16] = {};
        uint64_t dst = 0;
        Frames d = {};
        int n_cams, cams_null, batch, dst_h, dst_w, channels, dtype, interp, blend, feather, rgb, mode, border, listed;
        in >> n_cams >> cams_null >> dst >> batch >> dst_h >> dst_w >> channels >> d.fs >> d.rs >> dtype >> interp >> blend >> feather >> rgb >> mode >> border >> listed;
        d.base = ptr(dst);
        if (!read_map_cameras(in, listed, cams)) return malformed(line);
        double bv[4] = {1.0, 2.0, 3.0, 4.0};
        const int nb = nv12 ? 3 : channels;
        if (border == 2 && nb >= 1 && nb <= 4) bv[nb - 1] = NAN;
        TilePlan p = {};
        Call calls[BEVWARP_STITCH_MAX_CAMERAS];
        const auto describe = [&](const bevwarp_map_camera& k) {
            return nv12 ? stitch_maps_nv12_call(k, d, batch, dst_h, dst_w, interp, blend, rgb, mode) : stitch_maps_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, mode);
        };
        const double* constant = (border && mode == BEVWARP_BORDER_CONSTANT) ? bv : nullptr;  // (read by the constant border only)
        print_stitch(stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{constant, nb}}, batch, dst_h, dst_w, 256, 4, p, calls), p);
        return 0;
    });
}
