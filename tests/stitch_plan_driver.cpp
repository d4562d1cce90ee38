// stitch_plan_driver.cpp -- the host side of bevwarp_warp_stitch (bev_amd/csrc/host_plan.h: stitch_check over stitch_call) from the command
// line, for tests/test_stitch_cpu.py, which builds it with g++ under the address and undefined-behaviour sanitizers.  One case per line
// of stdin, one line of numbers per case on stdout.  The call is made as bevwarp_api.hip makes it (a base of 0 is a null pointer; no
// pointer is dereferenced but the camera array and the border value, which are HOST):
//   stitch n_cams cams_null dst batch dst_h dst_w channels dst_fs dst_rs dtype interp blend feather border_mode border
//          then per described camera (`listed` of them, which may differ from n_cams): src src_h src_w fs rs m_count m_inv_null
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last channel
//       -> stitch_check's status, then the plan's status and total_tiles (kBorderTileW x kBorderTileH) where the status is BEVWARP_OK, else 0 0
#include "plan_driver_io.h"

int main() {
    return run_cases([](const std::string& cmd, std::istream& in, const std::string& line) {
        static const double m_inv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (cmd != "stitch") return -1;
        bevwarp_camera cams[16] = {};
        uint64_t dst = 0;
        Frames d = {};
        int n_cams, cams_null, batch, dst_h, dst_w, channels, dtype, interp, blend, feather, mode, border, listed;
        in >> n_cams >> cams_null >> dst >> batch >> dst_h >> dst_w >> channels >> d.fs >> d.rs >> dtype >> interp >> blend >> feather >> mode >> border >> listed;
        d.base = ptr(dst);
        if (!in || listed < 0 || listed > 16) return malformed(line);
        for (int k = 0; k < listed; k++) {
            uint64_t src = 0;
            int m_null = 0;
            in >> src >> cams[k].src_h >> cams[k].src_w >> cams[k].frame_stride >> cams[k].row_stride >> cams[k].m_count >> m_null;
            cams[k].src = ptr(src);
            cams[k].M_inv = m_null ? nullptr : m_inv;
        }
        if (!in) return malformed(line);
        double bv[4] = {1.0, 2.0, 3.0, 4.0};
        if (border == 2 && channels >= 1 && channels <= 4) bv[channels - 1] = NAN;
        TilePlan p = {};
        Call calls[BEVWARP_STITCH_MAX_CAMERAS];
        const auto describe = [&](const bevwarp_camera& k) { return stitch_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, mode); };
        const double* constant = (border && mode == BEVWARP_BORDER_CONSTANT) ? bv : nullptr;  // (read by the constant border only)
        print_stitch(stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{constant, channels}}, batch, dst_h, dst_w, 256, 4, p, calls), p);
        return 0;
    });
}
