// stitch_maps_plan_driver.cpp -- the host side of bevwarp_stitch_maps and bevwarp_stitch_maps_nv12 (bev_amd/csrc/host_plan.h:
// stitch_maps_status, stitch_maps_nv12_status) from the command line, for tests/test_stitch_maps_cpu.py, which builds it with g++ under
// the address and undefined-behaviour sanitizers.  One case per line of stdin, one line of numbers per case on stdout.  The call is made
// as bevwarp_api.hip makes it (a base of 0 is a null pointer; no pointer is dereferenced but the camera array and the border value, which
// are HOST):
//   maps | nv12   n_cams cams_null dst batch dst_h dst_w channels dst_fs dst_rs dtype interp blend feather rgb_order border_mode border listed
//          then per described camera (`listed` of them, which may differ from n_cams):
//            src uv src_h src_w fs rs uv_fs uv_rs xy frac xy_fs xy_rs frac_fs frac_rs map_count
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last channel (nv12: of 3; channels, dtype are not looked at)
//       -> the status, then the plan's status and total_tiles (kBorderTileW x kBorderTileH) where the status is BEVWARP_OK, else 0 0
#include <inttypes.h>
#include <math.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

int main() {
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd != "maps" && cmd != "nv12") {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        const bool nv12 = cmd == "nv12";
        bevwarp_map_camera cams[16] = {};
        uint64_t dst = 0;
        Frames d = {};
        int n_cams, cams_null, batch, dst_h, dst_w, channels, dtype, interp, blend, feather, rgb, mode, border, listed;
        in >> n_cams >> cams_null >> dst >> batch >> dst_h >> dst_w >> channels >> d.fs >> d.rs >> dtype >> interp >> blend >> feather >> rgb >> mode >> border >> listed;
        d.base = (const void*)(uintptr_t)dst;
        if (!in || listed < 0 || listed > 16) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        for (int k = 0; k < listed; k++) {
            uint64_t src = 0, uv = 0, xy = 0, frac = 0;
            bevwarp_map_camera& c = cams[k];
            in >> src >> uv >> c.src_h >> c.src_w >> c.frame_stride >> c.row_stride >> c.uv_frame_stride >> c.uv_row_stride >> xy >> frac >> c.xy_frame_stride >>
                c.xy_row_stride >> c.frac_frame_stride >> c.frac_row_stride >> c.map_count;
            c.src = (const void*)(uintptr_t)src, c.uv = (const void*)(uintptr_t)uv;
            c.map_xy = (const void*)(uintptr_t)xy, c.map_frac = (const void*)(uintptr_t)frac;
        }
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        double bv[4] = {1.0, 2.0, 3.0, 4.0};
        const int nb = nv12 ? 3 : channels;
        if (border == 2 && nb >= 1 && nb <= 4) bv[nb - 1] = NAN;
        TilePlan p = {};
        const bevwarp_map_camera* cp = cams_null ? nullptr : cams;
        const int st = nv12 ? stitch_maps_nv12_status(cp, n_cams, d, batch, dst_h, dst_w, interp, blend, feather, rgb, mode, border ? bv : nullptr, 256, 4, p)
                            : stitch_maps_status(cp, n_cams, d, batch, dst_h, dst_w, channels, dtype, interp, blend, feather, mode, border ? bv : nullptr, 256, 4, p);
        printf("%d %d %" PRId64 "\n", st, st == BEVWARP_OK ? p.status : 0, st == BEVWARP_OK ? p.total_tiles : 0);
    }
    return 0;
}
