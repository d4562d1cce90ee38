// nv12_planes_plan_driver.cpp -- the argument checks of bev_amd/csrc/host_plan.h for an NV12 warp into channel planes
// (check_warp_nv12_planes), its wide-store decision and the launch plan that follows, for tests/test_nv12_planes_cpu.py (built with g++
// under the address and undefined-behaviour sanitizers).  One case per line of stdin, one line of numbers per case on stdout:
//   nv12p y_base uv_base dst_base batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_ps dst_rs m_count interp rgb_order plane_dtype
//       -> check_warp_nv12_planes's status, wide stores admitted (nv12_planes_wide_stores_ok), plan_border's status and total_tiles
// A base of 0 is a null pointer.  No pointer is dereferenced.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

int main() {
    static const double minv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd != "nv12p") {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        uint64_t y, uv, dst;
        int batch, src_h, src_w, dst_h, dst_w, m_count, interp, rgb, plane_dtype;
        int64_t y_fs, y_rs, uv_fs, uv_rs, dst_fs, dst_ps, dst_rs;
        in >> y >> uv >> dst >> batch >> src_h >> src_w >> dst_h >> dst_w >> y_fs >> y_rs >> uv_fs >> uv_rs >> dst_fs >> dst_ps >> dst_rs >> m_count >> interp >> rgb >>
            plane_dtype;
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        // (positional, as bevwarp_api.hip fills it)
        const Nv12PlanesCall c = {{(const void*)(uintptr_t)y, (const void*)(uintptr_t)uv, (const void*)(uintptr_t)dst, batch, src_h, src_w, dst_h, dst_w, y_fs, y_rs,
                                   uv_fs, uv_rs, dst_fs, dst_rs, minv, m_count, interp, rgb},
                                  dst_ps, plane_dtype};
        const int st = check_warp_nv12_planes(c);
        int plan_st = 0;
        int64_t tiles = 0;
        if (st == BEVWARP_OK && batch > 0) {
            const TilePlan p = plan_border(batch, dst_h, dst_w, 256, 4);
            plan_st = p.status, tiles = p.status == BEVWARP_OK ? p.total_tiles : 0;
        }
        printf("%d %d %d %" PRId64 "\n", st, (int)nv12_planes_wide_stores_ok(c), plan_st, tiles);
    }
    return 0;
}
