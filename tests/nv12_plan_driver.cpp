// nv12_plan_driver.cpp -- the argument checks of bev_amd/csrc/host_plan.h for an NV12 warp (check_warp_nv12) and the launch plan that
// follows them, for tests/test_nv12_cpu.py (built with g++ under the address and undefined-behaviour sanitizers).  One case per line of
// stdin, one line of numbers per case on stdout:
//   nv12 y_base uv_base dst_base batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_rs m_count interp rgb_order
//       -> check_warp_nv12's status, wide stores admitted (wide_stores_ok of the destination), plan_border's status and total_tiles
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
        if (cmd != "nv12") {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        uint64_t y, uv, dst;
        int batch, src_h, src_w, dst_h, dst_w, m_count, interp, rgb;
        int64_t y_fs, y_rs, uv_fs, uv_rs, dst_fs, dst_rs;
        in >> y >> uv >> dst >> batch >> src_h >> src_w >> dst_h >> dst_w >> y_fs >> y_rs >> uv_fs >> uv_rs >> dst_fs >> dst_rs >> m_count >> interp >> rgb;
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        // (positional, as bevwarp_api.hip fills it)
        const Nv12Call c = {(const void*)(uintptr_t)y, (const void*)(uintptr_t)uv, (const void*)(uintptr_t)dst, batch, src_h, src_w, dst_h, dst_w,
                            y_fs, y_rs, uv_fs, uv_rs, dst_fs, dst_rs, minv, m_count, interp, rgb};
        const int st = check_warp_nv12(c);
        int plan_st = 0;
        int64_t tiles = 0;
        if (st == BEVWARP_OK && batch > 0) {
            const TilePlan p = plan_border(batch, dst_h, dst_w, 256, 4);
            plan_st = p.status, tiles = p.status == BEVWARP_OK ? p.total_tiles : 0;
        }
        printf("%d %d %d %" PRId64 "\n", st, (int)wide_stores_ok(c.dst_image(), store_align(BEVWARP_U8, 3, false)), plan_st, tiles);
    }
    return 0;
}
