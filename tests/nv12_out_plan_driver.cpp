// nv12_out_plan_driver.cpp -- the argument checks of bev_amd/csrc/host_plan.h for the warps into NV12 (check_warp_to_nv12,
// check_warp_nv12_to_nv12) and the launch plan that follows them, for tests/test_nv12_out_cpu.py (built with g++ under the address and
// undefined-behaviour sanitizers).  One case per line of stdin, one line of numbers per case on stdout:
//   bgr  src_base dst_y_base dst_uv_base batch src_h src_w dst_h dst_w src_fs src_rs dy_fs dy_rs duv_fs duv_rs m_count interp rgb_order
//   nv12 y_base uv_base dst_y_base dst_uv_base batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dy_fs dy_rs duv_fs duv_rs m_count interp
//       -> the check's status, wide stores admitted for the Y plane and for the UV plane, plan_border's status and total_tiles
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
        Nv12OutCall c = {};
        uint64_t src = 0, y = 0, uv = 0, dy = 0, duv = 0;
        if (cmd == "bgr") {
            in >> src >> dy >> duv >> c.batch >> c.src_h >> c.src_w >> c.dst_h >> c.dst_w >> c.src_fs >> c.src_rs >> c.dy_fs >> c.dy_rs >> c.duv_fs >> c.duv_rs >>
                c.m_count >> c.interp >> c.rgb_order;
        } else if (cmd == "nv12") {
            c.nv12_src = true;
            in >> y >> uv >> dy >> duv >> c.batch >> c.src_h >> c.src_w >> c.dst_h >> c.dst_w >> c.y_fs >> c.y_rs >> c.uv_fs >> c.uv_rs >> c.dy_fs >> c.dy_rs >>
                c.duv_fs >> c.duv_rs >> c.m_count >> c.interp;
        } else {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        c.src = (const void*)(uintptr_t)src, c.y = (const void*)(uintptr_t)y, c.uv = (const void*)(uintptr_t)uv;
        c.dst_y = (const void*)(uintptr_t)dy, c.dst_uv = (const void*)(uintptr_t)duv, c.minv = minv;
        const int st = c.nv12_src ? check_warp_nv12_to_nv12(c) : check_warp_to_nv12(c);
        int plan_st = 0;
        int64_t tiles = 0;
        if (st == BEVWARP_OK && c.batch > 0) {
            const TilePlan p = plan_border(c.batch, c.dst_h, c.dst_w, 256, 4);
            plan_st = p.status, tiles = p.status == BEVWARP_OK ? p.total_tiles : 0;
        }
        printf("%d %d %d %d %" PRId64 "\n", st, (int)nv12_out_wide_stores_ok(c.dst_y_image()), (int)nv12_out_wide_stores_ok(c.dst_uv_image()), plan_st, tiles);
    }
    return 0;
}
