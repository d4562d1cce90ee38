// remap_nv12_plan_driver.cpp -- the host side of bevwarp_remap_nv12 and bevwarp_remap_nv12_planes (bev_amd/csrc/host_plan.h:
// remap_nv12_call, remap_nv12_planes_call, plan_remap) from the command line, for tests/test_remap_nv12_cpu.py, which builds it with g++
// under the address and undefined-behaviour sanitizers.  One case per line of stdin, one line of numbers per case on stdout.  The calls
// are built as bevwarp_api.hip builds them (a base of 0 is a null pointer; no pointer is dereferenced):
//   pix    y uv dst xy frac batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_rs map_count xy_fs xy_rs frac_fs frac_rs interp mode rgb
//   planes y uv dst xy frac batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_ps dst_rs map_count xy_fs xy_rs frac_fs frac_rs interp mode rgb plane_dtype
//       -> check_call's status, then plan_remap's status, frames_per_item and total_tiles (256 x 4 tiles, at most 2 frames per item, 4096
//          items to fill: the library's values) where the call goes on to a launch, else 0 0 0
#include <inttypes.h>
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
        if (cmd != "pix" && cmd != "planes") {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        const bool planes = cmd == "planes";
        uint64_t y = 0, uv = 0, dst = 0, xy = 0, frac = 0;
        Frames fy = {}, fuv = {}, d = {}, mx = {}, mf = {};
        Sizes z = {};
        int64_t dst_ps = 0;
        int map_count, interp, mode, rgb, plane_dtype = 0;
        in >> y >> uv >> dst >> xy >> frac >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w >> fy.fs >> fy.rs >> fuv.fs >> fuv.rs >> d.fs;
        if (planes) in >> dst_ps;
        in >> d.rs >> map_count >> mx.fs >> mx.rs >> mf.fs >> mf.rs >> interp >> mode >> rgb;
        if (planes) in >> plane_dtype;
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        fy.base = (const void*)(uintptr_t)y, fuv.base = (const void*)(uintptr_t)uv, d.base = (const void*)(uintptr_t)dst;
        mx.base = (const void*)(uintptr_t)xy, mf.base = (const void*)(uintptr_t)frac;
        const Call c = planes ? remap_nv12_planes_call(fy, fuv, d, dst_ps, mx, mf, z, map_count, interp, rgb, mode, plane_dtype)
                              : remap_nv12_call(fy, fuv, d, mx, mf, z, map_count, interp, rgb, mode);
        const int st = check_call(c);
        RemapPlan p = {};
        const bool launches = st == BEVWARP_OK && c.batch > 0;
        if (launches) p = plan_remap(c.batch, map_count, c.dst_h, c.dst_w, 256, 4, 2, kRemapFillItems);
        const bool ok = launches && p.status == BEVWARP_OK;
        printf("%d %d %d %" PRId64 "\n", st, p.status, ok ? p.frames_per_item : 0, ok ? p.total_tiles : 0);
    }
    return 0;
}
