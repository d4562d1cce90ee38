// planes16_plan_driver.cpp -- the argument checks and the wide-store decision of bev_amd/csrc/host_plan.h for channel planes of 2-byte
// (and 4-byte) elements, for tests/test_planes16_cpu.py (built with g++ under the address and undefined-behaviour sanitizers).  One case
// per line of stdin, one line of numbers per case on stdout:
//   planes src_base dst_base batch channels dst_h dst_w frame_stride plane_stride row_stride plane_elem
//       -> check_warp's status, store_align, call_wide_stores_ok, bytes of a destination row (dst_image().row_bytes)
// The source is batch frames of 8 x 8 pixels, `channels` 8-bit values each, tightly packed at src_base.
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
        if (cmd != "planes") {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        uint64_t src_base, dst_base;
        int batch, channels, dst_h, dst_w, elem;
        int64_t fs, ps, rs;
        in >> src_base >> dst_base >> batch >> channels >> dst_h >> dst_w >> fs >> ps >> rs >> elem;
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        // (positional, as bevwarp_api.hip fills it; the plane element size is the trailing member)
        WarpCall c = {{(const void*)(uintptr_t)src_base, 8, 8, (int64_t)64 * channels, (int64_t)8 * channels}, {(const void*)(uintptr_t)dst_base, dst_h, dst_w, fs, rs}, batch, channels,
                      BEVWARP_U8, BEVWARP_LINEAR, minv, 1, nullptr, nullptr, true, ps, nullptr, nullptr};
        const WarpCall f32_default = c;
        if (f32_default.plane_elem != 4) return 3;  // the member defaults to the float32 case
        c.plane_elem = elem;
        printf("%d %d %d %" PRIu64 "\n", check_warp(c), store_align(c.dtype, c.channels, c.planar, c.plane_elem), (int)call_wide_stores_ok(c), c.dst_image().row_bytes);
    }
    return 0;
}
