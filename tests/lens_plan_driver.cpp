// lens_plan_driver.cpp -- the host checks of bevwarp_warp_lens (bev_amd/csrc/host_plan.h: lens_call, lens_status) from the command line,
// for tests/test_lens_cpu.py, which builds it with g++ under the address and undefined-behaviour sanitizers.  One case per line of
// stdin, one line of numbers per case on stdout.  The call is built as bevwarp_api.hip builds it (a base of 0 is a null pointer; no
// pointer is dereferenced):
//   call src dst batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs m_count m_ray_null dtype interp border_mode
//       -> check_call's status, then plan_border's status and total_tiles (kBorderTileW x kBorderTileH) where the call goes on to a
//          launch, else 0 0
//   lens fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 r2_max     (strtod's spellings: inf, -inf, nan)      -> lens_status
//   lens_null                                                                                  -> lens_status of a NULL lens
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

int main() {
    static const double m_ray[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "call") {
            uint64_t src = 0, dst = 0;
            Frames s = {}, d = {};
            Sizes z = {};
            int channels, m_null, dtype, interp, mode;
            in >> src >> dst >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w >> channels >> s.fs >> s.rs >> d.fs >> d.rs >> z.m_count >> m_null >> dtype >> interp >> mode;
            s.base = (const void*)(uintptr_t)src, d.base = (const void*)(uintptr_t)dst;
            z.minv = m_null ? nullptr : m_ray;
            const Call c = lens_call(s, d, z, channels, dtype, interp, mode);
            const int st = check_call(c);
            TilePlan p = {};
            if (st == BEVWARP_OK && c.batch > 0) p = plan_border(c.batch, c.dst_h, c.dst_w, 256, 4);
            printf("%d %d %" PRId64, st, p.status, p.status == BEVWARP_OK ? p.total_tiles : 0);
        } else if (cmd == "lens") {
            double v[13];
            std::string tok;
            for (int i = 0; i < 13; i++) {
                if (!(in >> tok)) break;
                char* end = nullptr;
                v[i] = strtod(tok.c_str(), &end);
                if (end == tok.c_str() || *end) in.setstate(std::ios::failbit);
            }
            if (in) printf("%d", lens_status(v, v[12]));
        } else if (cmd == "lens_null") {
            printf("%d", lens_status(nullptr, 1.0));
        } else {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        if (!in) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        printf("\n");
    }
    return 0;
}
