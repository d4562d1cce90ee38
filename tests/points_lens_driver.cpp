// points_lens_driver.cpp -- the host checks of bevwarp_project_points_lens (bev_amd/csrc/host_plan.h: points_lens_status) from the command
// line, for tests/test_points_lens_cpu.py, which builds it with g++ under the address and undefined-behaviour sanitizers.  One case per
// line of stdin, one status per case on stdout.  Pointers are numbers (0 is a null pointer; none is dereferenced):
//   status in out residual n h direction iters tol_px dtype lens r2_max [12 lens values]
//       h: 0 NULL, 1 the identity, 2 with a NaN, 3 with an inf;  lens: 0 NULL, 1 the 12 values that follow
//       tol_px, r2_max and the lens values in strtod's spellings (inf, -inf, nan, -0.0)
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

static bool number(std::istringstream& in, double& v) {
    std::string tok;
    if (!(in >> tok)) return false;
    char* end = nullptr;
    v = strtod(tok.c_str(), &end);
    return end != tok.c_str() && !*end;
}

int main() {
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd != "status") {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        uint64_t src = 0, dst = 0, res = 0;
        int64_t n = 0;
        int h = 0, direction = 0, iters = 0, dtype = 0, has_lens = 0;
        double tol_px = 0, r2_max = 0, lens[12] = {};
        double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        bool ok = bool(in >> src >> dst >> res >> n >> h >> direction >> iters) && number(in, tol_px) && bool(in >> dtype >> has_lens) && number(in, r2_max);
        for (int i = 0; ok && has_lens && i < 12; i++) ok = number(in, lens[i]);
        if (!ok || h < 0 || h > 3) {
            fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        if (h == 2) H[4] = NAN;
        if (h == 3) H[8] = INFINITY;
        printf("%d\n", points_lens_status((const void*)(uintptr_t)src, (const void*)(uintptr_t)dst, (const void*)(uintptr_t)res, n, h ? H : nullptr,
                                          has_lens ? lens : nullptr, r2_max, direction, iters, tol_px, dtype));
    }
    return 0;
}
