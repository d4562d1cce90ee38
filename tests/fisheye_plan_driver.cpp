// fisheye_plan_driver.cpp -- the host checks of BEVWARP_LENS_FISHEYE (bev_amd/csrc/host_plan.h: take_fisheye_flag, fisheye_status,
// lens_model_status, points_model_status, build_map_model_status) from the command line, for tests/test_fisheye_cpu.py, which builds it
// with g++ under the address and undefined-behaviour sanitizers.  One case per line of stdin, one line of numbers per case on stdout.  The
// calls are built as bevwarp_api.hip builds them (a base of 0 is a null pointer; no pointer is dereferenced):
//   lens fx fy cx cy k1 k2 k3 k4 r0 r1 r2 r3 theta_max   (strtod's spellings: inf, -inf, nan)   -> fisheye_status
//   lens_null                                                                                 -> fisheye_status of a NULL lens
//   flag word                                                                                 -> take_fisheye_flag: the flag, the word left
//   warp interp lens theta_max       (lens: 0 NULL, 1 good, 2 a NaN entry, 3 fx == 0, 4 a reserved entry != 0)
//       -> check_call of lens_call on an 8 x 8 call with the word's flag taken out, then lens_model_status (0 where the call has failed)
//   points in out residual n h lens theta_max direction iters tol_px dtype    (h: 0 NULL, 1 good, 2 a NaN entry)   -> points_model_status, the flag taken out
//   build m xy frac m_count lens theta_max interp dst_h dst_w xy_rs frac_rs                  -> build_map_model_status, the flag taken out
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <limits>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

static double number(std::istringstream& in) {
    std::string tok;
    if (!(in >> tok)) return 0.0;
    char* end = nullptr;
    const double v = strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end) in.setstate(std::ios::failbit);
    return v;
}

static const double* lens_of(int which, double* v) {
    static const double good[12] = {200.0, 204.0, 319.5, 179.5, -0.02, 0.004, -0.001, 0.0002, 0, 0, 0, 0};
    for (int i = 0; i < 12; i++) v[i] = good[i];
    if (which == 2) v[5] = std::numeric_limits<double>::quiet_NaN();
    if (which == 3) v[0] = 0.0;
    if (which == 4) v[10] = 1e-300;
    return which ? v : nullptr;
}

int main() {
    static const double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    static const double m_nan[9] = {1, 0, 0, 0, std::numeric_limits<double>::quiet_NaN(), 0, 0, 0, 1};
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        double v[13];
        if (cmd == "lens") {
            for (int i = 0; i < 13; i++) v[i] = number(in);
            if (in) printf("%d", fisheye_status(v, v[12]));
        } else if (cmd == "lens_null") {
            printf("%d", fisheye_status(nullptr, 1.0));
        } else if (cmd == "flag") {
            int word;
            in >> word;
            const bool f = take_fisheye_flag(word);
            printf("%d %d", (int)f, word);
        } else if (cmd == "warp") {
            int interp, which;
            in >> interp >> which;
            const double theta_max = number(in);
            const bool fisheye = take_fisheye_flag(interp);
            const Call c = lens_call({(const void*)16, 192, 24}, {(const void*)(1 << 20), 192, 24}, {1, 8, 8, 8, 8, 1, m}, 3, BEVWARP_U8, interp, BEVWARP_BORDER_CONSTANT);
            const int st = check_call(c);
            printf("%d %d", st, st == BEVWARP_OK ? lens_model_status(fisheye, lens_of(which, v), theta_max) : 0);
        } else if (cmd == "points") {
            uint64_t src, dst, res;
            int64_t n;
            int h, which, direction, iters, dtype;
            in >> src >> dst >> res >> n >> h >> which;
            const double theta_max = number(in);
            in >> direction >> iters;
            const double tol = number(in);
            in >> dtype;
            const bool fisheye = take_fisheye_flag(direction);
            printf("%d", points_model_status(fisheye, (const void*)(uintptr_t)src, (const void*)(uintptr_t)dst, (const void*)(uintptr_t)res, n, h == 0 ? nullptr : (h == 2 ? m_nan : m),
                                             lens_of(which, v), theta_max, direction, iters, tol, dtype));
        } else if (cmd == "build") {
            uint64_t mp, xy, frac;
            int m_count, which, interp, dst_h, dst_w;
            Frames fxy = {}, ffr = {};
            in >> mp >> xy >> frac >> m_count >> which;
            const double theta_max = number(in);
            in >> interp >> dst_h >> dst_w >> fxy.rs >> ffr.rs;
            fxy.base = (const void*)(uintptr_t)xy, ffr.base = (const void*)(uintptr_t)frac;
            fxy.fs = (int64_t)dst_h * fxy.rs, ffr.fs = (int64_t)dst_h * ffr.rs;
            const bool fisheye = take_fisheye_flag(interp);
            TilePlan p;
            const int st = build_map_model_status(fisheye, mp ? m : nullptr, m_count, lens_of(which, v), theta_max, interp, fxy, ffr, dst_h, dst_w, 256, 4, p);
            printf("%d %" PRId64, st, st == BEVWARP_OK ? p.total_tiles : 0);
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
