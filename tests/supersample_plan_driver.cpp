// supersample_plan_driver.cpp -- the host checks of BEVWARP_SUPERSAMPLE_* (bev_amd/csrc/host_plan.h: take_supersample, border_mode_known,
// supersample_call, plan_supersample) from the command line, for tests/test_supersample_cpu.py, which builds it with g++ under the address
// and undefined-behaviour sanitizers.  One case per line of stdin, one line of numbers per case on stdout.  The calls are built as
// bevwarp_api.hip builds them (a base of 0 is a null pointer; no pointer is dereferenced):
//   field word                       -> take_supersample: k, the word left
//   call src dst minv batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs m_count dtype interp mode
//       -> bevwarp_warp_border's checks of a word that carries the field (k > 1; anything else is a malformed case): k, the status -- an
//          unknown border mode first, then check_call of supersample_call --, then plan_supersample's status, bw0 and total_tiles
//          (256 x 4 tiles) where the call goes on to a launch, else 0 0 0
//   other entry interp               (entry: warp, lens, remap, build)
//       -> the status of that entry's checks on a good 8 x 8 call with `interp` as its word (no entry but bevwarp_warp_border takes the
//          field out)
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

int main() {
    static const double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "field") {
            int word;
            in >> word;
            const int k = take_supersample(word);
            printf("%d %d", k, word);
        } else if (cmd == "call") {
            uint64_t src = 0, dst = 0, minv = 0;
            Frames s = {}, d = {};
            Sizes z = {};
            int channels, dtype, interp, mode;
            in >> src >> dst >> minv >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w >> channels >> s.fs >> s.rs >> d.fs >> d.rs >> z.m_count >> dtype >> interp >> mode;
            s.base = (const void*)(uintptr_t)src, d.base = (const void*)(uintptr_t)dst, z.minv = (const double*)(uintptr_t)minv;
            const int k = take_supersample(interp);
            if (k == 1) in.setstate(std::ios::failbit);
            int st = BEVWARP_ERR_UNSUPPORTED;
            TilePlan p = {};
            bool ok = false;
            if (border_mode_known(mode)) {
                const Call c = supersample_call(s, d, z, channels, dtype, interp, mode, k);
                st = check_call(c);
                if (st == BEVWARP_OK && c.batch > 0) {
                    p = plan_supersample(c.batch, c.dst_h, c.dst_w, 256, 4, k);
                    ok = p.status == BEVWARP_OK;
                }
            }
            printf("%d %d %d %d %" PRId64, k, st, p.status, ok ? p.bw0 : 0, ok ? p.total_tiles : 0);
        } else if (cmd == "other") {
            std::string entry;
            int interp;
            in >> entry >> interp;
            const Frames src = {(const void*)16, 192, 24}, dst = {(const void*)(1 << 20), 192, 24};
            const Frames xy = {(const void*)(1 << 24), 256, 32}, fr = {(const void*)(1 << 26), 128, 16};
            const Sizes z = {1, 8, 8, 8, 8, 1, m};
            int st = 1;
            if (entry == "warp") {
                st = check_call(warp_call(src, dst, z, 3, BEVWARP_U8, interp, false));
            } else if (entry == "lens") {
                int word = interp;
                take_fisheye_flag(word);
                st = check_call(lens_call(src, dst, z, 3, BEVWARP_U8, word, BEVWARP_BORDER_CONSTANT));
            } else if (entry == "remap") {
                int word = interp;
                const bool bicubic = take_map_bicubic_flag(word);
                st = check_call(remap_call(src, dst, xy, fr, z, 1, 3, BEVWARP_U8, word, BEVWARP_BORDER_CONSTANT, bicubic));
            } else if (entry == "build") {
                TilePlan p = {};
                int word = interp;
                const bool fisheye = take_fisheye_flag(word);
                static const double lens[12] = {100, 100, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0};
                st = build_map_model_status(fisheye, m, 1, fisheye ? lens : nullptr, 1.0, word, xy, fr, 8, 8, 256, 4, p);
            } else {
                in.setstate(std::ios::failbit);
            }
            printf("%d", st);
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
