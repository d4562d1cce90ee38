// remap_plan_driver.cpp -- the host side of bevwarp_remap and bevwarp_build_map (bev_amd/csrc/host_plan.h: remap_call, plan_remap,
// build_map_status) from the command line, for tests/test_remap_cpu.py, which builds it with g++ under the address and
// undefined-behaviour sanitizers.  One case per line of stdin, one line of numbers per case on stdout.  The calls are built as
// bevwarp_api.hip builds them (a base of 0 is a null pointer; no pointer is dereferenced but the lens, which is HOST):
//   call src dst xy frac batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs map_count xy_fs xy_rs frac_fs frac_rs dtype interp mode
//       -> check_call's status, then plan_remap's status, frames_per_item and total_tiles (256 x 4 tiles, at most 8 frames per item -- the
//          library's own bound is lower --, 4096 items to fill) where the call goes on to a launch, else 0 0 0
//   plan batch map_count dst_h dst_w max_fpi fill
//       -> plan_remap's status, frames_per_item, groups, total_tiles, and `covered`: 1 when decoding every item t of the grid as the
//          kernel does -- group t / tiles_per_frame, tile t mod tiles_per_frame, frames group * fpi ... min(batch, (group + 1) * fpi) - 1
//          -- visits every (frame, tile) exactly once (checked item by item: keep batch * tiles small), else 0
//   build m_null m_count lens(0 none, 1 good, 2 NaN entry) r2_max interp xy frac dst_h dst_w xy_fs xy_rs frac_fs frac_rs
//       -> build_map_status's status, then the plan's total_tiles where the status is BEVWARP_OK, else 0
#include <inttypes.h>
#include <math.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host_plan.h"

using namespace bevwarp::plan;

int main() {
    static const double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "call") {
            uint64_t src = 0, dst = 0, xy = 0, frac = 0;
            Frames s = {}, d = {}, mx = {}, mf = {};
            Sizes z = {};
            int channels, map_count, dtype, interp, mode;
            in >> src >> dst >> xy >> frac >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w >> channels >> s.fs >> s.rs >> d.fs >> d.rs >> map_count >> mx.fs >> mx.rs >>
                mf.fs >> mf.rs >> dtype >> interp >> mode;
            s.base = (const void*)(uintptr_t)src, d.base = (const void*)(uintptr_t)dst, mx.base = (const void*)(uintptr_t)xy, mf.base = (const void*)(uintptr_t)frac;
            const Call c = remap_call(s, d, mx, mf, z, map_count, channels, dtype, interp, mode);
            const int st = check_call(c);
            RemapPlan p = {};
            const bool launches = st == BEVWARP_OK && c.batch > 0;
            if (launches) p = plan_remap(c.batch, map_count, c.dst_h, c.dst_w, 256, 4, 8, kRemapFillItems);
            const bool ok = launches && p.status == BEVWARP_OK;
            printf("%d %d %d %" PRId64, st, p.status, ok ? p.frames_per_item : 0, ok ? p.total_tiles : 0);
        } else if (cmd == "plan") {
            int batch, map_count, dst_h, dst_w, max_fpi;
            int64_t fill;
            in >> batch >> map_count >> dst_h >> dst_w >> max_fpi >> fill;
            if (!in) {
                fprintf(stderr, "malformed case: %s\n", line.c_str());
                return 2;
            }
            const RemapPlan p = plan_remap(batch, map_count, dst_h, dst_w, 256, 4, max_fpi, fill);
            int covered = 0;
            if (p.status == BEVWARP_OK && (int64_t)batch * p.tiles_per_frame <= (1 << 24)) {
                std::vector<int> seen((size_t)batch * p.tiles_per_frame, 0);
                bool in_range = p.total_tiles == (int64_t)p.groups * p.tiles_per_frame && p.frames_per_item >= 1 && p.frames_per_item <= max_fpi;
                for (int64_t t = 0; t < p.total_tiles && in_range; t++) {
                    const int64_t g = t / p.tiles_per_frame, tile = t % p.tiles_per_frame;
                    const int64_t b0 = g * p.frames_per_item, b1 = b0 + p.frames_per_item < batch ? b0 + p.frames_per_item : batch;
                    if (b0 >= batch) in_range = false;
                    for (int64_t b = b0; b < b1; b++) seen[(size_t)(b * p.tiles_per_frame + tile)]++;
                }
                covered = in_range;
                for (int v : seen) covered = covered && v == 1;
            }
            printf("%d %d %d %" PRId64 " %d", p.status, p.status == BEVWARP_OK ? p.frames_per_item : 0, p.status == BEVWARP_OK ? p.groups : 0,
                   p.status == BEVWARP_OK ? p.total_tiles : 0, covered);
        } else if (cmd == "build") {
            uint64_t xy = 0, frac = 0;
            Frames mx = {}, mf = {};
            int m_null, m_count, lens_kind, interp, dst_h, dst_w;
            std::string r2s;
            in >> m_null >> m_count >> lens_kind >> r2s >> interp >> xy >> frac >> dst_h >> dst_w >> mx.fs >> mx.rs >> mf.fs >> mf.rs;
            if (!in) {
                fprintf(stderr, "malformed case: %s\n", line.c_str());
                return 2;
            }
            const double r2_max = strtod(r2s.c_str(), nullptr);
            mx.base = (const void*)(uintptr_t)xy, mf.base = (const void*)(uintptr_t)frac;
            double lens[12] = {800.0, 810.0, 319.5, 239.5, -0.3, 0.1, 0.001, -0.0005, -0.01, 0.9, -0.3, 0.02};
            if (lens_kind == 2) lens[5] = NAN;
            TilePlan p = {};
            const int st = build_map_status(m_null ? nullptr : m, m_count, lens_kind ? lens : nullptr, r2_max, interp, mx, mf, dst_h, dst_w, 256, 4, p);
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
