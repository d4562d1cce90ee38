// remap_cubic_plan_driver.cpp -- the host checks of BEVWARP_MAP_BICUBIC (bev_amd/csrc/host_plan.h: take_map_bicubic_flag, remap_call) from the
// command line, for tests/test_remap_cubic_cpu.py, which builds it with g++ under the address and undefined-behaviour sanitizers.  One case
// per line of stdin, one line of numbers per case on stdout.  The calls are built as bevwarp_api.hip builds them (a base of 0 is a null
// pointer; no pointer is dereferenced):
//   flag word                        -> take_map_bicubic_flag: the flag, the word left
//   call src dst xy frac batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs map_count xy_fs xy_rs frac_fs frac_rs dtype interp mode
//       -> bevwarp_remap's checks with the word's flag taken out: the flag, check_call's status, then plan_remap's status, frames_per_item
//          and total_tiles (256 x 4 tiles, at most 8 frames per item, 4096 items to fill) where the call goes on to a launch, else 0 0 0
//   other entry interp               (entry: build, nv12, nv12_planes, to_nv12, nv12_to_nv12, planes, stitch, stitch_nv12)
//       -> the status of that entry's checks on a good 8 x 8 call with `interp` as its word (no entry but bevwarp_remap takes the flag out)
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
        if (cmd == "flag") {
            int word;
            in >> word;
            const bool f = take_map_bicubic_flag(word);
            printf("%d %d", (int)f, word);
        } else if (cmd == "call") {
            uint64_t src = 0, dst = 0, xy = 0, frac = 0;
            Frames s = {}, d = {}, mx = {}, mf = {};
            Sizes z = {};
            int channels, map_count, dtype, interp, mode;
            in >> src >> dst >> xy >> frac >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w >> channels >> s.fs >> s.rs >> d.fs >> d.rs >> map_count >> mx.fs >> mx.rs >>
                mf.fs >> mf.rs >> dtype >> interp >> mode;
            s.base = (const void*)(uintptr_t)src, d.base = (const void*)(uintptr_t)dst, mx.base = (const void*)(uintptr_t)xy, mf.base = (const void*)(uintptr_t)frac;
            const bool bicubic = take_map_bicubic_flag(interp);
            const Call c = remap_call(s, d, mx, mf, z, map_count, channels, dtype, interp, mode, bicubic);
            const int st = check_call(c);
            RemapPlan p = {};
            const bool launches = st == BEVWARP_OK && c.batch > 0;
            if (launches) p = plan_remap(c.batch, map_count, c.dst_h, c.dst_w, 256, 4, 8, kRemapFillItems);
            const bool ok = launches && p.status == BEVWARP_OK;
            printf("%d %d %d %d %" PRId64, (int)bicubic, st, p.status, ok ? p.frames_per_item : 0, ok ? p.total_tiles : 0);
        } else if (cmd == "other") {
            std::string entry;
            int interp;
            in >> entry >> interp;
            const Frames src = {(const void*)16, 192, 24}, y = {(const void*)16, 64, 8}, uv = {(const void*)4096, 32, 8};
            const Frames dst = {(const void*)(1 << 20), 192, 24}, dy = {(const void*)(1 << 20), 64, 8}, duv = {(const void*)(1 << 21), 32, 8};
            const Frames planes = {(const void*)(1 << 20), 768, 32};
            const Frames xy = {(const void*)(1 << 24), 256, 32}, fr = {(const void*)(1 << 26), 128, 16};
            const Sizes z = {1, 8, 8, 8, 8, 0, nullptr};
            bevwarp_map_camera k = {};
            k.src = src.base, k.frame_stride = 192, k.row_stride = 24, k.map_xy = xy.base, k.map_frac = fr.base;
            k.xy_frame_stride = 256, k.xy_row_stride = 32, k.frac_frame_stride = 128, k.frac_row_stride = 16, k.src_h = 8, k.src_w = 8, k.map_count = 1;
            int st = 1;
            if (entry == "build") {
                TilePlan p = {};
                st = build_map_status(m, 1, nullptr, 0.0, interp, xy, fr, 8, 8, 256, 4, p);
            } else if (entry == "nv12") {
                st = check_call(remap_nv12_call(y, uv, dst, xy, fr, z, 1, interp, 0, BEVWARP_BORDER_CONSTANT));
            } else if (entry == "nv12_planes") {
                st = check_call(remap_nv12_planes_call(y, uv, planes, 256, xy, fr, z, 1, interp, 0, BEVWARP_BORDER_CONSTANT, BEVWARP_F32));
            } else if (entry == "to_nv12") {
                st = check_call(remap_to_nv12_call(src, dy, duv, xy, fr, z, 1, interp, 0, BEVWARP_BORDER_CONSTANT));
            } else if (entry == "nv12_to_nv12") {
                st = check_call(remap_nv12_to_nv12_call(y, uv, dy, duv, xy, fr, z, 1, interp, BEVWARP_BORDER_CONSTANT));
            } else if (entry == "planes") {
                st = check_call(remap_planes_call(src, planes, 256, xy, fr, z, 1, interp, BEVWARP_BORDER_CONSTANT, BEVWARP_F32));
            } else if (entry == "stitch") {
                st = check_call(stitch_maps_call(k, dst, 1, 8, 8, 3, BEVWARP_U8, interp, BEVWARP_STITCH_OVER, BEVWARP_BORDER_CONSTANT));
            } else if (entry == "stitch_nv12") {
                k.src = y.base, k.frame_stride = 64, k.row_stride = 8, k.uv = uv.base, k.uv_frame_stride = 32, k.uv_row_stride = 8;
                st = check_call(stitch_maps_nv12_call(k, dst, 1, 8, 8, interp, BEVWARP_STITCH_OVER, 0, BEVWARP_BORDER_CONSTANT));
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
