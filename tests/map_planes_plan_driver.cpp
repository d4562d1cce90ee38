// map_planes_plan_driver.cpp -- the host side of bevwarp_remap_planes, bevwarp_stitch_maps_planes and bevwarp_stitch_maps_nv12_planes
// (bev_amd/csrc/host_plan.h: remap_planes_call, stitch_check over stitch_maps_planes_call, plan_remap) from the command line, for
// tests/test_map_planes_cpu.py, which builds it with g++ under the address and undefined-behaviour sanitizers.  One case per line of
// stdin, one line of numbers per case on stdout.  The calls are built as bevwarp_api.hip builds them (a base of 0 is a null pointer; no
// pointer is dereferenced but the camera array and the border value, scale and bias, which are HOST):
//   planes         src dst xy frac batch src_h src_w dst_h dst_w src_fs src_rs dst_fs dst_ps dst_rs map_count xy_fs xy_rs frac_fs frac_rs interp
//                  mode plane_dtype
//       -> check_call's status, then plan_remap's status, frames_per_item and total_tiles (256 x 4 tiles, at most 2 frames per item, 4096
//          items to fill: the library's values) where the call goes on to a launch, else 0 0 0
//   sbgr | snv12   n_cams cams_null dst batch dst_h dst_w dst_fs dst_ps dst_rs interp blend feather rgb plane_dtype border scale bias listed
//                  then per described camera (`listed` of them, which may differ from n_cams):
//                    src uv src_h src_w fs rs uv_fs uv_rs xy frac xy_fs xy_rs frac_fs frac_rs map_count
//       border, scale, bias: 0 = NULL, 1 = finite values, 2 = a NaN in the last of the 3 channels
//       -> the status, then the plan's status and total_tiles where the status is BEVWARP_OK, else 0 0
#include "plan_driver_io.h"

int main() {
    return run_cases([](const std::string& cmd, std::istream& in, const std::string& line) {
        if (cmd == "planes") {
            uint64_t src = 0, dst = 0, xy = 0, frac = 0;
            Frames fs = {}, fd = {}, mx = {}, mf = {};
            Sizes z = {};
            int64_t dst_ps;
            int map_count, interp, mode, plane_dtype;
            in >> src >> dst >> xy >> frac >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w >> fs.fs >> fs.rs >> fd.fs >> dst_ps >> fd.rs >> map_count >> mx.fs >>
                mx.rs >> mf.fs >> mf.rs >> interp >> mode >> plane_dtype;
            if (!in) return malformed(line);
            fs.base = ptr(src), fd.base = ptr(dst), mx.base = ptr(xy), mf.base = ptr(frac);
            const Call c = remap_planes_call(fs, fd, dst_ps, mx, mf, z, map_count, interp, mode, plane_dtype);
            const int st = check_call(c);
            RemapPlan p = {};
            const bool launches = st == BEVWARP_OK && c.batch > 0;
            if (launches) p = plan_remap(c.batch, map_count, c.dst_h, c.dst_w, 256, 4, 2, kRemapFillItems);
            const bool ok = launches && p.status == BEVWARP_OK;
            printf("%d %d %d %" PRId64 "\n", st, p.status, ok ? p.frames_per_item : 0, ok ? p.total_tiles : 0);
        } else if (cmd == "sbgr" || cmd == "snv12") {
            const bool nv12 = cmd == "snv12";
            bevwarp_map_camera cams[16] = {};
            uint64_t dst = 0;
            Frames fd = {};
            int64_t dst_ps;
            int n_cams, cams_null, batch, dst_h, dst_w, interp, blend, feather, rgb, plane_dtype, border, scale, bias, listed;
            in >> n_cams >> cams_null >> dst >> batch >> dst_h >> dst_w >> fd.fs >> dst_ps >> fd.rs >> interp >> blend >> feather >> rgb >> plane_dtype >> border >> scale >>
                bias >> listed;
            fd.base = ptr(dst);
            if (!read_map_cameras(in, listed, cams)) return malformed(line);
            double bv[3] = {1.0, 2.0, 3.0}, sc[3] = {0.5, 0.25, 2.0}, bi[3] = {-1.0, 0.0, 1.0};
            if (border == 2) bv[2] = NAN;
            if (scale == 2) sc[2] = NAN;
            if (bias == 2) bi[2] = NAN;
            TilePlan p = {};
            Call calls[BEVWARP_STITCH_MAX_CAMERAS];
            const auto describe = [&](const bevwarp_map_camera& k) {
                return stitch_maps_planes_call(nv12, k, fd, dst_ps, batch, dst_h, dst_w, interp, blend, nv12 ? rgb : 0, plane_dtype);
            };
            print_stitch(stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{border ? bv : nullptr, 3}, {scale ? sc : nullptr, 3}, {bias ? bi : nullptr, 3}},
                                      batch, dst_h, dst_w, 256, 4, p, calls),
                         p);
        } else {
            return -1;
        }
        return 0;
    });
}
