// plan_driver_io.h -- what the stand-alone drivers of the stitches (stitch_plan_driver.cpp, stitch_maps_plan_driver.cpp,
// remap_nv12_out_plan_driver.cpp, map_planes_plan_driver.cpp) share: the loop over the case lines of stdin, the reading of a pointer and of
// a bevwarp_map_camera, and the printed line of a stitch.  Each driver keeps its own command words and its own line formats.
#pragma once
#include <inttypes.h>
#include <math.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

inline const void* ptr(uint64_t v) { return (const void*)(uintptr_t)v; }  // (a base of 0 is a null pointer)

inline int malformed(const std::string& line) {
    fprintf(stderr, "malformed case: %s\n", line.c_str());
    return 2;
}

// One case per line of stdin: one_case(cmd, in, line) reads the line's fields after the command word from `in`, prints the case's line of
// numbers and returns 0; it returns malformed(line) for a line it cannot read and -1 for a command word it does not know.  Blank lines
// are skipped.  The driver's exit status.
template <class OneCase>
int run_cases(OneCase one_case) {
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        const int r = one_case(cmd, in, line);
        if (r < 0) fprintf(stderr, "unknown case: %s\n", line.c_str());
        if (r) return 2;
    }
    return 0;
}

// The `listed` described cameras of a stitch through maps, each as
//   src uv src_h src_w fs rs uv_fs uv_rs xy frac xy_fs xy_rs frac_fs frac_rs map_count
// into cams[16]; false: the line is malformed -- the fields before the cameras or the cameras could not be read, or listed is out of range.
inline bool read_map_cameras(std::istream& in, int listed, bevwarp_map_camera* cams) {
    if (!in || listed < 0 || listed > 16) return false;
    for (int k = 0; k < listed; k++) {
        uint64_t src = 0, uv = 0, xy = 0, frac = 0;
        bevwarp_map_camera& c = cams[k];
        in >> src >> uv >> c.src_h >> c.src_w >> c.frame_stride >> c.row_stride >> c.uv_frame_stride >> c.uv_row_stride >> xy >> frac >> c.xy_frame_stride >>
            c.xy_row_stride >> c.frac_frame_stride >> c.frac_row_stride >> c.map_count;
        c.src = ptr(src), c.uv = ptr(uv), c.map_xy = ptr(xy), c.map_frac = ptr(frac);
    }
    return (bool)in;
}

// a stitch's line: the status, then the plan's status and total_tiles where the status is BEVWARP_OK, else 0 0
inline void print_stitch(int st, const TilePlan& p) { printf("%d %d %" PRId64 "\n", st, st == BEVWARP_OK ? p.status : 0, st == BEVWARP_OK ? p.total_tiles : 0); }
