// plan_driver_io.h -- what the families of tests/host_plan_driver.cpp share: the loop over the case lines of stdin with its two error
// exits, the readers of a line's fields and the printers of a case's line.  On a line a pointer is a number (0: a null pointer; none is
// dereferenced) and a double is in strtod's spellings (inf, -inf, nan, -0.0).
#pragma once
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

// One case per line of stdin: one_case(cmd, in) reads the line's fields after the command word from `in` and prints the case's numbers;
// it returns -1 for a command word it does not know, and leaves `in` failed for a line it cannot read.  Blank lines are skipped.  The
// driver's exit status.
template <class OneCase>
int run_cases(OneCase one_case) {
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (one_case(cmd, in) < 0) {
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
inline void malformed(std::istream& in) { in.setstate(std::ios::failbit); }

// ---- readers ---------------------------------------------------------------------------------------------------------------------------------
inline const void* read_ptr(std::istream& in) {
    uint64_t v = 0;
    in >> v;
    return (const void*)(uintptr_t)v;
}
inline double read_number(std::istream& in) {
    std::string tok;
    if (!(in >> tok)) return 0.0;
    char* end = nullptr;
    const double v = strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end) malformed(in);
    return v;
}
// Frames as the lines have them: the bases of all images first, the strides (frame, row) after the sizes
template <class... F>
void read_bases(std::istream& in, F&... f) {
    ((f.base = read_ptr(in)), ...);
}
template <class... F>
void read_strides(std::istream& in, F&... f) {
    ((in >> f.fs >> f.rs), ...);
}
// batch src_h src_w dst_h dst_w (the matrix count follows the strides)
inline Sizes read_sizes(std::istream& in, const double* minv = nullptr) {
    Sizes z = {};
    in >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w;
    z.minv = minv;
    return z;
}
// The `listed` described cameras of a stitch through maps into cams[16], each as
//   src uv src_h src_w fs rs uv_fs uv_rs xy frac xy_fs xy_rs frac_fs frac_rs map_count        and, with_reserved, its `reserved` word
// A line whose fields before the cameras could not be read, or whose `listed` is out of range, is malformed.
inline void read_map_cameras(std::istream& in, int listed, bevwarp_map_camera* cams, bool with_reserved = false) {
    if (!in || listed < 0 || listed > 16) return malformed(in);
    for (int k = 0; k < listed; k++) {
        bevwarp_map_camera& c = cams[k];
        c.src = read_ptr(in), c.uv = read_ptr(in);
        in >> c.src_h >> c.src_w >> c.frame_stride >> c.row_stride >> c.uv_frame_stride >> c.uv_row_stride;
        c.map_xy = read_ptr(in), c.map_frac = read_ptr(in);
        in >> c.xy_frame_stride >> c.xy_row_stride >> c.frac_frame_stride >> c.frac_row_stride >> c.map_count;
        if (with_reserved) in >> c.reserved;
    }
}
// A border value, scale or bias (HOST) as a line selects it: 0 = NULL, 1 = the n finite values of v, 2 = a NaN in the last of them
inline const double* selected(int which, double* v, int n) {
    if (which == 2 && n >= 1 && n <= 4) v[n - 1] = NAN;
    return which ? v : nullptr;
}

// ---- printers --------------------------------------------------------------------------------------------------------------------------------
inline void print_plan(const TilePlan& p) {
    printf("%d %d %d %d %" PRId64 " %d %d %d %d %u %u %u", p.status, p.tile_h, p.tiles_x, p.tiles_per_frame, p.total_tiles, p.chunk, p.stagger, p.tail_split, p.bw0,
           p.tpf_magic, p.tx_magic, p.bw0_magic);
}
// a stitch's line: the status, then the plan's status and total_tiles where the status is BEVWARP_OK, else 0 0
inline void print_stitch(int st, const TilePlan& p) { printf("%d %d %" PRId64, st, st == BEVWARP_OK ? p.status : 0, st == BEVWARP_OK ? p.total_tiles : 0); }
// A checked call's line (st, p: flat_grid's, remap_grid's or supersample_grid's): the status, the family's `wide` flags, then the plan's
// status, its `field` (frames_per_item or bw0; below 0: none) and total_tiles -- zeros where the call does not go on to a launch, the last
// two also where the plan has failed
inline void print_checked(int st, const TilePlan& p, int field = -1, std::initializer_list<int> wide = {}) {
    const bool ok = p.status == BEVWARP_OK;
    printf("%d ", st);
    for (int w : wide) printf("%d ", w);
    printf("%d ", p.status);
    if (field >= 0) printf("%d ", ok ? field : 0);
    printf("%" PRId64, ok ? p.total_tiles : 0);
}
