// host_plan_driver.cpp -- bev_amd/csrc/host_plan.h from the command line, for tests/test_host_plan.py (built with g++ under the
// address and undefined-behaviour sanitizers).  One case per line of stdin, one line of numbers per case on stdout:
//   rows batch dst_h dst_w dtype tw rpp resident        -> status tile_h tiles_x tiles_per_frame total_tiles chunk stagger tail_split bw0 tpf_magic tx_magic bw0_magic
//   composite dst_h dst_w tw rpp max_rows cus           -> the same
//   border batch dst_h dst_w tw th mode src_h src_w     -> the same, then per_x off_x mag_x per_y off_y mag_y
//   overlap s(base rows row_bytes rs fs) d(...) batch   -> 0 | 1
//   layout base rows row_bytes rs fs batch elem         -> status
//   size rows cols rs max_rows max_cols mul24           -> status
//   magic n_max d                                       -> magic, and how many n <= n_max it divides wrongly (-1: "divide")
//   magic_at n d                                        -> magic, quotient by it (by division when the magic is 0), n / d
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "host_plan.h"

using namespace bevwarp::plan;

static uint32_t fast_div(uint32_t n, uint32_t d, uint32_t magic) { return magic ? (uint32_t)(((uint64_t)n * magic) >> 32) : n / d; }  // (coords.h)

static void print_plan(const TilePlan& p) {
    printf("%d %d %d %d %" PRId64 " %d %d %d %d %u %u %u", p.status, p.tile_h, p.tiles_x, p.tiles_per_frame, p.total_tiles, p.chunk, p.stagger, p.tail_split, p.bw0,
           p.tpf_magic, p.tx_magic, p.bw0_magic);
}

static Image read_image(std::istream& in) {
    Image im = {};
    in >> im.base >> im.rows >> im.row_bytes >> im.rs >> im.fs;
    return im;
}

int main() {
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "rows") {
            int batch, dst_h, dst_w, dtype, tw, rpp;
            int64_t resident;
            in >> batch >> dst_h >> dst_w >> dtype >> tw >> rpp >> resident;
            print_plan(plan_rows(batch, dst_h, dst_w, dtype, tw, rpp, resident));
        } else if (cmd == "composite") {
            int dst_h, dst_w, tw, rpp, max_rows;
            int64_t cus;
            in >> dst_h >> dst_w >> tw >> rpp >> max_rows >> cus;
            print_plan(plan_composite(dst_h, dst_w, tw, rpp, max_rows, cus));
        } else if (cmd == "border") {
            int batch, dst_h, dst_w, tw, th, mode, src_h, src_w;
            in >> batch >> dst_h >> dst_w >> tw >> th >> mode >> src_h >> src_w;
            print_plan(plan_border(batch, dst_h, dst_w, tw, th));
            const BorderPeriod x = border_period(mode, src_w), y = border_period(mode, src_h);
            printf(" %u %u %u %u %u %u", x.per, x.off, x.mag, y.per, y.off, y.mag);
        } else if (cmd == "overlap") {
            Image s = read_image(in), d = read_image(in);
            in >> s.batch;
            d.batch = s.batch;
            printf("%d", (int)regions_overlap(s, d));
        } else if (cmd == "layout") {
            Image im = read_image(in);
            int elem;
            in >> im.batch >> elem;
            printf("%d", layout_status(im, elem));
        } else if (cmd == "size") {
            Image im = {};
            int cols, max_rows, max_cols, mul24;
            in >> im.rows >> cols >> im.rs >> max_rows >> max_cols >> mul24;
            printf("%d", size_status(im, cols, max_rows, max_cols, mul24 != 0));
        } else if (cmd == "magic") {
            uint64_t n_max;
            uint32_t d;
            in >> n_max >> d;
            const uint32_t m = div_magic(n_max, d);
            int64_t wrong = m ? 0 : -1;
            for (uint64_t n = 0; m && n <= n_max; n++) wrong += fast_div((uint32_t)n, d, m) != (uint32_t)n / d;
            printf("%u %" PRId64, m, wrong);
        } else if (cmd == "magic_at") {
            uint64_t n;
            uint32_t d;
            in >> n >> d;
            const uint32_t m = div_magic(n, d);
            printf("%u %u %u", m, fast_div((uint32_t)n, d, m), (uint32_t)n / d);
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
