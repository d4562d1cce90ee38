// host_plan_driver.cpp -- bev_amd/csrc/host_plan.h from the command line, for the CPU tests (tests/hostplan.py builds it with g++ under
// the address and undefined-behaviour sanitizers).  One case per line of stdin, one line of numbers per case on stdout:
//   rows batch dst_h dst_w dtype tw rpp resident        -> status tile_h tiles_x tiles_per_frame total_tiles chunk stagger tail_split bw0 tpf_magic tx_magic bw0_magic
//   composite dst_h dst_w tw rpp max_rows cus           -> the same
//   border batch dst_h dst_w tw th mode src_h src_w     -> the same, then per_x off_x mag_x per_y off_y mag_y
//   overlap s(base rows row_bytes rs fs) d(...) batch   -> 0 | 1
//   layout base rows row_bytes rs fs batch elem         -> status
//   size rows cols rs max_rows max_cols mul24           -> status
//   magic n_max d                                       -> magic, and how many n <= n_max it divides wrongly (-1: "divide")
//   magic_at n d                                        -> magic, quotient by it (by division when the magic is 0), n / d
// The entry points' calls, built as bevwarp_api.hip builds them (a base of 0 is a null pointer; no pointer is dereferenced).  `checked` is
// check_call's status, then plan_border's status and total_tiles (kBorderTileW x kBorderTileH) where the call goes on to a launch, else 0 0:
//   warp src dst batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs m_count dtype interp cubic_ok
//       -> status, wide stores admitted, source pixels loaded whole (pixel_loads_ok)
//   planes src dst batch channels dst_h dst_w dst_fs dst_ps dst_rs plane_elem      (the source: tightly packed 8 x 8 frames of 8-bit pixels)
//       -> status, store_align, wide stores admitted, bytes of a destination row
//   nv12 y uv dst batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_rs m_count interp rgb_order
//       -> checked with "wide stores admitted" after the status
//   nv12p y uv dst batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_ps dst_rs m_count interp rgb_order plane_dtype
//       -> the same
//   to_nv12 src dst_y dst_uv batch src_h src_w dst_h dst_w src_fs src_rs dy_fs dy_rs duv_fs duv_rs m_count interp rgb_order
//   nv12_to_nv12 y uv dst_y dst_uv batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dy_fs dy_rs duv_fs duv_rs m_count interp
//       -> checked with "wide stores admitted" for the Y plane and for the UV plane after the status
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

static Frames read_base(std::istream& in) {  // (strides follow the sizes on a line)
    uint64_t base = 0;
    in >> base;
    return {(const void*)(uintptr_t)base, 0, 0};
}
static Sizes read_sizes(std::istream& in, const double* minv) {  // (the matrix count follows the strides)
    Sizes z = {};
    in >> z.batch >> z.src_h >> z.src_w >> z.dst_h >> z.dst_w;
    z.minv = minv;
    return z;
}
static void read_strides(std::istream& in, Frames& f) { in >> f.fs >> f.rs; }

// check_call's status, `wide` flags, and the flat grid's plan where bevwarp_api.hip goes on to it
static void print_checked(const Call& c, int wide0, int wide1 = -1) {
    const int st = check_call(c);
    TilePlan p = {};
    if (st == BEVWARP_OK && c.batch > 0) p = plan_border(c.batch, c.dst_h, c.dst_w, 256, 4);
    printf("%d %d ", st, wide0);
    if (wide1 >= 0) printf("%d ", wide1);
    printf("%d %" PRId64, p.status, p.status == BEVWARP_OK ? p.total_tiles : 0);
}

int main() {
    static const double minv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
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
        } else if (cmd == "warp") {
            Frames src = read_base(in), dst = read_base(in);
            Sizes z = read_sizes(in, minv);
            int channels, dtype, interp, cubic_ok;
            in >> channels;
            read_strides(in, src), read_strides(in, dst);
            in >> z.m_count >> dtype >> interp >> cubic_ok;
            const Call c = warp_call(src, dst, z, channels, dtype, interp, cubic_ok != 0);
            printf("%d %d %d", check_call(c), (int)wide_stores_ok(c.writes[0], store_align(dtype, channels, false)),
                   (int)pixel_loads_ok(c.reads[0].im, pixel_load_align(dtype, channels)));
        } else if (cmd == "planes") {
            Frames src = read_base(in), dst = read_base(in);
            Sizes z = {0, 8, 8, 0, 0, 1, minv};
            int channels, elem;
            int64_t ps;
            in >> z.batch >> channels >> z.dst_h >> z.dst_w >> dst.fs >> ps >> dst.rs >> elem;
            src.fs = (int64_t)64 * channels, src.rs = (int64_t)8 * channels;
            const Call c = warp_call(src, dst, z, channels, BEVWARP_U8, BEVWARP_LINEAR, false, elem, ps);
            const int align = store_align(BEVWARP_U8, channels, true, elem);
            printf("%d %d %d %" PRIu64, check_call(c), align, (int)wide_stores_ok(c.writes[0], align), c.writes[0].im.row_bytes);
        } else if (cmd == "nv12" || cmd == "nv12p") {
            Frames y = read_base(in), uv = read_base(in), dst = read_base(in);
            Sizes z = read_sizes(in, minv);
            int interp, rgb, plane_dtype = 0;
            int64_t ps = 0;
            read_strides(in, y), read_strides(in, uv);
            in >> dst.fs;
            if (cmd == "nv12p") in >> ps;
            in >> dst.rs >> z.m_count >> interp >> rgb;
            if (cmd == "nv12p") in >> plane_dtype;
            const Call c = cmd == "nv12" ? nv12_call(y, uv, dst, z, interp, rgb) : nv12_planes_call(y, uv, dst, ps, z, interp, rgb, plane_dtype);
            print_checked(c, wide_stores_ok(c.writes[0], store_align(BEVWARP_U8, 3, cmd == "nv12p", c.writes[0].elem)));
        } else if (cmd == "to_nv12" || cmd == "nv12_to_nv12") {
            const bool nv12_src = cmd == "nv12_to_nv12";
            Frames src = read_base(in), uv = nv12_src ? read_base(in) : Frames{}, dy = read_base(in), duv = read_base(in);
            Sizes z = read_sizes(in, minv);
            int interp, rgb = 0;
            read_strides(in, src);
            if (nv12_src) read_strides(in, uv);
            read_strides(in, dy), read_strides(in, duv);
            in >> z.m_count >> interp;
            if (!nv12_src) in >> rgb;
            const Call c = nv12_src ? nv12_to_nv12_call(src, uv, dy, duv, z, interp) : to_nv12_call(src, dy, duv, z, interp, rgb);
            print_checked(c, wide_stores_ok(c.writes[0], 4), wide_stores_ok(c.writes[1], 4));
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
