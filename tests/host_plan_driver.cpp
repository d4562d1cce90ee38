// host_plan_driver.cpp -- bev_amd/csrc/host_plan.h from the command line, for the CPU tests (tests/hostplan.py builds it with g++ under
// the address and undefined-behaviour sanitizers; a GPU test builds it plainly).  The one program of every test of the C ABI's host side:
//   host_plan_driver FAMILY < lines
// FAMILY names one group of entry points below; its function's comment documents that family's lines.  One case per line of stdin, one
// line of numbers per case on stdout (tests/plan_driver_io.h: the loop, the readers, the printers).  A call is built with host_plan.h's
// describers and taken through host_plan.h's own steps -- flat_grid, remap_grid, supersample_grid, build_map_model_status, stitch_check --
// which are the ones bevwarp_api.hip runs.  A base of 0 is a null pointer; no pointer is dereferenced but the HOST ones: matrices, lenses,
// camera arrays, border values, scales and biases.  Tiles are 256 x 4 (kBorderTileW x kBorderTileH) in every family.
#include <string.h>

#include <limits>
#include <vector>

#include "plan_driver_io.h"

static const double kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

static uint32_t fast_div(uint32_t n, uint32_t d, uint32_t magic) { return magic ? (uint32_t)(((uint64_t)n * magic) >> 32) : n / d; }  // (coords.h)

// a flat-grid entry's checked line, with the family's `wide` flags after the status
static void print_flat(const Call& c, std::initializer_list<int> wide = {}) {
    TilePlan p;
    const int st = flat_grid(c, 256, 4, p);
    print_checked(st, p, -1, wide);
}
// a map sampler's checked line: frames_per_item before total_tiles (at most max_fpi frames per item, kRemapFillItems items to fill)
static void print_remap(const Call& c, int max_fpi) {
    RemapPlan p;
    const int st = remap_grid(c, 256, 4, max_fpi, kRemapFillItems, p);
    print_checked(st, p, p.frames_per_item);
}
// a stitch's line (print_stitch) from stitch_check; gains: of a stitch under BEVWARP_STITCH_GAIN.  The status.
template <class Camera, class Describe>
static int print_stitch_check(const Camera* cams, int n_cams, int blend, int feather, Describe describe, std::initializer_list<HostValues> values, int batch, int dst_h,
                              int dst_w, uint32_t* gains = nullptr) {
    TilePlan p = {};
    Call calls[BEVWARP_STITCH_MAX_CAMERAS];
    const int st = stitch_check(cams, n_cams, blend, feather, describe, values, batch, dst_h, dst_w, 256, 4, p, calls, gains);
    print_stitch(st, p);
    return st;
}

// plan -- the launch plans, the image rules and the calls of the warps:
//   rows batch dst_h dst_w dtype tw rpp resident        -> status tile_h tiles_x tiles_per_frame total_tiles chunk stagger tail_split bw0 tpf_magic tx_magic bw0_magic
//   composite dst_h dst_w tw rpp max_rows cus           -> the same
//   border batch dst_h dst_w tw th mode src_h src_w     -> the same, then per_x off_x mag_x per_y off_y mag_y
//   overlap s(base rows row_bytes rs fs) d(...) batch   -> 0 | 1
//   layout base rows row_bytes rs fs batch elem         -> status
//   size rows cols rs max_rows max_cols mul24           -> status
//   magic n_max d                                       -> magic, and how many n <= n_max it divides wrongly (-1: "divide")
//   magic_at n d                                        -> magic, quotient by it (by division when the magic is 0), n / d
// `checked` is flat_grid's status, then plan_border's status and total_tiles where the call goes on to a launch, else 0 0:
//   warp src dst batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs m_count dtype interp cubic_ok
//       -> check_call's status, wide stores admitted, source pixels loaded whole (pixel_loads_ok)
//   planes src dst batch channels dst_h dst_w dst_fs dst_ps dst_rs plane_elem      (the source: tightly packed 8 x 8 frames of 8-bit pixels)
//       -> check_call's status, store_align, wide stores admitted, bytes of a destination row
//   nv12 y uv dst batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_rs m_count interp rgb_order
//       -> checked with "wide stores admitted" after the status
//   nv12p y uv dst batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_ps dst_rs m_count interp rgb_order plane_dtype
//       -> the same
//   to_nv12 src dst_y dst_uv batch src_h src_w dst_h dst_w src_fs src_rs dy_fs dy_rs duv_fs duv_rs m_count interp rgb_order
//   nv12_to_nv12 y uv dst_y dst_uv batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dy_fs dy_rs duv_fs duv_rs m_count interp
//       -> checked with "wide stores admitted" for the Y plane and for the UV plane after the status
static Image read_image(std::istream& in) {
    Image im = {};
    in >> im.base >> im.rows >> im.row_bytes >> im.rs >> im.fs;
    return im;
}
static int plan_family(const std::string& cmd, std::istream& in) {
    if (cmd == "rows") {
        int batch = 0, dst_h = 0, dst_w = 0, dtype = 0, tw = 0, rpp = 0;
        int64_t resident = 0;
        in >> batch >> dst_h >> dst_w >> dtype >> tw >> rpp >> resident;
        print_plan(plan_rows(batch, dst_h, dst_w, dtype, tw, rpp, resident));
    } else if (cmd == "composite") {
        int dst_h = 0, dst_w = 0, tw = 0, rpp = 0, max_rows = 0;
        int64_t cus = 0;
        in >> dst_h >> dst_w >> tw >> rpp >> max_rows >> cus;
        print_plan(plan_composite(dst_h, dst_w, tw, rpp, max_rows, cus));
    } else if (cmd == "border") {
        int batch = 0, dst_h = 0, dst_w = 0, tw = 0, th = 0, mode = 0, src_h = 0, src_w = 0;
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
        int elem = 1;
        in >> im.batch >> elem;
        printf("%d", layout_status(im, elem));
    } else if (cmd == "size") {
        Image im = {};
        int cols = 0, max_rows = 0, max_cols = 0, mul24 = 0;
        in >> im.rows >> cols >> im.rs >> max_rows >> max_cols >> mul24;
        printf("%d", size_status(im, cols, max_rows, max_cols, mul24 != 0));
    } else if (cmd == "magic") {
        uint64_t n_max = 0;
        uint32_t d = 1;
        in >> n_max >> d;
        const uint32_t m = div_magic(n_max, d);
        int64_t wrong = m ? 0 : -1;
        for (uint64_t n = 0; m && n <= n_max; n++) wrong += fast_div((uint32_t)n, d, m) != (uint32_t)n / d;
        printf("%u %" PRId64, m, wrong);
    } else if (cmd == "magic_at") {
        uint64_t n = 0;
        uint32_t d = 1;
        in >> n >> d;
        const uint32_t m = div_magic(n, d);
        printf("%u %u %u", m, fast_div((uint32_t)n, d, m), (uint32_t)n / d);
    } else if (cmd == "warp") {
        Frames src = {}, dst = {};
        int channels = 0, dtype = 0, interp = 0, cubic_ok = 0;
        read_bases(in, src, dst);
        Sizes z = read_sizes(in, kIdentity);
        in >> channels;
        read_strides(in, src, dst);
        in >> z.m_count >> dtype >> interp >> cubic_ok;
        const Call c = warp_call(src, dst, z, channels, dtype, interp, cubic_ok != 0);
        printf("%d %d %d", check_call(c), (int)wide_stores_ok(c.writes[0], store_align(dtype, channels, false)),
               (int)pixel_loads_ok(c.reads[0].im, pixel_load_align(dtype, channels)));
    } else if (cmd == "planes") {
        Frames src = {}, dst = {};
        Sizes z = {0, 8, 8, 0, 0, 1, kIdentity};
        int channels = 0, elem = 0;
        int64_t ps = 0;
        read_bases(in, src, dst);
        in >> z.batch >> channels >> z.dst_h >> z.dst_w >> dst.fs >> ps >> dst.rs >> elem;
        src.fs = (int64_t)64 * channels, src.rs = (int64_t)8 * channels;
        const Call c = warp_call(src, dst, z, channels, BEVWARP_U8, BEVWARP_LINEAR, false, elem, ps);
        const int align = store_align(BEVWARP_U8, channels, true, elem);
        printf("%d %d %d %" PRIu64, check_call(c), align, (int)wide_stores_ok(c.writes[0], align), c.writes[0].im.row_bytes);
    } else if (cmd == "nv12" || cmd == "nv12p") {
        const bool planes = cmd == "nv12p";
        Frames y = {}, uv = {}, dst = {};
        int interp = 0, rgb = 0, plane_dtype = 0;
        int64_t ps = 0;
        read_bases(in, y, uv, dst);
        Sizes z = read_sizes(in, kIdentity);
        read_strides(in, y, uv);
        in >> dst.fs;
        if (planes) in >> ps;
        in >> dst.rs >> z.m_count >> interp >> rgb;
        if (planes) in >> plane_dtype;
        const Call c = planes ? nv12_planes_call(y, uv, dst, ps, z, interp, rgb, plane_dtype) : nv12_call(y, uv, dst, z, interp, rgb);
        print_flat(c, {wide_stores_ok(c.writes[0], store_align(BEVWARP_U8, 3, planes, c.writes[0].elem))});
    } else if (cmd == "to_nv12" || cmd == "nv12_to_nv12") {
        const bool nv12_src = cmd == "nv12_to_nv12";
        Frames src = {}, uv = {}, dy = {}, duv = {};
        int interp = 0, rgb = 0;
        read_bases(in, src);
        if (nv12_src) read_bases(in, uv);
        read_bases(in, dy, duv);
        Sizes z = read_sizes(in, kIdentity);
        read_strides(in, src);
        if (nv12_src) read_strides(in, uv);
        read_strides(in, dy, duv);
        in >> z.m_count >> interp;
        if (!nv12_src) in >> rgb;
        const Call c = nv12_src ? nv12_to_nv12_call(src, uv, dy, duv, z, interp) : to_nv12_call(src, dy, duv, z, interp, rgb);
        print_flat(c, {wide_stores_ok(c.writes[0], 4), wide_stores_ok(c.writes[1], 4)});
    } else {
        return -1;
    }
    return 0;
}

// What the remap and remap_cubic families share, bevwarp_remap's call:
//   call src dst xy frac batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs map_count xy_fs xy_rs frac_fs frac_rs dtype interp mode
//       -> [take_flag: BEVWARP_MAP_BICUBIC taken out of the word, the flag first,] remap_grid's status, then plan_remap's status,
//          frames_per_item and total_tiles (at most 8 frames per item -- the library's own bound is lower --, 4096 items to fill) where the
//          call goes on to a launch, else 0 0 0
static void remap_call_line(std::istream& in, bool take_flag) {
    Frames s = {}, d = {}, mx = {}, mf = {};
    int channels = 0, map_count = 0, dtype = 0, interp = 0, mode = 0;
    read_bases(in, s, d, mx, mf);
    const Sizes z = read_sizes(in);
    in >> channels;
    read_strides(in, s, d);
    in >> map_count;
    read_strides(in, mx, mf);
    in >> dtype >> interp >> mode;
    const bool bicubic = take_flag && take_map_bicubic_flag(interp);
    if (take_flag) printf("%d ", (int)bicubic);
    print_remap(remap_call(s, d, mx, mf, z, map_count, channels, dtype, interp, mode, bicubic), 8);
}
// remap -- bevwarp_remap and bevwarp_build_map (the lens is HOST):
//   call ...                         (above, the flag left in the word)
//   plan batch map_count dst_h dst_w max_fpi fill
//       -> plan_remap's status, frames_per_item, groups, total_tiles, and `covered`: 1 when decoding every item t of the grid as the
//          kernel does -- group t / tiles_per_frame, tile t mod tiles_per_frame, frames group * fpi ... min(batch, (group + 1) * fpi) - 1
//          -- visits every (frame, tile) exactly once (checked item by item: keep batch * tiles small), else 0
//   build m_null m_count lens(0 none, 1 good, 2 NaN entry) r2_max interp xy frac dst_h dst_w xy_fs xy_rs frac_fs frac_rs
//       -> build_map_status's status, then the plan's total_tiles where the status is BEVWARP_OK, else 0
static int remap_family(const std::string& cmd, std::istream& in) {
    if (cmd == "call") {
        remap_call_line(in, false);
    } else if (cmd == "plan") {
        int batch = 0, map_count = 0, dst_h = 0, dst_w = 0, max_fpi = 0;
        int64_t fill = 0;
        in >> batch >> map_count >> dst_h >> dst_w >> max_fpi >> fill;
        if (!in) return 0;
        const RemapPlan p = plan_remap(batch, map_count, dst_h, dst_w, 256, 4, max_fpi, fill);
        const bool ok = p.status == BEVWARP_OK;
        int covered = 0;
        if (ok && (int64_t)batch * p.tiles_per_frame <= (1 << 24)) {
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
        printf("%d %d %d %" PRId64 " %d", p.status, ok ? p.frames_per_item : 0, ok ? p.groups : 0, ok ? p.total_tiles : 0, covered);
    } else if (cmd == "build") {
        Frames mx = {}, mf = {};
        int m_null = 0, m_count = 0, lens_kind = 0, interp = 0, dst_h = 0, dst_w = 0;
        in >> m_null >> m_count >> lens_kind;
        const double r2_max = read_number(in);
        in >> interp;
        read_bases(in, mx, mf);
        in >> dst_h >> dst_w;
        read_strides(in, mx, mf);
        double lens[12] = {800.0, 810.0, 319.5, 239.5, -0.3, 0.1, 0.001, -0.0005, -0.01, 0.9, -0.3, 0.02};
        if (lens_kind == 2) lens[5] = NAN;
        TilePlan p = {};
        const int st = build_map_status(m_null ? nullptr : kIdentity, m_count, lens_kind ? lens : nullptr, r2_max, interp, mx, mf, dst_h, dst_w, 256, 4, p);
        printf("%d %" PRId64, st, st == BEVWARP_OK ? p.total_tiles : 0);
    } else {
        return -1;
    }
    return 0;
}

// remap_cubic -- BEVWARP_MAP_BICUBIC (take_map_bicubic_flag, remap_call):
//   flag word                        -> take_map_bicubic_flag: the flag, the word left
//   call ...                         (above, the flag taken out as bevwarp_remap does)
//   other entry interp               (entry: build, nv12, nv12_planes, to_nv12, nv12_to_nv12, planes, stitch, stitch_nv12)
//       -> the status of that entry's checks on a good 8 x 8 call with `interp` as its word (no entry but bevwarp_remap takes the flag out)
static int remap_cubic_family(const std::string& cmd, std::istream& in) {
    if (cmd == "flag") {
        int word = 0;
        in >> word;
        const bool f = take_map_bicubic_flag(word);
        printf("%d %d", (int)f, word);
    } else if (cmd == "call") {
        remap_call_line(in, true);
    } else if (cmd == "other") {
        std::string entry;
        int interp = 0;
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
            st = build_map_status(kIdentity, 1, nullptr, 0.0, interp, xy, fr, 8, 8, 256, 4, p);
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
            malformed(in);
        }
        printf("%d", st);
    } else {
        return -1;
    }
    return 0;
}

// remap_nv12 -- bevwarp_remap_nv12 and bevwarp_remap_nv12_planes:
//   pix    y uv dst xy frac batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_rs map_count xy_fs xy_rs frac_fs frac_rs interp mode rgb
//   planes y uv dst xy frac batch src_h src_w dst_h dst_w y_fs y_rs uv_fs uv_rs dst_fs dst_ps dst_rs map_count xy_fs xy_rs frac_fs frac_rs interp mode rgb plane_dtype
//       -> remap_grid's status, then plan_remap's status, frames_per_item and total_tiles (at most 2 frames per item, 4096 items to fill:
//          the library's values) where the call goes on to a launch, else 0 0 0
static int remap_nv12_family(const std::string& cmd, std::istream& in) {
    if (cmd != "pix" && cmd != "planes") return -1;
    const bool planes = cmd == "planes";
    Frames fy = {}, fuv = {}, d = {}, mx = {}, mf = {};
    int64_t dst_ps = 0;
    int map_count = 0, interp = 0, mode = 0, rgb = 0, plane_dtype = 0;
    read_bases(in, fy, fuv, d, mx, mf);
    const Sizes z = read_sizes(in);
    read_strides(in, fy, fuv);
    in >> d.fs;
    if (planes) in >> dst_ps;
    in >> d.rs >> map_count;
    read_strides(in, mx, mf);
    in >> interp >> mode >> rgb;
    if (planes) in >> plane_dtype;
    print_remap(planes ? remap_nv12_planes_call(fy, fuv, d, dst_ps, mx, mf, z, map_count, interp, rgb, mode, plane_dtype)
                       : remap_nv12_call(fy, fuv, d, mx, mf, z, map_count, interp, rgb, mode),
                2);
    return 0;
}

// remap_nv12_out -- bevwarp_remap_to_nv12, bevwarp_remap_nv12_to_nv12, bevwarp_stitch_maps_to_nv12 and bevwarp_stitch_maps_nv12_to_nv12:
//   bgr | nv12     src uv dst_y dst_uv xy frac batch src_h src_w dst_h dst_w src_fs src_rs uv_fs uv_rs y_fs y_rs duv_fs duv_rs map_count xy_fs xy_rs
//                  frac_fs frac_rs interp mode rgb                      (bgr: uv and its strides are not looked at; nv12: rgb is not)
//       -> as the remap_nv12 family's lines
//   sbgr | snv12   n_cams cams_null dst_y dst_uv batch dst_h dst_w y_fs y_rs duv_fs duv_rs interp blend feather rgb border listed
//                  then the `listed` described cameras (read_map_cameras), which may differ from n_cams
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last of the 3 channels
//       -> the status, then the plan's status and total_tiles where the status is BEVWARP_OK, else 0 0
static int remap_nv12_out_family(const std::string& cmd, std::istream& in) {
    if (cmd == "bgr" || cmd == "nv12") {
        Frames fs = {}, fuv = {}, fdy = {}, fduv = {}, mx = {}, mf = {};
        int map_count = 0, interp = 0, mode = 0, rgb = 0;
        read_bases(in, fs, fuv, fdy, fduv, mx, mf);
        const Sizes z = read_sizes(in);
        read_strides(in, fs, fuv, fdy, fduv);
        in >> map_count;
        read_strides(in, mx, mf);
        in >> interp >> mode >> rgb;
        print_remap(cmd == "nv12" ? remap_nv12_to_nv12_call(fs, fuv, fdy, fduv, mx, mf, z, map_count, interp, mode)
                                  : remap_to_nv12_call(fs, fdy, fduv, mx, mf, z, map_count, interp, rgb, mode),
                    2);
    } else if (cmd == "sbgr" || cmd == "snv12") {
        const bool nv12 = cmd == "snv12";
        bevwarp_map_camera cams[16] = {};
        Frames fdy = {}, fduv = {};
        int n_cams = 0, cams_null = 0, batch = 0, dst_h = 0, dst_w = 0, interp = 0, blend = 0, feather = 0, rgb = 0, border = 0, listed = 0;
        in >> n_cams >> cams_null;
        read_bases(in, fdy, fduv);
        in >> batch >> dst_h >> dst_w;
        read_strides(in, fdy, fduv);
        in >> interp >> blend >> feather >> rgb >> border >> listed;
        read_map_cameras(in, listed, cams);
        if (!in) return 0;
        double bv[3] = {1.0, 2.0, 3.0};
        const auto describe = [&](const bevwarp_map_camera& k) { return stitch_maps_nv12_out_call(nv12, k, fdy, fduv, batch, dst_h, dst_w, interp, blend, nv12 ? 0 : rgb); };
        print_stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{selected(border, bv, 3), 3}}, batch, dst_h, dst_w);
    } else {
        return -1;
    }
    return 0;
}

// map_planes -- bevwarp_remap_planes, bevwarp_stitch_maps_planes and bevwarp_stitch_maps_nv12_planes:
//   planes         src dst xy frac batch src_h src_w dst_h dst_w src_fs src_rs dst_fs dst_ps dst_rs map_count xy_fs xy_rs frac_fs frac_rs interp
//                  mode plane_dtype
//       -> as the remap_nv12 family's lines
//   sbgr | snv12   n_cams cams_null dst batch dst_h dst_w dst_fs dst_ps dst_rs interp blend feather rgb plane_dtype border scale bias listed
//                  then the `listed` described cameras (read_map_cameras), which may differ from n_cams
//       border, scale, bias: 0 = NULL, 1 = finite values, 2 = a NaN in the last of the 3 channels
//       -> the status, then the plan's status and total_tiles where the status is BEVWARP_OK, else 0 0
static int map_planes_family(const std::string& cmd, std::istream& in) {
    if (cmd == "planes") {
        Frames fs = {}, fd = {}, mx = {}, mf = {};
        int64_t dst_ps = 0;
        int map_count = 0, interp = 0, mode = 0, plane_dtype = 0;
        read_bases(in, fs, fd, mx, mf);
        const Sizes z = read_sizes(in);
        read_strides(in, fs);
        in >> fd.fs >> dst_ps >> fd.rs >> map_count;
        read_strides(in, mx, mf);
        in >> interp >> mode >> plane_dtype;
        print_remap(remap_planes_call(fs, fd, dst_ps, mx, mf, z, map_count, interp, mode, plane_dtype), 2);
    } else if (cmd == "sbgr" || cmd == "snv12") {
        const bool nv12 = cmd == "snv12";
        bevwarp_map_camera cams[16] = {};
        Frames fd = {};
        int64_t dst_ps = 0;
        int n_cams = 0, cams_null = 0, batch = 0, dst_h = 0, dst_w = 0, interp = 0, blend = 0, feather = 0, rgb = 0, plane_dtype = 0, border = 0, scale = 0, bias = 0, listed = 0;
        in >> n_cams >> cams_null;
        read_bases(in, fd);
        in >> batch >> dst_h >> dst_w >> fd.fs >> dst_ps >> fd.rs >> interp >> blend >> feather >> rgb >> plane_dtype >> border >> scale >> bias >> listed;
        read_map_cameras(in, listed, cams);
        if (!in) return 0;
        double bv[3] = {1.0, 2.0, 3.0}, sc[3] = {0.5, 0.25, 2.0}, bi[3] = {-1.0, 0.0, 1.0};
        const auto describe = [&](const bevwarp_map_camera& k) {
            return stitch_maps_planes_call(nv12, k, fd, dst_ps, batch, dst_h, dst_w, interp, blend, nv12 ? rgb : 0, plane_dtype);
        };
        print_stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{selected(border, bv, 3), 3}, {selected(scale, sc, 3), 3}, {selected(bias, bi, 3), 3}},
                           batch, dst_h, dst_w);
    } else {
        return -1;
    }
    return 0;
}

// lens -- bevwarp_warp_lens (lens_call, lens_status):
//   call src dst batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs m_count m_ray_null dtype interp border_mode
//       -> flat_grid's status, then plan_border's status and total_tiles where the call goes on to a launch, else 0 0
//   lens fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 r2_max     -> lens_status
//   lens_null                                           -> lens_status of a NULL lens
static int lens_family(const std::string& cmd, std::istream& in) {
    if (cmd == "call") {
        Frames s = {}, d = {};
        int channels = 0, m_null = 0, dtype = 0, interp = 0, mode = 0;
        read_bases(in, s, d);
        Sizes z = read_sizes(in);
        in >> channels;
        read_strides(in, s, d);
        in >> z.m_count >> m_null >> dtype >> interp >> mode;
        z.minv = m_null ? nullptr : kIdentity;
        print_flat(lens_call(s, d, z, channels, dtype, interp, mode));
    } else if (cmd == "lens") {
        double v[13];
        for (double& x : v) x = read_number(in);
        if (in) printf("%d", lens_status(v, v[12]));
    } else if (cmd == "lens_null") {
        printf("%d", lens_status(nullptr, 1.0));
    } else {
        return -1;
    }
    return 0;
}

// fisheye -- BEVWARP_LENS_FISHEYE (take_fisheye_flag, fisheye_status, lens_model_status, points_model_status, build_map_model_status):
//   lens fx fy cx cy k1 k2 k3 k4 r0 r1 r2 r3 theta_max   -> fisheye_status
//   lens_null                                            -> fisheye_status of a NULL lens
//   flag word                                            -> take_fisheye_flag: the flag, the word left
//   warp interp lens theta_max       (lens: 0 NULL, 1 good, 2 a NaN entry, 3 fx == 0, 4 a reserved entry != 0)
//       -> flat_grid's status of lens_call on an 8 x 8 call with the word's flag taken out, then lens_model_status (0 where the call has failed)
//   points in out residual n h lens theta_max direction iters tol_px dtype    (h: 0 NULL, 1 good, 2 a NaN entry)   -> points_model_status, the flag taken out
//   build m xy frac m_count lens theta_max interp dst_h dst_w xy_rs frac_rs                  -> build_map_model_status, the flag taken out
static const double* fisheye_lens(int which, double* v) {
    static const double good[12] = {200.0, 204.0, 319.5, 179.5, -0.02, 0.004, -0.001, 0.0002, 0, 0, 0, 0};
    memcpy(v, good, sizeof(good));
    if (which == 2) v[5] = NAN;
    if (which == 3) v[0] = 0.0;
    if (which == 4) v[10] = 1e-300;
    return which ? v : nullptr;
}
static int fisheye_family(const std::string& cmd, std::istream& in) {
    static const double m_nan[9] = {1, 0, 0, 0, std::numeric_limits<double>::quiet_NaN(), 0, 0, 0, 1};
    double v[13];
    if (cmd == "lens") {
        for (double& x : v) x = read_number(in);
        if (in) printf("%d", fisheye_status(v, v[12]));
    } else if (cmd == "lens_null") {
        printf("%d", fisheye_status(nullptr, 1.0));
    } else if (cmd == "flag") {
        int word = 0;
        in >> word;
        const bool f = take_fisheye_flag(word);
        printf("%d %d", (int)f, word);
    } else if (cmd == "warp") {
        int interp = 0, which = 0;
        in >> interp >> which;
        const double theta_max = read_number(in);
        const bool fisheye = take_fisheye_flag(interp);
        TilePlan p;
        const int st = flat_grid(lens_call({(const void*)16, 192, 24}, {(const void*)(1 << 20), 192, 24}, {1, 8, 8, 8, 8, 1, kIdentity}, 3, BEVWARP_U8, interp, BEVWARP_BORDER_CONSTANT),
                                 256, 4, p);
        printf("%d %d", st, st == BEVWARP_OK ? lens_model_status(fisheye, fisheye_lens(which, v), theta_max) : 0);
    } else if (cmd == "points") {
        int64_t n = 0;
        int h = 0, which = 0, direction = 0, iters = 0, dtype = 0;
        const void *src = read_ptr(in), *dst = read_ptr(in), *res = read_ptr(in);
        in >> n >> h >> which;
        const double theta_max = read_number(in);
        in >> direction >> iters;
        const double tol = read_number(in);
        in >> dtype;
        const bool fisheye = take_fisheye_flag(direction);
        printf("%d", points_model_status(fisheye, src, dst, res, n, h == 0 ? nullptr : (h == 2 ? m_nan : kIdentity), fisheye_lens(which, v), theta_max, direction, iters, tol, dtype));
    } else if (cmd == "build") {
        int m_count = 0, which = 0, interp = 0, dst_h = 0, dst_w = 0;
        Frames fxy = {}, ffr = {};
        const void* mp = read_ptr(in);
        read_bases(in, fxy, ffr);
        in >> m_count >> which;
        const double theta_max = read_number(in);
        in >> interp >> dst_h >> dst_w >> fxy.rs >> ffr.rs;
        fxy.fs = (int64_t)dst_h * fxy.rs, ffr.fs = (int64_t)dst_h * ffr.rs;
        const bool fisheye = take_fisheye_flag(interp);
        TilePlan p;
        const int st = build_map_model_status(fisheye, mp ? kIdentity : nullptr, m_count, fisheye_lens(which, v), theta_max, interp, fxy, ffr, dst_h, dst_w, 256, 4, p);
        printf("%d %" PRId64, st, st == BEVWARP_OK ? p.total_tiles : 0);
    } else {
        return -1;
    }
    return 0;
}

// points_lens -- bevwarp_project_points_lens (points_lens_status):
//   status in out residual n h direction iters tol_px dtype lens r2_max [12 lens values]          -> the status
//       h: 0 NULL, 1 the identity, 2 with a NaN, 3 with an inf;  lens: 0 NULL, 1 the 12 values that follow
static int points_lens_family(const std::string& cmd, std::istream& in) {
    if (cmd != "status") return -1;
    int64_t n = 0;
    int h = 0, direction = 0, iters = 0, dtype = 0, has_lens = 0;
    double lens[12] = {}, H[9];
    const void *src = read_ptr(in), *dst = read_ptr(in), *res = read_ptr(in);
    in >> n >> h >> direction >> iters;
    const double tol_px = read_number(in);
    in >> dtype >> has_lens;
    const double r2_max = read_number(in);
    for (int i = 0; has_lens && i < 12; i++) lens[i] = read_number(in);
    if (h < 0 || h > 3) malformed(in);
    if (!in) return 0;
    memcpy(H, kIdentity, sizeof(H));
    if (h == 2) H[4] = NAN;
    if (h == 3) H[8] = INFINITY;
    printf("%d", points_lens_status(src, dst, res, n, h ? H : nullptr, has_lens ? lens : nullptr, r2_max, direction, iters, tol_px, dtype));
    return 0;
}

// stitch -- bevwarp_warp_stitch (stitch_check over stitch_call; the camera array and the border value are HOST):
//   stitch n_cams cams_null dst batch dst_h dst_w channels dst_fs dst_rs dtype interp blend feather border_mode border listed
//          then per described camera (`listed` of them, which may differ from n_cams): src src_h src_w fs rs m_count m_inv_null
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last channel
//       -> stitch_check's status, then the plan's status and total_tiles where the status is BEVWARP_OK, else 0 0
static int stitch_family(const std::string& cmd, std::istream& in) {
    if (cmd != "stitch") return -1;
    bevwarp_camera cams[16] = {};
    Frames d = {};
    int n_cams = 0, cams_null = 0, batch = 0, dst_h = 0, dst_w = 0, channels = 0, dtype = 0, interp = 0, blend = 0, feather = 0, mode = 0, border = 0, listed = 0;
    in >> n_cams >> cams_null;
    read_bases(in, d);
    in >> batch >> dst_h >> dst_w >> channels;
    read_strides(in, d);
    in >> dtype >> interp >> blend >> feather >> mode >> border >> listed;
    if (listed < 0 || listed > 16) malformed(in);
    for (int k = 0; in && k < listed; k++) {
        int m_null = 0;
        cams[k].src = read_ptr(in);
        in >> cams[k].src_h >> cams[k].src_w >> cams[k].frame_stride >> cams[k].row_stride >> cams[k].m_count >> m_null;
        cams[k].M_inv = m_null ? nullptr : kIdentity;
    }
    if (!in) return 0;
    double bv[4] = {1.0, 2.0, 3.0, 4.0};
    const auto describe = [&](const bevwarp_camera& k) { return stitch_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, mode); };
    const double* constant = mode == BEVWARP_BORDER_CONSTANT ? selected(border, bv, channels) : nullptr;  // (read by the constant border only)
    print_stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{constant, channels}}, batch, dst_h, dst_w);
    return 0;
}

// What the stitch_maps and stitch_gain families share, the six stitches through maps (stitch_check over stitch_maps_call and its kin):
//   maps | nv12 | to_nv12 | nv12_to_nv12 | planes | nv12_planes
//          n_cams cams_null dst batch dst_h dst_w channels dst_fs dst_rs dtype interp blend feather rgb_order border_mode border
//          [gain: dst2 dst2_fs dst2_rs plane_dtype] listed
//          then the `listed` described cameras (read_map_cameras; gain: each with its `reserved` word), which may differ from n_cams
//       blend: the word as the caller passes it; gain: BEVWARP_STITCH_GAIN is taken out of it as the entries do, every check sees the rest.
//       dst2, dst2_fs, dst2_rs: the plane of pairs of an NV12 destination; dst2_fs is the plane stride of a destination of planes.
//       border: 0 = NULL, 1 = finite values, 2 = a NaN in the last channel (channels of `maps`, otherwise 3; nv12: channels, dtype are not
//       looked at).  The entries with a border mode read the border value under the constant border only; the others always.
//       -> the status, the plan's status and total_tiles where the status is BEVWARP_OK (else 0 0), and, gain: whether the flag was set, and
//          where it was and the status is BEVWARP_OK the n_cams gain words as they were checked
static int stitch_maps_line(const std::string& cmd, std::istream& in, bool gain) {
    const bool nv12 = cmd == "nv12" || cmd == "nv12_to_nv12" || cmd == "nv12_planes";
    const bool to_nv12 = cmd == "to_nv12" || cmd == "nv12_to_nv12", planes = cmd == "planes" || cmd == "nv12_planes";
    if (gain ? (cmd != "maps" && !nv12 && !to_nv12 && !planes) : (cmd != "maps" && cmd != "nv12")) return -1;
    bevwarp_map_camera cams[16] = {};
    Frames d = {}, d2 = {};
    int n_cams = 0, cams_null = 0, batch = 0, dst_h = 0, dst_w = 0, channels = 0, dtype = 0, interp = 0, blend = 0, feather = 0, rgb = 0, mode = 0, border = 0, plane_dtype = 0, listed = 0;
    in >> n_cams >> cams_null;
    read_bases(in, d);
    in >> batch >> dst_h >> dst_w >> channels;
    read_strides(in, d);
    in >> dtype >> interp >> blend >> feather >> rgb >> mode >> border;
    if (gain) {
        read_bases(in, d2);
        read_strides(in, d2);
        in >> plane_dtype;
    }
    in >> listed;
    read_map_cameras(in, listed, cams, gain);
    if (!in) return 0;
    double bv[4] = {1.0, 2.0, 3.0, 4.0};
    const int nb = cmd == "maps" ? channels : 3;
    const bool gained = gain && take_gain_flag(blend);
    uint32_t gains[BEVWARP_STITCH_MAX_CAMERAS] = {};
    const auto describe = [&](const bevwarp_map_camera& k) {
        if (to_nv12) return stitch_maps_nv12_out_call(nv12, k, d, d2, batch, dst_h, dst_w, interp, blend, nv12 ? 0 : rgb);
        if (planes) return stitch_maps_planes_call(nv12, k, d, d2.fs, batch, dst_h, dst_w, interp, blend, nv12 ? rgb : 0, plane_dtype);
        return nv12 ? stitch_maps_nv12_call(k, d, batch, dst_h, dst_w, interp, blend, rgb, mode)
                    : stitch_maps_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, mode, gained);
    };
    const double* constant = (to_nv12 || planes || mode == BEVWARP_BORDER_CONSTANT) ? selected(border, bv, nb) : nullptr;
    const int st = print_stitch_check(cams_null ? nullptr : cams, n_cams, blend, feather, describe, {{constant, nb}}, batch, dst_h, dst_w, gained ? gains : nullptr);
    if (gain) printf(" %d", (int)gained);
    for (int k = 0; gained && st == BEVWARP_OK && k < n_cams; k++) printf(" %" PRIu32, gains[k]);
    return 0;
}
// stitch_maps -- bevwarp_stitch_maps and bevwarp_stitch_maps_nv12: the lines `maps` and `nv12` above
static int stitch_maps_family(const std::string& cmd, std::istream& in) { return stitch_maps_line(cmd, in, false); }
// stitch_gain -- the six stitches through maps under BEVWARP_STITCH_GAIN: all six lines above, with the gain fields
static int stitch_gain_family(const std::string& cmd, std::istream& in) { return stitch_maps_line(cmd, in, true); }

// supersample -- BEVWARP_SUPERSAMPLE_* (take_supersample, supersample_grid):
//   field word                       -> take_supersample: k, the word left
//   call src dst minv batch src_h src_w dst_h dst_w channels src_fs src_rs dst_fs dst_rs m_count dtype interp mode
//       -> bevwarp_warp_border's checks of a word that carries the field (k > 1; anything else is a malformed case): k, supersample_grid's
//          status -- an unknown border mode first, then check_call of supersample_call --, then plan_supersample's status, bw0 and
//          total_tiles where the call goes on to a launch, else 0 0 0
//   other entry interp               (entry: warp, lens, remap, build)
//       -> the status of that entry's checks on a good 8 x 8 call with `interp` as its word (no entry but bevwarp_warp_border takes the
//          field out)
static int supersample_family(const std::string& cmd, std::istream& in) {
    if (cmd == "field") {
        int word = 0;
        in >> word;
        const int k = take_supersample(word);
        printf("%d %d", k, word);
    } else if (cmd == "call") {
        Frames s = {}, d = {};
        int channels = 0, dtype = 0, interp = 0, mode = 0;
        read_bases(in, s, d);
        const double* minv = (const double*)read_ptr(in);
        Sizes z = read_sizes(in, minv);
        in >> channels;
        read_strides(in, s, d);
        in >> z.m_count >> dtype >> interp >> mode;
        const int k = take_supersample(interp);
        if (k == 1) malformed(in);
        Call c;
        TilePlan p;
        const int st = supersample_grid(s, d, z, channels, dtype, interp, mode, k, 256, 4, c, p);
        printf("%d ", k);
        print_checked(st, p, p.bw0);
    } else if (cmd == "other") {
        std::string entry;
        int interp = 0;
        in >> entry >> interp;
        const Frames src = {(const void*)16, 192, 24}, dst = {(const void*)(1 << 20), 192, 24};
        const Frames xy = {(const void*)(1 << 24), 256, 32}, fr = {(const void*)(1 << 26), 128, 16};
        const Sizes z = {1, 8, 8, 8, 8, 1, kIdentity};
        int st = 1, word = interp;
        if (entry == "warp") {
            st = check_call(warp_call(src, dst, z, 3, BEVWARP_U8, interp, false));
        } else if (entry == "lens") {
            take_fisheye_flag(word);
            st = check_call(lens_call(src, dst, z, 3, BEVWARP_U8, word, BEVWARP_BORDER_CONSTANT));
        } else if (entry == "remap") {
            const bool bicubic = take_map_bicubic_flag(word);
            st = check_call(remap_call(src, dst, xy, fr, z, 1, 3, BEVWARP_U8, word, BEVWARP_BORDER_CONSTANT, bicubic));
        } else if (entry == "build") {
            TilePlan p = {};
            const bool fisheye = take_fisheye_flag(word);
            static const double lens[12] = {100, 100, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0};
            st = build_map_model_status(fisheye, kIdentity, 1, fisheye ? lens : nullptr, 1.0, word, xy, fr, 8, 8, 256, 4, p);
        } else {
            malformed(in);
        }
        printf("%d", st);
    } else {
        return -1;
    }
    return 0;
}

int main(int argc, char** argv) {
    static const struct {
        const char* name;
        int (*one_case)(const std::string&, std::istream&);
    } families[] = {{"plan", plan_family},           {"remap", remap_family},   {"remap_cubic", remap_cubic_family}, {"remap_nv12", remap_nv12_family},
                    {"remap_nv12_out", remap_nv12_out_family}, {"map_planes", map_planes_family}, {"lens", lens_family},     {"fisheye", fisheye_family},
                    {"points_lens", points_lens_family},       {"stitch", stitch_family},         {"stitch_maps", stitch_maps_family}, {"stitch_gain", stitch_gain_family},
                    {"supersample", supersample_family}};
    for (const auto& f : families)
        if (argc == 2 && !strcmp(argv[1], f.name)) return run_cases(f.one_case);
    fprintf(stderr, "usage: host_plan_driver FAMILY < lines   (FAMILY:");
    for (const auto& f : families) fprintf(stderr, " %s", f.name);
    fprintf(stderr, ")\n");
    return 2;
}
