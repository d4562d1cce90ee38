// bevwarp_api.hip -- the extern "C" surface declared in include/bevwarp.h.  Every entry point reads: check the arguments, plan the
// launch (both in host_plan.h, plain C++ that the CPU tests compile on their own), copy the plan into the kernel arguments, launch.
// No allocation, no synchronisation, no CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bevwarp.h"
#include "host_plan.h"
#include "cubic_tab.h"
#include "points_lens.h"
#include "warp_border.h"
#include "warp_cubic.h"
#include "warp_kernels.h"
#include "warp_lens.h"
#include "warp_map.h"
#include "warp_map_nv12.h"
#include "warp_map_nv12_out.h"
#include "warp_map_planes.h"
#include "warp_nv12.h"
#include "warp_nv12_out.h"
#include "warp_stitch.h"
#include "warp_stitch_maps.h"
#include "warp_stitch_maps_nv12_out.h"
#include "warp_stitch_maps_planes.h"
#include "warp_supersample.h"

#pragma clang fp contract(off)

namespace {

thread_local char g_hip_error[256] = "";

int hip_fail(hipError_t e) {
    snprintf(g_hip_error, sizeof(g_hip_error), "%s: %s", hipGetErrorName(e), hipGetErrorString(e));
    return BEVWARP_ERR_HIP;
}

int launched(hipError_t e) { return e == hipSuccess ? BEVWARP_OK : hip_fail(e); }

using namespace bevwarp;
using namespace bevwarp::plan;

// a plan's grid in any kernel's arguments ...
template <class Args>
void copy_grid(Args& a, const TilePlan& p) {
    a.bw0 = p.bw0, a.tiles_x = p.tiles_x, a.tiles_per_frame = p.tiles_per_frame;
    a.tpf_magic = p.tpf_magic, a.tx_magic = p.tx_magic, a.bw0_magic = p.bw0_magic;
}
// ... and all its fields in the row kernel's
void copy_plan(WarpArgs& a, const TilePlan& p) {
    copy_grid(a, p);
    a.tile_h = p.tile_h, a.total_tiles = p.total_tiles, a.chunk = p.chunk, a.stagger = p.stagger, a.tail_split = p.tail_split;
}
// the frames a kernel samples (a.src and its two strides; a camera of a stitch has the same three)
template <class Args>
void fill_source(Args& a, const Image& s) {
    a.src = (const uint8_t*)s.base, a.src_fs = s.fs, a.src_rs = s.rs;
}
// the kernels' plane format of a plane type that the checks have let through
int plane_kind(int plane_dtype) { return plane_dtype == BEVWARP_F32 ? kPlaneF32 : (plane_dtype == BEVWARP_F16 ? kPlaneF16 : kPlaneBF16); }
// What the flat-grid entry points (border, bicubic, NV12, NV12 planes, into NV12) share: the checks and the grid (plan::flat_grid: st, p),
// and in the zeroed arguments the shared frame's part (flat_frame.h) -- the first written image, the matrices, the grid -- and the source's
// sides.  items = 0: nothing to launch, the status is the call's (c is not looked at where st is not BEVWARP_OK).  (dst_vec_ok follows each
// entry point's own layout rule.)
template <class Args>
int flat_grid_args(const Call& c, int st, const TilePlan& p, Args& a, int64_t& items) {
    items = 0;
    if (st != BEVWARP_OK) return st;
    if (c.batch == 0 || p.status != BEVWARP_OK) return p.status;  // (an empty batch: p is zeros)
    memset(&a, 0, sizeof(a));
    const Image& d = c.writes[0].im;
    a.dst = (uint8_t*)d.base, a.minv = c.minv;
    a.dst_fs = d.fs, a.dst_rs = d.rs, a.dst_h = c.dst_h, a.dst_w = c.dst_w;
    a.m_stride = c.m_count == 1 ? 0 : 9;
    copy_grid(a, p);
    a.src_h = c.src_h, a.src_w = c.src_w;
    items = p.total_tiles;
    return BEVWARP_OK;
}
template <class Args>
int flat_grid_args(const Call& c, Args& a, int64_t& items) {
    TilePlan p;
    const int st = plan::flat_grid(c, kBorderTileW, kBorderTileH, p);
    return flat_grid_args(c, st, p, a, items);
}
// ... and the NV12 kernels' source: the two planes the call reads
template <class Args>
void fill_nv12_source(Args& a, const Call& c) {
    const Image &y = c.reads[0].im, &uv = c.reads[1].im;
    a.y = (const uint8_t*)y.base, a.uv = (const uint8_t*)uv.base;
    a.y_fs = y.fs, a.y_rs = y.rs, a.uv_fs = uv.fs, a.uv_rs = uv.rs;
}
// border_value (HOST, `channels` doubles or NULL) as the kernels take it: float32, and saturate_cast<uchar> (round half to even, clamp)
template <class U8>
int border_values(const double* border_value, int channels, float* f, U8* u8) {
    for (int k = 0; k < 4; k++) {
        const double b = (border_value && k < channels) ? border_value[k] : 0.0;
        if (!isfinite(b)) return BEVWARP_ERR_NOT_FINITE;
        f[k] = (float)b;
        const double r = nearbyint(b);
        u8[k] = (U8)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
    return BEVWARP_OK;
}
// ... and of the NV12 entry points' 3 channels: the 8-bit values (bu[4]), which the kernels take packed, byte k = channel k
int border_bytes(const double* border_value, uint8_t* bu) {
    float bf[4];
    return border_values(border_value, 3, bf, bu);
}
uint32_t packed4(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }  // (up to 4 channels likewise)
uint32_t packed3(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16); }
// The plane kernels of the NV12 sources sample B, G, R: sampled channel k is the destination's channel k (BGR) or 2 - k (RGB), with that
// channel's plane, scale, bias and border value -- the channel order is nothing but this table (a: the kernel's ch_off, pscale, pbias;
// bu: the border bytes in the destination's order, bs: in the sampled order)
template <class Args>
int sampled_channel_table(Args& a, int rgb_order, int64_t dst_plane_stride, const double* scale, const double* bias, const uint8_t* bu, uint8_t* bs) {
    for (int k = 0; k < 3; k++) {
        const int ch = rgb_order ? 2 - k : k;
        const double sc = scale ? scale[ch] : 1.0, bi = bias ? bias[ch] : 0.0;
        if (!isfinite(sc) || !isfinite(bi)) return BEVWARP_ERR_NOT_FINITE;
        a.pscale[k] = (float)sc, a.pbias[k] = (float)bi;
        a.ch_off[k] = (int64_t)ch * dst_plane_stride;
        bs[k] = bu[ch];
    }
    return BEVWARP_OK;
}
// What the map samplers (bevwarp_remap and its NV12 kin) share: the checks and plan_remap's grid of items of frames_per_item frames
// (plan::remap_grid), and in the zeroed arguments the destination, the grid, the source's sides with the index remap of the border mode,
// and the map planes --
// reads[first_map] and, bilinear, reads[first_map + 1].  items = 0: nothing to launch, the status is the call's.
template <class Args>
int remap_grid_args(const Call& c, Args& a, int first_map, int interp, int border_mode, int64_t& items) {
    items = 0;
    RemapPlan p;
    const int st = plan::remap_grid(c, kBorderTileW, kBorderTileH, kRemapMaxFramesPerItem, plan::kRemapFillItems, p);
    if (st != BEVWARP_OK) return st;
    if (c.batch == 0 || p.status != BEVWARP_OK) return p.status;  // (an empty batch: p is zeros)
    memset(&a, 0, sizeof(a));
    const Image& d = c.writes[0].im;
    a.dst = (uint8_t*)d.base, a.dst_fs = d.fs, a.dst_rs = d.rs, a.dst_h = c.dst_h, a.dst_w = c.dst_w;
    copy_grid(a, p);
    a.src_h = c.src_h, a.src_w = c.src_w;
    if (border_mode != BEVWARP_BORDER_CONSTANT && border_mode != BEVWARP_BORDER_TRANSPARENT) {
        const plan::BorderPeriod px = plan::border_period(border_mode, c.src_w), py = plan::border_period(border_mode, c.src_h);
        a.per_x = px.per, a.off_x = px.off, a.mag_x = px.mag;
        a.per_y = py.per, a.off_y = py.off, a.mag_y = py.mag;
    }
    const Image &ixy = c.reads[first_map].im, *ifr = (interp == BEVWARP_LINEAR) ? &c.reads[first_map + 1].im : nullptr;
    a.xy = (const uint8_t*)ixy.base, a.xy_fs = ixy.fs, a.xy_rs = ixy.rs;
    if (ifr) a.frac = (const uint8_t*)ifr->base, a.frac_fs = ifr->fs, a.frac_rs = ifr->rs;
    a.batch = c.batch, a.frames_per_item = p.frames_per_item;
    a.map_vec_ok = plan::map_vec_ok(ixy, ifr);
    items = p.total_tiles;
    return BEVWARP_OK;
}
// One camera of bevwarp_warp_stitch in the kernel's arguments, from its checked call (stitch_call); align: pixel_load_align of its pixels ...
void fill_camera(StitchCamera& s, const Call& c, int align) {
    fill_source(s, c.reads[0].im);
    s.minv = c.minv, s.src_h = c.src_h, s.src_w = c.src_w, s.m_stride = c.m_count == 1 ? 0 : 9;
    s.src_vec_ok = plan::pixel_loads_ok(c.reads[0].im, align);
}
// ... and of a stitch through maps (stitch_maps_call and its kin): what the call reads -- the frames (NV12: Y, then the pairs), the xy plane
// and, bilinear, the frac plane -- and the two flags of its lane-wide accesses
void fill_camera(StitchMapCamera& s, const Call& c, int align) {
    const int first_map = c.even_src ? 2 : 1;
    const Image &src = c.reads[0].im, &ixy = c.reads[first_map].im, *ifr = c.n_reads > first_map + 1 ? &c.reads[first_map + 1].im : nullptr;
    fill_source(s, src);
    if (c.even_src) {
        const Image& uv = c.reads[1].im;
        s.uv = (const uint8_t*)uv.base, s.uv_fs = uv.fs, s.uv_rs = uv.rs;
    }
    s.xy = (const uint8_t*)ixy.base, s.xy_fs = ixy.fs, s.xy_rs = ixy.rs;  // (a shared map: read_map_planes has zeroed its frame strides)
    if (ifr) s.frac = (const uint8_t*)ifr->base, s.frac_fs = ifr->fs, s.frac_rs = ifr->rs;
    s.src_h = c.src_h, s.src_w = c.src_w;
    s.src_vec_ok = plan::pixel_loads_ok(src, align);
    s.map_vec_ok = plan::map_vec_ok(ixy, ifr);
}
// What the seven stitches share: stitch_check over the cameras' calls (describe(cams[k]); values: the HOST arrays, the border value first --
// a stitch with a border mode passes it under the constant border only, `fill`), and for a call that goes on to a launch, in the zeroed
// arguments, the canvas (the image every camera's checked call writes), the grid, the feather width, the border pixel, and every camera
// from its checked call: what was checked is what is launched.  calls: BEVWARP_STITCH_MAX_CAMERAS entries of the caller's, which reads the
// other written images from them.  dtype, channels: of the sampled pixels.  items = 0: nothing to launch, the status is the call's.
// blend: without BEVWARP_STITCH_GAIN (plan::take_gain_flag).  Under the flag a is Gained<> arguments, and stitch_check looks at every
// camera's gain word at its documented place and leaves the checked words in a.gains, taken by value like everything else of the array.
template <class Args>
uint32_t* gains_of(Args&) { return nullptr; }
template <class Args>
uint32_t* gains_of(Gained<Args>& a) { return a.gains; }
template <class Args, class Camera, class Describe>
int stitch_grid_args(Args& a, Call* calls, int64_t& items, const Camera* cams, int n_cams, int blend, int feather, Describe describe,
                     std::initializer_list<plan::HostValues> values, int batch, int dst_h, int dst_w, int dtype, int channels, bool fill) {
    items = 0;
    TilePlan p;
    uint32_t gains[BEVWARP_STITCH_MAX_CAMERAS] = {};
    const int st = plan::stitch_check(cams, n_cams, blend, feather, describe, values, batch, dst_h, dst_w, kBorderTileW, kBorderTileH, p, calls, gains_of(a) ? gains : nullptr);
    if (st != BEVWARP_OK || batch == 0) return st;
    memset(&a, 0, sizeof(a));
    if (uint32_t* g = gains_of(a)) memcpy(g, gains, sizeof(gains));
    const Image& d = calls[0].writes[0].im;
    a.dst = (uint8_t*)d.base, a.dst_fs = d.fs, a.dst_rs = d.rs, a.dst_h = dst_h, a.dst_w = dst_w;
    copy_grid(a, p);
    a.dst_vec_ok = plan::wide_stores_ok(d, plan::store_align(dtype, channels, false));
    for (int k = 0; k < n_cams; k++) fill_camera(a.cams[k], calls[k], plan::pixel_load_align(dtype, channels));
    a.n_cams = n_cams, a.feather = feather, a.fill = fill;
    uint8_t bu[4];  // (stitch_check has found the border value finite)
    border_values(values.begin()->v, channels, a.bv_f, bu);
    a.bv_u8 = packed4(bu);
    items = p.total_tiles;
    return BEVWARP_OK;
}
}  // namespace

#ifdef BEVWARP_CLOCK
namespace bevwarp { hipError_t debug_read_clock(unsigned long long* out4, int reset); }
extern "C" int bevwarp_debug_clock(unsigned long long* out4, int reset) { return (int)bevwarp::debug_read_clock(out4, reset); }
#endif

extern "C" {

int bevwarp_version(void) { return BEVWARP_ABI_VERSION; }

const char* bevwarp_strerror(int status) {
    switch (status) {
        case BEVWARP_OK: return "ok";
        case BEVWARP_ERR_BAD_ARG: return "bad argument (null pointer, non-positive size or misaligned stride)";
        case BEVWARP_ERR_UNSUPPORTED: return "unsupported dtype / channel count / interpolation / border mode";
        case BEVWARP_ERR_TOO_LARGE: return "source image side exceeds 32767 px, a row 16 MiB or a frame 2 GiB";
        case BEVWARP_ERR_NOT_FINITE: return "homography contains NaN or Inf";
        case BEVWARP_ERR_HIP: return "HIP runtime error (see bevwarp_last_hip_error)";
        case BEVWARP_ERR_OVERLAP: return "source and destination overlap in memory (an in-place warp would read taps that other workgroups have already overwritten)";
        default: return "unknown status";
    }
}

const char* bevwarp_last_hip_error(void) { return g_hip_error; }

int bevwarp_invert_homography(const double* S, double* D, int n) {
    if (!S || !D || n < 0) return BEVWARP_ERR_BAD_ARG;
    if (!finite9(S, n)) return BEVWARP_ERR_NOT_FINITE;
    for (int k = 0; k < n; k++, S += 9, D += 9) {
        // cv::invert, 3x3 double: cofactors times 1/det, in this evaluation order
        double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
        if (d == 0.0) {
            memset(D, 0, 9 * sizeof(double));
            continue;
        }
        d = 1.0 / d;
        double t[9];
        t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
        t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
        t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
        t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
        t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
        t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
        t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
        t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
        t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
        memcpy(D, t, sizeof(t));
    }
    return BEVWARP_OK;
}

}  // extern "C"

namespace {
// bevwarp_warp and its planar and verdict-table variants (plane_format: WarpArgs::planar of a planar call)
int warp_impl(const Call& c, int channels, int dtype, int interp, const double* border_value, void* stream, int plane_format = 0, const double* scale = nullptr,
              const double* bias = nullptr, void* classes = nullptr, int classes_mode = 0) {
    const int st = plan::check_call(c);
    if (st != BEVWARP_OK || c.batch == 0) return st;
    const TilePlan p = plan::plan_rows(c.batch, c.dst_h, c.dst_w, dtype, tile_width(dtype), rows_per_pass(), resident_workgroups(dtype, channels, interp));
    if (p.status != BEVWARP_OK) return p.status;

    const Image& s = c.reads[0].im;
    const WrittenImage& d = c.writes[0];
    WarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = (const uint8_t*)s.base, a.dst = (uint8_t*)d.im.base, a.minv = c.minv;
    a.src_fs = s.fs, a.src_rs = s.rs, a.dst_fs = d.im.fs, a.dst_rs = d.im.rs;
    a.src_h = c.src_h, a.src_w = c.src_w, a.dst_h = c.dst_h, a.dst_w = c.dst_w;
    a.m_stride = c.m_count == 1 ? 0 : 9;
    a.batch = c.batch;
    copy_plan(a, p);
    a.dst_vec_ok = plan::wide_stores_ok(d, plan::store_align(dtype, channels, d.planar, d.elem));
    if (d.planar) {
        a.planar = plane_format;
        a.dst_ps = d.plane_stride;
        for (int k = 0; k < 4; k++) {
            const double sc = (scale && k < channels) ? scale[k] : 1.0, bi = (bias && k < channels) ? bias[k] : 0.0;
            if (!isfinite(sc) || !isfinite(bi)) return BEVWARP_ERR_NOT_FINITE;
            a.pscale[k] = (float)sc;
            a.pbias[k] = (float)bi;
        }
    }
    if (border_values(border_value, channels, a.bval_f, a.bval_u8) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    if (classes) {
        if ((uintptr_t)classes % 4) return BEVWARP_ERR_BAD_ARG;
        if (classes_mode == BEVWARP_CLASSES_FILL)
            a.classify_out = (uint32_t*)classes;
        else
            a.tile_class = (const uint32_t*)classes;
    }
    return launched(launch_warp(a, dtype, channels, interp, (hipStream_t)stream));
}
// bevwarp_warp_border under BEVWARP_SUPERSAMPLE_* (c, st, p: plan::supersample_grid's; k = c.supersample): the border kernel's arguments,
// the border pixel of the constant border, and the fine matrix's two constants
int supersample_impl(const Call& c, int checked, const TilePlan& p, int channels, int dtype, int interp, int border_mode, const double* border_value, void* stream) {
    SupersampleArgs a;
    int64_t items;
    const int st = flat_grid_args(c, checked, p, a, items);
    if (!items) return st;
    fill_source(a, c.reads[0].im);
    const bool constant = border_mode == BEVWARP_BORDER_CONSTANT;
    if (!constant) {
        const plan::BorderPeriod px = plan::border_period(border_mode, c.src_w), py = plan::border_period(border_mode, c.src_h);
        a.per_x = px.per, a.off_x = px.off, a.mag_x = px.mag;
        a.per_y = py.per, a.off_y = py.off, a.mag_y = py.mag;
    }
    uint8_t bu[4];  // (border_value is read by the constant border only)
    if (border_values(constant ? border_value : nullptr, channels, a.bv_f, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    a.bv_u8 = packed4(bu);
    const int k = c.supersample;
    a.log2k = k == 2 ? 1 : (k == 4 ? 2 : 3);
    a.inv_k = 1.0 / k, a.centre = (1.0 - k) / (2.0 * k);
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(dtype, channels, false));
    a.src_vec_ok = plan::pixel_loads_ok(c.reads[0].im, plan::pixel_load_align(dtype, channels));
    return launched(launch_warp_supersample(a, dtype, channels, interp, border_mode, items, (hipStream_t)stream));
}
}  // namespace

extern "C" {

int bevwarp_warp(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                 int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, const double* M_inv,
                 int m_count, int dtype, int interp, const double* border_value, void* stream) {
    if (interp == BEVWARP_CUBIC)  // the bicubic kernel has every border, the constant one included
        return bevwarp_warp_border(src, dst, batch, src_h, src_w, dst_h, dst_w, channels, src_frame_stride, src_row_stride, dst_frame_stride, dst_row_stride,
                                   M_inv, m_count, dtype, interp, BEVWARP_BORDER_CONSTANT, border_value, stream);
    return warp_impl(plan::warp_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv},
                                     channels, dtype, interp, false),
                     channels, dtype, interp, border_value, stream);
}

int bevwarp_warp_border(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                        int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, const double* M_inv,
                        int m_count, int dtype, int interp, int border_mode, const double* border_value, void* stream) {
    const int k = plan::take_supersample(interp);
    if (k > 1) {  // the supersampled warp: a kernel of its own for all five borders it has, the constant one included
        Call c;
        TilePlan p;
        const int st = plan::supersample_grid({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride},
                                              {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv}, channels, dtype, interp, border_mode, k, kBorderTileW, kBorderTileH, c, p);
        return supersample_impl(c, st, p, channels, dtype, interp, border_mode, border_value, stream);
    }
    const bool cubic = interp == BEVWARP_CUBIC;
    if (border_mode == BEVWARP_BORDER_CONSTANT && !cubic)  // the constant border is bevwarp_warp itself
        return bevwarp_warp(src, dst, batch, src_h, src_w, dst_h, dst_w, channels, src_frame_stride, src_row_stride, dst_frame_stride, dst_row_stride,
                            M_inv, m_count, dtype, interp, border_value, stream);
    if (!plan::border_mode_known(border_mode)) return BEVWARP_ERR_UNSUPPORTED;  // (BORDER_ISOLATED too)
    // (border_value is read by no mode but the constant one, as in OpenCV)
    const Call c = plan::warp_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv},
                                   channels, dtype, interp, true);
    CubicArgs a;  // (the border kernel takes its BorderArgs part)
    int64_t items;
    const int st = flat_grid_args(c, a, items);
    if (!items) return st;
    fill_source(a, c.reads[0].im);
    // the 4 taps of a bicubic window reach one index beyond a saturated one: a period plan of their own
    const plan::BorderPeriod px = cubic ? cubic::window_period(border_mode, src_w) : plan::border_period(border_mode, src_w);
    const plan::BorderPeriod py = cubic ? cubic::window_period(border_mode, src_h) : plan::border_period(border_mode, src_h);
    a.per_x = px.per, a.off_x = px.off, a.mag_x = px.mag;
    a.per_y = py.per, a.off_y = py.off, a.mag_y = py.mag;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(dtype, channels, false));
    a.src_vec_ok = plan::pixel_loads_ok(c.reads[0].im, plan::pixel_load_align(dtype, channels));
    if (!cubic) return launched(launch_warp_border(a, dtype, channels, interp, border_mode, items, (hipStream_t)stream));
    if (border_values(border_mode == BEVWARP_BORDER_CONSTANT ? border_value : nullptr, channels, a.cv_f, a.cv_u8) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    return launched(launch_warp_cubic(a, dtype, channels, border_mode, items, (hipStream_t)stream));
}

int bevwarp_warp_lens(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels, int64_t src_frame_stride,
                      int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, const double* M_ray, int m_count, const double* lens,
                      double r2_max, int dtype, int interp, int border_mode, const double* border_value, void* stream) {
    const bool fisheye = plan::take_fisheye_flag(interp);
    const Call c = plan::lens_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, {batch, src_h, src_w, dst_h, dst_w, m_count, M_ray},
                                   channels, dtype, interp, border_mode);
    LensArgs a;
    int64_t items;
    int st = flat_grid_args(c, a, items);
    if (!items) return st;
    if ((st = plan::lens_model_status(fisheye, lens, r2_max)) != BEVWARP_OK) return st;
    const bool transparent = border_mode == BEVWARP_BORDER_TRANSPARENT;
    uint8_t bu[4];  // (border_value is read by the constant border only)
    if (border_values(transparent ? nullptr : border_value, channels, a.bv_f, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    a.bv_u8 = packed4(bu);
    fill_source(a, c.reads[0].im);
    memcpy(a.lens, lens, sizeof(a.lens));
    a.r2_max = r2_max;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(dtype, channels, false));
    a.src_vec_ok = plan::pixel_loads_ok(c.reads[0].im, plan::pixel_load_align(dtype, channels));
    return launched((fisheye ? launch_warp_fisheye : launch_warp_lens)(a, dtype, channels, interp, transparent, items, (hipStream_t)stream));
}

int bevwarp_build_map(const double* M, int m_count, const double* lens, double r2_max, int interp, void* map_xy, void* map_frac, int dst_h, int dst_w,
                      int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride, void* stream) {
    const Frames xy = {map_xy, xy_frame_stride, xy_row_stride}, fr = {map_frac, frac_frame_stride, frac_row_stride};
    TilePlan p;
    const bool fisheye = plan::take_fisheye_flag(interp);
    const int st = plan::build_map_model_status(fisheye, M, m_count, lens, r2_max, interp, xy, fr, dst_h, dst_w, kBorderTileW, kBorderTileH, p);
    if (st != BEVWARP_OK) return st;
    const bool linear = interp == BEVWARP_LINEAR;
    MapBuildArgs a;
    memset(&a, 0, sizeof(a));
    a.dst = (uint8_t*)map_xy, a.minv = M, a.m_stride = 9;
    a.dst_fs = m_count == 1 ? 0 : xy_frame_stride, a.dst_rs = xy_row_stride, a.dst_h = dst_h, a.dst_w = dst_w;
    a.frac = linear ? (uint8_t*)map_frac : nullptr, a.frac_fs = m_count == 1 ? 0 : frac_frame_stride, a.frac_rs = frac_row_stride;
    copy_grid(a, p);
    const Image ixy = Frames{map_xy, a.dst_fs, xy_row_stride}.image(dst_h, (uint64_t)dst_w * 4, m_count);
    const Image ifr = Frames{map_frac, a.frac_fs, frac_row_stride}.image(dst_h, (uint64_t)dst_w * 2, m_count);
    a.dst_vec_ok = plan::map_vec_ok(ixy, linear ? &ifr : nullptr);
    if (lens) memcpy(a.lens, lens, sizeof(a.lens)), a.r2_max = r2_max;
    if (fisheye) return launched(launch_build_map_fisheye(a, interp, p.total_tiles, (hipStream_t)stream));
    return launched(launch_build_map(a, interp, lens != nullptr, p.total_tiles, (hipStream_t)stream));
}

int bevwarp_remap(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels, int64_t src_frame_stride,
                  int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, const void* map_xy, const void* map_frac, int map_count,
                  int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride, int dtype, int interp, int border_mode,
                  const double* border_value, void* stream) {
    const bool bicubic = plan::take_map_bicubic_flag(interp);
    const Call c = plan::remap_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, {map_xy, xy_frame_stride, xy_row_stride},
                                    {map_frac, frac_frame_stride, frac_row_stride}, {batch, src_h, src_w, dst_h, dst_w, 0, nullptr}, map_count, channels, dtype,
                                    interp, border_mode, bicubic);
    RemapArgs a;
    int64_t items;
    const int st = remap_grid_args(c, a, 1, interp, border_mode, items);
    if (!items) return st;
    if (bicubic) {  // the 4 taps of a bicubic window reach one index beyond a saturated one: bevwarp_warp_border's period plan, every mode
        const plan::BorderPeriod px = cubic::window_period(border_mode, src_w), py = cubic::window_period(border_mode, src_h);
        a.per_x = px.per, a.off_x = px.off, a.mag_x = px.mag;
        a.per_y = py.per, a.off_y = py.off, a.mag_y = py.mag;
    }
    uint8_t bu[4];  // (border_value is read by the constant border only)
    if (border_values(border_mode == BEVWARP_BORDER_CONSTANT ? border_value : nullptr, channels, a.bv_f, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    a.bv_u8 = packed4(bu);
    fill_source(a, c.reads[0].im);
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(dtype, channels, false));
    a.src_vec_ok = plan::pixel_loads_ok(c.reads[0].im, plan::pixel_load_align(dtype, channels));
    if (bicubic) return launched(launch_remap_cubic(a, dtype, channels, border_mode, items, (hipStream_t)stream));
    return launched(launch_remap(a, dtype, channels, interp, border_mode, items, (hipStream_t)stream));
}

int bevwarp_remap_nv12(const void* y, const void* uv, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t y_frame_stride,
                       int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                       const void* map_xy, const void* map_frac, int map_count, int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride,
                       int64_t frac_row_stride, int interp, int border_mode, int rgb_order, const double* border_value, void* stream) {
    const Call c = plan::remap_nv12_call({y, y_frame_stride, y_row_stride}, {uv, uv_frame_stride, uv_row_stride}, {dst, dst_frame_stride, dst_row_stride},
                                         {map_xy, xy_frame_stride, xy_row_stride}, {map_frac, frac_frame_stride, frac_row_stride},
                                         {batch, src_h, src_w, dst_h, dst_w, 0, nullptr}, map_count, interp, rgb_order, border_mode);
    RemapNv12Args a;
    int64_t items;
    const int st = remap_grid_args(c, a, 2, interp, border_mode, items);
    if (!items) return st;
    uint8_t bu[4];  // (in the destination's channel order, as given: the border value is not converted; read by the constant border only)
    if (border_bytes(border_mode == BEVWARP_BORDER_CONSTANT ? border_value : nullptr, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    fill_nv12_source(a, c);
    a.bv_u8 = packed3(bu);
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(BEVWARP_U8, 3, false));
    return launched(launch_remap_nv12(a, interp, border_mode, rgb_order, items, (hipStream_t)stream));
}

int bevwarp_remap_nv12_planes(const void* y, const void* uv, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t y_frame_stride,
                              int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                              int64_t dst_row_stride, const void* map_xy, const void* map_frac, int map_count, int64_t xy_frame_stride, int64_t xy_row_stride,
                              int64_t frac_frame_stride, int64_t frac_row_stride, int interp, int border_mode, int rgb_order, const double* border_value,
                              const double* scale, const double* bias, int plane_dtype, void* stream) {
    const Call c = plan::remap_nv12_planes_call({y, y_frame_stride, y_row_stride}, {uv, uv_frame_stride, uv_row_stride}, {dst, dst_frame_stride, dst_row_stride},
                                                dst_plane_stride, {map_xy, xy_frame_stride, xy_row_stride}, {map_frac, frac_frame_stride, frac_row_stride},
                                                {batch, src_h, src_w, dst_h, dst_w, 0, nullptr}, map_count, interp, rgb_order, border_mode, plane_dtype);
    RemapNv12PlanesArgs a;
    int64_t items;
    const int st = remap_grid_args(c, a, 2, interp, border_mode, items);
    if (!items) return st;
    uint8_t bu[4];  // (in the destination's channel order, as given; read by the constant border only)
    if (border_bytes(border_mode == BEVWARP_BORDER_CONSTANT ? border_value : nullptr, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(BEVWARP_U8, 3, true, c.writes[0].elem));
    a.plane = plane_kind(plane_dtype);
    uint8_t bs[3];
    if (sampled_channel_table(a, rgb_order, dst_plane_stride, scale, bias, bu, bs) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    fill_nv12_source(a, c);
    a.bv_u8 = packed3(bs);
    return launched(launch_remap_nv12_planes(a, interp, border_mode, items, (hipStream_t)stream));
}

int bevwarp_warp_stitch(const bevwarp_camera* cams, int n_cams, void* dst, int batch, int dst_h, int dst_w, int channels, int64_t dst_frame_stride,
                        int64_t dst_row_stride, int dtype, int interp, int blend, int feather, int border_mode, const double* border_value, void* stream) {
    const Frames d = {dst, dst_frame_stride, dst_row_stride};
    const bool fill = border_mode == BEVWARP_BORDER_CONSTANT;  // (border_value is read by the constant border only)
    Call calls[BEVWARP_STITCH_MAX_CAMERAS];
    StitchArgs a;
    int64_t items;
    const int st = stitch_grid_args(
        a, calls, items, cams, n_cams, blend, feather, [&](const bevwarp_camera& k) { return plan::stitch_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, border_mode); },
        {{fill ? border_value : nullptr, channels}}, batch, dst_h, dst_w, dtype, channels, fill);
    if (!items) return st;
    return launched(launch_warp_stitch(a, dtype, channels, interp, blend, items, (hipStream_t)stream));
}

int bevwarp_stitch_maps(const bevwarp_map_camera* cams, int n_cams, void* dst, int batch, int dst_h, int dst_w, int channels, int64_t dst_frame_stride,
                        int64_t dst_row_stride, int dtype, int interp, int blend, int feather, int border_mode, const double* border_value, void* stream) {
    const Frames d = {dst, dst_frame_stride, dst_row_stride};
    const bool fill = border_mode == BEVWARP_BORDER_CONSTANT;  // (border_value is read by the constant border only)
    const bool gained = plan::take_gain_flag(blend);
    Call calls[BEVWARP_STITCH_MAX_CAMERAS];
    int64_t items;
    const auto run = [&](auto& a, auto launch) {
        const int st = stitch_grid_args(
            a, calls, items, cams, n_cams, blend, feather,
            [&](const bevwarp_map_camera& k) { return plan::stitch_maps_call(k, d, batch, dst_h, dst_w, channels, dtype, interp, blend, border_mode, gained); },
            {{fill ? border_value : nullptr, channels}}, batch, dst_h, dst_w, dtype, channels, fill);
        return items ? launched(launch(a, dtype, channels, interp, blend, items, (hipStream_t)stream)) : st;
    };
    if (gained) {
        Gained<StitchMapsArgs> a;
        return run(a, launch_stitch_gain);
    }
    StitchMapsArgs a;
    return run(a, launch_stitch_maps);
}

int bevwarp_stitch_maps_nv12(const bevwarp_map_camera* cams, int n_cams, void* dst, int batch, int dst_h, int dst_w, int64_t dst_frame_stride, int64_t dst_row_stride,
                             int interp, int blend, int feather, int rgb_order, int border_mode, const double* border_value, void* stream) {
    const Frames d = {dst, dst_frame_stride, dst_row_stride};
    const bool fill = border_mode == BEVWARP_BORDER_CONSTANT;  // (border_value is read by the constant border only)
    const bool gained = plan::take_gain_flag(blend);
    Call calls[BEVWARP_STITCH_MAX_CAMERAS];
    int64_t items;
    const auto run = [&](auto& a, auto launch) {  // (the border value is in the destination's channel order, as given: it is not converted)
        const int st = stitch_grid_args(
            a, calls, items, cams, n_cams, blend, feather,
            [&](const bevwarp_map_camera& k) { return plan::stitch_maps_nv12_call(k, d, batch, dst_h, dst_w, interp, blend, rgb_order, border_mode); },
            {{fill ? border_value : nullptr, 3}}, batch, dst_h, dst_w, BEVWARP_U8, 3, fill);
        return items ? launched(launch(a, interp, blend, rgb_order, items, (hipStream_t)stream)) : st;
    };
    if (gained) {
        Gained<StitchMapsArgs> a;
        return run(a, launch_stitch_gain_nv12);
    }
    StitchMapsArgs a;
    return run(a, launch_stitch_maps_nv12);
}

int bevwarp_warp_nv12(const void* y, const void* uv, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t y_frame_stride,
                      int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                      const double* M_inv, int m_count, int interp, int rgb_order, const double* border_value, void* stream) {
    const Call c = plan::nv12_call({y, y_frame_stride, y_row_stride}, {uv, uv_frame_stride, uv_row_stride}, {dst, dst_frame_stride, dst_row_stride},
                                   {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv}, interp, rgb_order);
    Nv12Args a;
    int64_t items;
    const int st = flat_grid_args(c, a, items);
    if (!items) return st;
    uint8_t bu[4];  // (in the destination's channel order, as given: the border value is not converted)
    if (border_bytes(border_value, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    fill_nv12_source(a, c);
    a.border = packed3(bu);
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(BEVWARP_U8, 3, false));
    return launched(launch_warp_nv12(a, interp, rgb_order, items, (hipStream_t)stream));
}

int bevwarp_warp_nv12_planes(const void* y, const void* uv, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t y_frame_stride,
                             int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                             int64_t dst_row_stride, const double* M_inv, int m_count, int interp, int rgb_order, const double* border_value,
                             const double* scale, const double* bias, int plane_dtype, void* stream) {
    const Call c = plan::nv12_planes_call({y, y_frame_stride, y_row_stride}, {uv, uv_frame_stride, uv_row_stride}, {dst, dst_frame_stride, dst_row_stride},
                                          dst_plane_stride, {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv}, interp, rgb_order, plane_dtype);
    Nv12PlanesArgs a;
    int64_t items;
    const int st = flat_grid_args(c, a, items);
    if (!items) return st;
    uint8_t bu[4];  // (in the destination's channel order, as given)
    if (border_bytes(border_value, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(BEVWARP_U8, 3, true, c.writes[0].elem));
    a.plane = plane_kind(plane_dtype);
    uint8_t bs[3];
    if (sampled_channel_table(a, rgb_order, dst_plane_stride, scale, bias, bu, bs) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    fill_nv12_source(a, c);
    a.border = packed3(bs);
    return launched(launch_warp_nv12_planes(a, interp, items, (hipStream_t)stream));
}

}  // extern "C"

namespace {
// bevwarp_warp_to_nv12 and bevwarp_warp_nv12_to_nv12 (the call reads two images): the checks, plan_border's grid, the border pixel, one launch
int warp_nv12_out_impl(const Call& c, int interp, int rgb_order, const double* border_value, void* stream) {
    Nv12OutArgs a;
    int64_t items;
    const int st = flat_grid_args(c, a, items);
    if (!items) return st;
    uint8_t bu[4];  // (in the warped pixel's channel order: a pixel value, converted by the kernel like any other)
    if (border_bytes(border_value, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    const Image& duv = c.writes[1].im;
    a.dst_uv = (uint8_t*)duv.base, a.duv_fs = duv.fs, a.duv_rs = duv.rs;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], 4);  // per plane: a lane's 4 Y bytes, and its two pairs, go out as one dword each
    a.uv_vec_ok = plan::wide_stores_ok(c.writes[1], 4);
    const bool nv12_src = c.n_reads == 2;
    if (nv12_src)
        fill_nv12_source(a, c);
    else
        fill_source(a, c.reads[0].im);
    a.border = packed3(bu);
    return launched(launch_warp_nv12_out(a, nv12_src, interp, rgb_order, items, (hipStream_t)stream));
}
}  // namespace

extern "C" {

int bevwarp_warp_to_nv12(const void* src, void* dst_y, void* dst_uv, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t src_frame_stride,
                         int64_t src_row_stride, int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride,
                         const double* M_inv, int m_count, int interp, int rgb_order, const double* border_value, void* stream) {
    return warp_nv12_out_impl(plan::to_nv12_call({src, src_frame_stride, src_row_stride}, {dst_y, y_frame_stride, y_row_stride}, {dst_uv, uv_frame_stride, uv_row_stride},
                                                 {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv}, interp, rgb_order),
                              interp, rgb_order, border_value, stream);
}

int bevwarp_warp_nv12_to_nv12(const void* y, const void* uv, void* dst_y, void* dst_uv, int batch, int src_h, int src_w, int dst_h, int dst_w,
                              int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int64_t dst_y_frame_stride,
                              int64_t dst_y_row_stride, int64_t dst_uv_frame_stride, int64_t dst_uv_row_stride, const double* M_inv, int m_count,
                              int interp, const double* border_value, void* stream) {
    return warp_nv12_out_impl(plan::nv12_to_nv12_call({y, y_frame_stride, y_row_stride}, {uv, uv_frame_stride, uv_row_stride}, {dst_y, dst_y_frame_stride, dst_y_row_stride},
                                                      {dst_uv, dst_uv_frame_stride, dst_uv_row_stride}, {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv}, interp),
                              interp, 0, border_value, stream);
}

}  // extern "C"

namespace {
// bevwarp_remap_to_nv12 and bevwarp_remap_nv12_to_nv12 (the call reads two planes of frames): the checks, plan_remap's grid, the border pixel,
// one launch
int remap_nv12_out_impl(const Call& c, int interp, int border_mode, int rgb_order, const double* border_value, void* stream) {
    const bool nv12_src = c.even_src;
    RemapNv12OutArgs a;
    int64_t items;
    const int st = remap_grid_args(c, a, nv12_src ? 2 : 1, interp, border_mode, items);
    if (!items) return st;
    uint8_t bu[4];  // (in the sampled pixel's channel order: a pixel value, converted by the kernel like any other; read by the constant border only)
    if (border_bytes(border_mode == BEVWARP_BORDER_CONSTANT ? border_value : nullptr, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    const Image& duv = c.writes[1].im;
    a.dst_uv = (uint8_t*)duv.base, a.duv_fs = duv.fs, a.duv_rs = duv.rs;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], 4);  // per plane: a lane's 4 Y bytes, and its two pairs, go out as one dword each
    a.uv_vec_ok = plan::wide_stores_ok(c.writes[1], 4);
    if (nv12_src)
        fill_nv12_source(a, c);
    else
        fill_source(a, c.reads[0].im);
    a.bv_u8 = packed3(bu);
    return launched(launch_remap_nv12_out(a, nv12_src, interp, border_mode, rgb_order, items, (hipStream_t)stream));
}
// bevwarp_stitch_maps_to_nv12 and bevwarp_stitch_maps_nv12_to_nv12
int stitch_maps_nv12_out_impl(bool nv12_src, const bevwarp_map_camera* cams, int n_cams, const Frames& dy, const Frames& duv, int batch, int dst_h, int dst_w, int interp,
                              int blend, int feather, int rgb_order, const double* border_value, void* stream) {
    const bool gained = plan::take_gain_flag(blend);
    Call calls[BEVWARP_STITCH_MAX_CAMERAS];
    int64_t items;
    const auto run = [&](auto& a, auto launch) {  // (the border value is a pixel in the sampled pixel's channel order: the kernel converts it like any other)
        const int st = stitch_grid_args(
            a, calls, items, cams, n_cams, blend, feather,
            [&](const bevwarp_map_camera& k) { return plan::stitch_maps_nv12_out_call(nv12_src, k, dy, duv, batch, dst_h, dst_w, interp, blend, nv12_src ? 0 : rgb_order); },
            {{border_value, 3}}, batch, dst_h, dst_w, BEVWARP_U8, 3, true);
        if (!items) return st;
        const Image &y = calls[0].writes[0].im, &uv = calls[0].writes[1].im;
        a.dst_uv = (uint8_t*)uv.base, a.duv_fs = uv.fs, a.duv_rs = uv.rs;
        a.dst_vec_ok = plan::wide_stores_ok(y, 4);  // per plane, as bevwarp_warp_to_nv12
        a.uv_vec_ok = plan::wide_stores_ok(uv, 4);
        return launched(launch(a, nv12_src, interp, blend, rgb_order, items, (hipStream_t)stream));
    };
    if (gained) {
        Gained<StitchMapsNv12OutArgs> a;
        return run(a, launch_stitch_gain_nv12_out);
    }
    StitchMapsNv12OutArgs a;
    return run(a, launch_stitch_maps_nv12_out);
}
// bevwarp_stitch_maps_planes and bevwarp_stitch_maps_nv12_planes
int stitch_maps_planes_impl(bool nv12_src, const bevwarp_map_camera* cams, int n_cams, const Frames& d, int64_t dst_plane_stride, int batch, int dst_h, int dst_w,
                            int interp, int blend, int feather, int rgb_order, const double* border_value, const double* scale, const double* bias, int plane_dtype,
                            void* stream) {
    const bool gained = plan::take_gain_flag(blend);
    Call calls[BEVWARP_STITCH_MAX_CAMERAS];
    int64_t items;
    const auto run = [&](auto& a, auto launch) {  // (border value, scale and bias are in the planes' channel order: the kernel converts NV12 taps to that order)
        const int st = stitch_grid_args(
            a, calls, items, cams, n_cams, blend, feather,
            [&](const bevwarp_map_camera& k) {
                return plan::stitch_maps_planes_call(nv12_src, k, d, dst_plane_stride, batch, dst_h, dst_w, interp, blend, nv12_src ? rgb_order : 0, plane_dtype);
            },
            {{border_value, 3}, {scale, 3}, {bias, 3}}, batch, dst_h, dst_w, BEVWARP_U8, 3, true);
        if (!items) return st;
        const WrittenImage& w = calls[0].writes[0];
        a.dst_vec_ok = plan::wide_stores_ok(w, plan::store_align(BEVWARP_U8, 3, true, w.elem));
        a.plane = plane_kind(plane_dtype);
        uint8_t bu[4] = {(uint8_t)a.bv_u8, (uint8_t)(a.bv_u8 >> 8), (uint8_t)(a.bv_u8 >> 16), 0}, bs[3];
        sampled_channel_table(a, 0, dst_plane_stride, scale, bias, bu, bs);  // (the identity; stitch_check has found scale and bias finite)
        return launched(launch(a, nv12_src, interp, blend, rgb_order, items, (hipStream_t)stream));
    };
    if (gained) {
        Gained<StitchMapsPlanesArgs> a;
        return run(a, launch_stitch_gain_planes);
    }
    StitchMapsPlanesArgs a;
    return run(a, launch_stitch_maps_planes);
}
}  // namespace

extern "C" {

int bevwarp_remap_to_nv12(const void* src, void* dst_y, void* dst_uv, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t src_frame_stride,
                          int64_t src_row_stride, int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, const void* map_xy,
                          const void* map_frac, int map_count, int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride,
                          int interp, int border_mode, int rgb_order, const double* border_value, void* stream) {
    return remap_nv12_out_impl(plan::remap_to_nv12_call({src, src_frame_stride, src_row_stride}, {dst_y, y_frame_stride, y_row_stride},
                                                        {dst_uv, uv_frame_stride, uv_row_stride}, {map_xy, xy_frame_stride, xy_row_stride},
                                                        {map_frac, frac_frame_stride, frac_row_stride}, {batch, src_h, src_w, dst_h, dst_w, 0, nullptr}, map_count, interp,
                                                        rgb_order, border_mode),
                               interp, border_mode, rgb_order, border_value, stream);
}

int bevwarp_remap_nv12_to_nv12(const void* y, const void* uv, void* dst_y, void* dst_uv, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t y_frame_stride,
                               int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int64_t dst_y_frame_stride, int64_t dst_y_row_stride,
                               int64_t dst_uv_frame_stride, int64_t dst_uv_row_stride, const void* map_xy, const void* map_frac, int map_count, int64_t xy_frame_stride,
                               int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride, int interp, int border_mode, const double* border_value,
                               void* stream) {
    return remap_nv12_out_impl(plan::remap_nv12_to_nv12_call({y, y_frame_stride, y_row_stride}, {uv, uv_frame_stride, uv_row_stride},
                                                             {dst_y, dst_y_frame_stride, dst_y_row_stride}, {dst_uv, dst_uv_frame_stride, dst_uv_row_stride},
                                                             {map_xy, xy_frame_stride, xy_row_stride}, {map_frac, frac_frame_stride, frac_row_stride},
                                                             {batch, src_h, src_w, dst_h, dst_w, 0, nullptr}, map_count, interp, border_mode),
                               interp, border_mode, 0, border_value, stream);
}

int bevwarp_stitch_maps_to_nv12(const bevwarp_map_camera* cams, int n_cams, void* dst_y, void* dst_uv, int batch, int dst_h, int dst_w, int64_t y_frame_stride,
                                int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int interp, int blend, int feather, int rgb_order,
                                const double* border_value, void* stream) {
    return stitch_maps_nv12_out_impl(false, cams, n_cams, {dst_y, y_frame_stride, y_row_stride}, {dst_uv, uv_frame_stride, uv_row_stride}, batch, dst_h, dst_w, interp,
                                     blend, feather, rgb_order, border_value, stream);
}

int bevwarp_stitch_maps_nv12_to_nv12(const bevwarp_map_camera* cams, int n_cams, void* dst_y, void* dst_uv, int batch, int dst_h, int dst_w, int64_t y_frame_stride,
                                     int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride, int interp, int blend, int feather,
                                     const double* border_value, void* stream) {
    return stitch_maps_nv12_out_impl(true, cams, n_cams, {dst_y, y_frame_stride, y_row_stride}, {dst_uv, uv_frame_stride, uv_row_stride}, batch, dst_h, dst_w, interp,
                                     blend, feather, 0, border_value, stream);
}

int bevwarp_remap_planes(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int64_t src_frame_stride, int64_t src_row_stride,
                         int64_t dst_frame_stride, int64_t dst_plane_stride, int64_t dst_row_stride, const void* map_xy, const void* map_frac, int map_count,
                         int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride, int interp, int border_mode,
                         const double* border_value, const double* scale, const double* bias, int plane_dtype, void* stream) {
    const Call c = plan::remap_planes_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, dst_plane_stride,
                                           {map_xy, xy_frame_stride, xy_row_stride}, {map_frac, frac_frame_stride, frac_row_stride},
                                           {batch, src_h, src_w, dst_h, dst_w, 0, nullptr}, map_count, interp, border_mode, plane_dtype);
    RemapPlanesArgs a;
    int64_t items;
    const int st = remap_grid_args(c, a, 1, interp, border_mode, items);
    if (!items) return st;
    uint8_t bu[4];  // (the 8-bit border pixel in the frames' channel order; read by the constant border only)
    if (border_bytes(border_mode == BEVWARP_BORDER_CONSTANT ? border_value : nullptr, bu) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    a.dst_vec_ok = plan::wide_stores_ok(c.writes[0], plan::store_align(BEVWARP_U8, 3, true, c.writes[0].elem));
    a.plane = plane_kind(plane_dtype);
    uint8_t bs[3];  // (plane k is channel k: the table is the identity)
    if (sampled_channel_table(a, 0, dst_plane_stride, scale, bias, bu, bs) != BEVWARP_OK) return BEVWARP_ERR_NOT_FINITE;
    fill_source(a, c.reads[0].im);
    a.bv_u8 = packed3(bs);
    return launched(launch_remap_planes(a, interp, border_mode, items, (hipStream_t)stream));
}

int bevwarp_stitch_maps_planes(const bevwarp_map_camera* cams, int n_cams, void* dst, int batch, int dst_h, int dst_w, int64_t dst_frame_stride,
                               int64_t dst_plane_stride, int64_t dst_row_stride, int interp, int blend, int feather, const double* border_value,
                               const double* scale, const double* bias, int plane_dtype, void* stream) {
    return stitch_maps_planes_impl(false, cams, n_cams, {dst, dst_frame_stride, dst_row_stride}, dst_plane_stride, batch, dst_h, dst_w, interp, blend, feather, 0,
                                   border_value, scale, bias, plane_dtype, stream);
}

int bevwarp_stitch_maps_nv12_planes(const bevwarp_map_camera* cams, int n_cams, void* dst, int batch, int dst_h, int dst_w, int64_t dst_frame_stride,
                                    int64_t dst_plane_stride, int64_t dst_row_stride, int interp, int blend, int feather, int rgb_order,
                                    const double* border_value, const double* scale, const double* bias, int plane_dtype, void* stream) {
    return stitch_maps_planes_impl(true, cams, n_cams, {dst, dst_frame_stride, dst_row_stride}, dst_plane_stride, batch, dst_h, dst_w, interp, blend, feather,
                                   rgb_order, border_value, scale, bias, plane_dtype, stream);
}

int bevwarp_warp_classes(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels, int64_t src_frame_stride,
                         int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, const double* M_inv, int m_count, int dtype, int interp,
                         const double* border_value, void* classes, int mode, void* stream) {
    if (!classes || (mode != BEVWARP_CLASSES_USE && mode != BEVWARP_CLASSES_FILL)) return BEVWARP_ERR_BAD_ARG;
    return warp_impl(plan::warp_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv},
                                     channels, dtype, interp, false),
                     channels, dtype, interp, border_value, stream, 0, nullptr, nullptr, classes, mode);
}

// The table of a launch geometry -- full tile, upper half, lower half per tile -- or the status of the warp it describes (tightly
// packed frames, one matrix).  Sizes and format only: no pointer is involved.
int64_t bevwarp_tile_classes_bytes(int batch, int src_h, int src_w, int dst_h, int dst_w, int channels, int dtype, int interp) {
    if (batch <= 0) return 0;
    Call c = plan::warp_call({}, {}, {batch, src_h, src_w, dst_h, dst_w, 1, nullptr}, channels, dtype, interp, false);
    c.reads[0].im.rs = (int64_t)c.reads[0].im.row_bytes;
    int st;
    if ((st = plan::sides_status(c)) != BEVWARP_OK || (st = plan::format_status(c)) != BEVWARP_OK || (st = plan::source_sizes_status(c)) != BEVWARP_OK) return st;
    const TilePlan p = plan::plan_rows(batch, dst_h, dst_w, dtype, tile_width(dtype), rows_per_pass(), resident_workgroups(dtype, channels, interp));
    return p.status != BEVWARP_OK ? (int64_t)p.status : 3 * p.total_tiles * (int64_t)sizeof(uint32_t);
}

int bevwarp_warp_planar(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                        int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                        int64_t dst_row_stride, const double* M_inv, int m_count, int dtype, int interp, const double* border_value,
                        const double* scale, const double* bias, void* stream) {
    return bevwarp_warp_planes(src, dst, batch, src_h, src_w, dst_h, dst_w, channels, src_frame_stride, src_row_stride, dst_frame_stride, dst_plane_stride,
                               dst_row_stride, M_inv, m_count, dtype, interp, border_value, scale, bias, BEVWARP_F32, stream);
}

int bevwarp_warp_planes(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                        int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                        int64_t dst_row_stride, const double* M_inv, int m_count, int dtype, int interp, const double* border_value,
                        const double* scale, const double* bias, int plane_dtype, void* stream) {
    if (plane_dtype != BEVWARP_F32 && plane_dtype != BEVWARP_F16 && plane_dtype != BEVWARP_BF16) return BEVWARP_ERR_UNSUPPORTED;
    return warp_impl(plan::warp_call({src, src_frame_stride, src_row_stride}, {dst, dst_frame_stride, dst_row_stride}, {batch, src_h, src_w, dst_h, dst_w, m_count, M_inv},
                                     channels, dtype, interp, false, plan::plane_elem_size(plane_dtype), dst_plane_stride),
                     channels, dtype, interp, border_value, stream, plane_kind(plane_dtype), scale, bias);
}

int bevwarp_composite(const void* bg, const void* fg, const void* mask, void* out, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && (!bg || !fg || !mask || !out))) return BEVWARP_ERR_BAD_ARG;
    return launched(launch_composite((const uint8_t*)bg, (const uint8_t*)fg, (const uint8_t*)mask, (uint8_t*)out, n, (hipStream_t)stream));
}

int bevwarp_warp_composite(const void* bg, int bg_h, int bg_w, int64_t bg_row_stride, const void* fg, const void* mask, int fg_h, int fg_w,
                           int64_t fg_row_stride, int64_t mask_row_stride, void* dst, int dst_h, int dst_w, int64_t dst_row_stride, int channels,
                           const double* M_inv_bg, const double* M_inv_cam, int fg_gray, void* stream) {
    if (!bg || !fg || !mask || !dst || !M_inv_bg || !M_inv_cam) return BEVWARP_ERR_BAD_ARG;
    if (bg_h <= 0 || bg_w <= 0 || fg_h <= 0 || fg_w <= 0 || dst_h <= 0 || dst_w <= 0) return BEVWARP_ERR_BAD_ARG;
    if (channels < 1 || channels > 4) return BEVWARP_ERR_UNSUPPORTED;
    if (fg_gray && channels != 3) return BEVWARP_ERR_UNSUPPORTED;  // BGR2GRAY needs three channels
    // 8-bit images, one frame each: background, foreground and mask (the foreground's size) are sampled, dst is written
    const Image srcs[3] = {{(uintptr_t)bg, bg_h, (uint64_t)bg_w * channels, bg_row_stride, 0, 1}, {(uintptr_t)fg, fg_h, (uint64_t)fg_w * channels, fg_row_stride, 0, 1},
                           {(uintptr_t)mask, fg_h, (uint64_t)fg_w * channels, mask_row_stride, 0, 1}};
    const int cols[3] = {bg_w, fg_w, fg_w};
    const Image d = {(uintptr_t)dst, dst_h, (uint64_t)dst_w * channels, dst_row_stride, 0, 1};
    int st = plan::layout_status(d, 1);
    for (int i = 0; i < 3 && st == BEVWARP_OK; i++) st = plan::layout_status(srcs[i], 1);
    if (st == BEVWARP_OK && (dst_w > plan::kMaxDstSide || dst_h > plan::kMaxDstSide)) st = BEVWARP_ERR_TOO_LARGE;
    for (int i = 0; i < 3 && st == BEVWARP_OK; i++) st = plan::source_size_status(srcs[i], cols[i]);
    for (int i = 0; i < 3 && st == BEVWARP_OK; i++)  // the destination must not overlap a source (as for bevwarp_warp)
        if (plan::regions_overlap(srcs[i], d)) st = BEVWARP_ERR_OVERLAP;
    if (st != BEVWARP_OK) return st;
    const TilePlan p = plan::plan_composite(dst_h, dst_w, tile_width(BEVWARP_U8), rows_per_pass(), composite_max_rows(),
                                            resident_workgroups(BEVWARP_U8, channels, BEVWARP_LINEAR) / 4);
    WarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = (const uint8_t*)bg, a.dst = (uint8_t*)dst, a.minv = M_inv_bg;
    a.src_rs = bg_row_stride, a.dst_rs = dst_row_stride;
    a.batch = 1, a.src_h = bg_h, a.src_w = bg_w, a.dst_h = dst_h, a.dst_w = dst_w;
    a.m_stride = 0;
    a.xsrc[0] = (const uint8_t*)fg, a.xsrc[1] = (const uint8_t*)mask;
    a.xminv[0] = a.xminv[1] = M_inv_cam;
    a.xsrc_rs[0] = fg_row_stride, a.xsrc_rs[1] = mask_row_stride;
    a.xsrc_h[0] = a.xsrc_h[1] = fg_h, a.xsrc_w[0] = a.xsrc_w[1] = fg_w;
    a.fg_gray = fg_gray != 0;
    copy_plan(a, p);
    a.dst_vec_ok = plan::wide_stores_ok(d, plan::store_align(BEVWARP_U8, channels, false));
    return launched(launch_warp_composite(a, channels, (hipStream_t)stream));
}

int bevwarp_resize(const void* src, void* dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels, int64_t src_frame_stride,
                   int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, int dtype, int interp, void* stream) {
    if (!src || !dst || batch < 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return BEVWARP_ERR_BAD_ARG;
    if (dtype != BEVWARP_U8 || interp != BEVWARP_LINEAR || channels < 1 || channels > 4) return BEVWARP_ERR_UNSUPPORTED;
    const Image s = {(uintptr_t)src, src_h, (uint64_t)src_w * channels, src_row_stride, src_frame_stride, batch};
    const Image d = {(uintptr_t)dst, dst_h, (uint64_t)dst_w * channels, dst_row_stride, dst_frame_stride, batch};
    if (plan::layout_status(s, 1) != BEVWARP_OK || plan::layout_status(d, 1) != BEVWARP_OK) return BEVWARP_ERR_BAD_ARG;
    // (sides up to 2^24; the grid carries destination rows and frames in 16 bits)
    if (plan::size_status(s, src_w, 1 << 24, 1 << 24, false) != BEVWARP_OK || plan::size_status(d, dst_w, 65535, 1 << 24, false) != BEVWARP_OK || batch > 65535)
        return BEVWARP_ERR_TOO_LARGE;
    if (batch == 0) return BEVWARP_OK;
    if (plan::regions_overlap(s, d)) return BEVWARP_ERR_OVERLAP;
    return launched(launch_resize_linear_u8((const uint8_t*)src, (uint8_t*)dst, batch, src_h, src_w, dst_h, dst_w, channels, src_frame_stride,
                                            src_row_stride, dst_frame_stride, dst_row_stride, (hipStream_t)stream));
}

int bevwarp_footprint(unsigned char* touched, int batch, int src_h, int src_w, int dst_h, int dst_w, const double* M_inv, int m_count,
                      int interp, void* stream) {
    if (!touched || !M_inv || batch < 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return BEVWARP_ERR_BAD_ARG;
    if (interp != BEVWARP_NEAREST && interp != BEVWARP_LINEAR) return BEVWARP_ERR_UNSUPPORTED;
    if (m_count != 1 && m_count != batch) return BEVWARP_ERR_BAD_ARG;
    if (src_w > 32767 || src_h > 32767 || dst_h > 65535 || batch > 65535) return BEVWARP_ERR_TOO_LARGE;
    if (batch == 0) return BEVWARP_OK;
    return launched(launch_footprint(touched, batch, src_h, src_w, dst_h, dst_w, M_inv, m_count == 1 ? 0 : 9,
                                     block_width(dst_w, dst_h), interp, (hipStream_t)stream));
}

int bevwarp_project_points(const void* in, void* out, int64_t n, int dim, const double* H, int dtype, void* stream) {
    if (!H || n < 0 || (n > 0 && (!in || !out))) return BEVWARP_ERR_BAD_ARG;
    if (dim != 2 && dim != 3) return BEVWARP_ERR_BAD_ARG;
    if (dtype != BEVWARP_F32 && dtype != BEVWARP_F64) return BEVWARP_ERR_UNSUPPORTED;
    if (!finite9(H, 1)) return BEVWARP_ERR_NOT_FINITE;
    const int esz = dtype == BEVWARP_F32 ? 4 : 8;
    const int need = dim == 2 ? 2 * esz : esz;  // 2-D points move as one 8 / 16 byte unit
    if (((uintptr_t)in % need) || ((uintptr_t)out % need)) return BEVWARP_ERR_BAD_ARG;
    return launched(launch_project_points(in, out, n, dim, H, dtype, (hipStream_t)stream));
}

int bevwarp_project_points_lens(const void* in, void* out, void* residual, int64_t n, const double* H, const double* lens, double r2_max, int direction,
                                int iters, double tol_px, int dtype, void* stream) {
    const bool fisheye = plan::take_fisheye_flag(direction);
    const int st = plan::points_model_status(fisheye, in, out, residual, n, H, lens, r2_max, direction, iters, tol_px, dtype);
    if (st != BEVWARP_OK || n == 0) return st;
    PointsLensArgs a;
    memcpy(a.H, H, sizeof(a.H));
    memcpy(a.lens, lens, sizeof(a.lens));
    a.r2_max = r2_max, a.tol_px = tol_px, a.iters = iters;
    return launched((fisheye ? launch_points_fisheye : launch_points_lens)(in, out, residual, n, a, direction, dtype, (hipStream_t)stream));
}

// H / H[2][2] when H is a similarity of the plane in the sense of bev/rbox.py:173-219 (last row ~ (0, 0, 1), equal scale on
// both axes -- the reference asserts both); scale = sqrt(h00^2 + h10^2)
static int normalise_similarity(const double* H, double* Hn, double* scale) {
    if (!H || !finite9(H, 1) || H[8] == 0.0) return BEVWARP_ERR_NOT_FINITE;
    for (int i = 0; i < 9; i++) Hn[i] = H[i] / H[8];
    if (fabs(Hn[6]) + fabs(Hn[7]) >= 1e-5) return BEVWARP_ERR_BAD_ARG;
    const double s0 = sqrt(Hn[0] * Hn[0] + Hn[3] * Hn[3]), s1 = sqrt(Hn[1] * Hn[1] + Hn[4] * Hn[4]);
    if (!(fabs(s0 - s1) < 1e-5)) return BEVWARP_ERR_BAD_ARG;
    *scale = s0;
    return BEVWARP_OK;
}

int bevwarp_rbox_transform(const void* boxes, int n, int stride, const double* H, int src_is_bev, void* out, int dtype, void* stream) {
    if (n < 0 || stride < 5 || (n > 0 && (!boxes || !out))) return BEVWARP_ERR_BAD_ARG;
    if (dtype != BEVWARP_F32 && dtype != BEVWARP_F64) return BEVWARP_ERR_UNSUPPORTED;
    double Hn[9], scale;
    const int st = normalise_similarity(H, Hn, &scale);
    if (st != BEVWARP_OK) return st;
    return launched(launch_rbox_transform(boxes, n, stride, Hn, scale, src_is_bev != 0, out, dtype, (hipStream_t)stream));
}

int bevwarp_tracker_step(const void* dets_bev, int n, int det_stride, const void* trks_world, int m, int trk_stride, const double* H_world_bev,
                         const double* H_img_world, double iou_threshold, void* dets_world, void* iou, unsigned char* candidates, void* dets_img,
                         int dtype, void* stream) {
    if (n < 0 || m < 0 || det_stride < 5 || trk_stride < 5) return BEVWARP_ERR_BAD_ARG;
    if (n > 0 && (!dets_bev || !dets_world)) return BEVWARP_ERR_BAD_ARG;
    if (n > 0 && m > 0 && (!trks_world || !iou || !candidates)) return BEVWARP_ERR_BAD_ARG;
    if (H_img_world && n > 0 && !dets_img) return BEVWARP_ERR_BAD_ARG;
    if (dtype != BEVWARP_F32 && dtype != BEVWARP_F64) return BEVWARP_ERR_UNSUPPORTED;
    if (n > 64000) return BEVWARP_ERR_TOO_LARGE;  // (grid rows: n scoring + n / 64 output workgroups <= 65535)
    if (!(iou_threshold == iou_threshold)) return BEVWARP_ERR_NOT_FINITE;
    double Hn[9], scale;
    const int st = normalise_similarity(H_world_bev, Hn, &scale);
    if (st != BEVWARP_OK) return st;
    if (H_img_world && !finite9(H_img_world, 1)) return BEVWARP_ERR_NOT_FINITE;
    return launched(launch_tracker_step(dets_bev, n, det_stride, trks_world, m, trk_stride, Hn, scale, H_img_world, iou_threshold, dets_world, iou,
                                        candidates, dets_img, dtype, (hipStream_t)stream));
}

int bevwarp_rbox_iou(const void* a, int na, int a_stride, const void* b, int nb, int b_stride, void* out, int dtype, void* stream) {
    if (na < 0 || nb < 0 || a_stride < 5 || b_stride < 5) return BEVWARP_ERR_BAD_ARG;
    if (na > 0 && nb > 0 && (!a || !b || !out)) return BEVWARP_ERR_BAD_ARG;
    if (dtype != BEVWARP_F32 && dtype != BEVWARP_F64) return BEVWARP_ERR_UNSUPPORTED;
    if (na > 65535) return BEVWARP_ERR_TOO_LARGE;
    return launched(launch_rbox_iou(a, na, a_stride, b, nb, b_stride, out, dtype, (hipStream_t)stream));
}

}  // extern "C"
