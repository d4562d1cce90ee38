// host_plan.h -- what the C ABI decides before a launch, as plain C++17 (no HIP): the argument checks and the launch geometry.
// bevwarp_api.hip is its only user in the library; tests/host_plan_driver.cpp compiles it with g++ under the address and
// undefined-behaviour sanitizers, and tests/golden/launch_plans.json pins every field of the plans.  Not installed.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bevwarp.h"

namespace bevwarp {
namespace plan {

inline bool finite9(const double* m, int n) {
    for (int i = 0; i < 9 * n; i++)
        if (!isfinite(m[i])) return false;
    return true;
}

// Evaluation block width of the reference algorithm (OpenCV WarpPerspectiveInvoker, BLOCK_SZ = 32):
// bh0 = min(16, h); bw0 = min(1024 / bh0, w).  Values depend on bw0 only.
inline int block_width(int dst_w, int dst_h) {
    const int bh0 = dst_h < 16 ? dst_h : 16;
    const int bw0 = 1024 / bh0;
    return bw0 < dst_w ? bw0 : dst_w;
}

// division by invariants as a multiply-high; exact while n_max * d < 2^32, else the kernel divides
inline uint32_t div_magic(uint64_t n_max, uint32_t d) { return (n_max * d < (1ull << 32) && d > 1) ? (uint32_t)((1ull << 32) / d) + 1u : 0u; }

// ---- images --------------------------------------------------------------------------------------------------------------
// One strided batch of images as a kernel walks it; all in bytes.  A single image: batch = 1, fs = 0.
struct Image {
    uintptr_t base;
    int rows;
    uint64_t row_bytes;
    int64_t rs, fs;  // row / frame stride
    int batch;
    uintptr_t end() const { return base + (uint64_t)(batch - 1) * fs + (uint64_t)(rows - 1) * rs + row_bytes; }  // (of the bounding byte range)
};

// Do the strides hold the rows and the frames, and is everything a multiple of the element size (1: no alignment asked)?
// (in 128 bits: a stride near 2^63 is a bad argument like any other, not an overflow)
inline int layout_status(const Image& im, int elem) {
    if (im.rs < 0 || (uint64_t)im.rs < im.row_bytes) return BEVWARP_ERR_BAD_ARG;
    if (im.batch > 1 && (__int128)im.fs < (__int128)im.rows * im.rs) return BEVWARP_ERR_BAD_ARG;
    if ((im.rs % elem) || (im.fs % elem) || (im.base % elem)) return BEVWARP_ERR_BAD_ARG;
    return BEVWARP_OK;
}

// Size limits of one image; every entry point passes its own.  mul24: a kernel that addresses the image with 24-bit multiplies
// -- a row stride below 16 MiB and a frame below 2 GiB.
inline int size_status(const Image& im, int cols, int max_rows, int max_cols, bool mul24) {
    if (cols > max_cols || im.rows > max_rows) return BEVWARP_ERR_TOO_LARGE;
    if (mul24 && (im.rs >= (1 << 24) || (int64_t)im.rows * im.rs >= ((int64_t)1 << 31))) return BEVWARP_ERR_TOO_LARGE;
    return BEVWARP_OK;
}

// Does some byte of a strided source coincide with some byte of a strided destination?  The kernel reads taps of a frame while
// other workgroups store: an in-place call would corrupt silently, so overlap is refused.  Bounding byte ranges first; when those
// intersect but both sides walk their rows with ONE common stride S (equal row strides; frame strides multiples of S, or one
// frame), every row of either side starts at a fixed residue mod S, and two regions of one allocation that lie side by side (the
// left-half ROI of an image warped into its right half, say) are disjoint exactly when their residue intervals are.
// (both sides have the same number of frames)
inline bool regions_overlap(const Image& s, const Image& d) {
    if (!(s.base < d.end() && d.base < s.end())) return false;
    if (s.rs == d.rs && s.rs > 0 && (s.batch == 1 || (s.fs % s.rs == 0 && d.fs % s.rs == 0)) && s.row_bytes + d.row_bytes <= (uint64_t)s.rs) {
        const uint64_t S = (uint64_t)s.rs, a = s.base % S, b = d.base % S;
        if ((b + S - a) % S >= s.row_bytes && (a + S - b) % S >= d.row_bytes) return false;  // column-disjoint: no row of one meets a row of the other
    }
    return true;
}

// Wide stores: one lane writes its 4 consecutive 8-bit pixels (4 C bytes; 12-byte stores need 4-byte alignment) or 16 bytes of
// float data (float planes of 8-bit sources included), or 4 elements of a plane (8 bytes of the 16-bit planes).  The frame stride
// counts even for a single frame.
inline int store_align(int dtype, int channels, bool planar, int plane_elem = 4) {
    if (planar) return 4 * plane_elem;
    return dtype == BEVWARP_U8 ? (channels == 4 ? 16 : (channels == 2 ? 8 : 4)) : 16;
}
inline bool wide_stores_ok(const Image& d, int align) { return d.base % align == 0 && d.rs % align == 0 && d.fs % align == 0; }
// (a planar call's wide stores: call_wide_stores_ok below -- the plane stride counts as well)
// The border kernel's whole-pixel loads: 8-bit pixels of 2 / 4 channels that are all 2- / 4-byte aligned (one load per tap).
inline int pixel_load_align(int dtype, int channels) { return (dtype == BEVWARP_U8 && (channels == 2 || channels == 4)) ? channels : (dtype == BEVWARP_U8 ? 1 : 4); }
inline bool pixel_loads_ok(const Image& s, int align) { return s.base % align == 0 && s.rs % align == 0 && (s.batch == 1 || s.fs % align == 0); }

// ---- a warp call (bevwarp_warp, _classes, _planar, _border) -----------------------------------------------------------------
struct Frames {  // an image batch as the ABI passes it
    const void* base;
    int h, w;
    int64_t fs, rs;
};
struct WarpCall {  // (an aggregate: every entry point fills it once, the optional parts default to none)
    Frames src, dst;
    int batch, channels, dtype, interp;
    const double* minv;
    int m_count;
    const double* border_value;
    void* stream;
    bool planar;  // bevwarp_warp_planar, _planes: channel planes, plane_stride bytes apart, instead of interleaved pixels of the source type
    int64_t plane_stride;
    const double *scale, *bias;
    void* classes;  // bevwarp_warp_classes
    int classes_mode;
    bool cubic_ok;  // bevwarp_warp, bevwarp_warp_border: the entry points behind which a bicubic kernel stands
    int plane_elem = 4;  // bytes of a plane's element: 4 (float32), 2 (bevwarp_warp_planes: float16, bfloat16)

    int elem() const { return dtype == BEVWARP_U8 ? 1 : 4; }
    Image src_image() const { return {(uintptr_t)src.base, src.h, (uint64_t)src.w * channels * elem(), src.rs, src.fs, batch}; }
    // (planar: one plane's rows; the planes of a frame are plane_stride apart)
    Image dst_image() const { return {(uintptr_t)dst.base, dst.h, (uint64_t)dst.w * (planar ? plane_elem : channels * elem()), dst.rs, dst.fs, batch}; }
};

// Does the call's destination admit the wide stores?  (planes: 4 elements per store, and the plane stride is a stride like the others)
inline bool call_wide_stores_ok(const WarpCall& c) {
    const int align = store_align(c.dtype, c.channels, c.planar, c.plane_elem);
    return wide_stores_ok(c.dst_image(), align) && (!c.planar || c.plane_stride % align == 0);
}

// The checks that need no pointer, in the order their statuses are documented: sizes, format, matrix count.
inline int format_status(const WarpCall& c) {
    if (c.batch < 0 || c.src.h <= 0 || c.src.w <= 0 || c.dst.h <= 0 || c.dst.w <= 0) return BEVWARP_ERR_BAD_ARG;
    const bool interp_ok = c.interp == BEVWARP_NEAREST || c.interp == BEVWARP_LINEAR || (c.interp == BEVWARP_CUBIC && c.cubic_ok);
    if ((c.dtype != BEVWARP_U8 && c.dtype != BEVWARP_F32) || !interp_ok || c.channels < 1 || c.channels > 4) return BEVWARP_ERR_UNSUPPORTED;
    if (c.m_count != 1 && c.m_count != c.batch) return BEVWARP_ERR_BAD_ARG;
    return BEVWARP_OK;
}

// The source limits of the warp kernels: sides of at most 32767 px (saturated 16-bit tap indices) and 24-bit multiplies.
inline int source_size_status(const Image& src, int cols) { return size_status(src, cols, 32767, 32767, true); }

// All argument checks of a warp: BEVWARP_OK or the status to return.  Null pointers, then format, layout, size, overlap.
inline int check_warp(const WarpCall& c) {
    if (!c.src.base || !c.dst.base || !c.minv) return BEVWARP_ERR_BAD_ARG;
    int st = format_status(c);
    if (st != BEVWARP_OK) return st;
    const Image s = c.src_image(), d = c.dst_image();
    if ((st = layout_status(s, c.elem())) != BEVWARP_OK) return st;
    if (c.planar) {  // destination: `channels` planes per frame -- the rule twice: rows in a plane (asked of a lone plane too), planes in a frame
        const Image rows_in_plane = {d.base, d.rows, d.row_bytes, d.rs, c.plane_stride, 2}, planes_in_frame = {d.base, c.channels, 0, c.plane_stride, d.fs, d.batch};
        if (layout_status(rows_in_plane, c.plane_elem) != BEVWARP_OK || layout_status(planes_in_frame, c.plane_elem) != BEVWARP_OK) return BEVWARP_ERR_BAD_ARG;
    } else if ((st = layout_status(d, c.elem())) != BEVWARP_OK) {
        return st;
    }
    if ((st = source_size_status(s, c.src.w)) != BEVWARP_OK || c.batch == 0) return st;
    if (c.planar) {  // (planes: bounding ranges only -- a frame's planes need not share the rows' stride)
        const uintptr_t d1 = d.end() + (uint64_t)(c.channels - 1) * c.plane_stride;
        return (s.base < d1 && d.base < s.end()) ? BEVWARP_ERR_OVERLAP : BEVWARP_OK;
    }
    return regions_overlap(s, d) ? BEVWARP_ERR_OVERLAP : BEVWARP_OK;
}

// ---- an NV12 warp call (bevwarp_warp_nv12) -------------------------------------------------------------------------------------
// The source is two images: src_h rows of src_w Y bytes, and src_h / 2 rows of src_w / 2 (U, V) pairs (src_w bytes, 2-byte elements).
// The destination is 8-bit, 3 channels.
struct Nv12Call {
    const void *y, *uv, *dst;
    int batch, src_h, src_w, dst_h, dst_w;
    int64_t y_fs, y_rs, uv_fs, uv_rs, dst_fs, dst_rs;
    const double* minv;
    int m_count, interp, rgb_order;

    Image y_image() const { return {(uintptr_t)y, src_h, (uint64_t)src_w, y_rs, y_fs, batch}; }
    Image uv_image() const { return {(uintptr_t)uv, src_h / 2, (uint64_t)src_w, uv_rs, uv_fs, batch}; }
    Image dst_image() const { return {(uintptr_t)dst, dst_h, (uint64_t)dst_w * 3, dst_rs, dst_fs, batch}; }
};

// ---- an NV12 warp into channel planes (bevwarp_warp_nv12_planes) ---------------------------------------------------------------------
// The source is an Nv12Call's; the destination is three planes per frame of dst_h rows of dst_w elements of `plane_dtype`.
struct Nv12PlanesCall {
    Nv12Call s;           // (dst, dst_fs, dst_rs: plane 0 of frame 0, the frame stride and a plane's row stride)
    int64_t dst_ps;       // bytes between the planes of a frame
    int plane_dtype;      // BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16

    // bytes of a plane's element; a plane type the entry point does not take asks no alignment (the layout is looked at first)
    int elem() const { return plane_dtype == BEVWARP_F32 ? 4 : ((plane_dtype == BEVWARP_F16 || plane_dtype == BEVWARP_BF16) ? 2 : 1); }
    Image plane_image() const { return {(uintptr_t)s.dst, s.dst_h, (uint64_t)s.dst_w * elem(), s.dst_rs, s.dst_fs, s.batch}; }  // one plane's rows
    uintptr_t dst_end() const { return plane_image().end() + 2 * (uint64_t)dst_ps; }  // (of the bounding byte range of all planes)
};

// All argument checks of the two NV12 warps (`planes`: the call into planes, or null), in the order the header documents: bad arguments
// (null pointers, sizes, odd source sides, layouts -- the interleaved destination's, or check_warp's rule for planes: rows in a plane,
// asked of a lone plane too, and planes in a frame -- then the matrix count), unsupported interpolation, channel order or plane type,
// source size limits per plane, overlap of the destination with either source plane (the planes may overlap each other: both are only
// read; a destination of planes is taken as its bounding byte range).
inline int check_nv12(const Nv12Call& c, const Nv12PlanesCall* planes) {
    if (!c.y || !c.uv || !c.dst || !c.minv) return BEVWARP_ERR_BAD_ARG;
    if (c.batch < 0 || c.src_h <= 0 || c.src_w <= 0 || c.dst_h <= 0 || c.dst_w <= 0 || (c.src_h & 1) || (c.src_w & 1)) return BEVWARP_ERR_BAD_ARG;
    const Image y = c.y_image(), uv = c.uv_image(), d = planes ? planes->plane_image() : c.dst_image();
    if (layout_status(y, 1) != BEVWARP_OK || layout_status(uv, 2) != BEVWARP_OK) return BEVWARP_ERR_BAD_ARG;
    if (planes) {
        const Image rows_in_plane = {d.base, d.rows, d.row_bytes, d.rs, planes->dst_ps, 2}, planes_in_frame = {d.base, 3, 0, planes->dst_ps, d.fs, d.batch};
        if (layout_status(rows_in_plane, planes->elem()) != BEVWARP_OK || layout_status(planes_in_frame, planes->elem()) != BEVWARP_OK) return BEVWARP_ERR_BAD_ARG;
    } else if (layout_status(d, 1) != BEVWARP_OK) {
        return BEVWARP_ERR_BAD_ARG;
    }
    if (c.m_count != 1 && c.m_count != c.batch) return BEVWARP_ERR_BAD_ARG;
    if ((c.interp != BEVWARP_NEAREST && c.interp != BEVWARP_LINEAR) || (c.rgb_order != 0 && c.rgb_order != 1)) return BEVWARP_ERR_UNSUPPORTED;
    if (planes && planes->plane_dtype != BEVWARP_F32 && planes->plane_dtype != BEVWARP_F16 && planes->plane_dtype != BEVWARP_BF16) return BEVWARP_ERR_UNSUPPORTED;
    int st;
    if ((st = source_size_status(y, c.src_w)) != BEVWARP_OK || (st = source_size_status(uv, c.src_w / 2)) != BEVWARP_OK || c.batch == 0) return st;
    if (planes) {
        const uintptr_t d1 = planes->dst_end();
        return ((y.base < d1 && d.base < y.end()) || (uv.base < d1 && d.base < uv.end())) ? BEVWARP_ERR_OVERLAP : BEVWARP_OK;
    }
    return (regions_overlap(y, d) || regions_overlap(uv, d)) ? BEVWARP_ERR_OVERLAP : BEVWARP_OK;
}
inline int check_warp_nv12(const Nv12Call& c) { return check_nv12(c, nullptr); }
inline int check_warp_nv12_planes(const Nv12PlanesCall& c) { return check_nv12(c.s, &c); }
// Does the call's destination admit the wide stores?  call_wide_stores_ok's rule: 4 plane elements per store, the plane stride counts.
inline bool nv12_planes_wide_stores_ok(const Nv12PlanesCall& c) {
    const int align = store_align(BEVWARP_U8, 3, true, c.elem());
    return wide_stores_ok(c.plane_image(), align) && c.dst_ps % align == 0;
}

// ---- a warp into NV12 (bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12) -------------------------------------------------------------
// The destination is two images, laid out like an Nv12Call's source: dst_h rows of dst_w Y bytes, and dst_h / 2 rows of dst_w / 2 (U, V)
// pairs (dst_w bytes, 2-byte elements).  The source is 8-bit, 3 channels (`src`) or, with `nv12_src`, the two planes of an Nv12Call.
struct Nv12OutCall {
    bool nv12_src;
    const void *src, *y, *uv;     // src (BGR / RGB frames) or y and uv; the other side is unused
    const void *dst_y, *dst_uv;
    int batch, src_h, src_w, dst_h, dst_w;
    int64_t src_fs, src_rs;       // of src
    int64_t y_fs, y_rs, uv_fs, uv_rs;  // of y and uv
    int64_t dy_fs, dy_rs, duv_fs, duv_rs;
    const double* minv;
    int m_count, interp, rgb_order;   // (rgb_order: of src; an NV12 source is sampled as B, G, R and passes 0)

    Image src_image() const { return {(uintptr_t)src, src_h, (uint64_t)src_w * 3, src_rs, src_fs, batch}; }
    Image y_image() const { return {(uintptr_t)y, src_h, (uint64_t)src_w, y_rs, y_fs, batch}; }
    Image uv_image() const { return {(uintptr_t)uv, src_h / 2, (uint64_t)src_w, uv_rs, uv_fs, batch}; }
    Image dst_y_image() const { return {(uintptr_t)dst_y, dst_h, (uint64_t)dst_w, dy_rs, dy_fs, batch}; }
    Image dst_uv_image() const { return {(uintptr_t)dst_uv, dst_h / 2, (uint64_t)dst_w, duv_rs, duv_fs, batch}; }
};

// Do the two planes a launch WRITES share bytes?  regions_overlap's rule, with one more refinement: in a batch of single-buffer frames
// (Y rows, then the rows of pairs, frame after frame) the Y images' bounding range spans every frame's pairs.  Where both planes walk
// the frames with one stride and a frame's two planes lie within one such stride of each other, planes of different frames cannot meet
// and frame 0 decides.
inline bool written_planes_overlap(const Image& a, const Image& b) {
    if (a.batch > 1 && a.fs == b.fs) {
        Image a0 = a, b0 = b;
        a0.batch = b0.batch = 1;
        const uintptr_t lo = a0.base < b0.base ? a0.base : b0.base, a1 = a0.end(), b1 = b0.end(), hi = a1 > b1 ? a1 : b1;
        if ((uint64_t)(hi - lo) <= (uint64_t)a.fs) return regions_overlap(a0, b0);
    }
    return regions_overlap(a, b);
}

// All argument checks of the two warps into NV12, in the order the header documents: bad arguments (null pointers, sizes, odd destination
// sides, odd sides of an NV12 source, the layout of every image -- the pairs' planes with 2-byte elements --, the matrix count), unsupported
// interpolation or channel order, the source's size limits, overlap of either destination plane with any source image and of the two
// destination planes with each other (source planes may overlap each other: both are only read).
inline int check_nv12_out(const Nv12OutCall& c) {
    if (c.nv12_src ? (!c.y || !c.uv) : !c.src) return BEVWARP_ERR_BAD_ARG;
    if (!c.dst_y || !c.dst_uv || !c.minv) return BEVWARP_ERR_BAD_ARG;
    if (c.batch < 0 || c.src_h <= 0 || c.src_w <= 0 || c.dst_h <= 0 || c.dst_w <= 0 || (c.dst_h & 1) || (c.dst_w & 1)) return BEVWARP_ERR_BAD_ARG;
    if (c.nv12_src && ((c.src_h & 1) || (c.src_w & 1))) return BEVWARP_ERR_BAD_ARG;
    const Image s = c.src_image(), y = c.y_image(), uv = c.uv_image(), dy = c.dst_y_image(), duv = c.dst_uv_image();
    if (c.nv12_src ? (layout_status(y, 1) != BEVWARP_OK || layout_status(uv, 2) != BEVWARP_OK) : layout_status(s, 1) != BEVWARP_OK) return BEVWARP_ERR_BAD_ARG;
    if (layout_status(dy, 1) != BEVWARP_OK || layout_status(duv, 2) != BEVWARP_OK) return BEVWARP_ERR_BAD_ARG;
    if (c.m_count != 1 && c.m_count != c.batch) return BEVWARP_ERR_BAD_ARG;
    if ((c.interp != BEVWARP_NEAREST && c.interp != BEVWARP_LINEAR) || (c.rgb_order != 0 && c.rgb_order != 1)) return BEVWARP_ERR_UNSUPPORTED;
    int st;
    if (c.nv12_src) {
        if ((st = source_size_status(y, c.src_w)) != BEVWARP_OK || (st = source_size_status(uv, c.src_w / 2)) != BEVWARP_OK) return st;
    } else if ((st = source_size_status(s, c.src_w)) != BEVWARP_OK) {
        return st;
    }
    if (c.batch == 0) return BEVWARP_OK;
    const bool meets_source = c.nv12_src ? (regions_overlap(y, dy) || regions_overlap(uv, dy) || regions_overlap(y, duv) || regions_overlap(uv, duv))
                                         : (regions_overlap(s, dy) || regions_overlap(s, duv));
    return (meets_source || written_planes_overlap(dy, duv)) ? BEVWARP_ERR_OVERLAP : BEVWARP_OK;
}
inline int check_warp_to_nv12(const Nv12OutCall& c) { return c.nv12_src ? BEVWARP_ERR_BAD_ARG : check_nv12_out(c); }
inline int check_warp_nv12_to_nv12(const Nv12OutCall& c) { return c.nv12_src ? check_nv12_out(c) : BEVWARP_ERR_BAD_ARG; }
// Wide stores, per plane: a lane's 4 Y bytes, and its two pairs, go out as one dword each where the plane's base and both strides are
// multiples of 4 (the frame stride counts even for a single frame).
inline bool nv12_out_wide_stores_ok(const Image& plane) { return wide_stores_ok(plane, 4); }

// ---- launch geometry ---------------------------------------------------------------------------------------------------------
struct TilePlan {
    int status;                  // BEVWARP_OK or BEVWARP_ERR_TOO_LARGE (the other fields are then meaningless)
    int tile_h;                  // rows per workgroup
    int tiles_x, tiles_per_frame;
    int64_t total_tiles;         // frames * tiles_per_frame
    int chunk, stagger, tail_split;  // (row kernel; WarpArgs explains them)
    int bw0;
    uint32_t tpf_magic, tx_magic, bw0_magic;  // div_magic of tiles_per_frame, tiles_x, bw0
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int kMaxDstSide = 1 << 20;  // (keeps every sum and product below in range)

// the grid of tw x p.tile_h tiles over `frames` destination frames, and the magics that depend on it alone
inline void tile_grid(TilePlan& p, int64_t frames, int dst_h, int dst_w, int tw) {
    p.bw0 = block_width(dst_w, dst_h);
    p.tiles_x = ceil_div(dst_w, tw);
    p.tiles_per_frame = p.tiles_x * ceil_div(dst_h, p.tile_h);
    p.total_tiles = frames * p.tiles_per_frame;
    p.tx_magic = div_magic((uint64_t)p.tiles_per_frame, (uint32_t)p.tiles_x);
    p.bw0_magic = div_magic((uint64_t)dst_w + tw, (uint32_t)p.bw0);
}

// The row kernel (warp_rows.h): tw = tile_width(dtype), rpp = rows_per_pass(), resident = resident_workgroups().
inline TilePlan plan_rows(int batch, int dst_h, int dst_w, int dtype, int tw, int rpp, int64_t resident) {
    TilePlan p = {};
    p.status = BEVWARP_ERR_TOO_LARGE;
    if (dst_w > kMaxDstSide || dst_h > kMaxDstSide) return p;
    // tile = tile_width x tile_h destination pixels per workgroup.  16 rows (four per wave) is what launches that fill the
    // chip and the HBM-bound float formats take; the ALU-bound 8-bit formats amortise the per-tile set-up over 24 rows once the launch
    // fills the chip more than twice (taller tiles gain on footprints that lie inside the frame and lose on those the
    // frame's edge cuts up, whose tiles differ widely in cost: A/B in DESIGN.md section 6).
    // Launches that do not fill the chip -- a camera's single frame, the reference's own call shape -- take lower tiles, down
    // to one pass per wave, until there is a workgroup for every resident slot: the frame's latency is then one tile's, spread
    // over all CUs (720p -> 512^2: 18.7 -> 12.3 us, 1080p -> 1024^2: 15.2 -> 11.5 us; from four frames up 16 rows win).
    const int64_t per_row_of_tiles = (int64_t)batch * ceil_div(dst_w, tw);
    p.tile_h = rpp * 4;
    while (p.tile_h > rpp && per_row_of_tiles * ceil_div(dst_h, p.tile_h) < resident) p.tile_h /= 2;
    const int tall = rpp * 6;  // (24 rows)
    if (dtype == BEVWARP_U8 && per_row_of_tiles * ceil_div(dst_h, tall) >= 2 * resident) p.tile_h = tall;
    tile_grid(p, batch, dst_h, dst_w, tw);
    const int64_t chunk = (p.total_tiles + 7) / 8;  // items per XCD
    if (chunk * 8 > 0x7fffffffLL) return p;
    p.chunk = (int)chunk;
    // Frames of one launch usually share a footprint: left alone, all eight XCDs would be in the same part of a frame --
    // outside tiles (store-bound) or interior tiles (latency-bound) -- at the same time.  XCD k starts k/8 of a frame in.
    p.stagger = chunk >= p.tiles_per_frame ? p.tiles_per_frame / 8 : 0;
    // one resident round of half-height workgroups at the end of launches of at least two rounds (tile_h / 2 stays a multiple
    // of 4); measured neutral to -2.5 % on footprints whose tiles cost alike, -8..-14 % on a perspective BEV from 12 frames up
    const int64_t round_per_xcd = resident / 8;
    p.tail_split = (p.tile_h % (2 * rpp) == 0 && chunk >= 2 * round_per_xcd) ? (int)round_per_xcd : 0;
    p.tpf_magic = div_magic((uint64_t)chunk * 8, (uint32_t)p.tiles_per_frame);
    p.status = BEVWARP_OK;
    return p;
}

// The composite (warp_rows<..., NSRC = 3>), one frame of sides <= 2^20: one 12-wave workgroup per tile, one workgroup per CU --
// the tallest tile (<= max_rows, the LDS copies' 16 rows) that still gives every CU a workgroup.
inline TilePlan plan_composite(int dst_h, int dst_w, int tw, int rpp, int max_rows, int64_t cus) {
    TilePlan p = {};
    p.tile_h = max_rows;
    while (p.tile_h > rpp && (int64_t)ceil_div(dst_w, tw) * ceil_div(dst_h, p.tile_h) < cus) p.tile_h /= 2;
    tile_grid(p, 1, dst_h, dst_w, tw);
    p.chunk = (int)((p.total_tiles + 7) / 8);
    p.tpf_magic = div_magic((uint64_t)p.chunk * 8, (uint32_t)p.tiles_per_frame);
    return p;
}

// The border kernel (warp_border.hip): tiles of tw x th (kBorderTileW x kBorderTileH) on a flat grid of total_tiles items.
inline TilePlan plan_border(int batch, int dst_h, int dst_w, int tw, int th) {
    TilePlan p = {};
    p.status = BEVWARP_ERR_TOO_LARGE;
    if (dst_w > kMaxDstSide || dst_h > kMaxDstSide) return p;
    p.tile_h = th;
    tile_grid(p, batch, dst_h, dst_w, tw);
    if (p.total_tiles > 0x7fffffffLL) return p;
    p.tpf_magic = div_magic((uint64_t)p.total_tiles, (uint32_t)p.tiles_per_frame);
    p.status = BEVWARP_OK;
    return p;
}

// The index remap of the border modes that take a remainder, for an axis of n source pixels: the period (unused by REPLICATE and
// TRANSPARENT), an offset that is a multiple of it and makes every saturated index (>= -32768) non-negative, and the period's magic.
struct BorderPeriod {
    uint32_t per, off, mag;
};
inline BorderPeriod border_period(int mode, int n) {
    BorderPeriod b;
    b.per = mode == BEVWARP_BORDER_WRAP ? (uint32_t)n : mode == BEVWARP_BORDER_REFLECT ? 2u * n : (n > 1 ? 2u * n - 2u : 1u);
    b.off = (32768u + b.per - 1u) / b.per * b.per;
    b.mag = div_magic((uint64_t)b.off + 32769u, b.per);
    return b;
}

}  // namespace plan
}  // namespace bevwarp
