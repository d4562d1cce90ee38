// host_plan.h -- what the C ABI decides before a launch, as plain C++17 (no HIP): the argument checks and the launch geometry.
// bevwarp_api.hip is its only user in the library; tests/host_plan_driver.cpp (one program, a family of case lines per entry-point group,
// with tests/plan_driver_io.h) compiles it with g++ under the address and undefined-behaviour sanitizers, and
// tests/golden/launch_plans.json pins every field of the plans.  Not installed.
#pragma once
#include <math.h>
#include <stdint.h>

#include <initializer_list>

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
// (a written image of planes: the overload below -- the plane stride counts as well)
// The border kernel's whole-pixel loads: 8-bit pixels of 2 / 4 channels that are all 2- / 4-byte aligned (one load per tap).
inline int pixel_load_align(int dtype, int channels) { return (dtype == BEVWARP_U8 && (channels == 2 || channels == 4)) ? channels : (dtype == BEVWARP_U8 ? 1 : 4); }
inline bool pixel_loads_ok(const Image& s, int align) { return s.base % align == 0 && s.rs % align == 0 && (s.batch == 1 || s.fs % align == 0); }

// ---- a call: the images it reads and the images it writes ------------------------------------------------------------------------
struct Frames {  // an image batch as the ABI passes it
    const void* base;
    int64_t fs, rs;
    Image image(int rows, uint64_t row_bytes, int batch) const { return {(uintptr_t)base, rows, row_bytes, rs, fs, batch}; }
};
struct ReadImage {
    Image im;
    int cols, elem;  // pixels of a row, for the size limits; bytes of an element: 1, 2 (a (U, V) pair) or 4 (float32)
    bool map;        // a map plane of bevwarp_remap and its NV12 kin: as large as the destination (no source limits); its batch is the map count
};
struct WrittenImage {
    Image im;  // (planar: one plane's rows)
    int elem;
    bool planar;           // channel planes instead of interleaved pixels: `planes` per frame (interleaved: 1) ...
    int planes;
    int64_t plane_stride;  // ... this many bytes apart
    uintptr_t end() const { return im.end() + (uint64_t)(planes - 1) * plane_stride; }  // (of the bounding byte range of all planes)
};
// The two images of a batch of NV12 frames: h rows of w Y bytes, and h / 2 rows of w / 2 (U, V) pairs (w bytes, 2-byte elements).
struct Nv12Images {
    Image y, uv;
};
inline Nv12Images nv12_images(Frames y, Frames uv, int h, int w, int batch) { return {y.image(h, (uint64_t)w, batch), uv.image(h / 2, (uint64_t)w, batch)}; }

// What the checks need of one entry point's arguments.  The functions of the last part of this section describe the entry points in
// these terms; bevwarp_api.hip and the tests' driver (tests/host_plan_driver.cpp) build their calls with them.
struct Sizes {  // (what every entry point passes besides its images and its format)
    int batch, src_h, src_w, dst_h, dst_w, m_count;
    const double* minv;
};
struct Call : Sizes {
    bool format_ok;     // the entry point takes this dtype, channel count, interpolation, channel order and plane type ...
    bool format_first;  // ... which is asked before the layouts (bevwarp_warp and its kin) or after the matrix count (the NV12 entry points)
    bool even_src, even_dst;  // NV12 frames have even sides
    int n_reads, n_writes;
    ReadImage reads[4];
    WrittenImage writes[2];
    int supersample;  // k of a supersampled call (supersample_call), whose fine grid has sides of their own to judge; 0: none

    void read(const Image& im, int cols, int elem) { reads[n_reads++] = {im, cols, elem, false}; }
    void read_map(const Image& im, int elem) { reads[n_reads++] = {im, 0, elem, true}; }
    void write(const Image& im, int elem) { writes[n_writes++] = {im, elem, false, 1, 0}; }
    void write_planes(const Image& im, int elem, int planes, int64_t plane_stride) { writes[n_writes++] = {im, elem, true, planes, plane_stride}; }
    void read_nv12(Frames y, Frames uv) {
        const Nv12Images f = nv12_images(y, uv, src_h, src_w, batch);
        even_src = true, read(f.y, src_w, 1), read(f.uv, src_w / 2, 2);
    }
    void write_nv12(Frames y, Frames uv) {
        const Nv12Images f = nv12_images(y, uv, dst_h, dst_w, batch);
        even_dst = true, write(f.y, 1), write(f.uv, 2);
    }
};

// Wide stores of a written image: with planes, the plane stride is a stride like the others.
inline bool wide_stores_ok(const WrittenImage& w, int align) { return wide_stores_ok(w.im, align) && (!w.planar || w.plane_stride % align == 0); }

// The source limits of the warp kernels: sides of at most 32767 px (saturated 16-bit tap indices) and 24-bit multiplies.
inline int source_size_status(const Image& src, int cols) { return size_status(src, cols, 32767, 32767, true); }

// The layout of a written image.  Planes: the rule twice -- rows in a plane (asked of a lone plane too), planes in a frame.
inline int layout_status(const WrittenImage& w) {
    if (!w.planar) return layout_status(w.im, w.elem);
    const Image &d = w.im, rows_in_plane = {d.base, d.rows, d.row_bytes, d.rs, w.plane_stride, 2}, planes_in_frame = {d.base, w.planes, 0, w.plane_stride, d.fs, d.batch};
    return (layout_status(rows_in_plane, w.elem) != BEVWARP_OK || layout_status(planes_in_frame, w.elem) != BEVWARP_OK) ? BEVWARP_ERR_BAD_ARG : BEVWARP_OK;
}

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

// ---- the checks: one routine per phase, each over all images of the call ---------------------------------------------------------------
inline int null_status(const Call& c) {
    bool null = !c.minv;
    for (int i = 0; i < c.n_reads; i++) null |= !c.reads[i].im.base;
    for (int i = 0; i < c.n_writes; i++) null |= !c.writes[i].im.base;
    return null ? BEVWARP_ERR_BAD_ARG : BEVWARP_OK;
}
inline int sides_status(const Call& c) {
    if (c.batch < 0 || c.src_h <= 0 || c.src_w <= 0 || c.dst_h <= 0 || c.dst_w <= 0) return BEVWARP_ERR_BAD_ARG;
    return ((c.even_src && ((c.src_h | c.src_w) & 1)) || (c.even_dst && ((c.dst_h | c.dst_w) & 1))) ? BEVWARP_ERR_BAD_ARG : BEVWARP_OK;
}
inline int layouts_status(const Call& c) {
    int st = BEVWARP_OK;
    for (int i = 0; i < c.n_reads && st == BEVWARP_OK; i++) st = layout_status(c.reads[i].im, c.reads[i].elem);
    for (int i = 0; i < c.n_writes && st == BEVWARP_OK; i++) st = layout_status(c.writes[i]);
    return st;
}
inline int matrix_count_status(const Call& c) { return (c.m_count != 1 && c.m_count != c.batch) ? BEVWARP_ERR_BAD_ARG : BEVWARP_OK; }
inline int format_status(const Call& c) { return c.format_ok ? BEVWARP_OK : BEVWARP_ERR_UNSUPPORTED; }
inline int source_sizes_status(const Call& c) {
    int st = BEVWARP_OK;
    for (int i = 0; i < c.n_reads && st == BEVWARP_OK; i++)
        if (!c.reads[i].map) st = source_size_status(c.reads[i].im, c.reads[i].cols);
    // (a supersampled call: the fine grid's columns and rows are ints of the coordinate walk)
    if (st == BEVWARP_OK && c.supersample > 1 && ((int64_t)c.supersample * c.dst_w > 0x7fffffffLL || (int64_t)c.supersample * c.dst_h > 0x7fffffffLL))
        st = BEVWARP_ERR_TOO_LARGE;
    return st;
}
// Every written image against every read one, and the written ones against each other; read images may overlap each other.  An image of
// planes is taken as its bounding byte range: a frame's planes need not share the rows' stride.  So is a map plane: it may have fewer
// frames than the destination, which regions_overlap's side-by-side rule does not foresee.
inline int overlap_status(const Call& c) {
    for (int i = 0; i < c.n_writes; i++)
        for (int k = 0; k < c.n_reads; k++) {
            const WrittenImage& w = c.writes[i];
            const Image& r = c.reads[k].im;
            if ((w.planar || c.reads[k].map) ? (r.base < w.end() && w.im.base < r.end()) : regions_overlap(r, w.im)) return BEVWARP_ERR_OVERLAP;
        }
    return (c.n_writes == 2 && written_planes_overlap(c.writes[0].im, c.writes[1].im)) ? BEVWARP_ERR_OVERLAP : BEVWARP_OK;
}

// All argument checks of a call, in either order include/bevwarp.h documents: BEVWARP_OK or the status to return.  (An empty batch ends
// the checks before the overlap: the caller returns on it as well.)
inline int check_call(const Call& c) {
    int (*const format_first[])(const Call&) = {null_status, sides_status, format_status, matrix_count_status, layouts_status, source_sizes_status};
    int (*const layouts_first[])(const Call&) = {null_status, sides_status, layouts_status, matrix_count_status, format_status, source_sizes_status};
    for (auto phase : c.format_first ? format_first : layouts_first) {
        const int st = phase(c);
        if (st != BEVWARP_OK) return st;
    }
    return c.batch == 0 ? BEVWARP_OK : overlap_status(c);
}

// ---- the entry points' calls -------------------------------------------------------------------------------------------------------------
// bevwarp_warp, _warp_border (cubic_ok: a bicubic kernel stands behind them), _warp_classes, and with plane_elem = 4 / 2 bevwarp_warp_planar /
// _warp_planes: `channels` planes of float32 / 16-bit elements, dst_ps apart, instead of interleaved pixels of the source type.
inline Call warp_call(Frames src, Frames dst, const Sizes& z, int channels, int dtype, int interp, bool cubic_ok, int plane_elem = 0, int64_t dst_ps = 0) {
    const int elem = dtype == BEVWARP_U8 ? 1 : 4;
    const bool interp_ok = interp == BEVWARP_NEAREST || interp == BEVWARP_LINEAR || (interp == BEVWARP_CUBIC && cubic_ok);
    Call c = {z, (dtype == BEVWARP_U8 || dtype == BEVWARP_F32) && interp_ok && channels >= 1 && channels <= 4, true};
    c.read(src.image(z.src_h, (uint64_t)z.src_w * channels * elem, z.batch), z.src_w, elem);
    if (plane_elem)
        c.write_planes(dst.image(z.dst_h, (uint64_t)z.dst_w * plane_elem, z.batch), plane_elem, channels, dst_ps);
    else
        c.write(dst.image(z.dst_h, (uint64_t)z.dst_w * channels * elem, z.batch), elem);
    return c;
}
// The border modes bevwarp_warp_border knows (OpenCV's BORDER_ISOLATED bit is none of them): asked before every other check of that entry.
inline bool border_mode_known(int border_mode) { return border_mode >= BEVWARP_BORDER_CONSTANT && border_mode <= BEVWARP_BORDER_TRANSPARENT; }
// BEVWARP_SUPERSAMPLE_2 / _4 / _8 in the `interp` word of bevwarp_warp_border (and of no other entry): the 2-bit field is taken out of the
// word, take_fisheye_flag's way, and every check then sees the word as it always did.  Returns k = 1, 2, 4 or 8; 1: the call is today's.
inline int take_supersample(int& word) {
    const int k = 1 << (((unsigned)word & (unsigned)BEVWARP_SUPERSAMPLE_MASK) >> 12);
    word &= ~BEVWARP_SUPERSAMPLE_MASK;
    return k;
}
// bevwarp_warp_border under the field (k > 1, border_mode known): bevwarp_warp's images and formats without bicubic and without the
// transparent border, and a fine grid of k dst_w x k dst_h pixels, whose sides source_sizes_status judges.  interp: without the field.
inline Call supersample_call(Frames src, Frames dst, const Sizes& z, int channels, int dtype, int interp, int border_mode, int k) {
    Call c = warp_call(src, dst, z, channels, dtype, interp, false);
    c.format_ok = c.format_ok && border_mode != BEVWARP_BORDER_TRANSPARENT;
    c.supersample = k;
    return c;
}
// bevwarp_warp_lens: bevwarp_warp's images and formats without bicubic, with the constant and the transparent border
inline Call lens_call(Frames src, Frames dst, const Sizes& z, int channels, int dtype, int interp, int border_mode) {
    Call c = warp_call(src, dst, z, channels, dtype, interp, false);
    c.format_ok = c.format_ok && (border_mode == BEVWARP_BORDER_CONSTANT || border_mode == BEVWARP_BORDER_TRANSPARENT);
    return c;
}
// What bevwarp_remap and its NV12 kin share: the map count stands where the other entry points have their matrix count, and the xy plane
// stands in the NULL check (no matrices) ...
inline Sizes map_sizes(Sizes z, Frames xy, int map_count) {
    z.m_count = map_count, z.minv = (const double*)xy.base;
    return z;
}
// ... and the two map planes are read images: map_count (1 or batch) frames of dst_h rows of dst_w int16 pairs, and (bilinear) of dst_w
// uint16.  The frac plane is an image under BEVWARP_LINEAR only (NULL there: a NULL image).  c: a call made with map_sizes.
inline void read_map_planes(Call& c, Frames xy, Frames frac, int interp) {
    const int n = (c.m_count == c.batch && c.batch > 0) ? c.batch : 1;
    if (n == 1) xy.fs = frac.fs = 0;  // (one map: its frame stride is not looked at)
    c.read_map(xy.image(c.dst_h, (uint64_t)c.dst_w * 4, n), 4);
    if (interp == BEVWARP_LINEAR) c.read_map(frac.image(c.dst_h, (uint64_t)c.dst_w * 2, n), 2);
}
// BEVWARP_MAP_BICUBIC in the `interp` word of bevwarp_remap (and of no other entry): taken out of the word, take_fisheye_flag's way.  True:
// the call samples a bilinear map bicubically, and what is left of the word must be BEVWARP_LINEAR (remap_call's `bicubic`).
inline bool take_map_bicubic_flag(int& word) {
    const bool bicubic = (word & BEVWARP_MAP_BICUBIC) != 0;
    word &= ~BEVWARP_MAP_BICUBIC;
    return bicubic;
}
// bevwarp_remap: bevwarp_warp's images and formats without bicubic, with all six borders, and the two map planes.  interp: without
// BEVWARP_MAP_BICUBIC (take_map_bicubic_flag), which `bicubic` carries: under it only a bilinear map is a format.
inline Call remap_call(Frames src, Frames dst, Frames xy, Frames frac, const Sizes& z, int map_count, int channels, int dtype, int interp, int border_mode,
                       bool bicubic = false) {
    Call c = warp_call(src, dst, map_sizes(z, xy, map_count), channels, dtype, interp, false);
    c.format_ok = c.format_ok && border_mode >= BEVWARP_BORDER_CONSTANT && border_mode <= BEVWARP_BORDER_TRANSPARENT && (!bicubic || interp == BEVWARP_LINEAR);
    read_map_planes(c, xy, frac, interp);
    return c;
}
// ... and its lens (HOST: fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) and r2_max (+inf: no limit), which check_call does not see
inline int lens_status(const double lens[12], double r2_max) {
    if (!lens) return BEVWARP_ERR_BAD_ARG;
    for (int i = 0; i < 12; i++)
        if (!isfinite(lens[i])) return BEVWARP_ERR_NOT_FINITE;
    if (lens[0] == 0.0 || lens[1] == 0.0 || !(r2_max >= 0.0)) return BEVWARP_ERR_BAD_ARG;  // (a NaN r2_max fails the comparison)
    return BEVWARP_OK;
}
// BEVWARP_LENS_FISHEYE in the `interp` word (bevwarp_warp_lens, bevwarp_build_map) or the `direction` word (bevwarp_project_points_lens):
// taken out of the word, which every check then sees as it always did.  True: the call is a fisheye one.
inline bool take_fisheye_flag(int& word) {
    const bool fisheye = (word & BEVWARP_LENS_FISHEYE) != 0;
    word &= ~BEVWARP_LENS_FISHEYE;
    return fisheye;
}
// ... under which the lens is HOST: fx, fy, cx, cy, k1, k2, k3, k4 and four reserved zeros, and r2_max carries theta_max (+inf: no limit):
// lens_status's order, the reserved entries next to fx and fy
inline int fisheye_status(const double lens[12], double theta_max) {
    if (!lens) return BEVWARP_ERR_BAD_ARG;
    for (int i = 0; i < 12; i++)
        if (!isfinite(lens[i])) return BEVWARP_ERR_NOT_FINITE;
    if (lens[0] == 0.0 || lens[1] == 0.0 || lens[8] != 0.0 || lens[9] != 0.0 || lens[10] != 0.0 || lens[11] != 0.0) return BEVWARP_ERR_BAD_ARG;
    return (theta_max >= 0.0) ? BEVWARP_OK : BEVWARP_ERR_BAD_ARG;  // (a NaN theta_max fails the comparison)
}
// the lens of either model, where bevwarp_warp_lens and bevwarp_project_points_lens look at it
inline int lens_model_status(bool fisheye, const double lens[12], double r2_max) { return fisheye ? fisheye_status(lens, r2_max) : lens_status(lens, r2_max); }
// bevwarp_project_points_lens: every check of the call, in the order include/bevwarp.h documents.  in, out, residual are device
// pointers (never dereferenced), H and lens HOST.  The byte ranges are compared in 128 bits: n next to 2^62 is a range like any other.
// direction: without BEVWARP_LENS_FISHEYE (take_fisheye_flag), which `fisheye` carries.
inline int points_model_status(bool fisheye, const void* in, const void* out, const void* residual, int64_t n, const double* H, const double* lens, double r2_max,
                               int direction, int iters, double tol_px, int dtype) {
    if (!in || !out || !H || n < 0) return BEVWARP_ERR_BAD_ARG;
    if (direction != BEVWARP_LENS_DISTORT && direction != BEVWARP_LENS_UNDISTORT) return BEVWARP_ERR_BAD_ARG;
    if (direction == BEVWARP_LENS_DISTORT && residual) return BEVWARP_ERR_BAD_ARG;
    if (direction == BEVWARP_LENS_UNDISTORT && (iters < 1 || iters > 100 || !(tol_px >= 0.0))) return BEVWARP_ERR_BAD_ARG;  // (a NaN tol_px fails the comparison)
    if (dtype != BEVWARP_F32 && dtype != BEVWARP_F64) return BEVWARP_ERR_UNSUPPORTED;
    const unsigned esz = dtype == BEVWARP_F32 ? 4 : 8;
    if (!finite9(H, 1)) return BEVWARP_ERR_NOT_FINITE;
    const int st = lens_model_status(fisheye, lens, r2_max);
    if (st != BEVWARP_OK) return st;
    if (residual) {
        typedef unsigned __int128 u128;
        const u128 r0 = (uintptr_t)residual, r1 = r0 + (u128)n * esz, pt = (u128)n * (2 * esz);
        const u128 i0 = (uintptr_t)in, o0 = (uintptr_t)out;
        if ((r0 < i0 + pt && i0 < r1) || (r0 < o0 + pt && o0 < r1)) return BEVWARP_ERR_OVERLAP;
    }
    // (last: the kernel moves a point as one 8- or 16-byte unit and a residual as one value)
    return (((uintptr_t)in | (uintptr_t)out) % (2 * esz) || (uintptr_t)residual % esz) ? BEVWARP_ERR_BAD_ARG : BEVWARP_OK;
}
// ... of the rational model
inline int points_lens_status(const void* in, const void* out, const void* residual, int64_t n, const double* H, const double* lens, double r2_max,
                              int direction, int iters, double tol_px, int dtype) {
    return points_model_status(false, in, out, residual, n, H, lens, r2_max, direction, iters, tol_px, dtype);
}
// The element size of a plane type (BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16), or 1 for none of the three
inline int plane_elem_size(int plane_dtype) { return plane_dtype == BEVWARP_F32 ? 4 : ((plane_dtype == BEVWARP_F16 || plane_dtype == BEVWARP_BF16) ? 2 : 1); }
// What the NV12 entry points share: nearest or bilinear, B, G, R or R, G, B.  Each adds its images.
inline Call nv12_family_call(const Sizes& z, int interp, int rgb_order, bool plane_ok = true) {
    return {z, (interp == BEVWARP_NEAREST || interp == BEVWARP_LINEAR) && (rgb_order == 0 || rgb_order == 1) && plane_ok, false};
}
// bevwarp_warp_nv12: to 8-bit pixels of 3 channels
inline Call nv12_call(Frames y, Frames uv, Frames dst, const Sizes& z, int interp, int rgb_order) {
    Call c = nv12_family_call(z, interp, rgb_order);
    c.read_nv12(y, uv);
    c.write(dst.image(z.dst_h, (uint64_t)z.dst_w * 3, z.batch), 1);
    return c;
}
// bevwarp_warp_nv12_planes: to three planes of `plane_dtype` (BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16), dst_ps apart.  A plane type the entry
// point does not take has 1-byte elements here: it asks no alignment, because the layout is looked at first.
inline Call nv12_planes_call(Frames y, Frames uv, Frames dst, int64_t dst_ps, const Sizes& z, int interp, int rgb_order, int plane_dtype) {
    const int elem = plane_elem_size(plane_dtype);
    Call c = nv12_family_call(z, interp, rgb_order, elem != 1);  // (1: none of the three)
    c.read_nv12(y, uv);
    c.write_planes(dst.image(z.dst_h, (uint64_t)z.dst_w * elem, z.batch), elem, 3, dst_ps);
    return c;
}
// bevwarp_remap_nv12: bevwarp_warp_nv12's images, formats and order of checks, with all six borders (a border mode outside them is an
// unsupported format) and bevwarp_remap's map planes; reads[2], reads[3]: the xy and the frac plane
inline Call remap_nv12_call(Frames y, Frames uv, Frames dst, Frames xy, Frames frac, const Sizes& z, int map_count, int interp, int rgb_order, int border_mode) {
    Call c = nv12_call(y, uv, dst, map_sizes(z, xy, map_count), interp, rgb_order);
    c.format_ok = c.format_ok && border_mode >= BEVWARP_BORDER_CONSTANT && border_mode <= BEVWARP_BORDER_TRANSPARENT;
    read_map_planes(c, xy, frac, interp);
    return c;
}
// bevwarp_remap_nv12_planes: bevwarp_warp_nv12_planes' likewise, with the five borders that write every pixel
inline Call remap_nv12_planes_call(Frames y, Frames uv, Frames dst, int64_t dst_ps, Frames xy, Frames frac, const Sizes& z, int map_count, int interp, int rgb_order,
                                   int border_mode, int plane_dtype) {
    Call c = nv12_planes_call(y, uv, dst, dst_ps, map_sizes(z, xy, map_count), interp, rgb_order, plane_dtype);
    c.format_ok = c.format_ok && border_mode >= BEVWARP_BORDER_CONSTANT && border_mode < BEVWARP_BORDER_TRANSPARENT;
    read_map_planes(c, xy, frac, interp);
    return c;
}
// bevwarp_warp_to_nv12: from 8-bit pixels of 3 channels
inline Call to_nv12_call(Frames src, Frames dst_y, Frames dst_uv, const Sizes& z, int interp, int rgb_order) {
    Call c = nv12_family_call(z, interp, rgb_order);
    c.read(src.image(z.src_h, (uint64_t)z.src_w * 3, z.batch), z.src_w, 1);
    c.write_nv12(dst_y, dst_uv);
    return c;
}
// bevwarp_warp_nv12_to_nv12 (the source is sampled as B, G, R)
inline Call nv12_to_nv12_call(Frames y, Frames uv, Frames dst_y, Frames dst_uv, const Sizes& z, int interp) {
    Call c = nv12_family_call(z, interp, 0);
    c.read_nv12(y, uv);
    c.write_nv12(dst_y, dst_uv);
    return c;
}
// bevwarp_remap_to_nv12: bevwarp_remap's order of checks (the format before the layouts) over 8-bit frames of 3 channels, with
// bevwarp_warp_to_nv12's destination where the interleaved one stood, the five borders that write every pixel, and the two map planes;
// reads[1], reads[2]: the xy and the frac plane
inline Call remap_to_nv12_call(Frames src, Frames dst_y, Frames dst_uv, Frames xy, Frames frac, const Sizes& z, int map_count, int interp, int rgb_order, int border_mode) {
    Call c = nv12_family_call(map_sizes(z, xy, map_count), interp, rgb_order, border_mode >= BEVWARP_BORDER_CONSTANT && border_mode < BEVWARP_BORDER_TRANSPARENT);
    c.format_first = true;
    c.read(src.image(z.src_h, (uint64_t)z.src_w * 3, z.batch), z.src_w, 1);
    c.write_nv12(dst_y, dst_uv);
    read_map_planes(c, xy, frac, interp);
    return c;
}
// bevwarp_remap_nv12_to_nv12: bevwarp_remap_nv12's order of checks (the layouts before the format) likewise (the source is sampled as
// B, G, R); reads[2], reads[3]: the xy and the frac plane
inline Call remap_nv12_to_nv12_call(Frames y, Frames uv, Frames dst_y, Frames dst_uv, Frames xy, Frames frac, const Sizes& z, int map_count, int interp, int border_mode) {
    Call c = nv12_to_nv12_call(y, uv, dst_y, dst_uv, map_sizes(z, xy, map_count), interp);
    c.format_ok = c.format_ok && border_mode >= BEVWARP_BORDER_CONSTANT && border_mode < BEVWARP_BORDER_TRANSPARENT;
    read_map_planes(c, xy, frac, interp);
    return c;
}

// bevwarp_remap_planes: bevwarp_remap's order of checks (the format before the layouts) over 8-bit frames of 3 channels, with
// bevwarp_warp_nv12_planes' destination where the interleaved one stood (three planes of `plane_dtype`, dst_ps apart; a plane type the
// entry point does not take has 1-byte elements here and is part of the format), the five borders that write every pixel, and the two
// map planes; reads[1], reads[2]: the xy and the frac plane
inline Call remap_planes_call(Frames src, Frames dst, int64_t dst_ps, Frames xy, Frames frac, const Sizes& z, int map_count, int interp, int border_mode,
                              int plane_dtype) {
    const int elem = plane_elem_size(plane_dtype);
    Call c = nv12_family_call(map_sizes(z, xy, map_count), interp, 0, elem != 1 && border_mode >= BEVWARP_BORDER_CONSTANT && border_mode < BEVWARP_BORDER_TRANSPARENT);
    c.format_first = true;
    c.read(src.image(z.src_h, (uint64_t)z.src_w * 3, z.batch), z.src_w, 1);
    c.write_planes(dst.image(z.dst_h, (uint64_t)z.dst_w * elem, z.batch), elem, 3, dst_ps);
    read_map_planes(c, xy, frac, interp);
    return c;
}

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

// The supersampled warp (warp_supersample.hip): plan_border's grid over the DESTINATION, while the evaluation blocks -- bw0 and its magic --
// are those of the k times finer grid the sub-samples are defined on.  A lane walks fine columns below k (dst_w + tw).
inline TilePlan plan_supersample(int batch, int dst_h, int dst_w, int tw, int th, int k) {
    TilePlan p = plan_border(batch, dst_h, dst_w, tw, th);
    if (p.status != BEVWARP_OK) return p;
    p.bw0 = block_width(k * dst_w, k * dst_h);
    p.bw0_magic = div_magic((uint64_t)k * ((uint64_t)dst_w + tw), (uint32_t)p.bw0);
    return p;
}

// The remap kernel (warp_map.hip): plan_border's tiles, one item per tile and GROUP of frames_per_item consecutive frames -- the item loads
// its tile's map entries once and walks the group's frames with them in registers.  Only a shared map (map_count == 1) is frame-invariant:
// per-frame maps take one frame per item.  A shared map takes the largest power of two up to max_fpi (the library passes 2: warp_map.h) that
// still leaves `fill` items (a few rounds of resident workgroups: enough to fill the machine and to even out tiles of different cost);
// the last group may be short.
// In the plan, tiles_per_frame and its magic decode the item into (group, tile); total_tiles counts items.
struct RemapPlan : TilePlan {
    int frames_per_item, groups;
};
inline RemapPlan plan_remap(int batch, int map_count, int dst_h, int dst_w, int tw, int th, int max_fpi, int64_t fill) {
    RemapPlan p = {};
    p.frames_per_item = 1;
    if (map_count == 1 && batch > 1) {
        const TilePlan one = plan_border(1, dst_h, dst_w, tw, th);
        if (one.status != BEVWARP_OK) {
            static_cast<TilePlan&>(p) = one;
            return p;
        }
        while (p.frames_per_item * 2 <= max_fpi && p.frames_per_item * 2 <= batch && ((int64_t)batch + p.frames_per_item * 2 - 1) / (p.frames_per_item * 2) * one.tiles_per_frame >= fill)
            p.frames_per_item *= 2;
    }
    p.groups = (int)(((int64_t)batch + p.frames_per_item - 1) / p.frames_per_item);  // (in 64 bits: a batch next to 2^31)
    static_cast<TilePlan&>(p) = plan_border(p.groups, dst_h, dst_w, tw, th);
    return p;
}
constexpr int64_t kRemapFillItems = 4096;  // (four rounds of 1024 resident 4-wave workgroups)

// ---- an entry point's steps up to its grid: bevwarp_api.hip and the tests' driver both call these -----------------------------------------
// The flat-grid entries (border, bicubic, lens, NV12, NV12 planes, into NV12): check_call's status, and in `p` the grid of tw x th tiles of a
// call that goes on to a launch (BEVWARP_OK and batch > 0) -- plan_supersample's of a supersampled call, else plan_border's --, zeros of any
// other.  The entry returns the status where it is not BEVWARP_OK, then p.status likewise.
inline int flat_grid(const Call& c, int tw, int th, TilePlan& p) {
    p = {};
    const int st = check_call(c);
    if (st == BEVWARP_OK && c.batch > 0) p = c.supersample > 1 ? plan_supersample(c.batch, c.dst_h, c.dst_w, tw, th, c.supersample) : plan_border(c.batch, c.dst_h, c.dst_w, tw, th);
    return st;
}
// The map samplers (bevwarp_remap and its kin; c.m_count is the map count): the same with plan_remap's grid.
inline int remap_grid(const Call& c, int tw, int th, int max_fpi, int64_t fill, RemapPlan& p) {
    p = {};
    const int st = check_call(c);
    if (st == BEVWARP_OK && c.batch > 0) p = plan_remap(c.batch, c.m_count, c.dst_h, c.dst_w, tw, th, max_fpi, fill);
    return st;
}
// bevwarp_warp_border under BEVWARP_SUPERSAMPLE_* (k > 1; interp: without the field): an unknown border mode is refused before every other
// check, then flat_grid of supersample_call, which is left in `c`.
inline int supersample_grid(Frames src, Frames dst, const Sizes& z, int channels, int dtype, int interp, int border_mode, int k, int tw, int th, Call& c, TilePlan& p) {
    p = {};
    if (!border_mode_known(border_mode)) return BEVWARP_ERR_UNSUPPORTED;
    return flat_grid(c = supersample_call(src, dst, z, channels, dtype, interp, border_mode, k), tw, th, p);
}

// bevwarp_build_map: every check of the call, in the order include/bevwarp.h documents, and in `p` plan_border's grid over the m_count maps.
// M, xy, frac are device pointers (never dereferenced), lens HOST or NULL.  interp: without BEVWARP_LENS_FISHEYE (take_fisheye_flag), which
// `fisheye` carries; a fisheye map has no pinhole chain to fall back to, so a NULL lens is refused there.
inline int build_map_model_status(bool fisheye, const double* M, int m_count, const double* lens, double r2_max, int interp, Frames xy, Frames frac, int dst_h, int dst_w,
                                  int tw, int th, TilePlan& p) {
    p = {};
    if (!M || !xy.base || m_count < 1 || dst_h <= 0 || dst_w <= 0) return BEVWARP_ERR_BAD_ARG;
    if (interp != BEVWARP_NEAREST && interp != BEVWARP_LINEAR) return BEVWARP_ERR_UNSUPPORTED;
    const bool with_frac = interp == BEVWARP_LINEAR;
    if (with_frac && !frac.base) return BEVWARP_ERR_BAD_ARG;
    if (m_count == 1) xy.fs = frac.fs = 0;
    const Image ixy = xy.image(dst_h, (uint64_t)dst_w * 4, m_count), ifr = frac.image(dst_h, (uint64_t)dst_w * 2, m_count);
    if (layout_status(ixy, 4) != BEVWARP_OK || (with_frac && layout_status(ifr, 2) != BEVWARP_OK)) return BEVWARP_ERR_BAD_ARG;
    p = plan_border(m_count, dst_h, dst_w, tw, th);
    if (p.status != BEVWARP_OK) return p.status;
    if (with_frac && regions_overlap(ixy, ifr)) return BEVWARP_ERR_OVERLAP;  // (both are written)
    return (lens || fisheye) ? lens_model_status(fisheye, lens, r2_max) : BEVWARP_OK;
}
// ... of the pinhole chain and the rational model
inline int build_map_status(const double* M, int m_count, const double* lens, double r2_max, int interp, Frames xy, Frames frac, int dst_h, int dst_w, int tw, int th,
                            TilePlan& p) {
    return build_map_model_status(false, M, m_count, lens, r2_max, interp, xy, frac, dst_h, dst_w, tw, th, p);
}
// the lane-wide accesses of the two planes: 16 bytes of xy, 8 bytes of frac (no frac plane: the xy plane decides)
inline bool map_vec_ok(const Image& xy, const Image* frac) { return wide_stores_ok(xy, 16) && (!frac || wide_stores_ok(*frac, 8)); }

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

// ---- the stitches: bevwarp_warp_stitch and the six through maps -- the whole of their host side but the launch ----------------------------------
// What every stitch narrows its camera's format to: the two blend rules, and the constant and the transparent border.
inline bool stitch_format_ok(int blend, int border_mode) {
    return (blend == BEVWARP_STITCH_OVER || blend == BEVWARP_STITCH_FEATHER) && (border_mode == BEVWARP_BORDER_CONSTANT || border_mode == BEVWARP_BORDER_TRANSPARENT);
}
// BEVWARP_STITCH_GAIN in the `blend` word of the six stitches through maps: taken out of the word, which every check then sees as it always
// did (take_fisheye_flag's way).  True: every camera's `reserved` is its gain word, G0 | G1 << 10 | G2 << 20 in Q8, bits 30 and 31 zero.
inline bool take_gain_flag(int& blend) {
    const bool gained = (blend & BEVWARP_STITCH_GAIN) != 0;
    blend &= ~BEVWARP_STITCH_GAIN;
    return gained;
}
// a camera's gain word as stitch_check reads it under the flag (bevwarp_warp_stitch has no gains: its check never asks)
inline uint32_t gain_word(const bevwarp_map_camera& k) { return (uint32_t)k.reserved; }
inline uint32_t gain_word(const bevwarp_camera&) { return 0u; }
inline bool gain_word_ok(uint32_t g) { return (g >> 30) == 0u; }
// bevwarp_warp_stitch, one camera of it: that camera's frames against the canvas -- bevwarp_warp's images and formats without bicubic,
// narrowed as above.  (stitch_check below runs the checks over all cameras.)
inline Call stitch_call(const bevwarp_camera& k, Frames dst, int batch, int dst_h, int dst_w, int channels, int dtype, int interp, int blend, int border_mode) {
    Call c = warp_call({k.src, k.frame_stride, k.row_stride}, dst, {batch, k.src_h, k.src_w, dst_h, dst_w, k.m_count, k.M_inv}, channels, dtype, interp, false);
    c.format_ok = c.format_ok && stitch_format_ok(blend, border_mode);
    return c;
}
// What a bevwarp_map_camera passes, as the remap calls take it: its frames (NV12: Y and the pairs), its two map planes, its sides.
struct MapCamera {
    Frames src, uv, xy, frac;
    Sizes z;
};
inline MapCamera map_camera(const bevwarp_map_camera& k, int batch, int dst_h, int dst_w) {
    return {{k.src, k.frame_stride, k.row_stride},
            {k.uv, k.uv_frame_stride, k.uv_row_stride},
            {k.map_xy, k.xy_frame_stride, k.xy_row_stride},
            {k.map_frac, k.frac_frame_stride, k.frac_row_stride},
            {batch, k.src_h, k.src_w, dst_h, dst_w, 0, nullptr}};
}
// bevwarp_stitch_maps, bevwarp_stitch_maps_nv12, one camera of either: that camera's frames and map planes against the canvas --
// bevwarp_remap's (bevwarp_remap_nv12's) call, its format narrowed to the two blend rules and to the constant and the transparent border.
// reads[]: the frames (NV12: Y, then the pairs), the xy plane and, bilinear, the frac plane.
// blend: without BEVWARP_STITCH_GAIN (take_gain_flag), which `gained` carries: the gain step knows 8-bit pixels of 3 channels only.
inline Call stitch_maps_call(const bevwarp_map_camera& k, Frames dst, int batch, int dst_h, int dst_w, int channels, int dtype, int interp, int blend, int border_mode,
                             bool gained = false) {
    const MapCamera m = map_camera(k, batch, dst_h, dst_w);
    Call c = remap_call(m.src, dst, m.xy, m.frac, m.z, k.map_count, channels, dtype, interp, border_mode);
    c.format_ok = c.format_ok && stitch_format_ok(blend, border_mode) && (!gained || (dtype == BEVWARP_U8 && channels == 3));
    return c;
}
inline Call stitch_maps_nv12_call(const bevwarp_map_camera& k, Frames dst, int batch, int dst_h, int dst_w, int interp, int blend, int rgb_order, int border_mode) {
    const MapCamera m = map_camera(k, batch, dst_h, dst_w);
    Call c = remap_nv12_call(m.src, m.uv, dst, m.xy, m.frac, m.z, k.map_count, interp, rgb_order, border_mode);
    c.format_ok = c.format_ok && stitch_format_ok(blend, border_mode);
    return c;
}
// bevwarp_stitch_maps_to_nv12, bevwarp_stitch_maps_nv12_to_nv12, one camera of either: bevwarp_remap_to_nv12's (bevwarp_remap_nv12_to_nv12's)
// call under BEVWARP_BORDER_CONSTANT -- there is no border mode: what no camera covers is the border pixel -- its format narrowed to the two
// blend rules.  nv12: the cameras' frames are NV12 (rgb_order is not looked at).
inline Call stitch_maps_nv12_out_call(bool nv12, const bevwarp_map_camera& k, Frames dst_y, Frames dst_uv, int batch, int dst_h, int dst_w, int interp, int blend,
                                      int rgb_order) {
    const MapCamera m = map_camera(k, batch, dst_h, dst_w);
    Call c = nv12 ? remap_nv12_to_nv12_call(m.src, m.uv, dst_y, dst_uv, m.xy, m.frac, m.z, k.map_count, interp, BEVWARP_BORDER_CONSTANT)
                  : remap_to_nv12_call(m.src, dst_y, dst_uv, m.xy, m.frac, m.z, k.map_count, interp, rgb_order, BEVWARP_BORDER_CONSTANT);
    c.format_ok = c.format_ok && stitch_format_ok(blend, BEVWARP_BORDER_CONSTANT);
    return c;
}
// bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes, one camera of either: bevwarp_remap_planes' (bevwarp_remap_nv12_planes') call
// likewise.  nv12: the cameras' frames are NV12 (otherwise rgb_order is not looked at).
inline Call stitch_maps_planes_call(bool nv12, const bevwarp_map_camera& k, Frames dst, int64_t dst_ps, int batch, int dst_h, int dst_w, int interp, int blend,
                                    int rgb_order, int plane_dtype) {
    const MapCamera m = map_camera(k, batch, dst_h, dst_w);
    Call c = nv12 ? remap_nv12_planes_call(m.src, m.uv, dst, dst_ps, m.xy, m.frac, m.z, k.map_count, interp, rgb_order, BEVWARP_BORDER_CONSTANT, plane_dtype)
                  : remap_planes_call(m.src, dst, dst_ps, m.xy, m.frac, m.z, k.map_count, interp, BEVWARP_BORDER_CONSTANT, plane_dtype);
    c.format_ok = c.format_ok && stitch_format_ok(blend, BEVWARP_BORDER_CONSTANT);
    return c;
}

// The status of a stitch in the order include/bevwarp.h documents: the camera array and count, the feather, under BEVWARP_STITCH_GAIN
// (gains != NULL; blend is the word without the flag) every camera's gain word in ascending k, every check of camera 0's call
// before camera 1's (describe(cams[k]): one of the calls above), the grid of tw x th tiles (kBorderTileW x kBorderTileH) over the canvas, and
// last the HOST values -- the border value, then scale, then bias: `n` doubles each, or NULL.  A stitch with a border mode passes its border
// value under BEVWARP_BORDER_CONSTANT only: no other mode reads it.  cams is HOST; no device pointer is dereferenced.
// Out: in `calls` (BEVWARP_STITCH_MAX_CAMERAS entries of the caller's) every camera's call as it was checked -- what is launched is filled
// from these -- in `p` the grid, and in `gains` (where given) the checked gain words; all are whole when the call goes on to a launch
// (BEVWARP_OK and batch > 0).
struct HostValues {
    const double* v;
    int n;
};
template <class Camera, class Describe>
int stitch_check(const Camera* cams, int n_cams, int blend, int feather, Describe describe, std::initializer_list<HostValues> values, int batch, int dst_h, int dst_w,
                 int tw, int th, TilePlan& p, Call* calls, uint32_t* gains = nullptr) {
    p = {};
    if (!cams || n_cams < 1 || n_cams > BEVWARP_STITCH_MAX_CAMERAS) return BEVWARP_ERR_BAD_ARG;
    if (blend == BEVWARP_STITCH_FEATHER && (feather < 1 || feather > 4096)) return BEVWARP_ERR_BAD_ARG;
    for (int k = 0; gains && k < n_cams; k++)
        if (!gain_word_ok(gains[k] = gain_word(cams[k]))) return BEVWARP_ERR_BAD_ARG;
    for (int k = 0; k < n_cams; k++) {  // every camera against the canvas; what the cameras read may overlap
        const int st = check_call(calls[k] = describe(cams[k]));
        if (st != BEVWARP_OK) return st;
    }
    p = plan_border(batch, dst_h, dst_w, tw, th);
    if (p.status != BEVWARP_OK) return p.status;
    for (const HostValues& h : values)
        for (int c = 0; h.v && c < h.n; c++)
            if (!isfinite(h.v[c])) return BEVWARP_ERR_NOT_FINITE;
    return BEVWARP_OK;
}

}  // namespace plan
}  // namespace bevwarp
