/*
 * bevwarp.h -- C ABI of libbevwarp.so, the MI355X (gfx950) BEV homography-warp path.
 *
 * The reference (minghanz/bev) has no FFI / plugin interface for this path: its pixel work is one
 * third-party call.  Every entry point below names the reference interface it stands in for
 * (paths relative to the reference repository root):
 *
 *   bevwarp_warp            cv2.warpPerspective(img, H_bev_img, (u_size, v_size))
 *                             vis_homo.py:89, vis_homo.py:91, bev/tool/compo.py:38,46,47
 *   bevwarp_warp_border     cv2.warpPerspective(img, H, dsize, dst, flags, borderMode): the drop-in surface's other borders
 *                             (the reference passes none; stitching cameras with BORDER_TRANSPARENT needs one)
 *   bevwarp_warp_lens       cv2.undistort(img, K, dist_coeff) + cv2.warpPerspective(undist, H_bev_img, (u_size, v_size)) on the frames a
 *                             camera delivers, in one resampling: Calib carries `dist_coeff` (bev/calib.py:25), Rt_from_pts_K_dist
 *                             takes `dist_coeffs` (bev/homo.py:130-135), and the material the reference was developed on went through
 *                             a separate undistortion pass first (KAB_SK_1_undist/..., vis_homo.py:30-31)
 *   bevwarp_build_map, bevwarp_remap
 *                           cv2.initUndistortRectifyMap / cv2.convertMaps once and cv2.remap per frame, for the camera loop of a FIXED
 *                             camera: one H_bev_img, one K, one Calib.dist_coeff (bev/calib.py:25) and then the same warp for every frame
 *                             of a video (vis_homo.py:85-91).  The coordinate chain of bevwarp_warp_border / bevwarp_warp_lens runs once
 *                             per camera and BEV geometry and is kept as OpenCV's fixed-point maps; every batch is then sampled through
 *                             them with no float64 at all.  bevwarp_remap is also the generic cv2.remap(src, map1, map2, ...)
 *   bevwarp_warp_stitch     one cv2.warpPerspective(img_k, H_bev_img_k, (u_size, v_size)) per camera of a site into ONE BEV image:
 *                             preset_calib("KoPER", 1 | 4) describes two cameras of one intersection in one world frame
 *                             (bev/constructor/homo_constr.py:19-25), BrnoCompSpeed sessions have a left, a centre and a right camera
 *                             (vis_homo.py:39-43).  All cameras in one launch, last-wins or blended where they overlap
 *   bevwarp_stitch_maps, bevwarp_stitch_maps_nv12
 *                           the same site with FIXED, possibly distorted cameras (Calib.dist_coeff, bev/calib.py:25), from BGR frames or
 *                             from the decoders' NV12 frames: one cv2.remap(img_k, map1_k, map2_k, ..., BORDER_TRANSPARENT) per camera
 *                             into ONE BEV image, through the maps bevwarp_build_map made once per camera -- all cameras in one launch,
 *                             last-wins or blended, no float64
 *   bevwarp_warp_classes, bevwarp_tile_classes_bytes
 *                           the same call inside a camera loop (one H_bev_img, every frame of the video): vis_homo.py:85-91
 *   bevwarp_invert_homography  the cv::invert(M) step inside that call (M is the forward src->dst map)
 *   bevwarp_warp_planar     the same warp (8-bit or float32 frames), written as normalised float32 channel planes in the same
 *                             pass (the layout step between vis_homo.py:89 and a detector's input;
 *                             the reference leaves it to its callers)
 *   bevwarp_warp_planes     the same planes as float32, float16 or bfloat16: the layout AND precision step between
 *                             vis_homo.py:89 and a detector's input (detectors on this hardware run in 16 bits; the `.half()` pass
 *                             behind bevwarp_warp_planar is folded into the warp's stores)
 *   bevwarp_warp_nv12       `ok, img = video.read()` + cv2.warpPerspective(img, H_bev_img, (u_size, v_size)), vis_homo.py:86-89,
 *                             without the decoder's colour-conversion pass: the warp samples the decoder's NV12 planes and
 *                             converts each tap (cv2.cvtColor(nv12, COLOR_YUV2BGR_NV12) never exists in memory)
 *   bevwarp_warp_nv12_planes  the same decoder frames, vis_homo.py:86-89, written straight as the detector-input planes of
 *                             bevwarp_warp_planes (float32, float16 or bfloat16): decoder -> BEV -> detector input in one launch,
 *                             with neither the converted frame nor the 8-bit BEV frame in memory
 *   bevwarp_remap_nv12, bevwarp_remap_nv12_planes
 *                           the two above for the camera loop of a FIXED, possibly distorted camera, vis_homo.py:85-91 with
 *                             Calib.dist_coeff (bev/calib.py:25): the decoder's NV12 frames sampled through the maps that
 *                             bevwarp_build_map made once -- cv2.remap(cv2.cvtColor(nv12, COLOR_YUV2BGR_NV12), map1, map2, ...) per
 *                             frame, with the lens in the map, no float64, and no converted frame in memory
 *   bevwarp_warp_to_nv12    cv2.warpPerspective(img, H_bev_img, (u_size, v_size)) + `writer.write(bev)`, vis_homo.py:109-111 and
 *                             bev/io/utils.py:89-99, without the BGR -> YUV 4:2:0 pass a video writer hides inside write(): the warp
 *                             stores the BEV frame as NV12, what an encoder takes (the tracker tools read the encoded bev.avi)
 *   bevwarp_warp_nv12_to_nv12  the same egress from a decoder's NV12 frames, vis_homo.py:85-111 and bev/io/utils.py:89-99:
 *                             decoder -> BEV -> encoder in one launch, with no BGR frame in memory on either side
 *   bevwarp_remap_to_nv12, bevwarp_remap_nv12_to_nv12, bevwarp_stitch_maps_to_nv12, bevwarp_stitch_maps_nv12_to_nv12
 *                           the same two egresses for FIXED, possibly distorted cameras, vis_homo.py:85-111 and bev/io/utils.py:89-99 with
 *                             Calib.dist_coeff (bev/calib.py:25): one camera or a site's cameras, BGR or decoder frames, sampled through
 *                             the maps bevwarp_build_map made once and stored as the NV12 frame an encoder takes -- one launch, no
 *                             float64, no BGR BEV frame in memory
 *   bevwarp_remap_planes, bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes
 *                           the detector-input planes of bevwarp_warp_planes for the same FIXED, possibly distorted cameras,
 *                             vis_homo.py:85-91 with Calib.dist_coeff (bev/calib.py:25): one camera's BGR frames or a site's cameras, BGR or
 *                             decoder frames, sampled through the maps bevwarp_build_map made once and written as normalised float32,
 *                             float16 or bfloat16 channel planes -- one launch, no float64, no 8-bit BEV frame or canvas in memory
 *   bevwarp_composite       composite_reg_img(bg, fg, fg_mask), bev/tool/compo.py:5-24 (the blend after the three warps
 *                             of composite_bev_img, :26-49)
 *   bevwarp_warp_composite  composite_bev_img(bg, fg, fg_mask, ...), bev/tool/compo.py:26-49: the three warps and the blend
 *                             in one launch, no warped image in memory
 *   bevwarp_footprint       -- measurement aid (SURVEY.md 8(d) "footprint_px"), no reference twin
 *   bevwarp_project_points  pts_world_bev(pts_src, H), bev/rbox.py:136-151; rbox_world_img, :221-226;
 *                             Calib.gen_center_in_world, bev/calib.py:135-138
 *   bevwarp_project_points_lens  the same three on the frames a distorted camera delivers -- rbox_world_img, bev/rbox.py:221-226 (world ->
 *                             RAW pixel) and Calib.gen_center_in_world, bev/calib.py:135-138 (RAW pixel -> world) -- through the lens the
 *                             reference carries and never applies to points: Calib.dist_coeff (bev/calib.py:25), Rt_from_pts_K_dist's
 *                             `dist_coeffs` (bev/homo.py:130-135).  What cv2.projectPoints / cv2.undistortPoints are for
 *   bevwarp_rbox_iou        iou_batch_rbox -> d3d.box.box2d_iou(.., method="rbox"),
 *                             bev/tracker/rbox_tracker.py:87-92 (call site :393-394)
 *   bevwarp_rbox_transform  rbox_world_bev(rbox_src, H, src), bev/rbox.py:173-219 (yaw conventions :20-36)
 *   bevwarp_tracker_step    one frame of bev/tool/rbox_tracking_BrnoCompSpeed.py:88-109 up to the assignment: detections
 *                             BEV -> world (rbox_world_bev), IoU against the trackers' predicted boxes (iou_batch_rbox),
 *                             the `iou > iou_threshold` gate of associate_detections_to_trackers
 *                             (bev/tracker/rbox_tracker.py:383-405) and the image-plane centres (rbox_world_img,
 *                             bev/rbox.py:221-226) -- ONE launch; the Hungarian assignment and the Kalman filters stay
 *                             on the host
 *
 * Conventions
 *   - Plain C: pointers, sizes, enums.  No torch / HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*; NULL = the default stream).
 *   - All data pointers are DEVICE pointers (HIP) unless marked HOST.  The library never allocates,
 *     frees or retains caller memory; every call is asynchronous and ordered on `stream`.
 *   - Images are interleaved HWC, strides in BYTES.  Homographies are 3x3 row-major float64.
 *   - Return value: BEVWARP_OK (0) or a negative bevwarp_status; bevwarp_strerror() describes it.
 *     Nothing throws across the ABI.  There is NO CPU fallback: without a HIP device calls fail.
 *   - Thread-safe and re-entrant: no global mutable state.
 */
#ifndef BEVWARP_H
#define BEVWARP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEVWARP_ABI_VERSION 7

typedef enum bevwarp_status {
    BEVWARP_OK = 0,
    BEVWARP_ERR_BAD_ARG = -1,      /* NULL pointer, non-positive size, misaligned stride                 */
    BEVWARP_ERR_UNSUPPORTED = -2,  /* dtype / channel count / interpolation outside the supported set    */
    BEVWARP_ERR_TOO_LARGE = -3,    /* source side > 32767 px (fixed-point map range), a source row >= 16 MiB or frame >= 2 GiB */
    BEVWARP_ERR_NOT_FINITE = -4,   /* homography contains NaN / Inf                                      */
    BEVWARP_ERR_HIP = -5,          /* a HIP runtime call failed; see bevwarp_last_hip_error()            */
    BEVWARP_ERR_OVERLAP = -6       /* source and destination share bytes (ABI v5; v4 reported BAD_ARG)   */
} bevwarp_status;

/* BEVWARP_F16 (IEEE binary16) and BEVWARP_BF16 (bfloat16) are plane types of bevwarp_warp_planes and bevwarp_warp_nv12_planes only: as a
 * pixel or point type every entry point answers BEVWARP_ERR_UNSUPPORTED for them. */
typedef enum bevwarp_dtype { BEVWARP_U8 = 0, BEVWARP_F32 = 1, BEVWARP_F64 = 2, BEVWARP_F16 = 3, BEVWARP_BF16 = 4 } bevwarp_dtype;

/* Same numeric values as cv2.INTER_NEAREST / cv2.INTER_LINEAR / cv2.INTER_CUBIC.  BEVWARP_CUBIC is taken by bevwarp_warp and
 * bevwarp_warp_border only; every other entry point with an `interp` returns BEVWARP_ERR_UNSUPPORTED for it. */
typedef enum bevwarp_interp { BEVWARP_NEAREST = 0, BEVWARP_LINEAR = 1, BEVWARP_CUBIC = 2 } bevwarp_interp;

int bevwarp_version(void);
const char *bevwarp_strerror(int status);
/* Text of the last HIP error seen by the calling thread ("" if none). */
const char *bevwarp_last_hip_error(void);

/* HOST helper.  M_inv[i] = inverse of M_fwd[i] (n matrices of 9 doubles each) with the closed-form
 * cofactor / (1/det) evaluation order OpenCV uses for 3x3 doubles; a singular matrix inverts to
 * all zeros.  Callers upload M_inv to the device and hand it to bevwarp_warp. */
int bevwarp_invert_homography(const double *M_fwd /*HOST*/, double *M_inv /*HOST*/, int n);

/*
 * dst[b] = warpPerspective(src[b], M[b], (dst_w, dst_h)) for b in [0, batch), BORDER_CONSTANT.
 *
 *   src, dst       device; `channels` interleaved values of `dtype` (BEVWARP_U8 | BEVWARP_F32) per pixel.
 *                  src and dst must not overlap (an in-place warp would read taps other workgroups have already
 *                  overwritten): the call returns BEVWARP_ERR_OVERLAP when the byte ranges [src, last byte of
 *                  frame batch-1] and [dst, last byte of frame batch-1] intersect -- unless both walk their rows
 *                  with one common stride (equal row strides, frame strides multiples of it) and their rows
 *                  occupy disjoint byte columns of that stride: two ROIs of one image that lie side by side are
 *                  accepted, as cv2.warpPerspective accepts them.
 *                  "each tap outside replaced by the border value": a pixel whose four taps are ALL outside
 *                  is the border value itself (float32 too), as in OpenCV's remapBilinear.
 *   *_frame_stride bytes between consecutive frames; *_row_stride bytes between rows (>= row bytes).
 *   M_inv          device; INVERSE (dst px -> src px) matrices, float64, row-major;
 *                  m_count == batch (one per frame) or 1 (shared by all frames).
 *   interp         BEVWARP_NEAREST: (X, Y) = round-half-even((x', y') / w'); copy or border.
 *                  BEVWARP_LINEAR : coordinates quantised to 1/32 px, 4 taps, each tap outside the
 *                  source replaced by the border value; u8 in 15-bit fixed point, f32 in float.
 *                  BEVWARP_CUBIC  : 16 taps, bevwarp_warp_border's BEVWARP_BORDER_CONSTANT (defined there).
 *   border_value   HOST, `channels` doubles, or NULL for 0.
 *   channels       1..4.   src_w, src_h <= 32767.
 */
int bevwarp_warp(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                 int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                 const double *M_inv, int m_count, int dtype, int interp, const double *border_value /*HOST*/,
                 void *stream);

/* Same numeric values as OpenCV's cv::BorderTypes (cv2.BORDER_*). */
typedef enum bevwarp_border {
    BEVWARP_BORDER_CONSTANT = 0,
    BEVWARP_BORDER_REPLICATE = 1,
    BEVWARP_BORDER_REFLECT = 2,
    BEVWARP_BORDER_WRAP = 3,
    BEVWARP_BORDER_REFLECT_101 = 4,
    BEVWARP_BORDER_TRANSPARENT = 5
} bevwarp_border;

/*
 * bevwarp_warp with OpenCV's other border modes: cv2.warpPerspective(..., borderMode=border_mode).  Arguments up to `interp`
 * and their checks are bevwarp_warp's; the coordinate maps (and their 1/32-px quantisation) are too.  Per destination pixel,
 * with (sx, sy) the integer source position (bilinear: X >> 5, Y >> 5) SATURATED TO INT16 as OpenCV's maps are:
 *   BEVWARP_BORDER_CONSTANT     exactly bevwarp_warp (nearest, bilinear: the call is delegated to it; border_value as there).
 *   BEVWARP_BORDER_REPLICATE    every tap index p (sx, sx + 1, sy, sy + 1; nearest: sx, sy) goes through OpenCV's
 *   BEVWARP_BORDER_REFLECT      borderInterpolate(p, len, mode) -- clamp / reflect with the edge pixel repeated (fedcba|abcd) /
 *   BEVWARP_BORDER_WRAP         p mod len / reflect about the edge pixel (dcb|abcd); len 1 maps every index to 0 -- and the
 *   BEVWARP_BORDER_REFLECT_101  four taps are blended as bevwarp_warp blends them.  No pixel is the border value.
 *   BEVWARP_BORDER_TRANSPARENT  only inliers are written: nearest 0 <= sx < src_w and 0 <= sy < src_h; bilinear
 *                               0 <= sx <= src_w - 2 and 0 <= sy <= src_h - 2 (remapBilinear's test: an identity warp leaves
 *                               the last source column and row unwritten).  Every other destination byte is neither read
 *                               nor written -- dst keeps what it held: warping several cameras into one canvas, one call each.
 *                               (All of them in one launch, blended where they overlap if asked: bevwarp_warp_stitch.)
 *   border_value  HOST; read by BEVWARP_BORDER_CONSTANT only (ignored otherwise, as in OpenCV).
 *   border_mode   any other value (OpenCV's BORDER_ISOLATED bit included) returns BEVWARP_ERR_UNSUPPORTED.
 * Semantics restated from OpenCV 3.x-4.x imgwarp.cpp (remapNearest / remapBilinear); parity unpinned, like the rest of the warp.
 *
 * interp == BEVWARP_CUBIC (cv2.INTER_CUBIC), all six modes -- remapBicubic, restated from memory, parity unpinned as above:
 *   maps      the bilinear maps (X, Y in 1/32 px).  The 4 x 4 tap window starts at sx = sat16(X >> 5) - 1, sy = sat16(Y >> 5) - 1
 *             (saturation first); (fy, fx) = (Y & 31, X & 31) selects the weights.
 *   weights   float32, A = -0.75, x = f / 32:  c0 = ((A(x+1) - 5A)(x+1) + 8A)(x+1) - 4A,  c1 = ((A+2)x - (A+3))x x + 1,
 *             c2 = the same of 1 - x,  c3 = 1 - c0 - c1 - c2;  W[4 i + j] = cy[i] * cx[j] (i the row).  8-bit pixels: each
 *             rounded to int16 at scale 32768 (half to even, saturated), then the entry's sum is brought to 32768 at one of
 *             the taps (i, j) in {2, 3} x {2, 3}: a deficit is added to the largest of them, a surplus taken off the smallest.
 *   inlier    0 <= sx < max(src_w - 3, 0) and 0 <= sy < max(src_h - 3, 0), any mode: all 16 taps are source pixels;
 *             sum = ((r0 + r1) + r2) + r3 with r_i = ((S[i][0] W[4i] + S[i][1] W[4i+1]) + S[i][2] W[4i+2]) + S[i][3] W[4i+3].
 *   otherwise TRANSPARENT writes the pixel only if (sx + 1, sy + 1) lies in the source (so it writes exactly the pixels whose
 *             integer position does -- an identity warp writes every pixel) and then continues with REFLECT_101's indices;
 *             CONSTANT stores the border value itself when the whole window is outside (sx >= src_w, sx + 4 <= 0, sy >= src_h
 *             or sy + 4 <= 0); else, with cv the border value (CONSTANT) or 0 and every tap index through borderInterpolate
 *             (-1 = outside, CONSTANT only): sum = cv * ONE, then tap by tap, rows outermost, sum = sum + (S - cv) * W,
 *             taps outside skipped.
 *   result    8-bit: integers, ONE = 32768, clamp((sum + 16384) >> 15, 0, 255) -- bicubic overshoots, both clamps are live.
 *             float32: ONE = 1, every multiply and add rounded to float32 in the order written, no FMA; the two orders
 *             (row sums for inliers, tap by tap otherwise) are both part of the definition.
 */
int bevwarp_warp_border(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                        int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                        const double *M_inv, int m_count, int dtype, int interp, int border_mode,
                        const double *border_value /*HOST*/, void *stream);

/*
 * BEVWARP_SUPERSAMPLE_2 / _4 / _8: the supersampled warp, a 2-bit field ORed into `interp` of bevwarp_warp_border -- and of no other
 * entry: every other entry judges the whole word and refuses one that carries these bits.  The field is taken out of the word before any
 * check; with the field 0 the call is the one described above, bit for bit and status for status.  With k = 1 << ((interp >> 12) & 3)
 * in {2, 4, 8}, every destination pixel is the average of the k x k pixels that bevwarp_warp_border ITSELF writes on a k times finer
 * grid: a BEV whose far half is minified several times over is sampled k^2 times per pixel instead of once, in one pass, with no fine
 * frame in memory.  M_inv is the same device matrix as ever (destination pixel -> source pixel), m_count 1 or batch.  Every line below
 * is one correctly rounded float64 operation, no FMA:
 *   fine matrix   c = (1 - k) / (2 k), exact (-0.25, -0.375, -0.4375); for each row r of M_inv
 *                     F[r][0] = M[r][0] / k,   F[r][1] = M[r][1] / k,   F[r][2] = (M[r][0] c + M[r][1] c) + M[r][2]:
 *                 the centre of fine pixel (x', y') is the destination coordinate ((x' + 0.5) / k - 0.5, (y' + 0.5) / k - 0.5).
 *   fine sample   s(x', y') = the pixel bevwarp_warp_border writes at (x', y') of a (k dst_w) x (k dst_h) destination with inverse matrix
 *                 F and the call's interp, border_mode and border_value: the evaluation blocks of THAT grid (width
 *                 min(1024 / min(16, k dst_h), k dst_w) -- no multiple of k in general, a pixel's sub-columns may lie in two blocks),
 *                 32 / W, half-to-even rounding, NaN -> INT_MAX, int16 saturation, the 8-bit 15-bit blend and the float32 blend, and
 *                 BEVWARP_BORDER_CONSTANT's "all four taps outside -> the border value itself".
 *   reduce        8-bit, per channel: (sum of the k^2 sub-samples + k^2 / 2) >> (2 log2 k).
 *                 float32: acc = s(k x, k y); then, rows outermost (j = 0..k-1, i = 0..k-1, the first skipped),
 *                 acc = acc + s(k x + i, k y + j), each addition rounded to float32; the pixel is acc * (1 / k^2), one float32 multiply.
 *                 NaN and +-inf propagate as IEEE says; denormals are not flushed.
 *   formats       BEVWARP_U8 | BEVWARP_F32, 1-4 channels, BEVWARP_NEAREST | BEVWARP_LINEAR, and the five borders that write every
 *                 pixel: CONSTANT (a mode of the supersampled kernel -- the call is NOT delegated to bevwarp_warp), REPLICATE, REFLECT,
 *                 WRAP, REFLECT_101.  Under the field BEVWARP_CUBIC and BEVWARP_BORDER_TRANSPARENT are BEVWARP_ERR_UNSUPPORTED, judged
 *                 where the format is judged; k dst_w or k dst_h beyond INT_MAX is BEVWARP_ERR_TOO_LARGE, judged where the source's
 *                 size is judged.  Every other check and the checks' order are bevwarp_warp_border's: an unknown border_mode first,
 *                 NULLs, sides, the format, m_count, strides, sizes, overlap, and a non-finite border_value last (CONSTANT only).
 *                 batch == 0 is BEVWARP_OK and launches nothing.
 * With k > 1 the identity matrix is NOT the identity image: the sub-samples sit at +-1/(2k), +-3/(2k), ... off the pixel's centre, so
 * every pixel is a small box filter of its neighbourhood.  The ramp row 0, 32, ..., 224 under k = 2, bilinear, REPLICATE becomes
 * 4, 32, 64, ..., 192, 220.
 * Cost: k^2 times the coordinate chains and tap gathers of bevwarp_warp_border, against a fine frame set
 * written once and read once by the two-pass route.
 */
#define BEVWARP_SUPERSAMPLE_2    0x1000
#define BEVWARP_SUPERSAMPLE_4    0x2000
#define BEVWARP_SUPERSAMPLE_8    0x3000
#define BEVWARP_SUPERSAMPLE_MASK 0x3000      /* k = 1 << ((interp >> 12) & 3) */

/*
 * The warp of frames as a distorted camera delivers them: the lens model is a step of the coordinate chain, and the raw frame is sampled
 * once.  Destination pixel -> normalised undistorted camera plane (M_ray) -> distorted image point (OpenCV's rational model: k1..k6, p1,
 * p2; no thin-prism or tilt terms; the fisheye model is BEVWARP_LENS_FISHEYE below) -> the taps and the blend of bevwarp_warp_border.  This is OUR chain, the natural extension
 * of bevwarp_warp's, not a restatement of cv2.undistort + cv2.warpPerspective (which resample twice) or of initUndistortRectifyMap
 * (which accumulates its row terms): parity with OpenCV is unpinned.  It is bit-reproducible: every step below is one correctly rounded
 * float64 + - * / (IEEE division, no FMA), in the order written.
 *   M_ray         device float64, row-major 3 x 3, m_count == batch or 1: destination pixel -> normalised undistorted camera plane.  With
 *                 M_inv the inverse homography (destination px -> undistorted source px) and K = [fx 0 cx; 0 fy cy; 0 0 1], rows
 *                 (m0 - cx m2) / fx, (m1 - cy m2) / fy, m2 of M_inv.
 *   lens          HOST, 12 doubles: fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 (OpenCV's coefficient order).  One lens per call.
 *   r2_max        HOST double: a pixel whose r2 (below) exceeds it is OUTSIDE whatever its coordinates say; +inf = no limit.  A
 *                 polynomial lens model is not monotonic: beyond the radius where d/dr [r kr(r^2)] = 0 it folds back and paints ghost
 *                 copies of the frame into the destination.  Callers pass that radius squared.
 * Per destination pixel (x, y), with R = M_ray, bx the origin of its evaluation block and x1 = x - bx (blocks as in bevwarp_warp):
 *   X0 = (R0 bx + R1 y) + R2        Y0 = (R3 bx + R4 y) + R5        W0 = (R6 bx + R7 y) + R8
 *   Xn = X0 + R0 x1                 Yn = Y0 + R3 x1                 W  = W0 + R6 x1
 *   Wr = (W != 0) ? 1 / W : 0       xn = Xn Wr                      yn = Yn Wr
 *   x2 = xn xn     y2 = yn yn     r2 = x2 + y2     xy2 = 2 (xn yn)
 *   num = 1 + ((k3 r2 + k2) r2 + k1) r2       den = 1 + ((k6 r2 + k5) r2 + k4) r2       kr = num / den
 *   xd = (xn kr + p1 xy2) + p2 (r2 + 2 x2)    yd = (yn kr + p1 (r2 + 2 y2)) + p2 xy2
 *   u  = fx xd + cx                           v  = fy yd + cy
 *   nearest: X = rs(u), Y = rs(v)             bilinear: X = rs(32 u), Y = rs(32 v)      rs: clamp to int32, round half to even, NaN -> INT_MAX
 *   valid = (r2 <= r2_max)                    (false for a NaN r2)
 * From (X, Y) on the pixel is bevwarp_warp_border's: sx = sat16(X >> 5), fx = X & 31 (nearest: sx = sat16(X)), likewise y; the four taps,
 * the 8-bit fixed-point and the float32 blend, and "all four taps outside -> the border value itself" are unchanged.  A pixel that is not
 * valid is outside: BEVWARP_BORDER_CONSTANT stores the border value, BEVWARP_BORDER_TRANSPARENT neither reads nor writes it.  A pole of
 * the rational model (den == 0) needs no special case: +-inf and NaN land on INT_MAX / INT_MIN, outside every admissible source.
 *   dtype BEVWARP_U8 | BEVWARP_F32, channels 1..4, interp BEVWARP_NEAREST | BEVWARP_LINEAR, border_mode BEVWARP_BORDER_CONSTANT |
 *   BEVWARP_BORDER_TRANSPARENT; anything else (BEVWARP_CUBIC, the four index-remapping borders, the 16-bit types) is
 *   BEVWARP_ERR_UNSUPPORTED.  border_value: HOST, `channels` doubles or NULL = 0, read by BEVWARP_BORDER_CONSTANT only.
 * Status: bevwarp_warp's checks in bevwarp_warp's order (the border mode counts as part of the format); then, for a non-empty batch,
 * the lens: BEVWARP_ERR_BAD_ARG for a NULL lens, BEVWARP_ERR_NOT_FINITE for a lens entry that is NaN or +-inf, BEVWARP_ERR_BAD_ARG for
 * fx == 0, fy == 0, r2_max NaN or r2_max < 0; then BEVWARP_ERR_NOT_FINITE for border_value.  batch == 0 is BEVWARP_OK and launches nothing.
 */
/*
 * BEVWARP_LENS_FISHEYE: the equidistant (fisheye) lens model of cv2.fisheye, selected by ORing the flag into `interp` (bevwarp_warp_lens,
 * bevwarp_build_map) or into `direction` (bevwarp_project_points_lens), as OpenCV's own flags word carries WARP_INVERSE_MAP.  Without the
 * flag every entry is what it was, bit for bit and status for status; with it, the flag is taken out of the word before any check, so what
 * is left of the word is judged exactly as before.  The rational model divides the ray by its depth (xn = Xn / W) and cannot express a ray
 * at 90 degrees or more from the optical axis; this one never divides by W, and such a ray is a pixel like any other.
 *   lens          HOST, 12 doubles: fx, fy, cx, cy, k1, k2, k3, k4, 0, 0, 0, 0 -- k1..k4 are cv2.fisheye's D; no skew; the last four
 *                 entries are reserved and must be 0.
 *   r2_max        carries theta_max: the angle from the optical axis, in radians, beyond which a ray is OUTSIDE; +inf = no limit.  Callers
 *                 pass the angle where theta poly(theta^2) stops growing (its derivative's first root), at most pi.
 *   M_ray         as above, but the ray R (x, y, 1) is NOT divided, so the sign of M_ray matters for this model and for no other: -M_ray is
 *                 the camera looking backwards.  Callers orient it so that the pixels the camera sees have W > 0.  For an affine
 *                 BEV-to-world map -- every BEVWorldSpec -- W has one sign relation to the scene over the whole destination, and one sign
 *                 serves all of it.
 * Everything is float64, every line below one correctly rounded operation (IEEE + - * / and square root, no FMA), in the order written.
 * No library arctangent is called (two libraries do not agree on the last bit); atan_pos is part of the definition:
 *   A[i] = the double nearest to atan(i / 8), i = 0..8:  0x0.0p+0, 0x1.fd5ba9aac2f6ep-4, 0x1.f5b75f92c80ddp-3, 0x1.6f61941e4def1p-2,
 *          0x1.dac670561bb4fp-2, 0x1.1e00babdefeb4p-1, 0x1.4978fa3269ee1p-1, 0x1.700a7c5784634p-1, 0x1.921fb54442d18p-1
 *   PIO2_HI = 0x1.921fb54442d18p+0 (nearest to pi / 2)      PIO2_LO = 0x1.1a62633145c07p-54 (nearest to pi / 2 - PIO2_HI)
 *   PI_HI   = 0x1.921fb54442d18p+1                          PI_LO   = 0x1.1a62633145c07p-53
 *   c3 = 1.0 / 3.0, c5 = 1.0 / 5.0, ... c15 = 1.0 / 15.0    (each one division)
 *   atan_pos(t), t >= 0 (+inf and NaN admitted):
 *     big = t > 1          r = big ? 1 / t : t
 *     i = rint(8 r)        (half to even; 8 r is exact)       c = i / 8
 *     z = (r - c) / (1 + r c)          z2 = z z
 *     p = c15;  p = c13 - z2 p;  p = c11 - z2 p;  p = c9 - z2 p;  p = c7 - z2 p;  p = c5 - z2 p;  p = c3 - z2 p
 *     a = A[i] + (z - (z z2) p)        (i clamped to 0..8)
 *     atan_pos = big ? (PIO2_HI - a) + PIO2_LO : a
 *   atan_pos(0) = 0, atan_pos(+inf) = PIO2_HI, atan_pos(NaN) = NaN; elsewhere it is within 2 ulp of the arctangent (1.52 measured).
 * "The fisheye steps" on a ray (Xn, Yn, W):
 *   q = Xn Xn + Yn Yn     rho = sqrt(q)     t = rho / |W|     a = atan_pos(t)
 *   theta = (W < 0) ? (PI_HI - a) + PI_LO : a             (W == 0, rho > 0: t = +inf, theta = PIO2_HI;  0 / 0: NaN)
 *   th2 = theta theta     poly = 1 + (((k4 th2 + k3) th2 + k2) th2 + k1) th2     thd = theta poly
 *   g = (rho != 0) ? thd / rho : 0
 *   xd = Xn g     yd = Yn g     u = fx xd + cx     v = fy yd + cy
 *   valid = (theta <= theta_max)                          (false for a NaN theta)
 * bevwarp_warp_lens | BEVWARP_LENS_FISHEYE: (Xn, Yn, W) come from the same evaluation-block row walk (the first two lines of the chain
 * above, R = M_ray); the fisheye steps stand where the lines `Wr = ...` to `valid = ...` stood; from (u, v) on -- the rs rounding, NaN ->
 * INT_MAX, sat16, the taps, the blends, "a pixel that is not valid is outside" -- nothing changes.  Formats, borders and the order of the
 * status checks are unchanged; at the place of the lens: BEVWARP_ERR_BAD_ARG for a NULL lens, BEVWARP_ERR_NOT_FINITE for an entry that is
 * NaN or +-inf, BEVWARP_ERR_BAD_ARG for fx == 0, fy == 0, a reserved entry != 0, theta_max NaN or < 0.
 */
#define BEVWARP_LENS_FISHEYE 0x100
int bevwarp_warp_lens(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                      int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                      const double *M_ray, int m_count, const double *lens /*HOST, 12*/, double r2_max, int dtype, int interp,
                      int border_mode, const double *border_value /*HOST*/, void *stream);

/*
 * Fixed-camera warp maps: the coordinates once (bevwarp_build_map), the pixels per batch (bevwarp_remap).
 *
 * THE MAP FORMAT is OpenCV's fixed-point pair, 6 bytes per destination pixel.  For a destination of dst_h x dst_w pixels:
 *   map_xy     int16 pairs (sx, sy) per pixel, sx first: 4 bytes per pixel, rows xy_row_stride BYTES apart, base and strides multiples
 *              of 4 (CV_16SC2).
 *   map_frac   uint16 per pixel, (fy << 5) | fx with fx, fy in 0..31: rows frac_row_stride BYTES apart, base and strides multiples of 2
 *              (CV_16UC1).  A reader uses fx = v & 31, fy = (v >> 5) & 31 and ignores the higher bits, as OpenCV masks them.  Unused for
 *              BEVWARP_NEAREST, where it may be NULL.
 * A map is built for ONE interpolation, and sx differs by it: with (X, Y) the integer coordinates of the chain (bevwarp_warp_border,
 * bevwarp_warp_lens: pixels for nearest, 1/32 px for bilinear),
 *   BEVWARP_NEAREST   sx = sat16(X), sy = sat16(Y)
 *   BEVWARP_LINEAR    sx = sat16(X >> 5), sy = sat16(Y >> 5); fx = X & 31, fy = Y & 31 of the UNSATURATED X, Y
 * which is exactly what the warp kernels derive from (X, Y).  Several maps (frames of a map) lie *_frame_stride bytes apart.
 * A base and strides that are all multiples of 16 (map_xy) and of 8 (map_frac) enable a lane's wide accesses; nothing else depends on it.
 *
 * INVALID PIXELS.  A pixel the lens chain declares invalid (r2 > r2_max, or r2 NaN) is stored as (sx, sy) = (-32768, -32768), frac 0.
 * Its taps are at columns -32768 and -32767 and rows -32768 and -32767: all negative, so every tap is outside every admissible source
 * (sides 1..32767).  Therefore BEVWARP_BORDER_CONSTANT yields the border value itself -- nearest: the one tap is outside; bilinear: all four
 * taps are outside, which is the border value itself for 8-bit and float32 pixels alike -- and BEVWARP_BORDER_TRANSPARENT does not write the
 * pixel (sx is no inlier).  Both are what bevwarp_warp_lens does with an invalid pixel.  (A VALID pixel whose coordinates saturate to the same
 * entry has the same four taps outside: the two cannot be told apart, and need not be.)  Under the four index-remapping borders such an
 * entry is whatever source pixel borderInterpolate maps index -32768 / -32767 to: lens maps are meant for CONSTANT and TRANSPARENT.
 *
 * bevwarp_build_map writes m_count maps.
 *   M             device float64, m_count row-major 3 x 3 matrices.  lens == NULL: M is M_inv (destination px -> source px) and the
 *                 coordinates are bevwarp_warp_border's chain -- evaluation blocks, Xn (32 / W), round half to even, NaN -> INT_MAX.
 *                 lens != NULL: M is M_ray and the coordinates are bevwarp_warp_lens's chain, operation for operation.
 *   lens, r2_max  HOST, exactly bevwarp_warp_lens's; lens NULL: the pinhole chain (r2_max is not looked at).
 *   interp        BEVWARP_NEAREST | BEVWARP_LINEAR (anything else: BEVWARP_ERR_UNSUPPORTED), optionally | BEVWARP_LENS_FISHEYE: M is M_ray,
 *                 lens and r2_max (theta_max) are bevwarp_warp_lens's under that flag, and the coordinates are its chain with the fisheye
 *                 steps, operation for operation.  The map format is unchanged -- an invalid pixel (theta > theta_max, or NaN) is the
 *                 (-32768, -32768), frac 0 entry -- so bevwarp_remap, its NV12 and plane kin and every stitch through maps serve a fisheye
 *                 camera as they stand.  A fisheye map has no pinhole chain behind it: lens NULL is BEVWARP_ERR_BAD_ARG.
 *   map_xy, map_frac   device, WRITTEN; map_frac may be NULL for BEVWARP_NEAREST (it is not written then).
 * Status, in this order: BEVWARP_ERR_BAD_ARG (M or map_xy NULL, m_count < 1, a non-positive side); BEVWARP_ERR_UNSUPPORTED (interp);
 * BEVWARP_ERR_BAD_ARG (map_frac NULL under BEVWARP_LINEAR; a plane whose base or stride is misaligned, whose row stride is below a row,
 * or whose maps overlap their successors); BEVWARP_ERR_TOO_LARGE (a side > 2^20, or more than 2^31 - 1 tiles); BEVWARP_ERR_OVERLAP (the
 * two planes share bytes); the lens as in bevwarp_warp_lens (under BEVWARP_LENS_FISHEYE: as there under the flag, a NULL lens included).
 * With m_count == 1 the frame strides are not looked at.
 *
 * bevwarp_remap samples `batch` frames through map_count maps: dst[b] = remap(src[b], map[map_count == 1 ? 0 : b]).
 *   src, dst, batch, sizes, channels, the four strides, dtype, border_value   as bevwarp_warp_border, with the same checks.
 *   map_xy, map_frac   device, READ; map_count == 1 (shared by all frames; frame strides not looked at) or == batch.  dst must not overlap
 *                 either plane (bounding byte ranges).  map_frac NULL under BEVWARP_LINEAR is BEVWARP_ERR_BAD_ARG.
 *   interp        BEVWARP_NEAREST | BEVWARP_LINEAR: the interpolation the map was built for.  (BEVWARP_LINEAR | BEVWARP_MAP_BICUBIC: below.)
 *   border_mode   all six.  From (sx, sy, fx, fy) on the pixel is defined to the bit by the existing entries: BEVWARP_BORDER_CONSTANT is
 *                 bevwarp_warp_lens's sampler -- each tap outside the source is replaced by the border pixel, all four taps outside -> the
 *                 border value itself --, the other five modes are bevwarp_warp_border's.  With a map from bevwarp_build_map the result
 *                 equals bevwarp_warp / bevwarp_warp_border (pinhole map) and bevwarp_warp_lens (lens map; CONSTANT, TRANSPARENT) by bits.
 * Status: bevwarp_warp's checks in bevwarp_warp's order, the map count standing for the matrix count, the two planes being read images
 * (NULL, alignment, strides: BEVWARP_ERR_BAD_ARG) without the source size limits, BEVWARP_CUBIC and the 16-bit types
 * BEVWARP_ERR_UNSUPPORTED; BEVWARP_ERR_OVERLAP; BEVWARP_ERR_TOO_LARGE for a destination side > 2^20; BEVWARP_ERR_NOT_FINITE for border_value
 * (BEVWARP_BORDER_CONSTANT only).  batch == 0 is BEVWARP_OK and launches nothing.
 * Restated from memory of OpenCV's remap / convertMaps (imgwarp.cpp); parity with OpenCV is unpinned, like the rest of the warp.
 *
 * BEVWARP_MAP_BICUBIC: bicubic sampling (cv2.INTER_CUBIC) through a BILINEAR map, selected by ORing the flag into `interp` of bevwarp_remap --
 * and of no other entry.  OpenCV's bicubic is defined on the bilinear map (bevwarp_warp_border, interp == BEVWARP_CUBIC, "maps"), so no map
 * is built for it: a BEVWARP_LINEAR map entry holds everything the bicubic sampler needs, and bevwarp_build_map, the map format and every
 * existing map stay as they are.  Without the flag every call is what it was, bit for bit and status for status.  With it, the flag is
 * taken out of the word before any check, and what is left must be BEVWARP_LINEAR: BEVWARP_NEAREST | flag, BEVWARP_CUBIC | flag and any
 * other remainder are BEVWARP_ERR_UNSUPPORTED, judged where `interp` is judged without the flag.  Every other check is that of a
 * BEVWARP_LINEAR call, in the same order: a NULL map_frac is BEVWARP_ERR_BAD_ARG, border_value is BEVWARP_ERR_NOT_FINITE under
 * BEVWARP_BORDER_CONSTANT only, batch == 0 is BEVWARP_OK and launches nothing.
 * Per destination pixel, with the entry (sx, sy) as stored (int16) and its frac word v:
 *   fx = v & 31, fy = (v >> 5) & 31; higher bits are ignored.
 *   The 4 x 4 tap window starts at wx = sx - 1, wy = sy - 1, computed in int32 (-32769 is a window position like any other).  This is the
 *   sat16(X >> 5) - 1 of bevwarp_warp_border's BEVWARP_CUBIC, because the map stores the saturated value.
 * From (wx, wy, fy, fx) on the pixel is bevwarp_warp_border's BEVWARP_CUBIC text above, with (wx, wy) for its (sx, sy), unchanged: the weights;
 * the inlier test; BEVWARP_BORDER_TRANSPARENT's rule (the pixel is written iff it is an inlier or the entry's own (sx, sy) lies in the source);
 * BEVWARP_BORDER_CONSTANT's shortcut for a window that is wholly outside; the general path tap by tap through borderInterpolate; the two
 * summation orders; the 8-bit clamp((sum + 16384) >> 15, 0, 255); float32 with every multiply and add rounded, no FMA.  Window indices lie
 * in [-32769, 32769].
 *   - With a pinhole map from bevwarp_build_map(..., BEVWARP_LINEAR) the result equals bevwarp_warp_border(..., BEVWARP_CUBIC, border_mode) by
 *     bits, in all six modes (BEVWARP_BORDER_CONSTANT: bevwarp_warp(..., BEVWARP_CUBIC)).
 *   - An invalid entry (-32768, -32768), frac 0 has its whole window at negative indices: BEVWARP_BORDER_CONSTANT stores the border value
 *     itself, BEVWARP_BORDER_TRANSPARENT does not write the pixel.
 *   - With a rational-lens or fisheye map this is bicubic resampling of a raw distorted frame in one pass; no other entry offers that.
 *   dtype BEVWARP_U8 | BEVWARP_F32, channels 1..4, all six border modes; shared or per-frame maps (map_count 1 or batch), as without the flag.
 * No other entry takes the flag: bevwarp_build_map, bevwarp_warp_lens, bevwarp_remap_nv12, bevwarp_remap_nv12_planes, bevwarp_remap_to_nv12,
 * bevwarp_remap_nv12_to_nv12, bevwarp_remap_planes and every stitch judge the whole word, and BEVWARP_LINEAR | BEVWARP_MAP_BICUBIC is
 * BEVWARP_ERR_UNSUPPORTED there.
 */
#define BEVWARP_MAP_BICUBIC 0x200
int bevwarp_build_map(const double *M, int m_count, const double *lens /*HOST, 12, or NULL*/, double r2_max, int interp,
                      void *map_xy, void *map_frac, int dst_h, int dst_w, int64_t xy_frame_stride, int64_t xy_row_stride,
                      int64_t frac_frame_stride, int64_t frac_row_stride, void *stream);
int bevwarp_remap(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                  int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                  const void *map_xy, const void *map_frac, int map_count, int64_t xy_frame_stride, int64_t xy_row_stride,
                  int64_t frac_frame_stride, int64_t frac_row_stride, int dtype, int interp, int border_mode,
                  const double *border_value /*HOST*/, void *stream);

/*
 * Several cameras warped into one canvas in one launch.  It replaces "warping several cameras into one canvas, one call each"
 * (bevwarp_warp_border, BEVWARP_BORDER_TRANSPARENT): the cameras of one site -- preset_calib("KoPER", 1 | 4),
 * bev/constructor/homo_constr.py:19-25 -- each with frames, sizes, strides and matrices of its own, and two rules for the pixels that
 * more than one camera sees.  Both are defined to the bit.
 *   cams          HOST, n_cams (1..BEVWARP_STITCH_MAX_CAMERAS) descriptions in list order; the array is read during the call only.
 *                 src: device, `batch` frames of src_h x src_w pixels (`channels` values of `dtype`: the call's); M_inv: device, m_count
 *                 (batch or 1) inverse matrices, canvas px -> THIS camera's px; strides in bytes; reserved: 0.
 *   dst           device, `batch` canvases of dst_h x dst_w pixels.  No camera's frames may overlap it (bevwarp_warp's rule, per camera);
 *                 the cameras' frames may overlap each other.
 * Per camera.  For frame b, destination pixel (x, y) and camera k, (X, Y), sx, sy, fx, fy are exactly bevwarp_warp_border's with camera
 * k's matrix of frame b: the evaluation blocks, 32 / W, round half to even, NaN -> INT_MAX, int16 saturation.  Camera k COVERS the
 * pixel iff it passes BEVWARP_BORDER_TRANSPARENT's inlier test for `interp` against camera k's own src_w, src_h; its value p_k is then
 * that entry's nearest copy or bilinear blend (8-bit: 15-bit fixed point; float32: the float blend).
 *   BEVWARP_STITCH_OVER     the pixel is p_k of the covering camera with the LARGEST k: bit for bit what n_cams successive
 *                           bevwarp_warp_border(..., BEVWARP_BORDER_TRANSPARENT) calls in list order leave on a canvas.  `feather` is ignored.
 *   BEVWARP_STITCH_FEATHER  `feather` F in 1..4096.  Covering camera k weighs w_k = min(d_k, F), an integer, with
 *                           d_k = min(sx + 1, src_w - sx, sy + 1, src_h - sy): the distance in whole source pixels to the nearest edge
 *                           of its frame (>= 1 for every inlier); W = sum of w_k.
 *                           - exactly one camera covers: the pixel is that p_k itself (outside overlaps FEATHER, OVER and the plain
 *                             TRANSPARENT warp agree by bits);
 *                           - 8-bit, two or more: (sum of w_k p_k + (W >> 1)) / W per channel, integers, truncating division (the sums
 *                             stay below 2^23; the result is at most 255: no clamp is live);
 *                           - float32, two or more: acc = 0, then in ascending k acc = acc + float(w_k) * p_k, every multiply and add
 *                             rounded to float32 (no FMA), then acc / float(W) as one correctly rounded float32 division.  A NaN gives
 *                             some NaN.
 *                           F = 1 is the plain mean of the covering cameras.
 * No camera covers: BEVWARP_BORDER_CONSTANT stores border_value, converted as bevwarp_warp converts it (HOST, `channels` doubles, NULL = 0);
 * BEVWARP_BORDER_TRANSPARENT neither reads nor writes the pixel.  One camera with BEVWARP_BORDER_CONSTANT is NOT bevwarp_warp: a pixel is
 * covered or it is the border value -- taps at the frame's edge are not blended with the border here.
 *   dtype BEVWARP_U8 | BEVWARP_F32, channels 1..4, interp BEVWARP_NEAREST | BEVWARP_LINEAR, blend one of the two, border_mode
 *   BEVWARP_BORDER_CONSTANT | BEVWARP_BORDER_TRANSPARENT; anything else (BEVWARP_CUBIC, the four index-remapping borders, the 16-bit types)
 *   is BEVWARP_ERR_UNSUPPORTED.
 * Status, in this order: BEVWARP_ERR_BAD_ARG for cams NULL, n_cams outside 1..8, or feather outside 1..4096 under BEVWARP_STITCH_FEATHER;
 * then per camera in ascending k bevwarp_warp's checks in bevwarp_warp's order of that camera's frames against dst (blend and border_mode
 * count as part of the format), the first status that is not BEVWARP_OK being returned; then BEVWARP_ERR_TOO_LARGE for a destination side
 * > 2^20; then BEVWARP_ERR_NOT_FINITE for border_value (BEVWARP_BORDER_CONSTANT only).  batch == 0 is BEVWARP_OK and launches nothing.
 */
#define BEVWARP_STITCH_MAX_CAMERAS 8
typedef struct bevwarp_camera {   /* HOST; 48 bytes */
    const void *src;              /* device: `batch` frames of src_h x src_w pixels (channels, dtype: the call's) */
    const double *M_inv;          /* device: m_count inverse matrices, canvas px -> THIS camera's px */
    int64_t frame_stride, row_stride;   /* bytes */
    int src_h, src_w;
    int m_count;                  /* batch or 1 */
    int reserved;                 /* 0 */
} bevwarp_camera;
#define BEVWARP_STITCH_OVER 0
#define BEVWARP_STITCH_FEATHER 1
int bevwarp_warp_stitch(const bevwarp_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w, int channels,
                        int64_t dst_frame_stride, int64_t dst_row_stride, int dtype, int interp, int blend, int feather,
                        int border_mode, const double *border_value /*HOST*/, void *stream);

/*
 * Several FIXED cameras sampled through their warp maps into one canvas in one launch: bevwarp_warp_stitch's cover test and blend rules
 * over bevwarp_remap's (bevwarp_remap_nv12's) map entries.  Each camera brings frames, sizes, strides and maps (THE MAP FORMAT above,
 * from bevwarp_build_map: pinhole or lens) of its own; no coordinate is computed and no float64 is touched.  It replaces a canvas fill
 * plus one bevwarp_remap(..., BEVWARP_BORDER_TRANSPARENT) per camera -- one pass over the canvas per camera, and no blend -- and gives
 * a site whose cameras are distorted the one-launch route that bevwarp_warp_stitch (pinhole only) cannot.  Defined to the bit.
 * For frame b, canvas pixel (x, y) and camera k:
 *   entry    (sx, sy, fx, fy) is the entry of camera k's map for frame (map_count == 1 ? 0 : b), read as bevwarp_remap reads it
 *            (fx = v & 31, fy = (v >> 5) & 31, higher bits ignored).
 *   cover    camera k COVERS the pixel iff the entry passes BEVWARP_BORDER_TRANSPARENT's inlier test for `interp` against camera k's own
 *            src_w, src_h (nearest: 0 <= sx < src_w, 0 <= sy < src_h; bilinear: 0 <= sx < src_w - 1, 0 <= sy < src_h - 1).  The
 *            invalid-pixel entry (-32768, -32768) never covers: a lens map's pixels beyond r2_max are not that camera's.
 *   value    p_k is what bevwarp_remap(..., BEVWARP_BORDER_TRANSPARENT) writes for that entry: the nearest copy, or the bilinear blend
 *            (8-bit: 15-bit fixed point; float32: the float blend).  bevwarp_stitch_maps_nv12: what bevwarp_remap_nv12(..., rgb_order,
 *            BEVWARP_BORDER_TRANSPARENT) writes -- every tap converted before the blend, 3 channels of 8 bits.
 *   blend    BEVWARP_STITCH_OVER and BEVWARP_STITCH_FEATHER are word for word bevwarp_warp_stitch's rules, with
 *            d_k = min(sx + 1, src_w - sx, sy + 1, src_h - sy) of the map entry and w_k = min(d_k, F): the single-cover rule, the integer
 *            mean for 8-bit pixels, the float32 sum in ascending k with one correctly rounded division.  Pixels no camera covers are
 *            border_value under BEVWARP_BORDER_CONSTANT (NV12: in the destination's channel order, not converted) and are neither read
 *            nor written under BEVWARP_BORDER_TRANSPARENT.
 * Hence (i) with pinhole maps from bevwarp_build_map the result is bevwarp_warp_stitch's for the same matrices, by bits; (ii) OVER is
 * what n_cams successive bevwarp_remap (bevwarp_remap_nv12) calls with BEVWARP_BORDER_TRANSPARENT leave on the canvas; (iii) the NV12
 * entry equals bevwarp_stitch_maps on the converted frames.
 *   cams     HOST, n_cams (1..BEVWARP_STITCH_MAX_CAMERAS) descriptions in list order; the array is read during the call only.  All
 *            pointers in it are device pointers; strides in bytes.  Two cameras may share one map, and what the cameras read may overlap.
 *   dst      device, `batch` canvases of dst_h x dst_w pixels; it must not overlap any image the call reads (frames, uv, xy or frac of
 *            any camera).
 *   bevwarp_stitch_maps       dtype BEVWARP_U8 | BEVWARP_F32, channels 1..4, interp BEVWARP_NEAREST | BEVWARP_LINEAR (the interpolation
 *                             every map was built for), blend one of the two, border_mode BEVWARP_BORDER_CONSTANT |
 *                             BEVWARP_BORDER_TRANSPARENT.
 *   bevwarp_stitch_maps_nv12  the same without dtype and channels (8 bits, 3 channels); even source sides; rgb_order 0 (B, G, R) | 1.
 *   Everything else is BEVWARP_ERR_UNSUPPORTED.
 * Status, in this order: BEVWARP_ERR_BAD_ARG for cams NULL, n_cams outside 1..8, or feather outside 1..4096 under BEVWARP_STITCH_FEATHER;
 * then per camera in ascending k bevwarp_remap's (bevwarp_remap_nv12's) checks in that entry's own order against dst (blend and
 * border_mode count as part of the format), the first status that is not BEVWARP_OK being returned; then BEVWARP_ERR_TOO_LARGE for a
 * destination side > 2^20; then BEVWARP_ERR_NOT_FINITE for border_value (BEVWARP_BORDER_CONSTANT only).  batch == 0 is BEVWARP_OK and
 * launches nothing.
 */
typedef struct bevwarp_map_camera {      /* HOST; 112 bytes */
    const void *src;                     /* interleaved frames; for the NV12 entry the Y plane */
    const void *uv;                      /* NV12 entry: the plane of (U, V) pairs; otherwise NULL, not looked at */
    int64_t frame_stride, row_stride;    /* of src / Y, bytes */
    int64_t uv_frame_stride, uv_row_stride;
    const void *map_xy, *map_frac;       /* THE MAP FORMAT; map_frac may be NULL for BEVWARP_NEAREST */
    int64_t xy_frame_stride, xy_row_stride, frac_frame_stride, frac_row_stride;
    int src_h, src_w;
    int map_count;                       /* 1 (shared by the batch) or batch */
    int reserved;                        /* 0; under BEVWARP_STITCH_GAIN (below) the camera's gain word, otherwise not looked at */
} bevwarp_map_camera;
int bevwarp_stitch_maps(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w, int channels,
                        int64_t dst_frame_stride, int64_t dst_row_stride, int dtype, int interp, int blend, int feather,
                        int border_mode, const double *border_value /*HOST*/, void *stream);
int bevwarp_stitch_maps_nv12(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w,
                             int64_t dst_frame_stride, int64_t dst_row_stride, int interp, int blend, int feather, int rgb_order,
                             int border_mode, const double *border_value /*HOST*/, void *stream);

/*
 * BEVWARP_STITCH_GAIN: per-camera exposure gains in the stitches through maps, selected by ORing the flag into `blend` of
 * bevwarp_stitch_maps, bevwarp_stitch_maps_nv12, bevwarp_stitch_maps_to_nv12, bevwarp_stitch_maps_nv12_to_nv12, bevwarp_stitch_maps_planes
 * and bevwarp_stitch_maps_nv12_planes (BEVWARP_LENS_FISHEYE's way: the flag is taken out of the word before any check, and what is left of
 * the word is judged exactly as without it).  Cameras of one site run their own auto-exposure; the gain is applied to every tap while it
 * is in registers, instead of one multiply-and-clamp pass over every camera's frames before each stitch.  Defined to the bit.
 *   the gain word   under the flag `reserved` of camera k is G0 | G1 << 10 | G2 << 20: each Gc in 0..1023 is a Q8 fixed-point gain
 *                   (256 is 1.0, the largest gain is 1023 / 256); bits 30 and 31 must be 0.  Read during the call only, by value.
 *   the gain step   every tap p of camera k -- after the NV12 conversion where the frames are NV12, before the interpolation -- is
 *                   replaced channel by channel by
 *                       gain(p, Gc) = min(255, (p * Gc + 128) >> 8)
 *                   where channel c is channel c of the pixel the sampler blends: the frames' own order, or for NV12 frames the order
 *                   rgb_order names (bevwarp_stitch_maps_nv12_to_nv12: B, G, R).  Gc = 256 is the identity, Gc = 0 gives 0.
 *   everything else is unchanged: the bilinear fixed-point blend, the cover test (a property of the map entry: it does not see the gain),
 *                   OVER, FEATHER, the single-cover rule, the border pixel (which is NOT gained), the NV12 and the plane store stages.
 * Hence the entry under the flag equals, by bits, the same entry without it on frames that were put through `gain` beforehand (NV12
 * frames: on the converted frames, through bevwarp_stitch_maps and its BGR kin).
 * Formats under the flag: 8 bits, 3 channels -- bevwarp_stitch_maps with another dtype or channel count is BEVWARP_ERR_UNSUPPORTED, where
 * the format is judged; both border modes where the entry has them.  bevwarp_warp_stitch does not know the flag (BEVWARP_ERR_UNSUPPORTED).
 * Status under the flag: the cams / n_cams / feather checks as without it; then BEVWARP_ERR_BAD_ARG for the first camera, in ascending k,
 * whose gain word has bit 30 or 31 set; then everything else as without it.  Without the flag `reserved` is not looked at.
 */
#define BEVWARP_STITCH_GAIN 0x100

/*
 * bevwarp_warp with the per-tile verdicts of an earlier launch (ABI v7).  Which way a tile is processed -- inside the frame, outside,
 * cut by its edge; turned, rectification-form, pair loads -- follows from the matrices, the sizes and the format alone, and deriving it
 * is a tenth of the 8-bit kernel's instructions.  A caller that warps many batches through the SAME matrices and geometry (a camera
 * loop: cv2.warpPerspective per frame with one H_bev_img, vis_homo.py:85-91) fills a table once and hands it to every later call:
 *
 *   classes   device, bevwarp_tile_classes_bytes(...) bytes, 4-byte aligned.
 *   mode      BEVWARP_CLASSES_FILL: write the verdicts, no pixel (src / dst are not accessed, but take the arguments of the warps
 *                                   the table is meant for: the table is only valid for that batch, those sizes, strides' alignment,
 *                                   format, interpolation and -- above all -- those M_inv CONTENTS);
 *             BEVWARP_CLASSES_USE : warp, reading the verdicts.  Entries that were never filled are classified as usual.
 * A table that does not belong to the matrices it is used with makes the kernel trust a wrong verdict (a tile taken for interior is
 * sampled without guards): like a wrong pointer, that is the caller's to get right.  bevwarp_warp never needs a table.
 */
#define BEVWARP_CLASSES_USE 0
#define BEVWARP_CLASSES_FILL 1
int64_t bevwarp_tile_classes_bytes(int batch, int src_h, int src_w, int dst_h, int dst_w, int channels, int dtype, int interp);
int bevwarp_warp_classes(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                         int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride,
                         const double *M_inv, int m_count, int dtype, int interp, const double *border_value /*HOST*/,
                         void *classes, int mode, void *stream);

/*
 * float32 PLANAR destination, one pass:
 *   dst[b][c][y][x] = (float)warp(src[b])[y][x][c] * scale[c] + bias[c]      (float32 multiply, then add)
 * where warp is exactly what bevwarp_warp computes for `dtype` (BEVWARP_U8 | BEVWARP_F32: same interpolation, rounding
 * and border).
 *   dst             device float32; dst_plane_stride bytes between channel planes, dst_row_stride between rows,
 *                   dst_frame_stride between frames (all multiples of 4; multiples of 16 enable the wide stores).
 *   scale, bias     HOST, `channels` doubles each (converted to float32); NULL = 1 and 0.
 * Overlap of src and dst: BEVWARP_ERR_OVERLAP when the bounding byte ranges intersect.
 */
int bevwarp_warp_planar(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                        int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                        int64_t dst_row_stride, const double *M_inv, int m_count, int dtype, int interp,
                        const double *border_value /*HOST*/, const double *scale /*HOST*/, const double *bias /*HOST*/,
                        void *stream);

/*
 * bevwarp_warp_planar with the planes' element type P = plane_dtype (BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16), one pass:
 *   v               = float32(warp(src[b])[y][x][c]) * float32(scale[c]) + float32(bias[c])
 *   dst[b][c][y][x] = convert_P(v)
 * v is exactly the value bevwarp_warp_planar stores: a float32 multiply, then a float32 add, each rounded, no FMA.  The result is what
 * `bevwarp_warp_planar(...)` followed by a float32 -> P conversion pass gives, double rounding included, without that pass:
 *   convert_F32   the identity: the call IS bevwarp_warp_planar.
 *   convert_F16   IEEE binary32 -> binary16, round to nearest, ties to even.  Overflow gives +-inf (65520 is the first value that rounds
 *                 to inf); subnormal results are kept (2^-24 is representable, the tie 2^-25 goes to 0); -0 stays -0.
 *   convert_BF16  rounds to the upper 16 bits, nearest, ties to even; the carry may reach inf; float32 subnormals give bfloat16
 *                 subnormals (not flushed).
 *   A NaN gives some NaN; its payload and sign are unspecified.
 *   dst             device; the three destination strides are in BYTES and multiples of the element size (2 for the 16-bit types); base
 *                   and strides that are all multiples of 8 enable the wide stores of the 16-bit planes (16 for float32).
 *   plane_dtype     any other value: BEVWARP_ERR_UNSUPPORTED.  interp: BEVWARP_CUBIC is BEVWARP_ERR_UNSUPPORTED, as for bevwarp_warp_planar.
 * Every other argument, the overlap rule and BEVWARP_ERR_NOT_FINITE for scale and bias are bevwarp_warp_planar's.
 */
int bevwarp_warp_planes(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                        int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                        int64_t dst_row_stride, const double *M_inv, int m_count, int dtype, int interp,
                        const double *border_value /*HOST*/, const double *scale /*HOST*/, const double *bias /*HOST*/,
                        int plane_dtype, void *stream);

/*
 * dst = bevwarp_warp(cvtColor(nv12, COLOR_YUV2BGR_NV12), ...) for 8-bit pixels, 3 channels, constant border, bit for bit, in one pass:
 * every tap is converted before the blend and the converted frame is never in memory.  The source is a video decoder's NV12 frame:
 *   y               device, src_h rows of src_w bytes (y_row_stride >= src_w, y_frame_stride between frames)
 *   uv              device, src_h / 2 rows of src_w / 2 interleaved (U, V) byte pairs -- src_w bytes per row.  Base, uv_row_stride and
 *                   uv_frame_stride are even (pairs are read as 16-bit words).  src_h and src_w are even.
 *                   Pixel (x, y) has Y = y[y][x], U = uv[y >> 1][2 (x >> 1)], V = uv[y >> 1][2 (x >> 1) + 1].
 *                   Both layouts found in practice fit: one (src_h * 3 / 2) x src_w buffer with uv = y + src_h * y_row_stride, and two
 *                   allocations.  y and uv may overlap each other (both are only read).
 *   conversion      OpenCV's 8-bit cvtYUV420sp2RGB: BT.601, limited range, 20-bit fixed point, all in int32, >> arithmetic
 *                   (restated from memory like the rest of the warp: parity with OpenCV is unpinned):
 *                       yy = max(0, Y - 16) * 1220542        u = U - 128        v = V - 128
 *                       R = clamp((yy + 524288 + 1673527 v) >> 20, 0, 255)
 *                       G = clamp((yy + 524288 -  852492 v - 409993 u) >> 20, 0, 255)
 *                       B = clamp((yy + 524288 + 2116026 u) >> 20, 0, 255)
 *   rgb_order       0: dst pixels are B, G, R (COLOR_YUV2BGR_NV12); 1: R, G, B (COLOR_YUV2RGB_NV12).
 *   interp          BEVWARP_NEAREST | BEVWARP_LINEAR.  Maps, 1/32-px quantisation, tap guards and blend are bevwarp_warp's: a tap inside the
 *                   frame is the converted pixel, a tap outside is border_value.
 *   border_value    HOST, 3 doubles in the DESTINATION's channel order (not converted), or NULL = 0.
 *   dst             device, dst_h x dst_w x 3 bytes; the wide-store rule is bevwarp_warp's.  M_inv, m_count, stream: as bevwarp_warp.
 * Status, in this order: BEVWARP_ERR_BAD_ARG (null pointer, non-positive size, odd src_w or src_h, a row stride below src_w for either
 * plane or below 3 dst_w, frames that overlap their successors, an odd uv base / row stride / frame stride, m_count not 1 or batch);
 * BEVWARP_ERR_UNSUPPORTED (BEVWARP_CUBIC or any other interp; rgb_order outside {0, 1}); BEVWARP_ERR_TOO_LARGE (either plane: a side
 * > 32767, a row stride >= 16 MiB, a plane >= 2 GiB); BEVWARP_ERR_OVERLAP (dst shares bytes with the y or the uv image, by
 * bevwarp_warp's rule); BEVWARP_ERR_TOO_LARGE again for a destination side > 2^20 (the launch plan's limit, looked at after the
 * overlap); BEVWARP_ERR_NOT_FINITE (border_value).  batch == 0 is BEVWARP_OK and launches nothing.
 */
int bevwarp_warp_nv12(const void *y, const void *uv, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w,
                      int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride,
                      int64_t dst_frame_stride, int64_t dst_row_stride, const double *M_inv, int m_count, int interp,
                      int rgb_order, const double *border_value /*HOST, 3 doubles or NULL*/, void *stream);

/*
 * bevwarp_warp_nv12 and the plane stage of bevwarp_warp_planes in one pass: stands in for `ok, img = video.read()` +
 * cv2.warpPerspective(img, H_bev_img, (u_size, v_size)), vis_homo.py:86-89, plus the detector-input step of bevwarp_warp_planes (layout and
 * precision between vis_homo.py:89 and a detector).  For P = plane_dtype (BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16) and channel c = 0, 1, 2 in
 * the DESTINATION's order (rgb_order 0: B, G, R; 1: R, G, B):
 *   p               = bevwarp_warp_nv12(y, uv, ..., interp, rgb_order, border_value)[b][y][x][c]        (an 8-bit value)
 *   v               = float32(p) * float32(scale[c]) + float32(bias[c])                              (multiply, then add, each rounded; no FMA)
 *   dst[b][c][y][x] = convert_P(v)
 * bit for bit what the two entry points give in sequence, double rounding included; neither the converted frame nor the 8-bit BEV frame
 * is in memory.  convert_P is exactly bevwarp_warp_planes's (F32: the identity; F16 / BF16: round to nearest, ties to even, overflow to
 * +-inf, subnormals kept, -0 kept).  A tap outside the frame is the 8-bit border value, as in bevwarp_warp_nv12: a pixel whose taps are
 * all outside is convert_P(float32(border[c]) * scale[c] + bias[c]).
 *   y, uv, src_h, src_w, the four source strides, M_inv, m_count, interp, rgb_order, the conversion and the (x >> 1, y >> 1) chroma
 *                   addressing: bevwarp_warp_nv12's, unchanged (nearest or bilinear, constant border, even source sides).
 *   dst             device, three planes per frame of dst_h rows of dst_w elements of P; dst_frame_stride, dst_plane_stride and
 *                   dst_row_stride in BYTES, multiples of the element size.  A base and strides that are all multiples of 4 elements
 *                   (16 bytes float32, 8 bytes 16-bit) enable the wide stores.
 *   border_value, scale, bias   HOST, 3 doubles each in the DESTINATION's channel order, or NULL = 0, 1 and 0.
 * Status, in this order: BEVWARP_ERR_BAD_ARG (everything bevwarp_warp_nv12 lists for y / uv / m_count; a destination base or stride that is
 * no multiple of the element size -- for a plane_dtype outside the three no alignment is asked --, a row stride below dst_w elements,
 * planes or frames that overlap their successors); BEVWARP_ERR_UNSUPPORTED (interp other than nearest / linear, rgb_order outside {0, 1},
 * plane_dtype outside {F32, F16, BF16}); BEVWARP_ERR_TOO_LARGE (either source plane, as bevwarp_warp_nv12); BEVWARP_ERR_OVERLAP (the bounding
 * byte range of all destination planes meets the y or the uv image's); BEVWARP_ERR_TOO_LARGE again for a destination side > 2^20;
 * BEVWARP_ERR_NOT_FINITE (border_value, scale, bias).  batch == 0 is BEVWARP_OK and launches nothing.
 */
int bevwarp_warp_nv12_planes(const void *y, const void *uv, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w,
                             int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride,
                             int64_t dst_frame_stride, int64_t dst_plane_stride, int64_t dst_row_stride,
                             const double *M_inv, int m_count, int interp, int rgb_order,
                             const double *border_value /*HOST, 3 or NULL*/, const double *scale /*HOST, 3 or NULL = 1*/,
                             const double *bias /*HOST, 3 or NULL = 0*/, int plane_dtype, void *stream);

/*
 * A video decoder's NV12 frames sampled through a fixed camera's warp maps: bevwarp_remap's pixels from bevwarp_warp_nv12's sources, in
 * one pass.  The map carries the lens (bevwarp_build_map: pinhole, or the rational model with the r2_max guard), so neither entry has a
 * lens or a matrix, and neither touches float64.  Both are defined by composing existing entries, bit for bit; the frame is 8-bit, 3 channels.
 *
 * bevwarp_remap_nv12:
 *   dst = bevwarp_remap(cvtColor(nv12, rgb_order ? COLOR_YUV2RGB_NV12 : COLOR_YUV2BGR_NV12), dst, ..., map_xy, map_frac, ..., BEVWARP_U8,
 *                       interp, border_mode, border_value)
 * with the converted frame never in memory: every tap is converted (bevwarp_warp_nv12's conversion) before the blend.
 *   y, uv, src_h, src_w, the four source strides, rgb_order   bevwarp_warp_nv12's: even sides, an even uv base and even uv strides, the
 *                 size limits of either plane.
 *   map_xy, map_frac, map_count, the four map strides, interp   bevwarp_remap's: map_count 1 (shared; frame strides not looked at) or
 *                 batch; the planes are read images without source limits; map_frac may be NULL for BEVWARP_NEAREST only; interp is
 *                 the interpolation the map was built for.
 *   border_mode   all six.  The index remap applies to the PIXEL index: a tap at remapped pixel (c, r) reads Y = y[r][c] and the chroma
 *                 pair uv[r >> 1][2 (c >> 1)], uv[r >> 1][2 (c >> 1) + 1] and is converted before the blend.  Under BEVWARP_BORDER_CONSTANT a
 *                 tap outside the frame is border_value in the DESTINATION's channel order, not converted (HOST, 3 doubles, NULL = 0;
 *                 not looked at under the other modes); BEVWARP_BORDER_TRANSPARENT writes the inliers only.  An invalid map entry
 *                 (-32768, -32768) behaves exactly as in bevwarp_remap.
 *   dst           device, dst_h x dst_w x 3 bytes; the wide-store rule is bevwarp_warp's.  It must not overlap y, uv or either map plane.
 * With a map from bevwarp_build_map (lens NULL) and BEVWARP_BORDER_CONSTANT the result also equals bevwarp_warp_nv12's for the same
 * matrix.
 * Status, in bevwarp_warp_nv12's order with the map count standing where the matrix count stood and the two map planes among the images
 * that are checked: BEVWARP_ERR_BAD_ARG (a null pointer -- map_frac under BEVWARP_LINEAR included --, a non-positive size, odd src_w or
 * src_h, a row stride below a row for any of the five images, frames or maps that overlap their successors, an odd uv base or stride, a
 * map_xy base or stride that is no multiple of 4 or a map_frac one that is no multiple of 2, map_count not 1 or batch);
 * BEVWARP_ERR_UNSUPPORTED (interp other than nearest / linear, rgb_order outside {0, 1}, border_mode outside the six);
 * BEVWARP_ERR_TOO_LARGE (either source plane, as bevwarp_warp_nv12); BEVWARP_ERR_OVERLAP (dst shares bytes with the y or the uv image, by
 * bevwarp_warp's rule, or with the bounding byte range of either map plane); BEVWARP_ERR_TOO_LARGE again for a destination side > 2^20;
 * BEVWARP_ERR_NOT_FINITE (border_value, BEVWARP_BORDER_CONSTANT only).  batch == 0 is BEVWARP_OK and launches nothing.
 *
 * bevwarp_remap_nv12_planes: for P = plane_dtype (BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16) and channel c in the DESTINATION's order,
 *   p               = bevwarp_remap_nv12(y, uv, ..., interp, border_mode, rgb_order, border_value)[b][y][x][c]      (an 8-bit value)
 *   v               = float32(p) * float32(scale[c]) + float32(bias[c])                              (multiply, then add, each rounded; no FMA)
 *   dst[b][c][y][x] = convert_P(v)
 * -- bevwarp_warp_nv12_planes' plane stage, unchanged (convert_P, the three destination strides in bytes, the wide-store rule, scale and
 * bias HOST, 3 doubles each in the destination's order, NULL = 1 and 0).  Neither the converted frame nor the 8-bit BEV frame is in memory.
 *   border_mode   the five modes that write every pixel; BEVWARP_BORDER_TRANSPARENT is BEVWARP_ERR_UNSUPPORTED (a canvas is kept as
 *                 8-bit pixels: bevwarp_remap_nv12 over it, then bevwarp_warp_planes).
 * Status, in bevwarp_warp_nv12_planes' order with the same two substitutions: BEVWARP_ERR_BAD_ARG (everything bevwarp_remap_nv12 lists;
 * the destination as bevwarp_warp_nv12_planes lists it); BEVWARP_ERR_UNSUPPORTED (interp, rgb_order, plane_dtype outside {F32, F16, BF16},
 * border_mode outside the five); BEVWARP_ERR_TOO_LARGE (either source plane); BEVWARP_ERR_OVERLAP (the bounding byte range of all
 * destination planes meets the y image's, the uv image's or either map plane's); BEVWARP_ERR_TOO_LARGE again for a destination side
 * > 2^20; BEVWARP_ERR_NOT_FINITE (border_value under BEVWARP_BORDER_CONSTANT only; scale, bias).  batch == 0 is BEVWARP_OK and launches nothing.
 */
int bevwarp_remap_nv12(const void *y, const void *uv, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w,
                       int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride,
                       int64_t dst_frame_stride, int64_t dst_row_stride, const void *map_xy, const void *map_frac, int map_count,
                       int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride,
                       int interp, int border_mode, int rgb_order, const double *border_value /*HOST, 3 doubles or NULL*/,
                       void *stream);
int bevwarp_remap_nv12_planes(const void *y, const void *uv, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w,
                              int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride,
                              int64_t dst_frame_stride, int64_t dst_plane_stride, int64_t dst_row_stride,
                              const void *map_xy, const void *map_frac, int map_count, int64_t xy_frame_stride,
                              int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride, int interp,
                              int border_mode, int rgb_order, const double *border_value /*HOST, 3 or NULL*/,
                              const double *scale /*HOST, 3 or NULL = 1*/, const double *bias /*HOST, 3 or NULL = 0*/,
                              int plane_dtype, void *stream);

/*
 * The warp written as NV12 for a video encoder, in one pass: stands in for cv2.warpPerspective(img, H_bev_img, (u_size, v_size)) followed by
 * `writer.write(bev)`, vis_homo.py:109-111 and bev/io/utils.py:89-99, whose writer converts every BGR frame to YUV 4:2:0 on the host.
 * Bit for bit
 *   (dst_y, dst_uv) = BGR->NV12( bevwarp_warp(src, ..., 3 channels, BEVWARP_U8, interp, border_value) )
 * and the warped BGR / RGB frame is never in memory.  With p the 8-bit warped pixel and R, G, B its channels as rgb_order names them:
 *       Y = ( 269484 R + 528482 G + 102760 B + (16  << 20) + (1 << 19)) >> 20
 *       U = (-155188 R - 305135 G + 460324 B + (128 << 20) + (1 << 19)) >> 20
 *       V = ( 460324 R - 385875 G -  74448 B + (128 << 20) + (1 << 19)) >> 20              (int32, >> arithmetic)
 *       dst_y [b][y][x]         = Y(p[b][y][x])                              every x, y
 *       dst_uv[b][y / 2][x / 2] = (U(p[b][y][x]), V(p[b][y][x]))             x even and y even only: no averaging over the 2 x 2 block
 *   conversion      OpenCV's 8-bit RGB -> YUV 4:2:0 two-plane path: BT.601, limited range, 20-bit fixed point (restated from memory like the
 *                   rest of the warp: parity with OpenCV is unpinned).  Over all 2^24 pixels the sums span 17,301,504 ... 246,986,634 (Y)
 *                   and 17,359,651 ... 252,124,636 (U, V), Y spans 16 ... 235 and U, V span 16 ... 240: int32 holds every sum and no
 *                   value is clamped.
 *   src             device, 8-bit, 3 channels, src_h x src_w pixels.  rgb_order 0: its pixels are B, G, R (what VideoCapture gives); 1: R, G, B.
 *   interp          BEVWARP_NEAREST | BEVWARP_LINEAR; maps, tap guards and blend are bevwarp_warp's.
 *   border_value    HOST, 3 doubles in the SOURCE pixel's channel order, or NULL = 0: a pixel value like any other, converted with the
 *                   pixel -- (0, 0, 0) gives Y, U, V = (16, 128, 128).
 *   dst_y, dst_uv   device; dst_h and dst_w are even.  The layout is bevwarp_warp_nv12's source layout, so a frame written here is accepted
 *                   there: dst_h rows of dst_w Y bytes (y_row_stride >= dst_w), dst_h / 2 rows of dst_w / 2 (U, V) byte pairs -- dst_w
 *                   bytes per row; the uv base, uv_row_stride and uv_frame_stride are even.  One (dst_h * 3 / 2) x dst_w buffer with
 *                   dst_uv = dst_y + dst_h * y_row_stride, and two allocations, both fit.  A plane whose base and both strides are
 *                   multiples of 4 is written with 4-byte stores (each plane by its own layout).
 * Status, in this order: BEVWARP_ERR_BAD_ARG (null pointer, non-positive size, odd dst_w or dst_h, a row stride below 3 src_w or below
 * dst_w for either destination plane, frames that overlap their successors, an odd uv base / row stride / frame stride, m_count not 1 or
 * batch); BEVWARP_ERR_UNSUPPORTED (interp other than nearest / linear; rgb_order outside {0, 1}); BEVWARP_ERR_TOO_LARGE (the source limits
 * of bevwarp_warp); BEVWARP_ERR_OVERLAP (either destination plane shares bytes with the source, by bevwarp_warp's rule, or the two
 * destination planes share bytes with each other -- both are written; the single-buffer layout is adjacent, not overlapping);
 * BEVWARP_ERR_TOO_LARGE again for a destination side > 2^20; BEVWARP_ERR_NOT_FINITE (border_value).  batch == 0 is BEVWARP_OK and
 * launches nothing.
 * Warping the Y and the UV plane separately (two bevwarp_warp calls of 1 and 2 channels) is NOT this: it blends in YUV.
 */
int bevwarp_warp_to_nv12(const void *src, void *dst_y, void *dst_uv, int batch, int src_h, int src_w, int dst_h, int dst_w,
                         int64_t src_frame_stride, int64_t src_row_stride,
                         int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride, int64_t uv_row_stride,
                         const double *M_inv, int m_count, int interp, int rgb_order,
                         const double *border_value /*HOST, 3 or NULL*/, void *stream);

/*
 * The same egress from a video decoder's NV12 frames: `video.read()` -> cv2.warpPerspective -> `writer.write(bev)`, vis_homo.py:85-111 and
 * bev/io/utils.py:89-99, in one launch with no BGR frame in memory on either side.  Bit for bit
 *   (dst_y, dst_uv) = BGR->NV12( bevwarp_warp_nv12(y, uv, ..., interp, rgb_order = 0, border_value) )
 * with bevwarp_warp_to_nv12's conversion and destination and bevwarp_warp_nv12's source (even src_h and src_w, every tap converted to B, G, R
 * before the blend).  border_value: HOST, 3 doubles in B, G, R order, or NULL = 0; converted with the pixel.  The intermediate channel
 * order changes nothing else.
 * Status, in this order: BEVWARP_ERR_BAD_ARG (null pointer, non-positive size, odd dst_w, dst_h, src_w or src_h, a row stride below src_w
 * for either source plane or below dst_w for either destination plane, frames that overlap their successors, an odd uv base / row stride /
 * frame stride -- source and destination alike --, m_count not 1 or batch); BEVWARP_ERR_UNSUPPORTED (interp other than nearest / linear);
 * BEVWARP_ERR_TOO_LARGE (either source plane, as bevwarp_warp_nv12); BEVWARP_ERR_OVERLAP (either destination plane shares bytes with either
 * source plane, or the destination planes with each other; the source planes may overlap each other); BEVWARP_ERR_TOO_LARGE again for a
 * destination side > 2^20; BEVWARP_ERR_NOT_FINITE (border_value).  batch == 0 is BEVWARP_OK and launches nothing.
 */
int bevwarp_warp_nv12_to_nv12(const void *y, const void *uv, void *dst_y, void *dst_uv, int batch, int src_h, int src_w,
                              int dst_h, int dst_w, int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride,
                              int64_t uv_row_stride, int64_t dst_y_frame_stride, int64_t dst_y_row_stride,
                              int64_t dst_uv_frame_stride, int64_t dst_uv_row_stride, const double *M_inv, int m_count,
                              int interp, const double *border_value /*HOST, 3 (B, G, R) or NULL*/, void *stream);

/*
 * The same egress through a fixed camera's warp maps: the map samplers (bevwarp_remap, bevwarp_remap_nv12, bevwarp_stitch_maps,
 * bevwarp_stitch_maps_nv12) with bevwarp_warp_to_nv12's store stage behind them, one launch each, no BGR BEV frame in memory and no float64.
 * It is the ending of the reference's loop -- warp, then `writer.write(bev)`, vis_homo.py:85-111 and bev/io/utils.py:89-99 -- for a site whose
 * cameras are fixed and distorted (the map carries the lens: bevwarp_build_map).  Each entry is defined by composing existing entries, bit
 * for bit:
 *   bevwarp_remap_to_nv12            BGR->NV12( bevwarp_remap(src, ..., 3 channels, BEVWARP_U8, interp, border_mode, border_value) )
 *   bevwarp_remap_nv12_to_nv12       BGR->NV12( bevwarp_remap_nv12(y, uv, ..., interp, border_mode, rgb_order = 0, border_value) )
 *   bevwarp_stitch_maps_to_nv12      BGR->NV12( bevwarp_stitch_maps(cams, ..., 3 channels, BEVWARP_U8, interp, blend, feather,
 *                                               BEVWARP_BORDER_CONSTANT, border_value) )
 *   bevwarp_stitch_maps_nv12_to_nv12 BGR->NV12( bevwarp_stitch_maps_nv12(cams, ..., interp, blend, feather, rgb_order = 0,
 *                                               BEVWARP_BORDER_CONSTANT, border_value) )
 *   BGR->NV12       bevwarp_warp_to_nv12's conversion, word for word: the 20-bit BT.601 limited-range sums above, Y for every pixel, the
 *                   (U, V) pair of pixel (x, y) for even x and even y only -- no averaging over the 2 x 2 block.
 *   rgb_order       names the SOURCE pixels' channel order (0: B, G, R; 1: R, G, B), as in bevwarp_warp_to_nv12.  The NV12 sources are
 *                   sampled as B, G, R; the intermediate order changes nothing else.
 *   border_value    HOST, 3 doubles in that order, or NULL = 0: a pixel, converted with the pixel -- (0, 0, 0) gives (16, 128, 128).  Remap
 *                   entries: the border pixel of bevwarp_remap's BEVWARP_BORDER_CONSTANT sampler (a tap outside the source is replaced
 *                   before the blend; an invalid map entry (-32768, -32768) yields the border pixel itself), not looked at under the other
 *                   modes.  Stitch entries: the pixel that no camera covers.
 *   border_mode     remap entries: the five modes that write every pixel, as bevwarp_remap_nv12_planes has them;
 *                   BEVWARP_BORDER_TRANSPARENT is BEVWARP_ERR_UNSUPPORTED (a canvas that is only partly updated is kept as 8-bit pixels).
 *                   The stitch entries have none: uncovered pixels are always the border value.
 *   dst_y, dst_uv   bevwarp_warp_to_nv12's destination with that entry's rules: even dst_h and dst_w, an even uv base and even uv strides,
 *                   the joined single-buffer layout accepted, 4-byte stores per plane where that plane's base and strides are multiples of 4.
 *                   Neither plane may overlap any image the call reads (frames, uv, xy or frac, of any camera), nor the other plane.
 *   maps, sources   as the entry each one composes: map_count 1 or batch, map_frac NULL for BEVWARP_NEAREST only, even source sides for
 *                   NV12 sources, bevwarp_map_camera as bevwarp_stitch_maps (bevwarp_stitch_maps_nv12) reads it.
 * Status.  bevwarp_remap_to_nv12, in bevwarp_remap's order with bevwarp_warp_to_nv12's destination checks standing where the interleaved
 * destination's stood: BEVWARP_ERR_BAD_ARG (a null pointer -- map_frac under BEVWARP_LINEAR included --, a non-positive size, odd dst_w or
 * dst_h); BEVWARP_ERR_UNSUPPORTED (interp other than nearest / linear, rgb_order outside {0, 1}, border_mode outside the five);
 * BEVWARP_ERR_BAD_ARG (map_count not 1 or batch; a row stride below a row for any of the five images, frames or maps that overlap their
 * successors, an odd uv base or stride, a map_xy base or stride that is no multiple of 4 or a map_frac one that is no multiple of 2);
 * BEVWARP_ERR_TOO_LARGE (the source limits of bevwarp_warp); BEVWARP_ERR_OVERLAP (either destination plane shares bytes with the source, by
 * bevwarp_warp's rule, or with the bounding byte range of either map plane, or the two destination planes with each other; the
 * single-buffer layout is adjacent, not overlapping); BEVWARP_ERR_TOO_LARGE again for a destination side > 2^20; BEVWARP_ERR_NOT_FINITE
 * (border_value, BEVWARP_BORDER_CONSTANT only).
 * bevwarp_remap_nv12_to_nv12, in bevwarp_remap_nv12's order likewise: BEVWARP_ERR_BAD_ARG (a null pointer, a non-positive size, an odd side
 * of the source or the destination, the layouts of all six images as above -- an odd uv base or stride on either side --, map_count not 1
 * or batch); BEVWARP_ERR_UNSUPPORTED (interp, border_mode outside the five); BEVWARP_ERR_TOO_LARGE (either source plane);
 * BEVWARP_ERR_OVERLAP (either destination plane with either source plane, with either map plane, or with the other destination plane);
 * BEVWARP_ERR_TOO_LARGE again; BEVWARP_ERR_NOT_FINITE (border_value, BEVWARP_BORDER_CONSTANT only).
 * The stitch entries, in bevwarp_stitch_maps' order: BEVWARP_ERR_BAD_ARG for cams NULL, n_cams outside 1..8, or feather outside 1..4096 under
 * BEVWARP_STITCH_FEATHER; then per camera in ascending k bevwarp_remap_to_nv12's (bevwarp_remap_nv12_to_nv12's) checks in that entry's own
 * order against both destination planes (blend counts as part of the format), the first status that is not BEVWARP_OK being returned;
 * then BEVWARP_ERR_TOO_LARGE for a destination side > 2^20; then BEVWARP_ERR_NOT_FINITE for border_value.
 * batch == 0 is BEVWARP_OK and launches nothing, for all four.
 */
int bevwarp_remap_to_nv12(const void *src, void *dst_y, void *dst_uv, int batch, int src_h, int src_w, int dst_h, int dst_w,
                          int64_t src_frame_stride, int64_t src_row_stride, int64_t y_frame_stride, int64_t y_row_stride,
                          int64_t uv_frame_stride, int64_t uv_row_stride, const void *map_xy, const void *map_frac, int map_count,
                          int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride,
                          int interp, int border_mode, int rgb_order, const double *border_value /*HOST, 3 or NULL*/, void *stream);
int bevwarp_remap_nv12_to_nv12(const void *y, const void *uv, void *dst_y, void *dst_uv, int batch, int src_h, int src_w,
                               int dst_h, int dst_w, int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride,
                               int64_t uv_row_stride, int64_t dst_y_frame_stride, int64_t dst_y_row_stride,
                               int64_t dst_uv_frame_stride, int64_t dst_uv_row_stride, const void *map_xy, const void *map_frac,
                               int map_count, int64_t xy_frame_stride, int64_t xy_row_stride, int64_t frac_frame_stride,
                               int64_t frac_row_stride, int interp, int border_mode,
                               const double *border_value /*HOST, 3 (B, G, R) or NULL*/, void *stream);
int bevwarp_stitch_maps_to_nv12(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst_y, void *dst_uv, int batch, int dst_h,
                                int dst_w, int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride,
                                int64_t uv_row_stride, int interp, int blend, int feather, int rgb_order,
                                const double *border_value /*HOST, 3 or NULL*/, void *stream);
int bevwarp_stitch_maps_nv12_to_nv12(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst_y, void *dst_uv, int batch,
                                     int dst_h, int dst_w, int64_t y_frame_stride, int64_t y_row_stride, int64_t uv_frame_stride,
                                     int64_t uv_row_stride, int interp, int blend, int feather,
                                     const double *border_value /*HOST, 3 (B, G, R) or NULL*/, void *stream);

/*
 * The map samplers straight to the normalised channel planes a detector takes: bevwarp_remap from 8-bit frames of 3 channels, and the two
 * stitches through maps, with bevwarp_warp_nv12_planes' plane stage behind them, one launch each, no 8-bit BEV frame or canvas in memory and
 * no float64.  (NV12 frames through one camera's map have bevwarp_remap_nv12_planes.)  Each entry is defined by composing existing entries,
 * bit for bit:
 *   bevwarp_remap_planes            planes( bevwarp_remap(src, ..., 3 channels, BEVWARP_U8, interp, border_mode, border_value) )
 *   bevwarp_stitch_maps_planes      planes( bevwarp_stitch_maps(cams, ..., 3 channels, BEVWARP_U8, interp, blend, feather,
 *                                           BEVWARP_BORDER_CONSTANT, border_value) )
 *   bevwarp_stitch_maps_nv12_planes planes( bevwarp_stitch_maps_nv12(cams, ..., interp, blend, feather, rgb_order,
 *                                           BEVWARP_BORDER_CONSTANT, border_value) )
 *   planes          bevwarp_warp_nv12_planes' plane stage, word for word: for P = plane_dtype (BEVWARP_F32 | BEVWARP_F16 | BEVWARP_BF16), p
 *                   the 8-bit pixel of the composed entry and c its channel,
 *                       v               = float32(p[c]) * float32(scale[c]) + float32(bias[c])      (multiply, then add, each rounded; no FMA)
 *                       dst[b][c][y][x] = convert_P(v)
 *                   with that entry's convert_P, its three destination strides in bytes, its alignment rule (base and strides multiples
 *                   of the element size) and its wide-store rule (4 elements per store where base and strides admit them).
 *   channels        plane c is channel c of the sampled pixel: interleaved frames are not swapped (B, G, R frames give B, G, R planes);
 *                   for bevwarp_stitch_maps_nv12_planes that is the destination's order as rgb_order names it (0: B, G, R; 1: R, G, B).
 *   scale, bias     HOST, 3 doubles each in the planes' order, NULL = 1 and 0.
 *   border_value    HOST, 3 doubles in the planes' order, or NULL = 0: an 8-bit pixel (saturate_cast<uchar>) that then passes through the
 *                   plane stage like any other.  bevwarp_remap_planes: the border pixel of bevwarp_remap's BEVWARP_BORDER_CONSTANT sampler
 *                   (a tap outside the source is replaced before the blend; an invalid map entry (-32768, -32768) yields the border pixel
 *                   itself), not looked at under the other modes.  Stitch entries: the pixel that no camera covers; BEVWARP_STITCH_FEATHER
 *                   is the 8-bit integer mean, then the plane stage.
 *   border_mode     bevwarp_remap_planes: the five modes that write every pixel; BEVWARP_BORDER_TRANSPARENT is BEVWARP_ERR_UNSUPPORTED, as
 *                   for bevwarp_remap_nv12_planes.  The stitch entries have none: uncovered pixels are always the border pixel.
 *   dst             device, batch x 3 planes of dst_h x dst_w elements.  The bounding byte range of all planes must not meet any image the
 *                   call reads (frames, uv, xy or frac, of any camera).
 *   maps, sources   as the entry each one composes: map_count 1 or batch, map_frac NULL for BEVWARP_NEAREST only, even source sides for
 *                   NV12 sources, bevwarp_map_camera as bevwarp_stitch_maps (bevwarp_stitch_maps_nv12) reads it.
 * Status.  bevwarp_remap_planes, in bevwarp_remap's order with bevwarp_warp_nv12_planes' destination checks standing where the interleaved
 * destination's stood: BEVWARP_ERR_BAD_ARG (a null pointer -- map_frac under BEVWARP_LINEAR included --, a non-positive size);
 * BEVWARP_ERR_UNSUPPORTED (interp other than nearest / linear, plane_dtype outside {F32, F16, BF16}, border_mode outside the five);
 * BEVWARP_ERR_BAD_ARG (map_count not 1 or batch; a row stride below a row for the source, either map plane or a destination plane, frames,
 * maps or planes that overlap their successors, a map_xy base or stride that is no multiple of 4 or a map_frac one that is no multiple of
 * 2, a destination base or stride that is no multiple of the element size); BEVWARP_ERR_TOO_LARGE (the source limits of bevwarp_warp);
 * BEVWARP_ERR_OVERLAP (the bounding byte range of all destination planes meets the source's or either map plane's); BEVWARP_ERR_TOO_LARGE
 * again for a destination side > 2^20; BEVWARP_ERR_NOT_FINITE (border_value under BEVWARP_BORDER_CONSTANT only; scale, bias).
 * The stitch entries, in bevwarp_stitch_maps' order: BEVWARP_ERR_BAD_ARG for cams NULL, n_cams outside 1..8, or feather outside 1..4096 under
 * BEVWARP_STITCH_FEATHER; then per camera in ascending k bevwarp_remap_planes' (bevwarp_remap_nv12_planes') checks in that entry's own order
 * against the destination planes (blend counts as part of the format), the first status that is not BEVWARP_OK being returned; then
 * BEVWARP_ERR_TOO_LARGE for a destination side > 2^20; then BEVWARP_ERR_NOT_FINITE for border_value, scale, bias, in that order.
 * batch == 0 is BEVWARP_OK and launches nothing, for all three.
 */
int bevwarp_remap_planes(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w,
                         int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_plane_stride,
                         int64_t dst_row_stride, const void *map_xy, const void *map_frac, int map_count, int64_t xy_frame_stride,
                         int64_t xy_row_stride, int64_t frac_frame_stride, int64_t frac_row_stride, int interp, int border_mode,
                         const double *border_value /*HOST, 3 or NULL*/, const double *scale /*HOST, 3 or NULL = 1*/,
                         const double *bias /*HOST, 3 or NULL = 0*/, int plane_dtype, void *stream);
int bevwarp_stitch_maps_planes(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w,
                               int64_t dst_frame_stride, int64_t dst_plane_stride, int64_t dst_row_stride, int interp, int blend,
                               int feather, const double *border_value /*HOST, 3 or NULL*/,
                               const double *scale /*HOST, 3 or NULL = 1*/, const double *bias /*HOST, 3 or NULL = 0*/,
                               int plane_dtype, void *stream);
int bevwarp_stitch_maps_nv12_planes(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w,
                                    int64_t dst_frame_stride, int64_t dst_plane_stride, int64_t dst_row_stride, int interp,
                                    int blend, int feather, int rgb_order, const double *border_value /*HOST, 3 or NULL*/,
                                    const double *scale /*HOST, 3 or NULL = 1*/, const double *bias /*HOST, 3 or NULL = 0*/,
                                    int plane_dtype, void *stream);

/*
 * out[i] = uint8(min(round_half_even(fg[i] * (mask[i] / 255) + bg[i] * (1 - mask[i] / 255)), 255)) for i in [0, n), computed in
 * float64 like the reference's numpy expression.  Device uint8 arrays of n bytes each (images of equal shape, any
 * channel count, flattened); `out` may alias `bg` or `fg`.
 */
int bevwarp_composite(const void *bg, const void *fg, const void *mask, void *out, int64_t n, void *stream);

/*
 * dst = composite_reg_img(warp(bg, M_bg), warp(fg, M_cam), warp(mask, M_cam)) -- bev/tool/compo.py:26-49 -- where the three
 * warps are bevwarp_warp's BEVWARP_U8 / BEVWARP_LINEAR / zero-border warp to (dst_w, dst_h) and the blend is
 * bevwarp_composite's, computed per pixel in one launch: the warped images are never written.  Bit-identical to the
 * three-warp sequence.
 *   bg (bg_h x bg_w), fg and mask (fg_h x fg_w each), dst: device uint8, `channels` (1..4) interleaved, strides in bytes.
 *   M_inv_bg, M_inv_cam: device, 9 float64 each, INVERSE maps (dst px -> bg px / camera px).
 *   fg_gray: non-zero = the reference's bw_mode (compo.py:13-14): the foreground is converted BGR -> grey -> BGR before it is
 *            warped, i.e. tap by tap ((1868 B + 9617 G + 4899 R + 8192) >> 14, OpenCV's 8-bit form); channels must be 3.
 * Overlap of dst with a source: BEVWARP_ERR_OVERLAP (same rule as bevwarp_warp).
 */
int bevwarp_warp_composite(const void *bg, int bg_h, int bg_w, int64_t bg_row_stride, const void *fg, const void *mask,
                           int fg_h, int fg_w, int64_t fg_row_stride, int64_t mask_row_stride, void *dst, int dst_h,
                           int dst_w, int64_t dst_row_stride, int channels, const double *M_inv_bg,
                           const double *M_inv_cam, int fg_gray, void *stream);

/*
 * dst[b] = cv2.resize(src[b], (dst_w, dst_h)) with the default INTER_LINEAR, uint8, `channels` (1..4) interleaved -- the resize of the
 * reference's "small" branch (img_small = cv2.resize(img, (new_u, new_v)), vis_homo.py:90) in front of its warp (:91).  OpenCV's classic
 * bilinear path: sampling at (d + 0.5) * scale - 0.5, 11-bit coefficients, replicated edge, an exact 2 x 2 decimation = the box mean
 * (restated from memory of resize.cpp; parity unpinned -- oracle/resize_oracle.c).  dtype must be BEVWARP_U8, interp BEVWARP_LINEAR.
 * Device pointers, strides in bytes; src and dst must not overlap (BEVWARP_ERR_OVERLAP).
 */
int bevwarp_resize(const void *src, void *dst, int batch, int src_h, int src_w, int dst_h, int dst_w, int channels,
                   int64_t src_frame_stride, int64_t src_row_stride, int64_t dst_frame_stride, int64_t dst_row_stride, int dtype,
                   int interp, void *stream);

/*
 * Marks every in-bounds source pixel that any tap of any destination pixel of the same warp would
 * read: touched[b][y][x] = 1 (device bytes, batch x src_h x src_w, caller zero-initialises).
 * sum(touched) is the exact "footprint_px" term of the algorithmic-bytes figure.
 */
int bevwarp_footprint(unsigned char *touched, int batch, int src_h, int src_w, int dst_h, int dst_w,
                      const double *M_inv, int m_count, int interp, void *stream);

/*
 * out[i] = dehomogenise(H @ (in[i], 1))            for dim == 2   (n x 2 in, n x 2 out)
 * out[i] = (H @ in[i]) / (H @ in[i])[2]            for dim == 3   (n x 3 in, n x 3 out)
 *   in, out  device, contiguous, dtype BEVWARP_F32 | BEVWARP_F64 (arithmetic is float64 either way).
 *   H        HOST, 9 doubles (copied at call time).  in == out is allowed.
 */
int bevwarp_project_points(const void *in, void *out, int64_t n, int dim, const double *H /*HOST*/, int dtype,
                           void *stream);

/*
 * bevwarp_project_points through bevwarp_warp_lens's lens model, in both directions: points of the plane H maps from -> pixels of the RAW
 * frame (BEVWARP_LENS_DISTORT), and pixels of the raw frame -> the plane H maps to (BEVWARP_LENS_UNDISTORT), which inverts the model by a
 * fixed number of fixed-point steps and gives every point a verdict.  Like the lens warp this is OUR chain: parity with OpenCV is unpinned
 * (cv2.projectPoints / cv2.undistortPoints).  The iteration is the classic undistortPoints step, but that function runs 5 steps (or stops on
 * its own criteria) and reports nothing; here `iters` is the caller's (the Python entry's default is 20: 5 steps leave 0.1 px on a 640-px
 * frame), no step is skipped, and a point whose reprojection misses by more than tol_px is NaN.  Bit-reproducible: every step below is one
 * correctly rounded float64 + - * / (IEEE division, no FMA), in the order written.
 *   in, out       device, n x 2, contiguous, dtype BEVWARP_F32 | BEVWARP_F64, aligned to a point (8 / 16 bytes).  in == out is allowed.
 *                 float32 inputs widen exactly; out and residual are the float64 results rounded to nearest.
 *   H             HOST, 9 doubles (copied at call time).
 *   lens, r2_max  exactly bevwarp_warp_lens's: the same 12 doubles, the same meaning.
 * "The lens steps" on (xn, yn) are bevwarp_warp_lens's lines `x2 = ...` to `v = fy yd + cy`, giving (u, v, r2).  With (x, y) a point:
 *   plane(x, y):  X = (h1 y + h2) + h0 x      Y = (h4 y + h5) + h3 x      W = (h7 y + h8) + h6 x
 *                 Wr = (W != 0) ? 1 / W : 0   result (X Wr, Y Wr)
 *                 (the operand order of bevwarp_warp_lens's first evaluation block: at the integer pixels of a destination no wider than
 *                 one block, DISTORT with M_ray reproduces that warp's u, v and r2 by bits)
 * BEVWARP_LENS_DISTORT.  H: the points' coordinates -> normalised UNDISTORTED camera plane (bevwarp_warp_lens's M_ray of the inverse
 * homography).  residual must be NULL; iters and tol_px are ignored.
 *   (xn, yn) = plane(in[i])        (u, v, r2) = the lens steps on (xn, yn)
 *   out[i] = (r2 <= r2_max) ? (u, v) : (NaN, NaN)                  (false for a NaN r2)
 * BEVWARP_LENS_UNDISTORT.  H: normalised undistorted camera plane -> the target's coordinates (H_world_img K, say).  (u, v) = in[i]:
 *   xd = (u - cx) / fx     yd = (v - cy) / fy     x = xd     y = yd
 *   `iters` times (1..100, no early exit):
 *       x2 = x x   y2 = y y   r2 = x2 + y2   xy2 = 2 (x y)          num, den as in bevwarp_warp_lens          ic = den / num
 *       dx = p1 xy2 + p2 (r2 + 2 x2)         dy = p1 (r2 + 2 y2) + p2 xy2
 *       x = (xd - dx) ic                     y = (yd - dy) ic
 *   (u', v', r2) = the lens steps on (x, y)
 *   e = max(|u' - u|, |v' - v|), NaN if either is NaN              valid = (r2 <= r2_max) and (e <= tol_px)
 *   out[i] = valid ? plane(x, y) : (NaN, NaN)
 *   residual[i] = e                 device, n values of dtype, or NULL; written for valid and invalid points alike
 *   tol_px        >= 0 pixels of the raw frame; +inf accepts every e that is not NaN.
 * direction | BEVWARP_LENS_FISHEYE: the same two directions through the fisheye model (bevwarp_warp_lens | BEVWARP_LENS_FISHEYE: the same lens,
 * r2_max carrying theta_max, atan_pos and "the fisheye steps").  ray(x, y, z) is H (x, y, z) in plane()'s operand order, NOT divided:
 *   X = (h1 y + h2 z) + h0 x      Y = (h4 y + h5 z) + h3 x      W = (h7 y + h8 z) + h6 x
 * BEVWARP_LENS_DISTORT | BEVWARP_LENS_FISHEYE.  H: the points' coordinates -> rays in the camera's frame (the oriented M_ray).
 *   (u, v, theta) = the fisheye steps on ray(x, y, 1)      out[i] = (theta <= theta_max) ? (u, v) : (NaN, NaN)
 *   (at the integer pixels of one evaluation block this reproduces the fisheye warp's u, v and theta by bits, as the rational one does)
 * BEVWARP_LENS_UNDISTORT | BEVWARP_LENS_FISHEYE.  H: rays in the camera's frame -> the target's coordinates (H_world_img K, say).  The
 * unknown is s = tan(theta / 2), in which the ray is rational, so atan_pos is the only transcendental step.  (u, v) = in[i]:
 *   xd = (u - cx) / fx    yd = (v - cy) / fy    thd = sqrt(xd xd + yd yd)    s = thd / 2
 *   d1 = 3 k1    d2 = 5 k2    d3 = 7 k3    d4 = 9 k4
 *   `iters` times (1..100, no early exit):
 *       theta = 2 atan_pos(s)    th2, poly as in the fisheye steps    f = theta poly - thd
 *       D = 1 + (((d4 th2 + d3) th2 + d2) th2 + d1) th2
 *       s = s - (f (1 + s s)) / (2 D)        s = (s < 0) ? 0 : s
 *   (rx, ry, rz) = (thd != 0) ? ((2 s) (xd / thd), (2 s) (yd / thd), 1 - s s) : (0, 0, 1)
 *   (u', v', theta') = the fisheye steps on (rx, ry, rz)       e = max(|u' - u|, |v' - v|), NaN if either is NaN
 *   valid = (theta' <= theta_max) and (e <= tol_px)
 *   (X, Y, W) = ray(rx, ry, rz)    Wr = (W != 0) ? 1 / W : 0    out[i] = valid ? (X Wr, Y Wr) : (NaN, NaN)    residual[i] = e
 *   These are Newton's steps: 5 reach 4.4e-16 rad for every theta up to 110 degrees of a lens that is monotonic there; the Python entry's
 *   default is 10.
 * A NaN that is stored is some NaN: its sign and payload are unspecified.
 * Status, in this order: BEVWARP_ERR_BAD_ARG for in, out or H NULL, n < 0, a direction outside the two, a residual under
 * BEVWARP_LENS_DISTORT, and under BEVWARP_LENS_UNDISTORT iters outside 1..100 or tol_px NaN or negative; BEVWARP_ERR_UNSUPPORTED for dtype;
 * BEVWARP_ERR_NOT_FINITE for H; the lens and r2_max as in bevwarp_warp_lens (NULL: BAD_ARG; NaN, +-inf: NOT_FINITE; fx == 0, fy == 0,
 * r2_max NaN or < 0: BAD_ARG; under BEVWARP_LENS_FISHEYE also a reserved entry != 0: BAD_ARG); BEVWARP_ERR_OVERLAP when residual's n values share a byte with in's or out's n points; last,
 * BEVWARP_ERR_BAD_ARG for in or out not aligned to a point or residual not aligned to a value.  n == 0 is BEVWARP_OK and launches nothing.
 */
#define BEVWARP_LENS_DISTORT 0     /* plane -> raw pixel */
#define BEVWARP_LENS_UNDISTORT 1   /* raw pixel -> plane */
/* (BEVWARP_LENS_FISHEYE, 0x100, is ORed into either) */
int bevwarp_project_points_lens(const void *in, void *out, void *residual /*device, may be NULL*/, int64_t n,
                                const double *H /*HOST, 9*/, const double *lens /*HOST, 12*/, double r2_max,
                                int direction, int iters, double tol_px, int dtype, void *stream);

/*
 * out[i][j] = IoU of rotated rectangles a[i], b[j].  Rows are [x, y, w, h, yaw, ...] with
 * `a_stride` / `b_stride` values per row (>= 5); at yaw 0 the length h lies along +x and the width w
 * along y (bev/rbox.py:87-95, the "world" convention).  out is na x nb, same dtype.
 *   dtype BEVWARP_F32 | BEVWARP_F64 (arithmetic is float64).
 */
int bevwarp_rbox_iou(const void *a, int na, int a_stride, const void *b, int nb, int b_stride, void *out, int dtype,
                     void *stream);

/*
 * out[i] = rbox_world_bev(boxes[i], H, src): rows [x, y, w, h, yaw, ...] (`stride` values per row, >= 5) through the
 * similarity H (HOST, 9 doubles; normalised by H[8]; BEVWARP_ERR_BAD_ARG when its last row is not (0, 0, 1) to 1e-5 or its
 * axes scale differently, the two conditions the reference asserts).  src_is_bev != 0: rows are BEV boxes (yaw from the
 * v axis), out rows are world boxes (yaw from the x axis); 0: the other way round.  out is n x 5, same dtype
 * (BEVWARP_F32 | BEVWARP_F64, arithmetic float64).
 */
int bevwarp_rbox_transform(const void *boxes, int n, int stride, const double *H /*HOST*/, int src_is_bev, void *out,
                           int dtype, void *stream);

/*
 * One tracker step, one launch:
 *   dets_world[i]     = rbox_world_bev(dets_bev[i], H_world_bev, "bev")                         n x 5
 *   iou[i][j]         = IoU(dets_world[i], trks_world[j])         (as bevwarp_rbox_iou)         n x m
 *   candidates[i][j]  = iou[i][j] > iou_threshold                 (uint8 0 / 1)                 n x m
 *   dets_img[i]       = dehomogenise(H_img_world @ (dets_world[i].xy, 1))   when H_img_world    n x 2
 * dets_bev rows have det_stride >= 5 values, trks_world rows trk_stride >= 5 (a tracker's state row may carry more).
 * H_world_bev as in bevwarp_rbox_transform; H_img_world (HOST, 9 doubles) may be NULL (then dets_img is not touched).
 * m == 0 is allowed (only dets_world / dets_img are produced).  n <= 64000.
 */
int bevwarp_tracker_step(const void *dets_bev, int n, int det_stride, const void *trks_world, int m, int trk_stride,
                         const double *H_world_bev /*HOST*/, const double *H_img_world /*HOST, may be NULL*/,
                         double iou_threshold, void *dets_world, void *iou, unsigned char *candidates, void *dets_img,
                         int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVWARP_H */
