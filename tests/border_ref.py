"""Numpy reference of the warp's border modes (bev_amd.warp.warp_perspective(border_mode=...), include/bevwarp.h
bevwarp_warp_border) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/parity.py.

The coordinate maps are oracle.warp_numpy's (fixed_point_maps: the 64 x 16 evaluation blocks, 32 / W, round half to even, NaN
to INT_MAX, int16 saturation); what differs between modes is which taps are read and whether a pixel is written, as OpenCV
3.x-4.x imgwarp.cpp's remapNearest / remapBilinear do it (restated from memory, parity unpinned):

  CONSTANT                 a tap outside the source is the border value; bilinear: all four outside -> the border value itself
  REPLICATE, REFLECT,      every tap index goes through borderInterpolate (OpenCV's loop, transcribed below); no shortcut
  WRAP, REFLECT_101
  TRANSPARENT              only inliers are written (nearest: 0 <= sx < w, 0 <= sy < h; bilinear: 0 <= sx <= w - 2,
                           0 <= sy <= h - 2); every other pixel keeps the canvas's value
"""
import numpy as np

from oracle.warp_numpy import INTER_TAB_SIZE, LINEAR, NEAREST, fixed_point_maps, invert3x3

CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = range(6)
MODES = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT)
SOURCE_READING = (REPLICATE, REFLECT, WRAP, REFLECT_101)
NAMES = {CONSTANT: "constant", REPLICATE: "replicate", REFLECT: "reflect", WRAP: "wrap", REFLECT_101: "reflect101", TRANSPARENT: "transparent"}
PAD_MODE = {REPLICATE: "edge", REFLECT: "symmetric", WRAP: "wrap", REFLECT_101: "reflect"}  # the numpy.pad twin of each


def _cdiv(a, b):
    """C's integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def border_interpolate(p, n, mode):
    """cv::borderInterpolate(p, len, borderType) for one index, as OpenCV's loop; -1 for CONSTANT outside."""
    if 0 <= p < n:
        return p
    if mode == REPLICATE:
        return 0 if p < 0 else n - 1
    if mode in (REFLECT, REFLECT_101):
        delta = 1 if mode == REFLECT_101 else 0
        if n == 1:
            return 0
        while True:
            if p < 0:
                p = -p - 1 + delta
            else:
                p = n - 1 - (p - n) - delta
            if 0 <= p < n:
                return p
    if mode == WRAP:
        if p < 0:
            p -= _cdiv(p - n + 1, n) * n
        if p >= n:
            p %= n
        return p
    if mode == CONSTANT:
        return -1
    raise ValueError(mode)


def border_index(p, n, mode):
    """border_interpolate over an integer array (the loop runs once per distinct index)."""
    p = np.asarray(p, dtype=np.int64)
    u, inv = np.unique(p, return_inverse=True)
    return np.array([border_interpolate(int(v), n, mode) for v in u], dtype=np.int64)[inv].reshape(p.shape)


def warp(src, M, dsize, interp=LINEAR, mode=REPLICATE, m_is_inverse=False, border_value=0.0, canvas=None):
    """cv2.warpPerspective(src, M, dsize, flags=interp, borderMode=mode, borderValue=border_value) on a (H, W) or (H, W, C)
    uint8 / float32 image.  TRANSPARENT writes into a copy of `canvas` (zeros when None) and returns it."""
    src = np.asarray(src)
    squeeze = src.ndim == 2
    s3 = src[:, :, None] if squeeze else src
    h, w, c = s3.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    Minv = np.asarray(M, np.float64).reshape(3, 3) if m_is_inverse else invert3x3(M)
    sx, sy, fx, fy = fixed_point_maps((dw, dh), Minv, interp)
    bv = np.broadcast_to(np.asarray(border_value, np.float64), (c,))
    cval = np.clip(np.rint(bv), 0, 255).astype(np.uint8) if s3.dtype == np.uint8 else bv.astype(np.float32)

    if mode == TRANSPARENT:  # inliers read their taps directly; the others are not written (their taps are never used)
        def ix(p):
            return np.clip(p, 0, w - 1)

        def iy(p):
            return np.clip(p, 0, h - 1)
    else:
        def ix(p):
            return border_index(p, w, mode)

        def iy(p):
            return border_index(p, h, mode)

    def tap(px, py):
        qx, qy = ix(px), iy(py)
        v = s3[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
        return np.where(((qx >= 0) & (qy >= 0))[..., None], v, cval[None, None, :])

    if interp == NEAREST:
        out = tap(sx, sy).astype(s3.dtype)
    elif s3.dtype == np.uint8:
        wx1, wy1 = fx.astype(np.int64), fy.astype(np.int64)
        wx0, wy0 = 32 - wx1, 32 - wy1
        w00, w01, w10, w11 = wy0 * wx0 * 32, wy0 * wx1 * 32, wy1 * wx0 * 32, wy1 * wx1 * 32
        acc = (tap(sx, sy).astype(np.int64) * w00[..., None] + tap(sx + 1, sy).astype(np.int64) * w01[..., None] +
               tap(sx, sy + 1).astype(np.int64) * w10[..., None] + tap(sx + 1, sy + 1).astype(np.int64) * w11[..., None])
        out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    else:
        s = np.float32(1.0 / INTER_TAB_SIZE)
        tx1, ty1 = fx.astype(np.float32) * s, fy.astype(np.float32) * s
        tx0, ty0 = np.float32(1) - tx1, np.float32(1) - ty1
        w00, w01, w10, w11 = ty0 * tx0, ty0 * tx1, ty1 * tx0, ty1 * tx1
        out = ((tap(sx, sy) * w00[..., None] + tap(sx + 1, sy) * w01[..., None]) + tap(sx, sy + 1) * w10[..., None]) + \
            tap(sx + 1, sy + 1) * w11[..., None]
        out = out.astype(np.float32)
    if mode == CONSTANT and interp != NEAREST:  # remapBilinear's constant-border shortcut (that mode only)
        all_out = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
        out = np.where(all_out[..., None], cval[None, None, :], out).astype(s3.dtype)
    if mode == TRANSPARENT:
        written = inliers(sx, sy, w, h, interp)
        base = np.zeros((dh, dw, c), s3.dtype) if canvas is None else np.array(canvas, dtype=s3.dtype).reshape(dh, dw, c)
        out = np.where(written[..., None], out, base)
    return out[:, :, 0] if squeeze else out


def inliers(sx, sy, w, h, interp):
    """The pixels TRANSPARENT writes."""
    if interp == NEAREST:
        return (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    return (sx >= 0) & (sx <= w - 2) & (sy >= 0) & (sy <= h - 2)


def written_mask(src_hw, M, dsize, interp=LINEAR, m_is_inverse=False):
    """(dst_h, dst_w) bool: the pixels a TRANSPARENT warp writes."""
    Minv = np.asarray(M, np.float64).reshape(3, 3) if m_is_inverse else invert3x3(M)
    sx, sy, _, _ = fixed_point_maps((int(dsize[0]), int(dsize[1])), Minv, interp)
    return inliers(sx, sy, int(src_hw[1]), int(src_hw[0]), interp)
