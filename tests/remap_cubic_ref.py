"""Numpy reference of bicubic sampling through a bilinear warp map (bev_amd.warp.remap(interpolation=INTER_CUBIC), include/bevwarp.h
BEVWARP_MAP_BICUBIC) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/remap_ref.py.

It knows nothing of matrices: it starts from map entries (sx, sy) and their frac words.  The tables are tests/cubic_ref's, the index function
is tests/border_ref's borderInterpolate; the sampler on (sx - 1, sy - 1, fy, fx) is restated here -- tests/test_remap_cubic_cpu.py ties it
to cubic_ref.warp by bits on pinhole maps.
"""
import numpy as np

from tests import border_ref as BR
from tests import cubic_ref as CR

CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = range(6)
MODES = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT)
F = np.float32


def classes(xy, w, h):
    """(inlier, partial, all_outside, transparent_written) bool masks over the map: cubic_ref.classes from entries."""
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    wx, wy = sx - 1, sy - 1
    inl = (wx >= 0) & (wx < max(w - 3, 0)) & (wy >= 0) & (wy < max(h - 3, 0))
    all_out = (wx >= w) | (wx + 4 <= 0) | (wy >= h) | (wy + 4 <= 0)
    written = inl | ((sx >= 0) & (sx < w) & (sy >= 0) & (sy < h))
    return inl, ~inl & ~all_out, all_out, written


def presums(src, xy, frac, mode=CONSTANT, border_value=0.0):
    """The 8-bit sums before the clamp, (dh, dw, C) int64 (the inlier's or the general path's, as the pixel takes them)."""
    return _sample(src, xy, frac, mode, border_value)[1]


def _sample(src, xy, frac, mode, border_value):
    s3 = src[:, :, None] if src.ndim == 2 else src
    h, w, c = s3.shape
    xy = np.asarray(xy)
    dh, dw = xy.shape[:2]
    wx, wy = xy[..., 0].astype(np.int64) - 1, xy[..., 1].astype(np.int64) - 1  # (int64: -32768 - 1 does not wrap)
    f = np.asarray(frac).astype(np.int64)
    fx, fy = f & 31, (f >> 5) & 31  # (higher bits are ignored)
    inl, _, all_out, written = classes(xy, w, h)
    is_u8 = s3.dtype == np.uint8
    bv = np.broadcast_to(np.asarray(border_value, np.float64), (c,)) if mode == CONSTANT else np.zeros(c)
    if is_u8:
        cv = np.clip(np.rint(bv), 0, 255).astype(np.int64)
        W = CR.fixed_table()[fy, fx].astype(np.int64)
        S, one = s3.astype(np.int64), np.int64(32768)
    else:
        cv = bv.astype(F)
        W = CR.float_table()[fy, fx]
        S, one = s3, F(1)
    mode1 = REFLECT_101 if mode == TRANSPARENT else mode
    xs = [BR.border_index(wx + j, w, mode1) for j in range(4)]
    ys = [BR.border_index(wy + i, h, mode1) for i in range(4)]
    with np.errstate(all="ignore"):
        # the general path: sum = cv * ONE, then tap by tap, rows outermost, taps outside skipped
        gen = np.broadcast_to(cv[None, None, :] * one, (dh, dw, c)).astype(S.dtype)
        for i in range(4):
            for j in range(4):
                ok = ((ys[i] >= 0) & (xs[j] >= 0))[..., None]
                t = S[np.clip(ys[i], 0, h - 1), np.clip(xs[j], 0, w - 1)]
                gen = np.where(ok, gen + (t - cv[None, None, :]) * W[..., 4 * i + j, None], gen)
        # inliers: the row sums, then the rows
        rows = []
        for i in range(4):
            yy = np.clip(wy + i, 0, h - 1)
            r = [S[yy, np.clip(wx + j, 0, w - 1)] * W[..., 4 * i + j, None] for j in range(4)]
            rows.append(((r[0] + r[1]) + r[2]) + r[3])
        inlier_sum = ((rows[0] + rows[1]) + rows[2]) + rows[3]
    assert gen.dtype == S.dtype and inlier_sum.dtype == S.dtype
    out = pre = np.where(inl[..., None], inlier_sum, gen)
    if is_u8:
        out = np.clip((out + 16384) >> 15, 0, 255)
    if mode == CONSTANT:
        out = np.where((all_out & ~inl)[..., None], cv[None, None, :], out)
    return out.astype(s3.dtype), pre, written


def remap_cubic(src, xy, frac, mode=CONSTANT, border_value=0.0, canvas=None):
    """bevwarp_remap(..., BEVWARP_LINEAR | BEVWARP_MAP_BICUBIC, mode) on a (H, W) or (H, W, C) uint8 / float32 image through the map
    (xy (dh, dw, 2) int16, frac (dh, dw) uint16 / int16).  TRANSPARENT writes into a copy of `canvas` (zeros when None)."""
    src = np.asarray(src)
    out, _, written = _sample(src, xy, frac, mode, border_value)
    dh, dw, c = out.shape
    if mode == TRANSPARENT:
        base = np.zeros((dh, dw, c), out.dtype) if canvas is None else np.array(canvas, dtype=out.dtype).reshape(dh, dw, c)
        out = np.where(written[..., None], out, base)
    return out[:, :, 0] if src.ndim == 2 else out
