"""Numpy definition of the fixed-camera warp maps (bev_amd.warp.build_warp_map / remap / convert_maps, include/bevwarp.h
bevwarp_build_map / bevwarp_remap) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/border_ref.py.

build() writes down what the trusted references' integers are in the map format: oracle.warp_numpy.fixed_point_maps (pinhole) or
tests/lens_ref.maps (lens), plus the sentinel rule -- an invalid pixel is (-32768, -32768), frac 0.  remap() is a sampler of its own
over the six border modes that knows nothing of matrices: it starts from (sx, sy, fx, fy).
"""
import numpy as np

from oracle.warp_numpy import LINEAR, NEAREST, fixed_point_maps
from tests import border_ref as BR
from tests import lens_ref as LR

CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = range(6)
MODES = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT)
SENTINEL = -32768


def build(dsize, M, lens=None, r2_max=np.inf, interp=LINEAR):
    """(xy, frac): (dh, dw, 2) int16 and (dh, dw) uint16 (None for nearest).  lens None: M is the inverse matrix (dst px -> src px);
    else M is the ray matrix and lens the 12 values of lens_ref.lens12."""
    dw, dh = int(dsize[0]), int(dsize[1])
    if lens is None:
        sx, sy, fx, fy = fixed_point_maps((dw, dh), np.asarray(M, np.float64).reshape(3, 3), interp)
        valid = np.ones((dh, dw), bool)
    else:
        sx, sy, fx, fy, valid = LR.maps((dw, dh), M, lens, r2_max, interp)
    sx, sy = np.where(valid, sx, SENTINEL), np.where(valid, sy, SENTINEL)
    assert sx.min() >= -32768 and sx.max() <= 32767 and sy.min() >= -32768 and sy.max() <= 32767
    xy = np.stack([sx, sy], axis=-1).astype(np.int16)
    if interp == NEAREST:
        return xy, None
    fx, fy = np.where(valid, fx, 0), np.where(valid, fy, 0)
    return xy, ((fy.astype(np.int64) << 5) | fx.astype(np.int64)).astype(np.uint16)


def written(xy, w, h, interp):
    """The pixels TRANSPARENT writes: the inliers."""
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    if interp == NEAREST:
        return (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    return (sx >= 0) & (sx <= w - 2) & (sy >= 0) & (sy <= h - 2)


def _index(p, n, mode):
    """Tap indices -> (source index, inside): CONSTANT keeps the clamped index and says whether the tap is inside; the four remapping
    modes go through borderInterpolate; TRANSPARENT clamps (only inliers are kept)."""
    if mode in (CONSTANT, TRANSPARENT):
        return np.clip(p, 0, n - 1), (p >= 0) & (p < n)
    return BR.border_index(p, n, mode), np.ones(p.shape, bool)


def remap(src, xy, frac, interp=LINEAR, mode=CONSTANT, border_value=0.0, canvas=None):
    """cv2.remap(src, xy, frac, interp, borderMode=mode, borderValue=border_value) on a (H, W) or (H, W, C) uint8 / float32 image, from
    the fixed-point maps.  TRANSPARENT writes into a copy of `canvas` (zeros when None)."""
    src = np.asarray(src)
    squeeze = src.ndim == 2
    s3 = src[:, :, None] if squeeze else src
    h, w, c = s3.shape
    xy = np.asarray(xy)
    dh, dw = xy.shape[:2]
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    bv = np.broadcast_to(np.asarray(border_value, np.float64), (c,))
    cval = np.clip(np.rint(bv), 0, 255).astype(np.uint8) if s3.dtype == np.uint8 else bv.astype(np.float32)

    def tap(px, py):
        qx, xin = _index(px, w, mode)
        qy, yin = _index(py, h, mode)
        return np.where((xin & yin)[..., None], s3[qy, qx], cval[None, None, :]), xin & yin

    if interp == NEAREST:
        out, _ = tap(sx, sy)
        out = out.astype(s3.dtype)
    else:
        f = np.asarray(frac).astype(np.int64)
        fx, fy = f & 31, (f >> 5) & 31  # (higher bits are ignored)
        (t00, i00), (t01, i01), (t10, i10), (t11, i11) = tap(sx, sy), tap(sx + 1, sy), tap(sx, sy + 1), tap(sx + 1, sy + 1)
        if s3.dtype == np.uint8:
            wx0, wy0 = 32 - fx, 32 - fy
            acc = (t00.astype(np.int64) * (wy0 * wx0 * 32)[..., None] + t01.astype(np.int64) * (wy0 * fx * 32)[..., None] +
                   t10.astype(np.int64) * (fy * wx0 * 32)[..., None] + t11.astype(np.int64) * (fy * fx * 32)[..., None])
            out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
        else:
            s = np.float32(1.0 / 32.0)
            tx1, ty1 = fx.astype(np.float32) * s, fy.astype(np.float32) * s
            tx0, ty0 = np.float32(1) - tx1, np.float32(1) - ty1
            with np.errstate(all="ignore"):
                out = ((t00 * (ty0 * tx0)[..., None] + t01 * (ty0 * tx1)[..., None]) + t10 * (ty1 * tx0)[..., None]) + t11 * (ty1 * tx1)[..., None]
            out = out.astype(np.float32)
        if mode == CONSTANT:  # all four taps outside: the border value itself
            none_in = ~(i00 | i01 | i10 | i11)
            out = np.where(none_in[..., None], cval[None, None, :], out).astype(s3.dtype)
    if mode == TRANSPARENT:
        base = np.zeros((dh, dw, c), s3.dtype) if canvas is None else np.array(canvas, dtype=s3.dtype).reshape(dh, dw, c)
        out = np.where(written(xy, w, h, interp)[..., None], out, base)
    return out[:, :, 0] if squeeze else out


def convert_maps(x, y, nearest=False):
    """convertMaps restated independently of bev_amd.warp.convert_maps, coordinate by coordinate in Python integers / floats: float32
    coordinate, times 32 in float32, round half to even, clamp to int32 (NaN -> INT_MAX), split."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    xy = np.zeros(x.shape + (2,), np.int16)
    frac = np.zeros(x.shape, np.uint16)

    def fixed(c):
        v = np.float32(c) if nearest else np.float32(np.float32(c) * np.float32(32.0))
        if np.isnan(v):
            return 2147483647
        return int(min(max(float(np.rint(np.float64(v))), -2147483648.0), 2147483647.0))

    with np.errstate(all="ignore"):
        for idx in np.ndindex(x.shape):
            X, Y = fixed(x[idx]), fixed(y[idx])
            if nearest:
                xy[idx] = (min(max(X, -32768), 32767), min(max(Y, -32768), 32767))
            else:
                xy[idx] = (min(max(X >> 5, -32768), 32767), min(max(Y >> 5, -32768), 32767))
                frac[idx] = ((Y & 31) << 5) | (X & 31)
    return xy, (None if nearest else frac)
