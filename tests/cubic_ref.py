"""Numpy reference of the bicubic warp (bev_amd.warp.warp_perspective(flags=INTER_CUBIC), include/bevwarp.h BEVWARP_CUBIC) --
TEST INFRASTRUCTURE ONLY, a plain module like tests/border_ref.py.

OpenCV 3.x-4.x's classic path (warpPerspective -> remap -> remapBicubic), restated from memory: parity with an installed cv2 is
unpinned, like the rest of the warp.  Every piece of the definition has one function here:

  coeffs_1d          the 32 x 4 float32 coefficients (A = -0.75)
  float_table        wf[fy, fx, k1 * 4 + k2] = cy[k1] * cx[k2], a float32 product
  fixed_table        wi = saturate_int16(rint(wf * 32768)), then the entry's sum is brought to 32768 at one of the four taps
                     (k1, k2) in {2, 3} x {2, 3} (OpenCV's ksize / 2 .. ksize / 2 + 1)
  warp               the maps of the bilinear warp (oracle.warp_numpy.fixed_point_maps), the window at (sx - 1, sy - 1) computed after
                     the int16 saturation, and per destination pixel one of: inlier (row-grouped sums), TRANSPARENT outside
                     (not written), CONSTANT all outside (the border value), or the general path (border-interpolated indices,
                     one tap at a time around the border value)
"""
import functools
import zlib

import numpy as np

from oracle.warp_numpy import LINEAR, fixed_point_maps, invert3x3
from tests.border_ref import CONSTANT, MODES, NAMES, REFLECT_101, SOURCE_READING, TRANSPARENT, border_interpolate  # noqa: F401

CUBIC = 2
F = np.float32


@functools.lru_cache(maxsize=None)
def coeffs_1d():
    """(32, 4) float32; every operation rounds to float32."""
    out = np.zeros((32, 4), F)
    A = F(-0.75)
    for i in range(32):
        x = F(i) * F(1.0 / 32)
        x1, xm = x + F(1), F(1) - x
        c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
        c1 = ((A + F(2)) * x - (A + F(3))) * x * x + F(1)
        c2 = ((A + F(2)) * xm - (A + F(3))) * xm * xm + F(1)
        c3 = F(1) - c0 - c1 - c2
        out[i] = (c0, c1, c2, c3)
    assert out.dtype == F
    return out


@functools.lru_cache(maxsize=None)
def float_table():
    """(32, 32, 16) float32, indexed [fy, fx, k1 * 4 + k2]."""
    c = coeffs_1d()
    return (c[:, None, :, None] * c[None, :, None, :]).astype(F).reshape(32, 32, 16)


@functools.lru_cache(maxsize=None)
def fixed_table(with_stats=False):
    """(32, 32, 16) int16 whose every entry sums to 32768; with_stats: (table, entries adjusted, diffs seen, values saturated)."""
    wf = float_table()
    scaled = wf * F(32768)
    assert scaled.dtype == F
    r = np.rint(scaled).astype(np.int64)
    wi = np.clip(r, -32768, 32767)
    saturated = int((wi != r).sum())
    adjusted, diffs = 0, set()
    for fy in range(32):
        for fx in range(32):
            e = wi[fy, fx]
            diff = int(e.sum()) - 32768
            if diff == 0:
                continue
            adjusted += 1
            diffs.add(diff)
            m = M = 2 * 4 + 2
            for k1 in (2, 3):
                for k2 in (2, 3):
                    k = k1 * 4 + k2
                    if e[k] < e[m]:
                        m = k
                    elif e[k] > e[M]:
                        M = k
            if diff < 0:
                e[M] -= diff
            else:
                e[m] -= diff
    assert (wi.sum(axis=2) == 32768).all() and np.abs(wi).max() <= 32767
    wi = wi.astype(np.int16)
    return (wi, adjusted, diffs, saturated) if with_stats else wi


def table_crc32(table):
    return zlib.crc32(np.ascontiguousarray(table, dtype=table.dtype.newbyteorder("<")).tobytes()) & 0xffffffff


def window(dsize, Minv):
    """(sx, sy, fx, fy): the first tap of the 4 x 4 window and the table index, from the bilinear maps."""
    sxm, sym, fx, fy = fixed_point_maps((int(dsize[0]), int(dsize[1])), Minv, LINEAR)
    return sxm.astype(np.int64) - 1, sym.astype(np.int64) - 1, fx, fy


def classes(src_hw, M, dsize, m_is_inverse=False):
    """(inlier, partial, all_outside, transparent_written) bool masks of shape (dst_h, dst_w).  partial: not an inlier, some tap
    inside; all_outside: CONSTANT's shortcut; transparent_written: what TRANSPARENT writes (inliers included)."""
    h, w = int(src_hw[0]), int(src_hw[1])
    Minv = np.asarray(M, np.float64).reshape(3, 3) if m_is_inverse else invert3x3(M)
    sx, sy, _, _ = window(dsize, Minv)
    inl = (sx >= 0) & (sx < max(w - 3, 0)) & (sy >= 0) & (sy < max(h - 3, 0))
    all_out = (sx >= w) | (sx + 4 <= 0) | (sy >= h) | (sy + 4 <= 0)
    written = inl | ((sx + 1 >= 0) & (sx + 1 < w) & (sy + 1 >= 0) & (sy + 1 < h))
    return inl, ~inl & ~all_out, all_out, written


def _index(p, n, mode):
    u, inv = np.unique(p, return_inverse=True)
    return np.array([border_interpolate(int(v), n, mode) for v in u], dtype=np.int64)[inv].reshape(p.shape)


def warp(src, M, dsize, mode=CONSTANT, m_is_inverse=False, border_value=0.0, canvas=None):
    """cv2.warpPerspective(src, M, dsize, flags=INTER_CUBIC, borderMode=mode, borderValue=border_value) on a (H, W) or (H, W, C)
    uint8 / float32 image.  TRANSPARENT writes into a copy of `canvas` (zeros when None) and returns it."""
    src = np.asarray(src)
    squeeze = src.ndim == 2
    s3 = src[:, :, None] if squeeze else src
    h, w, c = s3.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    Minv = np.asarray(M, np.float64).reshape(3, 3) if m_is_inverse else invert3x3(M)
    sx, sy, fx, fy = window((dw, dh), Minv)
    inl, _, all_out, written = classes((h, w), Minv, (dw, dh), m_is_inverse=True)
    is_u8 = s3.dtype == np.uint8
    bv = np.broadcast_to(np.asarray(border_value, np.float64), (c,)) if mode == CONSTANT else np.zeros(c)
    if is_u8:
        cv = np.clip(np.rint(bv), 0, 255).astype(np.int64)
        W = fixed_table()[fy, fx].astype(np.int64)  # (dh, dw, 16)
        S = s3.astype(np.int64)
        one = np.int64(32768)
    else:
        cv = bv.astype(F)
        W = float_table()[fy, fx]
        S = s3
        one = F(1)
    mode1 = REFLECT_101 if mode == TRANSPARENT else mode
    xs = [_index(sx + j, w, mode1) for j in range(4)]
    ys = [_index(sy + i, h, mode1) for i in range(4)]

    def tap(i, j):  # the source values (dh, dw, c) at the remapped tap; garbage where the index is -1 (masked by the caller)
        return S[np.clip(ys[i], 0, h - 1), np.clip(xs[j], 0, w - 1)]

    with np.errstate(all="ignore"):
        # step 4, every pixel: sum = cv * ONE, then one tap at a time
        gen = np.broadcast_to(cv[None, None, :] * one, (dh, dw, c)).astype(S.dtype)
        for i in range(4):
            for j in range(4):
                ok = ((ys[i] >= 0) & (xs[j] >= 0))[..., None]
                t = gen + (tap(i, j) - cv[None, None, :]) * W[..., 4 * i + j, None]
                gen = np.where(ok, t, gen)
        # step 1, inliers: row sums, then the rows
        rows = []
        for i in range(4):
            yy = np.clip(sy + i, 0, h - 1)

            def at(j):
                return S[yy, np.clip(sx + j, 0, w - 1)] * W[..., 4 * i + j, None]
            rows.append(((at(0) + at(1)) + at(2)) + at(3))
        inlier_sum = ((rows[0] + rows[1]) + rows[2]) + rows[3]
    assert gen.dtype == S.dtype and inlier_sum.dtype == S.dtype
    out = np.where(inl[..., None], inlier_sum, gen)
    if is_u8:
        out = np.clip((out + 16384) >> 15, 0, 255)
    if mode == CONSTANT:
        out = np.where((all_out & ~inl)[..., None], cv[None, None, :], out)
    out = out.astype(s3.dtype)
    if mode == TRANSPARENT:
        base = np.zeros((dh, dw, c), s3.dtype) if canvas is None else np.array(canvas, dtype=s3.dtype).reshape(dh, dw, c)
        out = np.where(written[..., None], out, base)
    return out[:, :, 0] if squeeze else out


def written_mask(src_hw, M, dsize, m_is_inverse=False):
    """(dst_h, dst_w) bool: the pixels a TRANSPARENT cubic warp writes."""
    return classes(src_hw, M, dsize, m_is_inverse)[3]
