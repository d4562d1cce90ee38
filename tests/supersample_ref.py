"""Numpy reference of the supersampled warp (bev_amd.warp.warp_perspective_supersampled, include/bevwarp.h BEVWARP_SUPERSAMPLE_*) -- TEST
INFRASTRUCTURE ONLY, a plain module like tests/border_ref.py.

By composition only: tests/border_ref.warp on the k times finer grid with the fine matrix, then the box reduce the header states -- 8-bit
(sum + k^2 / 2) >> 2 log2 k, float32 one rounded addition per sub-sample, rows outermost, then one multiply by 1 / k^2.
"""
import numpy as np

from oracle import warp_numpy as wn
from tests import border_ref as BR

FACTORS = (2, 4, 8)
FIELD = {1: 0, 2: 0x1000, 4: 0x2000, 8: 0x3000}  # BEVWARP_SUPERSAMPLE_*: the field of the ABI's interp word
MODES = (BR.CONSTANT, BR.REPLICATE, BR.REFLECT, BR.WRAP, BR.REFLECT_101)  # the borders that write every pixel


def fine_matrix(Minv, k):
    """F of the header: one correctly rounded float64 operation per line, no FMA (numpy has none)."""
    M = np.asarray(Minv, np.float64).reshape(3, 3)
    kd = np.float64(k)
    c = np.float64(1 - k) / np.float64(2 * k)
    F = np.empty((3, 3), np.float64)
    with np.errstate(all="ignore"):
        for r in range(3):
            F[r, 0] = M[r, 0] / kd
            F[r, 1] = M[r, 1] / kd
            a = M[r, 0] * c
            b = M[r, 1] * c
            F[r, 2] = (a + b) + M[r, 2]
    return F


def box_reduce(fine, k):
    """(k dh, k dw, C) -> (dh, dw, C): the reduce of the header, in its order."""
    kh, kw, c = fine.shape
    dh, dw = kh // k, kw // k
    cells = fine.reshape(dh, k, dw, k, c)  # [y, j, x, i]
    if fine.dtype == np.uint8:
        s = cells.astype(np.int64).sum(axis=(1, 3))
        return ((s + (k * k) // 2) >> (2 * int(np.log2(k)))).astype(np.uint8)
    acc = None
    with np.errstate(all="ignore"):
        for j in range(k):
            for i in range(k):
                s = cells[:, j, :, i].astype(np.float32)
                acc = s.copy() if acc is None else (acc + s).astype(np.float32)
        return (acc * np.float32(1.0 / (k * k))).astype(np.float32)


def warp(src, M, dsize, k, interp=wn.LINEAR, mode=BR.CONSTANT, m_is_inverse=False, border_value=0.0):
    """The supersampled warp of a (H, W) or (H, W, C) uint8 / float32 image; k = 1 is border_ref.warp."""
    dw, dh = int(dsize[0]), int(dsize[1])
    Minv = np.asarray(M, np.float64).reshape(3, 3) if m_is_inverse else wn.invert3x3(M)
    if k == 1:
        return BR.warp(src, Minv, (dw, dh), interp, mode, m_is_inverse=True, border_value=border_value)
    assert k in FACTORS and mode in MODES, (k, mode)
    fine = BR.warp(src, fine_matrix(Minv, k), (k * dw, k * dh), interp, mode, m_is_inverse=True, border_value=border_value)
    squeeze = fine.ndim == 2
    out = box_reduce(fine[:, :, None] if squeeze else fine, k)
    return out[:, :, 0] if squeeze else out


def block_width(w, h):
    """The evaluation block width of a w x h grid (bev_amd/csrc/host_plan.h, block_width)."""
    return min(1024 // min(16, h), w)


def assert_same(got, want, err_msg=""):
    """Bit equality with NaNs compared as NaNs (a NaN's payload is not part of the definition)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype, err_msg)
    if got.dtype == np.float32:
        gn, wn_ = np.isnan(got), np.isnan(want)
        np.testing.assert_array_equal(gn, wn_, err_msg=err_msg)
        np.testing.assert_array_equal(np.where(gn, np.float32(0), got).view(np.uint32), np.where(wn_, np.float32(0), want).view(np.uint32), err_msg=err_msg)
    else:
        np.testing.assert_array_equal(got, want, err_msg=err_msg)
