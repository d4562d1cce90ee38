"""The reference of the warps into NV12 (bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12; bev_amd.warp.warp_perspective_to_nv12,
warp_nv12_to_nv12) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/nv12_ref.py.

bgr_to_nv12        OpenCV's 8-bit RGB -> YUV 4:2:0 two-plane conversion (BT.601, limited range, 20-bit fixed point) in numpy int32: the
                   formula of include/bevwarp.h, restated from memory like the rest of the warp (parity with OpenCV is unpinned).  A (U, V)
                   pair is that of the pixel at the even column and even row of its 2 x 2 block: nothing is averaged.
warp_to_nv12       the definition: bgr_to_nv12 of oracle.cpu_oracle.warp_perspective
warp_nv12_to_nv12  the definition: bgr_to_nv12 of tests.nv12_ref.warp_nv12
"""
import numpy as np

from oracle import cpu_oracle
from tests import nv12_ref

# rows Y, U, V; columns R, G, B
COEF = ((269484, 528482, 102760), (-155188, -305135, 460324), (460324, -385875, -74448))
OFFSET = (16, 128, 128)
SHIFT, ROUND = 20, 1 << 19


def sums(R, G, B):
    """The three sums before the shift, in int64 (so that the caller can check that int32 holds them): (Y, U, V)."""
    R, G, B = (np.asarray(v, np.int64) for v in (R, G, B))
    return tuple(c[0] * R + c[1] * G + c[2] * B + (o << SHIFT) + ROUND for c, o in zip(COEF, OFFSET))


def yuv(R, G, B):
    """Arrays of R, G, B bytes -> (Y, U, V) uint8 arrays; int32 arithmetic, arithmetic >>, no clamp (none is live)."""
    R, G, B = (np.asarray(v).astype(np.int32) for v in (R, G, B))
    out = []
    for c, o in zip(COEF, OFFSET):
        s = np.int32(c[0]) * R + np.int32(c[1]) * G + np.int32(c[2]) * B + np.int32((o << SHIFT) + ROUND)
        assert s.dtype == np.int32
        v = s >> SHIFT
        assert v.min() >= 0 and v.max() <= 255
        out.append(v.astype(np.uint8))
    return tuple(out)


def bgr_to_nv12(img, rgb=False):
    """img (H, W, 3) uint8 with H and W even, its pixels B, G, R (rgb: R, G, B) -> (y (H, W), uv (H / 2, W / 2, 2))."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0, (img.shape, img.dtype)
    r, g, b = (img[..., 0], img[..., 1], img[..., 2]) if rgb else (img[..., 2], img[..., 1], img[..., 0])
    y, _, _ = yuv(r, g, b)
    _, u, v = yuv(r[0::2, 0::2], g[0::2, 0::2], b[0::2, 0::2])
    return y, np.stack([u, v], axis=-1)


def warp_to_nv12(src, M, dsize, interp=cpu_oracle.LINEAR, border_value=None, rgb=False, m_is_inverse=False, nthreads=1):
    """BGR -> NV12 of bevwarp_warp's result.  border_value is in the source pixel's channel order and is converted with the pixels."""
    return bgr_to_nv12(cpu_oracle.warp_perspective(src, M, dsize, interp, m_is_inverse=m_is_inverse, border_value=border_value, nthreads=nthreads), rgb)


def warp_nv12_to_nv12(y, uv, M, dsize, interp=cpu_oracle.LINEAR, border_value=None, m_is_inverse=False, nthreads=1):
    """BGR -> NV12 of bevwarp_warp_nv12's result (B, G, R order; border_value in that order)."""
    return bgr_to_nv12(nv12_ref.warp_nv12(y, uv, M, dsize, interp, border_value=border_value, rgb=False, m_is_inverse=m_is_inverse, nthreads=nthreads))
