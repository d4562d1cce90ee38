"""Numpy definition of the stitches through warp maps under BEVWARP_STITCH_GAIN (bev_amd.warp.remap_stitch*(..., gains=); include/bevwarp.h)
-- TEST INFRASTRUCTURE ONLY, a plain module like tests/map_planes_ref.py.

By composition only: the gained entry is the plain definition (tests/stitch_maps_ref.stitch) of frames put through `apply_gain`
beforehand -- NV12 frames: of the converted frames (tests/nv12_ref.nv12_to_bgr) -- and the NV12 and plane destinations are
tests/nv12_out_ref.bgr_to_nv12 and tests/remap_nv12_ref.planes_f32 of that canvas, as tests/remap_nv12_out_ref.py and
tests/map_planes_ref.py have them.  G is an integer array (n_cams, 3) of Q8 gains, 0..1023: channel c is channel c of the pixel the sampler
blends.  The border pixel is not gained."""
import numpy as np

from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import remap_nv12_ref as RN
from tests import stitch_maps_ref as SM


def gain(p, G):
    """min(255, (p * G + 128) >> 8) on integers (arrays broadcast)."""
    return np.minimum(255, (np.asarray(p, np.int64) * np.asarray(G, np.int64) + 128) >> 8)


def quantize(gains, n_cams):
    """rint(256 g) as an int64 array (n_cams, 3), from (n_cams,) or (n_cams, 3) floats."""
    g = np.rint(256.0 * np.asarray(gains, np.float64)).astype(np.int64)
    return np.ascontiguousarray(np.broadcast_to(g[:, None] if g.ndim == 1 else g, (n_cams, 3)))


def word(G3):
    return int(G3[0]) | int(G3[1]) << 10 | int(G3[2]) << 20


def apply_gain(frame, G3):
    """One camera's (..., 3) uint8 frames with channel c put through gain(., G3[c])."""
    assert frame.dtype == np.uint8 and frame.shape[-1] == 3
    return gain(frame, np.asarray(G3).reshape(3)).astype(np.uint8)


def stitch(srcs, G, maps, interp=SM.LINEAR, blend=SM.OVER, feather=64, mode=SM.CONSTANT, border_value=0.0, canvas=None):
    return SM.stitch([apply_gain(s, g) for s, g in zip(srcs, G)], maps, interp, blend, feather, mode, border_value, canvas)


def stitch_nv12(ys, uvs, G, maps, interp=SM.LINEAR, blend=SM.OVER, feather=64, mode=SM.CONSTANT, border_value=0.0, canvas=None, rgb=False):
    return stitch([NR.nv12_to_bgr(y, uv, rgb) for y, uv in zip(ys, uvs)], G, maps, interp, blend, feather, mode, border_value, canvas)


def stitch_to_nv12(srcs, G, maps, interp, blend=SM.OVER, feather=64, border_value=0.0, rgb=False):
    return NO.bgr_to_nv12(stitch(srcs, G, maps, interp, blend, feather, SM.CONSTANT, border_value)[0], rgb)


def stitch_nv12_to_nv12(ys, uvs, G, maps, interp, blend=SM.OVER, feather=64, border_value=0.0):
    return NO.bgr_to_nv12(stitch_nv12(ys, uvs, G, maps, interp, blend, feather, SM.CONSTANT, border_value, rgb=False)[0])


def stitch_planes(srcs, G, maps, interp, scale, bias, blend=SM.OVER, feather=64, border_value=0.0):
    return RN.planes_f32(stitch(srcs, G, maps, interp, blend, feather, SM.CONSTANT, border_value)[0], scale, bias)


def stitch_nv12_planes(ys, uvs, G, maps, interp, scale, bias, blend=SM.OVER, feather=64, border_value=0.0, rgb=False):
    return RN.planes_f32(stitch_nv12(ys, uvs, G, maps, interp, blend, feather, SM.CONSTANT, border_value, rgb=rgb)[0], scale, bias)


def overlap_stats(bevs, masks):
    """bev_amd.exposure.overlap_stats' numpy twin, from every camera's BEV ((B, dh, dw, 3) uint8) and cover mask ((B, dh, dw) bool):
    int64 N (n, n) and S (n, n, 3)."""
    n = len(bevs)
    N, S = np.zeros((n, n), np.int64), np.zeros((n, n, 3), np.int64)
    for i in range(n):
        for j in range(n):
            both = masks[i] & masks[j]
            N[i, j] = both.sum()
            S[i, j] = bevs[i].astype(np.int64)[both].sum(axis=0)
    return N, S
