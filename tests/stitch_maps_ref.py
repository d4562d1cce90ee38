"""Numpy definition of the multi-camera stitch through warp maps (bev_amd.warp.remap_stitch / remap_stitch_nv12, include/bevwarp.h
bevwarp_stitch_maps / bevwarp_stitch_maps_nv12) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/stitch_ref.py.

Composed from what is defined elsewhere: a camera's cover mask is remap_ref.written of its map, its pixel p_k is remap_ref.remap(...,
TRANSPARENT), its edge distance d_k is stitch_ref.edge_distance of the map entry.  What this module restates is the definition's camera
loop and the two blends (OVER: the covering camera with the largest k; FEATHER: integer weights min(d_k, F), int64 sums for 8-bit pixels,
float32 accumulation in ascending k and one float32 division for float32 pixels, the single-cover rule) and the two rules for uncovered
pixels.  The NV12 entry is the same over nv12_ref's converted frames."""
import numpy as np

from oracle.warp_numpy import LINEAR
from tests import nv12_ref as NR
from tests import remap_ref as RR
from tests import stitch_ref as SR

OVER, FEATHER = SR.OVER, SR.FEATHER
CONSTANT, TRANSPARENT = RR.CONSTANT, RR.TRANSPARENT


def cameras(srcs, maps, interp, feather):
    """Per camera (cover mask, p_k as (dh, dw, C), integer weight w_k -- 0 where the camera does not cover).  maps: (xy, frac) per camera."""
    out = []
    for src, (xy, frac) in zip(srcs, maps):
        src = np.asarray(src)
        h, w = src.shape[:2]
        dh, dw = xy.shape[:2]
        cover = RR.written(xy, w, h, interp)
        p = RR.remap(src, xy, frac, interp, RR.TRANSPARENT).reshape(dh, dw, -1)
        sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
        wk = np.where(cover, np.minimum(SR.edge_distance(sx, sy, w, h), int(feather)), 0).astype(np.int64)
        assert (wk[cover] >= 1).all()
        out.append((cover, p, wk))
    return out


def stitch(srcs, maps, interp=LINEAR, blend=OVER, feather=64, mode=CONSTANT, border_value=0.0, canvas=None):
    """(result, cover count) of bevwarp_stitch_maps on one frame: srcs a list of (H_k, W_k) or (H_k, W_k, C) uint8 / float32 images, maps
    their (xy, frac) pairs, all of one (dh, dw).  mode CONSTANT: uncovered pixels are border_value; TRANSPARENT: they keep `canvas`
    (zeros when None)."""
    srcs = [np.asarray(s) for s in srcs]
    dtype = srcs[0].dtype
    squeeze = srcs[0].ndim == 2
    c = 1 if squeeze else srcs[0].shape[2]
    dh, dw = maps[0][0].shape[:2]
    cams = cameras(srcs, maps, interp, feather)
    count = sum(cover.astype(np.int64) for cover, _, _ in cams)
    if mode == CONSTANT:
        bv = np.broadcast_to(np.asarray(border_value, np.float64), (c,))
        cval = np.clip(np.rint(bv), 0, 255).astype(np.uint8) if dtype == np.uint8 else bv.astype(np.float32)
        out = np.broadcast_to(cval, (dh, dw, c)).astype(dtype)
    else:
        out = np.zeros((dh, dw, c), dtype) if canvas is None else np.array(canvas, dtype=dtype).reshape(dh, dw, c)
    for cover, p, _ in cams:  # OVER; under FEATHER what this leaves where one camera covers is that camera's pixel
        out = np.where(cover[..., None], p, out)
    if blend == FEATHER:
        W = sum(wk for _, _, wk in cams)
        many = count >= 2
        Ws = np.where(many, W, 1)  # (no division by zero where nothing is divided)
        if dtype == np.uint8:
            num = sum(wk[..., None] * p.astype(np.int64) for _, p, wk in cams)
            assert num.max() < 1 << 23
            mean = (num + (Ws >> 1)[..., None]) // Ws[..., None]
            assert mean[many].max(initial=0) <= 255
        else:
            acc = np.zeros((dh, dw, c), np.float32)
            with np.errstate(all="ignore"):
                for cover, p, wk in cams:  # ascending k; each multiply and each add rounds to float32
                    prod = (wk.astype(np.float32)[..., None] * p).astype(np.float32)
                    acc = np.where(cover[..., None], (acc + prod).astype(np.float32), acc)
                mean = (acc / Ws.astype(np.float32)[..., None]).astype(np.float32)
        out = np.where(many[..., None], mean, out).astype(dtype)
    return (out[:, :, 0] if squeeze else out), count


def stitch_nv12(ys, uvs, maps, interp=LINEAR, blend=OVER, feather=64, mode=CONSTANT, border_value=0.0, canvas=None, rgb=False):
    """bevwarp_stitch_maps_nv12 on one frame: stitch() of the converted frames.  border_value is in the result's order, not converted."""
    return stitch([NR.nv12_to_bgr(y, uv, rgb) for y, uv in zip(ys, uvs)], maps, interp, blend, feather, mode, border_value, canvas)
