"""Numpy definition of the map samplers that write NV12 (bev_amd.warp.remap_to_nv12 / remap_nv12_to_nv12 / remap_stitch_to_nv12 /
remap_stitch_nv12_to_nv12; include/bevwarp.h bevwarp_remap_to_nv12, bevwarp_remap_nv12_to_nv12, bevwarp_stitch_maps_to_nv12,
bevwarp_stitch_maps_nv12_to_nv12) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/remap_nv12_ref.py.

By composition only: every function is tests/nv12_out_ref.bgr_to_nv12 of a definition that exists.  Each returns (y (dh, dw),
uv (dh / 2, dw / 2, 2)) of one frame; border_value is a pixel in the sampled frame's channel order and is converted with the pixels."""
from tests import nv12_out_ref as NO
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM


def remap_to_nv12(src, xy, frac, interp, mode=RR.CONSTANT, border_value=0.0, rgb=False):
    assert mode != RR.TRANSPARENT
    return NO.bgr_to_nv12(RR.remap(src, xy, frac, interp, mode, border_value), rgb)


def remap_nv12_to_nv12(y, uv, xy, frac, interp, mode=RR.CONSTANT, border_value=0.0):
    assert mode != RR.TRANSPARENT
    return NO.bgr_to_nv12(RN.remap_nv12(y, uv, xy, frac, interp, mode, border_value, rgb=False))


def stitch_to_nv12(srcs, maps, interp, blend=SM.OVER, feather=64, border_value=0.0, rgb=False):
    return NO.bgr_to_nv12(SM.stitch(srcs, maps, interp, blend, feather, SM.CONSTANT, border_value)[0], rgb)


def stitch_nv12_to_nv12(ys, uvs, maps, interp, blend=SM.OVER, feather=64, border_value=0.0):
    return NO.bgr_to_nv12(SM.stitch_nv12(ys, uvs, maps, interp, blend, feather, SM.CONSTANT, border_value, rgb=False)[0])
