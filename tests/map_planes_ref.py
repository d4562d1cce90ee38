"""Numpy definition of the map samplers that write channel planes (bev_amd.warp.remap_to_planar / remap_stitch_to_planar /
remap_stitch_nv12_to_planar; include/bevwarp.h bevwarp_remap_planes, bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes) -- TEST
INFRASTRUCTURE ONLY, a plain module like tests/remap_nv12_out_ref.py.

By composition only: every function is tests/remap_nv12_ref.planes_f32 (float32 multiply, then add, each rounded) of a definition that
exists.  Each returns the (3, dh, dw) float32 planes of one frame; a 16-bit result is planes16_ref.to_bits of them, which
remap_nv12_ref.assert_planes_equal applies.  border_value is an 8-bit pixel in the planes' channel order and passes through the plane
stage like any other pixel."""
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM


def remap_planes(src, xy, frac, interp, mode, scale, bias, border_value=0.0):
    assert mode != RR.TRANSPARENT
    return RN.planes_f32(RR.remap(src, xy, frac, interp, mode, border_value), scale, bias)


def stitch_planes(srcs, maps, interp, scale, bias, blend=SM.OVER, feather=64, border_value=0.0):
    return RN.planes_f32(SM.stitch(srcs, maps, interp, blend, feather, SM.CONSTANT, border_value)[0], scale, bias)


def stitch_nv12_planes(ys, uvs, maps, interp, scale, bias, blend=SM.OVER, feather=64, border_value=0.0, rgb=False):
    return RN.planes_f32(SM.stitch_nv12(ys, uvs, maps, interp, blend, feather, SM.CONSTANT, border_value, rgb=rgb)[0], scale, bias)
