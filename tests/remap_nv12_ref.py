"""Numpy definition of the NV12 map sampler (bev_amd.warp.remap_nv12 / remap_nv12_to_planar, include/bevwarp.h bevwarp_remap_nv12 /
bevwarp_remap_nv12_planes) -- TEST INFRASTRUCTURE ONLY, a plain module like tests/remap_ref.py.

Nothing is defined here that is not defined elsewhere: the pixels are tests/remap_ref.remap of tests/nv12_ref.nv12_to_bgr's converted
frame, the planes are tests/planes16_ref's plane stage (float32 multiply, then add, each rounded; to_bits for the 16-bit types) applied
to them."""
import numpy as np

from tests import nv12_ref as NR
from tests import planes16_ref as P16
from tests import remap_ref as RR


def remap_nv12(y, uv, xy, frac, interp, mode=RR.CONSTANT, border_value=0.0, canvas=None, rgb=False):
    """(dh, dw, 3) uint8.  border_value is in the result's channel order and is not converted; TRANSPARENT writes into a copy of canvas."""
    return RR.remap(NR.nv12_to_bgr(y, uv, rgb), xy, frac, interp, mode, border_value, canvas)


def planes_f32(pixels, scale, bias):
    """(3, dh, dw) float32 of (dh, dw, 3) uint8 pixels: float32(p) * float32(scale[c]) + float32(bias[c]), multiply then add, each rounded
    (planes16_ref.planes_f32's stage)."""
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (3,)).astype(np.float32)[:, None, None]
    bi = np.broadcast_to(np.asarray(bias, dtype=np.float64), (3,)).astype(np.float32)[:, None, None]
    with np.errstate(all="ignore"):
        out = pixels.transpose(2, 0, 1).astype(np.float32) * sc + bi
    assert out.dtype == np.float32
    return out


def remap_nv12_planes(y, uv, xy, frac, interp, mode, scale, bias, border_value=0.0, rgb=False):
    """(3, dh, dw) float32: the plane stage applied to remap_nv12 (the five modes that write every pixel)."""
    assert mode != RR.TRANSPARENT
    return planes_f32(remap_nv12(y, uv, xy, frac, interp, mode, border_value, rgb=rgb), scale, bias)


def assert_planes_equal(got, exp_f32, dtype, what=""):
    """A device result (torch tensor of float32 / float16 / bfloat16 planes) against float32 expected planes, by bits."""
    name = str(dtype).replace("torch.", "")
    if name == "float32":
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(exp_f32).view(np.uint32), err_msg=what)
    else:
        P16.assert_same16(P16.gpu_bits(got), P16.to_bits(exp_f32, dtype), dtype, what)
