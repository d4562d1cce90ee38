"""The map samplers that write channel planes (bevwarp_remap_planes, bevwarp_stitch_maps_planes, bevwarp_stitch_maps_nv12_planes;
remap_to_planar, remap_stitch_to_planar, remap_stitch_nv12_to_planar; SitePipeline) without a device: the numpy definition
(tests/map_planes_ref.py) tied to existing definitions by bits, what an invalid map entry gives, the C ABI's host checks under the
sanitizers (tests/host_plan_driver.cpp, family `map_planes`) and the same statuses, in their documented order, through the built library, the ABI
surface, the refusals of the Python entries and of SitePipeline, and the code objects of the two kernel units."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import codeobj
from tests import hostplan
from tests import map_planes_ref as MP
from tests import nv12_ref as NR
from tests import planes16_ref as P16
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests.test_abi import checked_declaration
from tests.test_lens_cpu import GEOMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
NAMES = ("bevwarp_remap_planes", "bevwarp_stitch_maps_planes", "bevwarp_stitch_maps_nv12_planes")
BORDER = (7.0, 200.0, 31.0)
SCALE, BIAS = (1.0 / 255.0, 0.017, 2.5), (-0.485, 0.25, 3.0)
F32, F16, BF16 = _lib.F32, _lib.F16, _lib.BF16


# ---- the definition tied to existing ones, by bits ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_definition_is_tied_to_existing_ones(geom, interp):
    sw, sh, dw, dh, M = GEOMS[geom]
    xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
    y, uv = NR.frame("uniform", 3, sh, sw)
    bgr = NR.nv12_to_bgr(y, uv)
    # with a pinhole map and CONSTANT it is planes16_ref.planes_f32 of the matrix warp
    for bv in (None, BORDER):
        got = MP.remap_planes(bgr, xy, frac, interp, RR.CONSTANT, SCALE, BIAS, 0.0 if bv is None else bv)
        np.testing.assert_array_equal(got.view(np.uint32), P16.planes_f32(bgr, M, (dw, dh), interp, SCALE, BIAS, bv).view(np.uint32))
    # one camera under the stitch is the single-camera definition under CONSTANT where the camera covers, and the border pixel's planes elsewhere
    cover = RR.written(xy, sw, sh, interp)
    assert cover.any() and not cover.all()
    for blend in (SM.OVER, SM.FEATHER):
        st = MP.stitch_planes([bgr], [(xy, frac)], interp, SCALE, BIAS, blend, 3, BORDER)
        one = MP.remap_planes(bgr, xy, frac, interp, RR.CONSTANT, SCALE, BIAS, BORDER)
        np.testing.assert_array_equal(st[:, cover].view(np.uint32), one[:, cover].view(np.uint32))
        edge = RN.planes_f32(np.array(BORDER, np.uint8).reshape(1, 1, 3), SCALE, BIAS)[:, 0, 0]
        assert (st[:, ~cover].view(np.uint32) == edge.view(np.uint32)[:, None]).all()
    # the NV12 stitch is the interleaved stitch on nv12_ref.nv12_to_bgr's frames
    y2, uv2 = NR.frame("uniform", 5, sh, sw)
    xy2, frac2 = RR.build((dw, dh), wn.invert3x3(M) @ np.array([[1.0, 0.0, 9.0], [0.0, 1.0, -5.0], [0.0, 0.0, 1.0]]), None, INF, interp)
    maps = [(xy, frac), (xy2, frac2)]
    for rgb in (False, True):
        for blend in (SM.OVER, SM.FEATHER):
            got = MP.stitch_nv12_planes([y, y2], [uv, uv2], maps, interp, SCALE, BIAS, blend, 3, BORDER, rgb=rgb)
            exp = MP.stitch_planes([NR.nv12_to_bgr(y, uv, rgb), NR.nv12_to_bgr(y2, uv2, rgb)], maps, interp, SCALE, BIAS, blend, 3, BORDER)
            np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_invalid_entries_give_the_converted_border_pixel(interp):
    """The sentinel (-32768, -32768) yields the 8-bit border pixel put through the plane stage; a float16 scale of 300 takes 255 to +inf."""
    sw, sh, dw, dh = 8, 6, 8, 4
    gx, gy = np.meshgrid(np.arange(dw, dtype=np.int16), np.arange(dh, dtype=np.int16))
    xy = np.stack([gx, gy], axis=-1)
    frac = None if interp == wn.NEAREST else np.zeros((dh, dw), np.uint16)
    holes = [(0, 2), (1, 4), (2, 7), (3, 3)]
    for r, c in holes:
        xy[r, c] = (RR.SENTINEL, RR.SENTINEL)
    y, uv = NR.frame("uniform", 9, sh, sw)
    bgr = NR.nv12_to_bgr(y, uv)
    border = (7.4, 255.0, 300.0)  # (saturate_cast: 7, 255, 255)
    want = (np.array([7, 255, 255], np.float32) * np.array(SCALE, np.float32) + np.array(BIAS, np.float32)).astype(np.float32)
    for name, got in (("remap", MP.remap_planes(bgr, xy, frac, interp, RR.CONSTANT, SCALE, BIAS, border)),
                      ("stitch", MP.stitch_planes([bgr], [(xy, frac)], interp, SCALE, BIAS, SM.FEATHER, 3, border)),
                      ("stitch nv12", MP.stitch_nv12_planes([y], [uv], [(xy, frac)], interp, SCALE, BIAS, SM.OVER, 64, border))):
        for r, c in holes:
            assert got[:, r, c].view(np.uint32).tolist() == want.view(np.uint32).tolist(), (name, r, c)
    got = MP.remap_planes(bgr, xy, frac, interp, RR.CONSTANT, (1.0, 300.0, 1.0), 0.0, border)
    bits = P16.to_bits(got, torch.float16)
    assert bits[1, 0, 2] == 0x7c00 and not P16.is_nan16(bits, torch.float16).any()   # 255 * 300 = 76500 > 65520: +inf, and no NaN anywhere


# ---- the host checks: one table of cases, run under the sanitizers and through the built library ----

D, XY, FR = 1 << 20, 1 << 24, 1 << 26
# an 8 x 8 B, G, R source at 4096 and three 8 x 8 planes at 2^20 (float32: rows of 32 bytes, planes 256 and frames 768 apart; 16-bit: half of
# each); one shared bilinear map at 2^24 and 2^26; never dereferenced
KEYS = ("src", "dst", "xy", "frac", "batch", "src_h", "src_w", "dst_h", "dst_w", "src_fs", "src_rs", "dst_fs", "dst_ps", "dst_rs", "map_count", "xy_fs", "xy_rs",
        "frac_fs", "frac_rs", "interp", "mode", "pdt")
P32 = dict(src=4096, dst=D, xy=XY, frac=FR, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, src_fs=192, src_rs=24, dst_fs=768, dst_ps=256, dst_rs=32, map_count=1,
           xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16, interp=1, mode=0, pdt=F32)
P16B = dict(P32, dst_fs=384, dst_ps=128, dst_rs=16, pdt=F16)
NONE = [0, 0, 0]
HUGE = (1 << 63) - 1


def _single_cases():
    """[(arguments, [check_call's status, plan_remap's status, frames per item, items])]"""
    out = []
    ok = [OK, OK, 1, 2]

    def case(want, _base=P32, **kw):
        out.append((dict(_base, **kw), want if isinstance(want, list) else [want] + NONE))

    def half(want, **kw):
        case(want, _base=P16B, **kw)

    case(ok), case(ok, interp=0), case(ok, interp=0, frac=0), case([OK] + NONE, batch=0), case(BAD_ARG, batch=0, map_count=7), half(ok), half(ok, pdt=BF16)
    # 1. BEVWARP_ERR_BAD_ARG: null pointers (the frac plane under bilinear only), sizes
    for k in ("src", "dst", "xy", "frac", "src_h", "src_w", "dst_h", "dst_w"):
        case(BAD_ARG, **{k: 0})
    case(BAD_ARG, xy=0, interp=0), case(BAD_ARG, batch=-1), case(ok, dst_w=7, dst_h=7, src_h=7, src_w=7, src_rs=21)
    # 2. BEVWARP_ERR_UNSUPPORTED: the interpolation, the five borders that write every pixel, the plane type -- bevwarp_remap's order: after
    #    the null pointers and the sides, before the map count, the layouts, the size limits and the overlap
    for i in (2, 3, -1):
        case(UNSUPPORTED, interp=i)
    for m in (5, 6, 16, -1):
        case(UNSUPPORTED, mode=m)
    for m in range(5):
        case(ok, mode=m), case(ok, mode=m, interp=0), half(ok, mode=m)
    for p in (_lib.U8, _lib.F64, 5, -1):
        case(UNSUPPORTED, pdt=p), half(UNSUPPORTED, pdt=p)
    case(UNSUPPORTED, interp=2, frac=0), case(UNSUPPORTED, interp=2, map_count=2), case(UNSUPPORTED, mode=5, xy_rs=28), case(UNSUPPORTED, pdt=0, dst_rs=3)
    case(UNSUPPORTED, mode=5, src_w=32768, src_rs=3 * 32768), case(UNSUPPORTED, interp=2, dst=4096), case(UNSUPPORTED, pdt=2, dst=D + 1)
    case(BAD_ARG, mode=5, dst_w=0), case(BAD_ARG, interp=2, src=0), case(BAD_ARG, pdt=0, dst=0)
    # 3. BEVWARP_ERR_BAD_ARG: the map count (1 or the batch), then the layouts
    three = dict(batch=3)
    case(BAD_ARG, map_count=0), case(BAD_ARG, map_count=2), case(BAD_ARG, map_count=2, **three), case([OK, OK, 1, 6], map_count=3, **three)
    case([OK, OK, 1, 6], map_count=1, xy_fs=1, frac_fs=1, **three), case(BAD_ARG, map_count=3, xy_fs=255, **three)
    case(BAD_ARG, src_rs=23), case(BAD_ARG, batch=2, src_fs=191), case(BAD_ARG, xy=XY + 2), case(BAD_ARG, xy_rs=28), case(BAD_ARG, frac=FR + 1), case(BAD_ARG, frac_rs=14)
    case(ok, xy=XY + 4, frac=FR + 2), case(ok, frac=FR + 1, frac_rs=3, interp=0)
    # ... the destination: rows in a plane, planes in a frame, frames in the batch; base and strides off the element size
    case(BAD_ARG, dst_rs=31), case(BAD_ARG, dst_rs=28), case(BAD_ARG, dst_ps=255), case(BAD_ARG, dst_ps=252), case(ok, dst_ps=260), case(ok, dst_rs=36, dst_ps=288)
    case(BAD_ARG, batch=2, dst_fs=767), case(BAD_ARG, batch=2, dst_fs=764), case(BAD_ARG, batch=2, dst_ps=260), case([OK, OK, 1, 4], batch=2, dst_ps=260, dst_fs=780)
    case(BAD_ARG, dst=D + 2), case(BAD_ARG, dst=D + 1), case(BAD_ARG, dst_rs=34), case(BAD_ARG, dst_ps=258), case(BAD_ARG, dst_fs=770), case(ok, dst=D + 4, dst_fs=772)
    half(ok, dst=D + 2), half(BAD_ARG, dst=D + 1), half(ok, dst_rs=18, dst_ps=144), half(BAD_ARG, dst_rs=17, dst_ps=144), half(ok, dst_ps=130), half(BAD_ARG, dst_ps=129)
    half(ok, dst_fs=386), half(BAD_ARG, dst_fs=385), half(BAD_ARG, dst_rs=15), half(BAD_ARG, dst_ps=127)
    # 4. BEVWARP_ERR_TOO_LARGE for the source, before the overlap; the maps have no such limit
    wide_w = dict(src_w=32768, src_rs=3 * 32768)
    case(TOO_LARGE, **wide_w), case(TOO_LARGE, src_h=32768), case(TOO_LARGE, src_rs=1 << 24), case(TOO_LARGE, dst=4096, **wide_w), case(ok, xy_rs=1 << 24, frac_rs=1 << 24)
    # 5. BEVWARP_ERR_OVERLAP: the bounding byte range of all planes over each image the call reads
    case(OVERLAP, dst=4096), case(OVERLAP, dst=4096 + 188), case(ok, dst=4096 + 192), case(ok, dst=4096 - 768), case(OVERLAP, dst=4096 - 764)
    case(OVERLAP, xy=D), case(OVERLAP, xy=D + 764), case(ok, xy=D + 768), case(OVERLAP, xy=D - 252), case(ok, xy=D - 256)
    case(OVERLAP, frac=D + 766), case(ok, frac=D + 768), case(OVERLAP, frac=D - 126), case(ok, frac=D - 128), case(ok, frac=D + 70, interp=0)  # (nearest: not read)
    gap = dict(dst_ps=512)  # a read image that lies wholly between two planes still meets their bounding range
    case(ok, **gap), case(OVERLAP, src=D + 256, **gap), case(OVERLAP, xy=D + 256, **gap), case(OVERLAP, frac=D + 768, **gap), case(OVERLAP, src=D + 1279, **gap)
    case(ok, src=D + 1280, **gap), half(OVERLAP, src=D + 383), half(ok, src=D + 384), half(OVERLAP, xy=D + 380), half(ok, xy=D + 384)
    case([OK, OK, 1, 4], batch=2), case(OVERLAP, batch=2, src=D + 1535), case([OK, OK, 1, 4], batch=2, src=D + 1536), case(OVERLAP, batch=2, dst_fs=1024, src=D + 1000)
    case(ok, xy=4096, frac=4096 + 64)                                             # the read images may overlap each other
    # 6. BEVWARP_ERR_TOO_LARGE from the launch plan, after the overlap; the frames-per-item plan
    tall = dict(dst_h=(1 << 20) + 2, dst=1 << 40, dst_ps=1 << 26, dst_fs=3 << 26, xy=1 << 44, frac=1 << 48)
    case([OK, TOO_LARGE, 0, 0], **tall), case(OVERLAP, **dict(tall, src=1 << 40))
    big = dict(batch=32, dst_h=1024, dst_w=1024, dst_rs=2048, dst_ps=2 << 20, dst_fs=6 << 20, dst=1 << 40, xy=1 << 44, frac=1 << 48, xy_rs=4096, xy_fs=1 << 22,
               frac_rs=2048, frac_fs=1 << 21)
    half([OK, OK, 2, 16 * 1024], map_count=1, **big), half([OK, OK, 1, 32 * 1024], map_count=32, **big)
    # strides next to 2^63: bad arguments or size limits, not overflows (the images' last bytes stay below 2^64)
    one_row, two_rows = dict(dst_h=1), dict(dst_h=2)
    case([OK, OK, 1, 1], dst=1 << 40, dst_ps=1 << 62, **one_row), case(BAD_ARG, dst=1 << 40, dst_rs=HUGE - 3, dst_ps=1 << 62, **one_row)
    case(BAD_ARG, dst_rs=HUGE - 3, dst_ps=HUGE - 3, **two_rows), case(BAD_ARG, dst_rs=HUGE, **two_rows), case(BAD_ARG, batch=3, dst_rs=HUGE - 3, dst_ps=HUGE - 3, dst_fs=HUGE - 3)
    case([OK, OK, 1, 1], xy=1 << 40, xy_rs=HUGE - 3, **two_rows), case([OK, OK, 1, 1], frac=1 << 40, frac_rs=HUGE - 1, **two_rows)
    case(BAD_ARG, batch=2, map_count=2, xy_rs=HUGE - 3, xy_fs=HUGE - 3), case(TOO_LARGE, src_rs=HUGE), case(BAD_ARG, src_rs=-1), case(BAD_ARG, dst_rs=-HUGE - 1)
    case(BAD_ARG, dst_ps=-4), case(BAD_ARG, batch=2, dst_fs=-768)
    return out


def _single_line(a):
    return "planes " + " ".join(str(a[k]) for k in KEYS)


CAM = dict(src=4096, uv=0, h=8, w=8, fs=192, rs=24, uv_fs=0, uv_rs=0, xy=XY, frac=FR, xy_fs=256, xy_rs=32, fr_fs=128, fr_rs=16, map_count=1)
NVCAM = dict(CAM, uv=8192, fs=64, rs=8, uv_fs=32, uv_rs=8)
CALL = dict(n=None, cams_null=0, dst=D, batch=1, dh=8, dw=8, dst_fs=768, dst_ps=256, dst_rs=32, interp=1, blend=0, feather=64, rgb=0, pdt=F32, border=2, scale=1, bias=1)
PASSES = NOT_FINITE  # a call that passes every check of its cameras and of the canvas ends on the NaN border value: nothing is launched


def _stitch_cases():
    """[(kind, cameras, call arguments, status)]: bevwarp_stitch_maps' table (tests/test_stitch_maps_cpu.py) for a canvas of planes."""
    out = []
    big = 2147483647
    for kind, k in (("sbgr", CAM), ("snv12", NVCAM)):
        def case(cams, want, _kind=kind, **kw):
            out.append((_kind, cams, dict(CALL, **kw), want))

        # 1. the call's own arguments: 0, 1, 8 and 9 cameras, the feather width
        case([], BAD_ARG, n=0), case([k], PASSES), case([k] * 8, PASSES), case([k] * 9, BAD_ARG), case([k], BAD_ARG, n=-1), case([k], BAD_ARG, cams_null=1)
        case([k] * 9, BAD_ARG, interp=2), case([dict(k, src=0)] * 9, BAD_ARG)
        for f, want in ((0, BAD_ARG), (1, PASSES), (4096, PASSES), (4097, BAD_ARG), (-big, BAD_ARG)):
            case([k], want, blend=1, feather=f)
        for f in (0, 4097):
            case([k], PASSES, blend=0, feather=f)  # OVER ignores it
        case([k], BAD_ARG, blend=1, feather=0, interp=2)
        # 2. per camera: the format (the blend and the plane type are part of it), null images, sides, the map count, layouts
        for bl in (2, -1):
            case([k], UNSUPPORTED, blend=bl)
        for i in (2, 3, -1):
            case([k], UNSUPPORTED, interp=i)
        for p in (_lib.U8, _lib.F64, 5, -1):
            case([k], UNSUPPORTED, pdt=p)
        half = dict(pdt=F16, dst_fs=384, dst_ps=128, dst_rs=16)
        case([k], PASSES, **half), case([k], PASSES, **dict(half, pdt=BF16)), case([k], PASSES, dst=D + 2, **half), case([k], BAD_ARG, dst=D + 1, **half)
        case([k], PASSES, interp=0), case([dict(k, frac=0)], PASSES, interp=0), case([dict(k, frac=0)], BAD_ARG), case([dict(k, xy=0)], BAD_ARG), case([dict(k, src=0)], BAD_ARG)
        case([k], BAD_ARG, dst=0), case([k], BAD_ARG, dw=0), case([k], PASSES, dw=7, dh=7), case([k], BAD_ARG, batch=-1)
        case([k], BAD_ARG, dst=D + 2), case([k], BAD_ARG, dst_rs=31), case([k], BAD_ARG, dst_rs=34), case([k], BAD_ARG, dst_ps=255), case([k], BAD_ARG, dst_ps=258)
        case([k], BAD_ARG, dst_fs=770), case([k], BAD_ARG, batch=2, dst_fs=764)
        two = dict(batch=2)
        for m in (0, 2, -1):
            case([dict(k, map_count=m)], BAD_ARG)
        case([dict(k, map_count=2)], PASSES, **two), case([k, dict(k, map_count=2)], PASSES, **two), case([dict(k, map_count=2, xy_fs=255)], BAD_ARG, **two)
        case([dict(k, xy=XY + 2)], BAD_ARG), case([dict(k, fr_rs=14)], BAD_ARG)
        # the first failing camera decides, not the first phase
        wide = dict(k, w=32768, rs=(3 if kind == "sbgr" else 1) * 32768, uv_rs=32768)
        case([wide], TOO_LARGE), case([k, k, dict(k, src=0)], BAD_ARG), case([k, k, wide], TOO_LARGE), case([wide, dict(k, src=0)], TOO_LARGE), case([dict(k, src=0), wide], BAD_ARG)
        case([k] * 7 + [dict(k, frac=0)], BAD_ARG), case([wide, k], UNSUPPORTED, blend=2)
        # the planes' bounding range against each read image of a later camera; the cameras may share every byte they read
        case([k, dict(k, src=D)], OVERLAP), case([k, dict(k, src=D + 767)], OVERLAP), case([k, dict(k, src=D + 768)], PASSES), case([k, dict(k, src=D - 63)], OVERLAP)
        case([k, dict(k, xy=D)], OVERLAP), case([k, dict(k, xy=D + 764)], OVERLAP), case([k, dict(k, xy=D + 768)], PASSES), case([k, dict(k, xy=D - 252)], OVERLAP)
        case([k, k, dict(k, frac=D + 766)], OVERLAP), case([k, k, dict(k, frac=D + 768)], PASSES), case([k, k, dict(k, frac=D - 126)], OVERLAP)
        case([k, dict(k, frac=D + 70)], PASSES, interp=0)                                                     # (nearest: not read)
        case([k, dict(k, src=D + 256)], OVERLAP, dst_ps=512), case([k, dict(k, xy=D + 256)], OVERLAP, dst_ps=512)    # (between two planes)
        case([k], PASSES, **two), case([k, dict(k, src=D + 1535)], OVERLAP, **two), case([k, dict(k, src=D + 1536)], PASSES, **two)
        case([k, k, k], PASSES), case([dict(k, xy=4096, frac=4096 + 64), k], PASSES), case([k, dict(k, src=D)], OK, batch=0, border=1)
        # strides next to 2^63
        case([dict(k, xy=1 << 40, xy_rs=HUGE - 3)], PASSES, dh=2), case([k], PASSES, dh=1, dst=1 << 40, dst_ps=1 << 62), case([k], BAD_ARG, dh=1, dst=1 << 40, dst_rs=HUGE - 3, dst_ps=1 << 62), case([k], BAD_ARG, dst_rs=HUGE)
        case([k], BAD_ARG, dh=2, dst_rs=HUGE - 3, dst_ps=HUGE - 3), case([dict(k, rs=HUGE)], TOO_LARGE), case([dict(k, rs=-1)], BAD_ARG)
        # 3. the destination's sides, 4. the border value, scale and bias, 5. the empty batch
        tall = dict(dh=(1 << 20) + 2, dst=1 << 40, dst_ps=1 << 26, dst_fs=3 << 26)
        case([dict(k, xy=1 << 44, frac=1 << 48)], TOO_LARGE, **tall), case([dict(k, xy=1 << 44, frac=1 << 48)], TOO_LARGE, batch=0, **tall)
        case([k], OK, border=0, scale=0, bias=0, batch=0), case([k], OK, border=1, batch=0), case([k], NOT_FINITE, border=2, batch=0), case([k, dict(k, src=0)], BAD_ARG, batch=0)
        case([k], NOT_FINITE, border=1, scale=2), case([k], NOT_FINITE, border=1, bias=2), case([k], NOT_FINITE, border=0, scale=0, bias=2)
        case([k], NOT_FINITE, border=1, scale=2, batch=0), case([k], NOT_FINITE, border=1, bias=2, batch=0)
    g, v = CAM, NVCAM
    out += [("sbgr", [g], dict(CALL, rgb=2), PASSES), ("sbgr", [dict(g, uv=1, uv_rs=-5)], dict(CALL), PASSES),                               # (neither is looked at)
            ("sbgr", [dict(g, h=7, w=7, rs=21)], dict(CALL), PASSES), ("sbgr", [dict(g, map_count=2)], dict(CALL, interp=2), UNSUPPORTED),   # the format first
            ("sbgr", [dict(g, map_count=2)], dict(CALL, pdt=0), UNSUPPORTED), ("sbgr", [g], dict(CALL, pdt=0, dst_rs=3), UNSUPPORTED),
            ("snv12", [v], dict(CALL, rgb=1), PASSES), ("snv12", [v], dict(CALL, rgb=2), UNSUPPORTED), ("snv12", [v], dict(CALL, rgb=-1), UNSUPPORTED),
            ("snv12", [dict(v, uv=0)], dict(CALL), BAD_ARG), ("snv12", [dict(v, h=7)], dict(CALL), BAD_ARG), ("snv12", [dict(v, w=7)], dict(CALL), BAD_ARG),
            ("snv12", [dict(v, uv=8193)], dict(CALL), BAD_ARG), ("snv12", [dict(v, uv_rs=9)], dict(CALL), BAD_ARG),
            ("snv12", [dict(v, map_count=2)], dict(CALL, interp=2), BAD_ARG), ("snv12", [dict(v, map_count=2)], dict(CALL, pdt=0), BAD_ARG),   # the format last
            ("snv12", [v, dict(v, uv=D + 766)], dict(CALL), OVERLAP), ("snv12", [v, dict(v, uv=D - 30)], dict(CALL), OVERLAP), ("snv12", [v, dict(v, uv=D - 32)], dict(CALL), PASSES),
            ("snv12", [v, dict(v, uv=D + 768)], dict(CALL), PASSES)]
    return out


def _stitch_line(kind, cams, a):
    n = len(cams) if a["n"] is None else a["n"]
    head = [n, a["cams_null"], a["dst"], a["batch"], a["dh"], a["dw"], a["dst_fs"], a["dst_ps"], a["dst_rs"], a["interp"], a["blend"], a["feather"], a["rgb"], a["pdt"],
            a["border"], a["scale"], a["bias"], len(cams)]
    body = [v for c in cams for v in (c["src"], c["uv"], c["h"], c["w"], c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"], c["frac"], c["xy_fs"], c["xy_rs"], c["fr_fs"],
                                      c["fr_rs"], c["map_count"])]
    return kind + " " + " ".join(str(v) for v in head + body)


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_call_descriptions_under_sanitizers(driver):
    single, stitch = _single_cases(), _stitch_cases()
    got = hostplan.run_driver(driver, [_single_line(a) for a, _ in single] + [_stitch_line(kind, cams, a) for kind, cams, a, _ in stitch], "map_planes")
    for (a, want), g in zip(single, got):
        assert g == want, (_single_line(a), g, want)
    for (kind, cams, a, want), g in zip(stitch, got[len(single):]):
        assert g[0] == want and (want == OK or g[1:] == [0, 0]), (_stitch_line(kind, cams, a), g, want)
    # the grid of a stitch that goes on to a launch: 256 x 4 tiles over the canvas, one frame per item whatever the map count
    for kind, k in (("sbgr", CAM), ("snv12", NVCAM)):
        lines = [_stitch_line(kind, [k] * n_, dict(CALL, border=1, **kw)) for n_, kw in ((1, {}), (8, {}), (3, dict(batch=5, dst_fs=768)), (1, dict(batch=0)))]
        assert hostplan.run_driver(driver, lines, "map_planes") == [[OK, OK, 2], [OK, OK, 2], [OK, OK, 10], [OK, OK, 0]]


def _d3(*v):
    return ctypes.cast((ctypes.c_double * 3)(*v), ctypes.c_void_p)


def _through_the_library(lib, a, border, scale, bias):
    P = ctypes.c_void_p
    return lib.bevwarp_remap_planes(P(a["src"]), P(a["dst"]), a["batch"], a["src_h"], a["src_w"], a["dst_h"], a["dst_w"], a["src_fs"], a["src_rs"], a["dst_fs"], a["dst_ps"],
                                    a["dst_rs"], P(a["xy"]), P(a["frac"]), a["map_count"], a["xy_fs"], a["xy_rs"], a["frac_fs"], a["frac_rs"], a["interp"], a["mode"], border,
                                    scale, bias, a["pdt"], None)


def _stitch_through_the_library(lib, kind, cams, a):
    arr = (_lib.MapCamera * max(len(cams), 1))(*[_lib.MapCamera(c["src"] or None, c["uv"] or None, c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"] or None, c["frac"] or None,
                                                                c["xy_fs"], c["xy_rs"], c["fr_fs"], c["fr_rs"], c["h"], c["w"], c["map_count"], 0) for c in cams])
    nan = float("nan")
    border = _d3(1.0, 2.0, nan if a["border"] == 2 else 3.0) if a["border"] else None
    scale = _d3(0.5, 0.25, nan if a["scale"] == 2 else 2.0) if a["scale"] else None
    bias = _d3(-1.0, 0.0, nan if a["bias"] == 2 else 1.0) if a["bias"] else None
    head = (None if a["cams_null"] else ctypes.addressof(arr), len(cams) if a["n"] is None else a["n"], a["dst"] or None, a["batch"], a["dh"], a["dw"], a["dst_fs"], a["dst_ps"],
            a["dst_rs"], a["interp"], a["blend"], a["feather"])
    tail = (border, scale, bias, a["pdt"], None)
    if kind == "snv12":
        return lib.bevwarp_stitch_maps_nv12_planes(*head, a["rgb"], *tail)
    return lib.bevwarp_stitch_maps_planes(*head, *tail)


def test_status_order_through_the_library():
    """Every call either fails a check or has nothing to launch: an empty batch, or -- after every other check -- a NaN in scale (which
    every border mode reads), in bias or in the border value."""
    lib = hostplan.built_lib()
    nan3, fine = _d3(1.0, float("nan"), 1.0), _d3(1.0, 2.0, 3.0)
    for a, (st, plan, _, _) in _single_cases():
        want = st if st != OK or a["batch"] == 0 else (plan if plan != OK else NOT_FINITE)
        assert _through_the_library(lib, a, fine, nan3, fine) == want, (_single_line(a), want)
    for a in (P32, P16B):
        for args in ((None, None, None), (nan3, nan3, nan3)):
            assert _through_the_library(lib, dict(a, batch=0), *args) == OK
        for args in ((nan3, None, None), (None, nan3, None), (None, None, nan3), (_d3(0.0, 0.0, INF), None, None), (fine, fine, _d3(-INF, 0.0, 0.0))):
            assert _through_the_library(lib, a, *args) == NOT_FINITE
        assert _through_the_library(lib, dict(a, mode=1, batch=0), nan3, None, None) == OK  # (the border value is the constant border's alone)
    for kind, cams, a, want in _stitch_cases():
        assert want != OK or a["batch"] == 0
        assert _stitch_through_the_library(lib, kind, cams, a) == want, (_stitch_line(kind, cams, a), want)


def test_abi_surface():
    lib = hostplan.built_lib()
    assert lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "#define BEVWARP_ABI_VERSION 7" in header
    for name, nargs, n64 in zip(NAMES, (26, 17, 18), (9, 3, 3)):
        decl = checked_declaration(name, nargs, n64)
        for arg in ("dst_plane_stride", "interp", "border_value", "scale", "bias", "plane_dtype"):
            assert arg in decl, (name, arg)
    assert ", ".join(NAMES) in header.split("Conventions")[0]
    from bev import warp as dropin
    from bev_amd import warp
    for name in ("remap_to_planar", "remap_stitch_to_planar", "remap_stitch_nv12_to_planar"):
        assert getattr(dropin, name) is getattr(warp, name)


# ---- the Python entries and SitePipeline: every refusal is a ValueError before any device work ----

class _ClaimsCuda(torch.Tensor):
    """A host tensor that answers is_cuda: the shape checks run without a device (nothing after them is reached)."""
    is_cuda = property(lambda self: True)


def _cpu_map(n=1, dh=6, dw=8, interp=1, device="cpu"):
    from bev_amd import warp
    return warp.WarpMap(torch.zeros((n, dh, dw, 2), dtype=torch.int16, device=device), torch.zeros((n, dh, dw), dtype=torch.int16, device=device) if interp == 1 else None,
                        interp, (dw, dh))


def test_python_entries_validate_before_the_device():
    from bev_amd import warp
    fake = lambda *shape: torch.zeros(shape, dtype=torch.uint8).as_subclass(_ClaimsCuda)  # noqa: E731
    img, img2, y2, uv2 = fake(8, 8, 3), fake(2, 8, 8, 3), fake(2, 8, 8), fake(2, 4, 4, 2)
    m = _cpu_map()
    single = lambda mp, **kw: warp.remap_to_planar(img2, mp, **kw)  # noqa: E731
    stitches = ((lambda mps, **kw: warp.remap_stitch_to_planar([img2] * len(mps), mps, **kw)),
                (lambda mps, **kw: warp.remap_stitch_nv12_to_planar([y2] * len(mps), [uv2] * len(mps), mps, **kw)))
    outs = ((dict(out_dtype=torch.float64), "out_dtype"), (dict(out_dtype=torch.uint8), "out_dtype"),
            (dict(out_dtype=torch.float16, out=torch.zeros((2, 3, 6, 8), dtype=torch.float32)), "out must be a torch.float16"),
            (dict(out=torch.zeros((2, 3, 5, 8), dtype=torch.float32)), "dsize is \\(8, 6\\), out is"), (dict(out=torch.zeros((2, 3, 6, 7), dtype=torch.float32)), "dsize is"),
            (dict(out=torch.zeros((3, 3, 6, 8), dtype=torch.float32)), "out must be a torch.float32 tensor of 288 elements"),
            (dict(out=torch.zeros((2, 3, 6, 16), dtype=torch.float32)[:, :, :, ::2]), "contiguous rows"))
    with pytest.raises(ValueError, match="needs a WarpMap"):
        single((torch.zeros((1, 6, 8, 2), dtype=torch.int16), None))
    with pytest.raises(ValueError, match="BORDER_TRANSPARENT"):
        single(m, border_mode=warp.BORDER_TRANSPARENT)
    with pytest.raises(ValueError, match="border mode"):
        single(m, border_mode=6)
    with pytest.raises(ValueError, match="holds 3 frames for a batch of 2"):
        single(_cpu_map(n=3))
    with pytest.raises(ValueError, match="the map is on"):
        single(_cpu_map(device="meta"))
    for kw, text in outs:
        with pytest.raises(ValueError, match=text):
            single(m, **kw)
    for f in stitches:
        for maps, kw, text in (([], {}, "1..8 cameras"), ([m] * 9, {}, "1..8 cameras"), ([m], dict(blend="mean"), "blend"), ([m], dict(blend="feather", feather=0), "1..4096"),
                               ([m], dict(blend="feather", feather=4097), "1..4096"), ([np.eye(3)], {}, "WarpMap per camera"), ([m, _cpu_map(dh=4)], {}, "map of camera 1 has dsize"),
                               ([m, _cpu_map(interp=0)], {}, "map of camera 1 .* interpolation 0"), ([m, _cpu_map(n=3)], {}, "holds 3 frames for a batch of 2"),
                               ([_cpu_map(device="meta")], {}, "the map is on")) + tuple(([m], kw, text) for kw, text in outs):
            with pytest.raises(ValueError, match=text):
                f(maps, **kw)
    with pytest.raises(ValueError, match="1 warp maps for 2 cameras"):
        warp.remap_stitch_to_planar([img2, img2], [m])
    with pytest.raises(ValueError, match="1 uv planes for 2 cameras"):
        warp.remap_stitch_nv12_to_planar([y2, y2], [uv2], [m, m])
    # the sources: 8-bit, 3 channels, on a device
    for src, text in ((torch.zeros((8, 8, 3), dtype=torch.uint8), "CUDA"), (img.numpy(), "CUDA"), (fake(8, 8, 3).float().as_subclass(_ClaimsCuda), "uint8"),
                      (fake(8, 8, 4), "\\(H, W, 3\\)"), (fake(8, 8), "\\(H, W, 3\\)"), (fake(8, 8, 1), "\\(H, W, 3\\)")):
        with pytest.raises(ValueError, match=text):
            warp.remap_to_planar(src, m)
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch_to_planar([src], [m])
    with pytest.raises(ValueError, match="camera 1 has 1 frames"):
        warp.remap_stitch_to_planar([img2, img], [m, m])
    for ys, uvs, text in (((7, 8), (3, 4, 2), "even sides"), ((8, 8), (4, 8, 2), "uv of shape")):
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch_nv12_to_planar([fake(*ys)], [fake(*uvs)], [m])
    with pytest.raises(ValueError, match="CUDA"):
        warp.remap_stitch_nv12_to_planar([torch.zeros((8, 8), dtype=torch.uint8)], [torch.zeros((4, 4, 2), dtype=torch.uint8)], [m])
    with pytest.raises(ValueError, match="camera 1 has 1 frames"):
        warp.remap_stitch_nv12_to_planar([y2, fake(8, 8)], [uv2, fake(4, 4, 2)], [m, m])


def test_site_pipeline_refusals():
    from bev_amd.pipeline import FramePipeline, SitePipeline
    m, hw = _cpu_map(), (8, 8)
    site = lambda hws, maps, dsize=(8, 6), **kw: SitePipeline(hws, maps, dsize, **dict(dict(device="cpu"), **kw))  # noqa: E731
    for hws, maps, kw, text in (([hw], [m, m], {}, "2 warp maps for 1 cameras"), ([hw, hw], [m], {}, "1 warp maps for 2 cameras"), ([], [], {}, "1..8 cameras, got 0"),
                                ([hw] * 9, [m] * 9, {}, "1..8 cameras, got 9"), ([hw], [np.eye(3)], {}, "camera 0 must be a bev_amd.warp.WarpMap of one frame, got ndarray"),
                                ([hw, hw], [m, _cpu_map(n=2)], {}, "camera 1 must be .* got 2 frames"), ([hw, hw], [m, _cpu_map(dh=4)], {}, "camera 1 was built for dsize"),
                                ([hw], [m], dict(dsize=(6, 8)), "camera 0 was built for dsize \\(8, 6\\), the pipeline's is \\(6, 8\\)"),
                                ([hw], [m], dict(device="cuda"), "camera 0 is on cpu, the pipeline runs on cuda"),
                                ([hw, hw], [m, _cpu_map(interp=0)], {}, "camera 1 has interpolation 0, camera 0's has 1"),
                                ([hw], [m], dict(src_format="yuv"), "unsupported src_format"), ([hw], [m], dict(dst_format="planar"), "unsupported dst_format"),
                                ([hw], [m], dict(dst_format="planes", plane_dtype=torch.float64), "unsupported plane_dtype"),
                                ([hw, (7, 8)], [m, m], dict(src_format="nv12"), "even frame sides, camera 1 has \\(7, 8\\)"),
                                ([(8, 7)], [m], dict(src_format="nv12", dst_format="planes"), "even frame sides"),
                                ([hw], [_cpu_map(dh=5)], dict(dsize=(8, 5), dst_format="nv12"), "needs an even dsize"),
                                ([hw], [_cpu_map(dw=7)], dict(dsize=(7, 6), dst_format="nv12", src_format="nv12"), "needs an even dsize"),
                                ([hw], [m], dict(depth=1), "depth must be >= 2"), ([hw], [m], dict(blend="mean"), "blend"),
                                ([hw], [m], dict(blend="feather", feather=0), "1..4096"), ([hw], [m], dict(scale=float("nan")), "scale must be finite"),
                                ([hw], [m], dict(bias=(0.0, float("inf"), 0.0)), "bias must be finite"), ([hw], [m], dict(border_value=(1.0, float("nan"), 2.0)), "border_value must be finite"),
                                ([hw], [m], dict(border_value=(1.0, 2.0)), "broadcast"), ([hw], [m], dict(scale=(1.0, 2.0, 3.0, 4.0)), "broadcast")):
        with pytest.raises(ValueError, match=text):
            site(hws, maps, **kw)
    for fmt in ("bgr", "nv12", "planes"):  # the map's own checks stand ahead of the format checks
        with pytest.raises(ValueError, match="pipeline runs on cuda"):
            site([hw], [m], dst_format=fmt, device="cuda")
    doc = SitePipeline.__init__.__doc__
    for name in ("bevwarp_stitch_maps", "bevwarp_stitch_maps_nv12", "bevwarp_stitch_maps_to_nv12", "bevwarp_stitch_maps_nv12_to_nv12", "bevwarp_stitch_maps_planes",
                 "bevwarp_stitch_maps_nv12_planes"):
        assert name in doc
    with pytest.raises(ValueError, match="warp_map .*planar"):  # FramePipeline keeps refusing planes through a map
        FramePipeline((8, 8), 3, None, (8, 6), warp_map=m, planar=True)


# ---- the code objects: the expected instances, no scratch, no LDS, at most 128 VGPRs ----

def test_single_camera_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_map_planes.hip", tmp_path, "warp_map_planes.h")
    assert all("remap_planes_kernel" in n for n in found)
    assert len(found) == 2 * 5 * 2, len(found)    # interpolation x border mode x {float32, 16-bit}
    codeobj.assert_lean(found)
    flags = codeobj.makefile_flags("warp_map_planes.hip", "plane_store.inc")
    assert "-fno-fast-math" in flags and "-ffp-contract=off" in flags
    codeobj.makefile_flags("warp_map_planes.hip", "map_entry_taps.inc")
    for header in ("remap_sample_u8x3.h", "remap_taps_u8x3.inc", "remap_frame_u8x3.inc", "tap_load.h"):  # (the sampler shared with the NV12-out unit)
        codeobj.makefile_flags("warp_map_planes.hip", header)


def test_stitch_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_stitch_maps_planes.hip", tmp_path, "warp_stitch_maps_planes.h")
    assert all("stitch_maps_planes_kernel" in n for n in found)
    assert len(found) == 3 * 2 * 2 * 2, len(found)    # {B, G, R frames; NV12 -> B, G, R; NV12 -> R, G, B} x interpolation x blend x {float32, 16-bit}
    codeobj.assert_lean(found)
    assert "-fno-fast-math" in codeobj.makefile_flags("warp_stitch_maps_planes.hip", "plane_store.inc")
    for header in ("stitch_sample.h", "stitch_maps_u8x3.inc", "tap_load.h", "nv12_sample.h"):  # (the shared stitch samplers and camera loop rebuild the unit)
        codeobj.makefile_flags("warp_stitch_maps_planes.hip", header)
