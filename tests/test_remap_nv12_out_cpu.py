"""The map samplers that write NV12 (bevwarp_remap_to_nv12, bevwarp_remap_nv12_to_nv12, bevwarp_stitch_maps_to_nv12,
bevwarp_stitch_maps_nv12_to_nv12; remap_to_nv12, remap_nv12_to_nv12, remap_stitch_to_nv12, remap_stitch_nv12_to_nv12) without a device:
the numpy definition (tests/remap_nv12_out_ref.py) tied to the definitions of the matrix warps into NV12 by bits, what an invalid map
entry gives, the C ABI's host checks under the sanitizers (tests/host_plan_driver.cpp, family `remap_nv12_out`) and the same statuses, in their
documented order, through the built library, the ABI surface, the refusals of the Python entries and of FramePipeline, and the code
objects of the two kernel units."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import codeobj
from tests import hostplan
from tests import nv12_out_ref as NO
from tests import nv12_ref as NR
from tests import remap_nv12_out_ref as RO
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests.test_abi import checked_declaration
from tests.test_lens_cpu import GEOMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
NAMES = ("bevwarp_remap_to_nv12", "bevwarp_remap_nv12_to_nv12", "bevwarp_stitch_maps_to_nv12", "bevwarp_stitch_maps_nv12_to_nv12")
BORDER = (7.0, 200.0, 31.0)


# ---- the definition tied to the matrix warps into NV12, by bits ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_pinhole_maps_reproduce_the_matrix_warps_into_nv12(geom, interp):
    """With a pinhole map and CONSTANT the definition IS nv12_out_ref.warp_to_nv12 / warp_nv12_to_nv12 for the same matrix."""
    sw, sh, dw, dh, M = GEOMS[geom]
    xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
    y, uv = NR.frame("uniform", 3, sh, sw)
    bgr = NR.nv12_to_bgr(y, uv)
    for bv in (None, BORDER):
        b = 0.0 if bv is None else bv
        for rgb in (False, True):
            for got, exp in zip(RO.remap_to_nv12(bgr, xy, frac, interp, RR.CONSTANT, b, rgb), NO.warp_to_nv12(bgr, M, (dw, dh), interp, border_value=bv, rgb=rgb)):
                np.testing.assert_array_equal(got, exp, err_msg="bgr source, border %s rgb %d" % (bv, rgb))
        for got, exp in zip(RO.remap_nv12_to_nv12(y, uv, xy, frac, interp, RR.CONSTANT, b), NO.warp_nv12_to_nv12(y, uv, M, (dw, dh), interp, border_value=bv)):
            np.testing.assert_array_equal(got, exp, err_msg="nv12 source, border %s" % (bv,))
    # one camera under the stitch is the camera's own pixels where it covers and the border pixel elsewhere
    cover = RR.written(xy, sw, sh, interp)
    sy, suv = RO.stitch_to_nv12([bgr], [(xy, frac)], interp, SM.OVER, 64, BORDER)
    ry, ruv = RO.remap_to_nv12(bgr, xy, frac, interp, RR.REPLICATE)
    np.testing.assert_array_equal(sy[cover], ry[cover])
    by, bu, bvv = (int(v) for v in NO.yuv(*BORDER[::-1]))
    assert cover.any() and not cover.all() and (sy[~cover] == by).all()
    assert (suv[~cover[0::2, 0::2]] == (bu, bvv)).all() and (suv[cover[0::2, 0::2]] == ruv[cover[0::2, 0::2]]).all()


@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_invalid_entries_give_the_converted_border_pixel(interp):
    """The sentinel (-32768, -32768) yields the border pixel itself, converted: its Y, and -- where the sentinel is the top-left pixel of a
    2 x 2 block -- the block's pair, although the block's three other pixels are valid."""
    sw, sh, dw, dh = 8, 6, 8, 4
    gx, gy = np.meshgrid(np.arange(dw, dtype=np.int16), np.arange(dh, dtype=np.int16))
    xy = np.stack([gx, gy], axis=-1)
    frac = None if interp == wn.NEAREST else np.zeros((dh, dw), np.uint16)
    holes = [(0, 2), (1, 4), (2, 7), (3, 3)]  # (row, column): an even / even position (a pair's), two mixed, and an odd / odd one
    for r, c in holes:
        xy[r, c] = (RR.SENTINEL, RR.SENTINEL)
    y, uv = NR.frame("uniform", 9, sh, sw)
    bgr = NR.nv12_to_bgr(y, uv)
    by, bu, bv = (int(v) for v in NO.yuv(*BORDER[::-1]))       # BORDER read as B, G, R
    ry, ru, rv = (int(v) for v in NO.yuv(*BORDER))              # ... and as R, G, B
    plain = NO.bgr_to_nv12(bgr[:dh, :dw])                       # (the identity map, frac 0: the frame's own pixels)
    for name, (gy_, guv_), want in (("bgr", RO.remap_to_nv12(bgr, xy, frac, interp, RR.CONSTANT, BORDER), (by, bu, bv)),
                                    ("rgb", RO.remap_to_nv12(bgr, xy, frac, interp, RR.CONSTANT, BORDER, rgb=True), (ry, ru, rv)),
                                    ("nv12", RO.remap_nv12_to_nv12(y, uv, xy, frac, interp, RR.CONSTANT, BORDER), (by, bu, bv)),
                                    ("stitch", RO.stitch_to_nv12([bgr], [(xy, frac)], interp, SM.FEATHER, 3, BORDER), (by, bu, bv)),
                                    ("stitch nv12", RO.stitch_nv12_to_nv12([y], [uv], [(xy, frac)], interp, SM.OVER, 64, BORDER), (by, bu, bv))):
        for r, c in holes:
            assert int(gy_[r, c]) == want[0], (name, r, c)
        assert guv_[0, 1].tolist() == list(want[1:]), name      # the pair of the block whose top-left pixel (0, 2) is invalid
        if name == "bgr" and interp == wn.NEAREST:              # ... and nothing else moved: the block's other pixels and the other pairs are the frame's
            keep = np.ones((dh, dw), bool)
            for r, c in holes:
                keep[r, c] = False
            assert (gy_[keep] == plain[0][keep]).all() and gy_[0, 3] == plain[0][0, 3] and gy_[1, 2] == plain[0][1, 2]
            pairs = np.ones((dh // 2, dw // 2), bool)
            pairs[0, 1] = False
            assert (guv_[pairs] == plain[1][pairs]).all()
    # the default border is the black pixel: (16, 128, 128)
    gy_, guv_ = RO.remap_to_nv12(bgr, xy, frac, interp)
    assert int(gy_[0, 2]) == 16 and guv_[0, 1].tolist() == [128, 128]


# ---- the host checks: one table of cases, run under the sanitizers and through the built library ----

D, XY, FR = 1 << 20, 1 << 24, 1 << 26
# an 8 x 8 source -- B, G, R pixels at 4096, or the planes Y at 4096 and four rows of four pairs at 8192 -- and an 8 x 8 destination in the
# joined layout at 2^20 (64 Y bytes, then 32 bytes of pairs; frames 96 apart); one shared bilinear map at 2^24 and 2^26; never dereferenced
KEYS = ("src", "uv", "dy", "duv", "xy", "frac", "batch", "src_h", "src_w", "dst_h", "dst_w", "src_fs", "src_rs", "uv_fs", "uv_rs", "y_fs", "y_rs", "duv_fs", "duv_rs",
        "map_count", "xy_fs", "xy_rs", "frac_fs", "frac_rs", "interp", "mode", "rgb")
BGR = dict(src=4096, uv=0, dy=D, duv=D + 64, xy=XY, frac=FR, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, src_fs=192, src_rs=24, uv_fs=0, uv_rs=0, y_fs=96, y_rs=8, duv_fs=96,
           duv_rs=8, map_count=1, xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16, interp=1, mode=0, rgb=0)
NV12 = dict(BGR, uv=8192, src_fs=64, src_rs=8, uv_fs=32, uv_rs=8)
NONE = [0, 0, 0]
HUGE = (1 << 63) - 1


def _single_cases():
    """[(kind, arguments, [check_call's status, plan_remap's status, frames per item, items])]"""
    out = []
    ok = [OK, OK, 1, 2]
    w20 = 1 << 20
    for kind, base in (("bgr", BGR), ("nv12", NV12)):
        def case(want, _base=base, _kind=kind, **kw):
            out.append((_kind, dict(_base, **kw), want if isinstance(want, list) else [want] + NONE))

        wide_w = dict(src_w=32768, src_rs=3 * 32768, uv_rs=32768) if kind == "bgr" else dict(src_w=32768, src_rs=32768, uv_rs=32768)
        case(ok), case(ok, interp=0), case(ok, interp=0, frac=0), case([OK] + NONE, batch=0), case(BAD_ARG, batch=0, map_count=7)
        # 1. BEVWARP_ERR_BAD_ARG: null pointers (the frac plane under bilinear only), sizes, odd destination sides
        for k in ("src", "dy", "duv", "xy", "frac", "src_h", "src_w", "dst_h", "dst_w"):
            case(BAD_ARG, **{k: 0})
        case(BAD_ARG, xy=0, interp=0), case(BAD_ARG, batch=-1), case(BAD_ARG, dst_w=7), case(BAD_ARG, dst_h=7), case(BAD_ARG, dst_w=7, dst_h=7), case(ok, dst_w=6, dst_h=6)
        # ... layouts: an odd uv base and odd uv strides of the destination, rows below a row, the map planes' alignment
        case(BAD_ARG, duv=D + 65), case(BAD_ARG, duv_rs=9), case(BAD_ARG, duv_fs=97), case(BAD_ARG, duv_rs=6), case(BAD_ARG, y_rs=7), case(ok, duv_rs=10, y_rs=9, dy=D - 200)
        case(BAD_ARG, batch=2, y_fs=63), case(BAD_ARG, batch=2, duv_fs=30), case(BAD_ARG, xy=XY + 2), case(BAD_ARG, xy_rs=28), case(BAD_ARG, frac=FR + 1), case(BAD_ARG, frac_rs=14)
        case(ok, xy=XY + 4, frac=FR + 2), case(ok, frac=FR + 1, frac_rs=3, interp=0)
        # ... the map count: 1 or the batch
        three = dict(batch=3)
        case(BAD_ARG, map_count=0), case(BAD_ARG, map_count=2), case(BAD_ARG, map_count=2, **three), case([OK, OK, 1, 6], map_count=3, **three)
        case([OK, OK, 1, 6], map_count=1, xy_fs=1, frac_fs=1, **three), case(BAD_ARG, map_count=3, xy_fs=255, **three)
        # 2. BEVWARP_ERR_UNSUPPORTED: the interpolation, the five borders that write every pixel
        for i in (2, 3, -1):
            case(UNSUPPORTED, interp=i)
        for m in (5, 6, 16, -1):
            case(UNSUPPORTED, mode=m)
        for m in range(5):
            case(ok, mode=m), case(ok, mode=m, interp=0)
        case(UNSUPPORTED, interp=2, frac=0)
        case(UNSUPPORTED, mode=5, **wide_w), case(UNSUPPORTED, interp=2, dy=4096)     # ... before the size limits and the overlap
        case(BAD_ARG, mode=5, dst_w=7), case(BAD_ARG, interp=2, src=0)                # ... after the null pointers and the sides
        # 3. BEVWARP_ERR_TOO_LARGE for the source, before the overlap; the maps have no such limit
        case(TOO_LARGE, **wide_w), case(TOO_LARGE, src_h=32768), case(TOO_LARGE, src_rs=1 << 24), case(TOO_LARGE, dy=4096, **wide_w), case(ok, xy_rs=1 << 24, frac_rs=1 << 24)
        # 4. BEVWARP_ERR_OVERLAP: each destination plane over each image the call reads, and over the other plane
        far = D + 4096
        case(OVERLAP, dy=4096), case(OVERLAP, dy=4096 + 62), case(ok, dy=4096 - 64), case(OVERLAP, dy=4096 - 62)
        case(OVERLAP, dy=far, duv=4096), case(OVERLAP, dy=far, duv=4096 - 30), case(ok, dy=far, duv=4096 - 32)
        case(OVERLAP, xy=D), case(OVERLAP, xy=D + 60), case(OVERLAP, xy=D + 64), case(OVERLAP, xy=D + 92), case(ok, xy=D + 96), case(OVERLAP, xy=D - 252), case(ok, xy=D - 256)
        case(OVERLAP, frac=D + 62), case(OVERLAP, frac=D + 64), case(OVERLAP, frac=D + 94), case(ok, frac=D + 96), case(OVERLAP, frac=D - 126), case(ok, frac=D - 128)
        case(ok, frac=D + 70, interp=0)                                               # (nearest: not read)
        case(OVERLAP, duv=D + 62), case(OVERLAP, duv=D), case(OVERLAP, duv=D - 30), case(ok, duv=D - 32), case(ok, duv=D + 64)  # the joined layout is adjacent
        case([OK, OK, 1, 4], batch=2), case(OVERLAP, batch=2, y_fs=94, duv_fs=94), case(OVERLAP, batch=2, duv=D + 62)  # ... frame after frame too
        case(ok, xy=4096, frac=4096 + 64)                                             # the read images may overlap each other
        # 5. BEVWARP_ERR_TOO_LARGE from the launch plan, after the overlap; the frames-per-item plan
        tall = dict(dst_h=w20 + 2, dy=1 << 40, duv=1 << 42, xy=1 << 44, frac=1 << 48)
        case([OK, TOO_LARGE, 0, 0], **tall), case(OVERLAP, **dict(tall, dy=4096))
        big = dict(batch=32, dst_h=1024, dst_w=1024, y_rs=1024, y_fs=1536 * 1024, duv_rs=1024, duv_fs=1536 * 1024, dy=1 << 40, duv=(1 << 40) + (1 << 20), xy=1 << 44,
                   frac=1 << 48, xy_rs=4096, xy_fs=1 << 22, frac_rs=2048, frac_fs=1 << 21)
        case([OK, OK, 2, 16 * 1024], map_count=1, **big), case([OK, OK, 1, 32 * 1024], map_count=32, **big)
        # strides next to 2^63: bad arguments or size limits, not overflows (two rows, one row of pairs: the images' last bytes stay below 2^64)
        two_rows = dict(dst_h=2)
        case([OK, OK, 1, 1], dy=1 << 40, duv=D, y_rs=HUGE, **two_rows), case([OK, OK, 1, 1], duv=1 << 40, duv_rs=HUGE - 1, **two_rows), case(BAD_ARG, duv_rs=HUGE, **two_rows)
        case([OK, OK, 1, 1], xy=1 << 40, xy_rs=HUGE - 3, **two_rows), case([OK, OK, 1, 1], frac=1 << 40, frac_rs=HUGE - 1, **two_rows)
        case(BAD_ARG, batch=3, y_rs=HUGE, y_fs=HUGE), case(BAD_ARG, batch=2, map_count=2, xy_rs=HUGE - 3, xy_fs=HUGE - 3), case(TOO_LARGE, src_rs=HUGE), case(BAD_ARG, src_rs=-1)
        case(BAD_ARG, y_rs=-HUGE - 1)
    # what differs between the two entries: the source's second plane, the channel order, and the order of the format and the layouts
    def b(want, **kw):
        out.append(("bgr", dict(BGR, **kw), want if isinstance(want, list) else [want] + NONE))

    def n(want, **kw):
        out.append(("nv12", dict(NV12, **kw), want if isinstance(want, list) else [want] + NONE))

    b(ok, rgb=1), b(UNSUPPORTED, rgb=2), b(UNSUPPORTED, rgb=-1), b(ok, uv=1, uv_rs=-5, uv_fs=3), b(ok, src_h=7, src_w=7, src_rs=21), b(BAD_ARG, src_rs=23)
    b(UNSUPPORTED, interp=2, map_count=2), b(UNSUPPORTED, mode=5, xy_rs=28), b(UNSUPPORTED, rgb=2, duv=D + 65)         # bevwarp_remap's order: the format first
    n(ok, rgb=2), n(BAD_ARG, uv=0), n(BAD_ARG, src_h=7), n(BAD_ARG, src_w=7), n(ok, src_h=6, src_w=6), n(BAD_ARG, uv=8193), n(BAD_ARG, uv_rs=9), n(BAD_ARG, uv_fs=33, batch=2)
    n(BAD_ARG, uv_rs=6), n(TOO_LARGE, uv_rs=1 << 24), n(TOO_LARGE, uv_rs=HUGE - 1), n(BAD_ARG, uv_rs=HUGE)
    n(BAD_ARG, interp=2, map_count=2), n(BAD_ARG, mode=5, xy_rs=28), n(BAD_ARG, mode=5, duv=D + 65)                     # bevwarp_remap_nv12's order: the format last
    n(OVERLAP, dy=8192), n(OVERLAP, dy=8192 + 30), n(ok, dy=8192 + 32, duv=8192 + 96), n(OVERLAP, dy=D + 4096, duv=8192 + 30), n(ok, dy=D + 4096, duv=8192 + 32)
    n(ok, uv=4096 + 8)                                                                                                    # the source planes may overlap each other
    return out


def _single_line(kind, a):
    return kind + " " + " ".join(str(a[k]) for k in KEYS)


CAM = dict(src=4096, uv=0, h=8, w=8, fs=192, rs=24, uv_fs=0, uv_rs=0, xy=XY, frac=FR, xy_fs=256, xy_rs=32, fr_fs=128, fr_rs=16, map_count=1)
NVCAM = dict(CAM, uv=8192, fs=64, rs=8, uv_fs=32, uv_rs=8)
CALL = dict(n=None, cams_null=0, dy=D, duv=D + 64, batch=1, dh=8, dw=8, y_fs=96, y_rs=8, duv_fs=96, duv_rs=8, interp=1, blend=0, feather=64, rgb=0, border=2)
PASSES = NOT_FINITE  # a call that passes every check of its cameras and of the canvas ends on the NaN border value: nothing is launched


def _stitch_cases():
    """[(kind, cameras, call arguments, status)]: bevwarp_stitch_maps' table (tests/test_stitch_maps_cpu.py) for the NV12 canvas."""
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
        # 2. per camera: the format (the blend is part of it), null images, sides, the map count, layouts
        for bl in (2, -1):
            case([k], UNSUPPORTED, blend=bl)
        for i in (2, 3, -1):
            case([k], UNSUPPORTED, interp=i)
        case([k], PASSES, interp=0), case([dict(k, frac=0)], PASSES, interp=0), case([dict(k, frac=0)], BAD_ARG), case([dict(k, xy=0)], BAD_ARG), case([dict(k, src=0)], BAD_ARG)
        case([k], BAD_ARG, dy=0), case([k], BAD_ARG, duv=0), case([k], BAD_ARG, dw=7), case([k], BAD_ARG, dh=7), case([k], PASSES, dw=6, dh=6), case([k], BAD_ARG, dw=0)
        case([k], BAD_ARG, duv=D + 65), case([k], BAD_ARG, duv_rs=9), case([k], BAD_ARG, duv_fs=97), case([k], BAD_ARG, y_rs=7), case([k], BAD_ARG, batch=-1)
        two = dict(batch=2)
        for m in (0, 2, -1):
            case([dict(k, map_count=m)], BAD_ARG)
        case([dict(k, map_count=2)], PASSES, **two), case([k, dict(k, map_count=2)], PASSES, **two), case([dict(k, map_count=2, xy_fs=255)], BAD_ARG, **two)
        case([dict(k, xy=XY + 2)], BAD_ARG), case([dict(k, fr_rs=14)], BAD_ARG)
        # the first failing camera decides, not the first phase
        wide = dict(k, w=32768, rs=(3 if kind == "sbgr" else 1) * 32768, uv_rs=32768)
        case([wide], TOO_LARGE), case([k, k, dict(k, src=0)], BAD_ARG), case([k, k, wide], TOO_LARGE), case([wide, dict(k, src=0)], TOO_LARGE), case([dict(k, src=0), wide], BAD_ARG)
        case([k] * 7 + [dict(k, frac=0)], BAD_ARG), case([wide, k], UNSUPPORTED, blend=2)
        # each destination plane against each read image of a later camera, and against the other plane; the cameras may share every byte they read
        far = D + 4096
        case([k, dict(k, src=D)], OVERLAP), case([k, dict(k, src=D + 64)], OVERLAP), case([k, dict(k, src=D + 95)], OVERLAP), case([k, dict(k, src=D + 96)], PASSES)
        case([k, dict(k, xy=D)], OVERLAP), case([k, dict(k, xy=D + 92)], OVERLAP), case([k, dict(k, xy=D + 96)], PASSES), case([k, dict(k, xy=D - 252)], OVERLAP)
        case([k, k, dict(k, frac=D + 62)], OVERLAP), case([k, k, dict(k, frac=D + 94)], OVERLAP), case([k, k, dict(k, frac=D + 96)], PASSES)
        case([k, dict(k, frac=D + 70)], PASSES, interp=0)                                                     # (nearest: not read)
        case([k], OVERLAP, duv=D + 62), case([k], OVERLAP, duv=D - 30), case([k], PASSES, duv=D - 32), case([k], PASSES, **two), case([k], OVERLAP, y_fs=94, duv_fs=94, **two)
        case([k, dict(k, src=far)], OVERLAP, dy=far, duv=far + 4096), case([k, dict(k, src=far + 4096)], OVERLAP, dy=far, duv=far + 4096)
        case([k, k, k], PASSES), case([dict(k, xy=4096, frac=4096 + 64), k], PASSES), case([k, dict(k, src=D)], OK, batch=0, border=1)
        # strides next to 2^63
        case([dict(k, xy=1 << 40, xy_rs=HUGE - 3)], PASSES, dh=2), case([k], PASSES, dh=2, dy=1 << 40, y_rs=HUGE), case([k], BAD_ARG, duv_rs=HUGE), case([dict(k, rs=HUGE)], TOO_LARGE)
        case([k], BAD_ARG, batch=3, y_rs=HUGE, y_fs=HUGE), case([dict(k, rs=-1)], BAD_ARG)
        # 3. the destination's sides, 4. the border value, 5. the empty batch
        w20 = 1 << 20
        tall = dict(dh=w20 + 2, dy=1 << 40, duv=1 << 42)
        case([dict(k, xy=1 << 44, frac=1 << 48)], TOO_LARGE, **tall), case([dict(k, xy=1 << 44, frac=1 << 48)], TOO_LARGE, batch=0, **tall)
        case([k], OK, border=0, batch=0), case([k], OK, border=1, batch=0), case([k], NOT_FINITE, border=2, batch=0), case([k, dict(k, src=0)], BAD_ARG, batch=0)
    g, v = CAM, NVCAM
    out += [("sbgr", [g], dict(CALL, rgb=1), PASSES), ("sbgr", [g], dict(CALL, rgb=2), UNSUPPORTED), ("sbgr", [dict(g, uv=1, uv_rs=-5)], dict(CALL), PASSES),
            ("sbgr", [dict(g, h=7, w=7, rs=21)], dict(CALL), PASSES), ("sbgr", [dict(g, map_count=2)], dict(CALL, interp=2), UNSUPPORTED),   # the format first
            ("snv12", [v], dict(CALL, rgb=2), PASSES), ("snv12", [dict(v, uv=0)], dict(CALL), BAD_ARG), ("snv12", [dict(v, h=7)], dict(CALL), BAD_ARG),
            ("snv12", [dict(v, uv=8193)], dict(CALL), BAD_ARG), ("snv12", [dict(v, uv_rs=9)], dict(CALL), BAD_ARG), ("snv12", [dict(v, map_count=2)], dict(CALL, interp=2), BAD_ARG),
            ("snv12", [v, dict(v, uv=D + 64)], dict(CALL), OVERLAP), ("snv12", [v, dict(v, uv=D - 30)], dict(CALL), OVERLAP), ("snv12", [v, dict(v, uv=D - 32)], dict(CALL), PASSES)]
    return out


def _stitch_line(kind, cams, a):
    n = len(cams) if a["n"] is None else a["n"]
    head = [n, a["cams_null"], a["dy"], a["duv"], a["batch"], a["dh"], a["dw"], a["y_fs"], a["y_rs"], a["duv_fs"], a["duv_rs"], a["interp"], a["blend"], a["feather"], a["rgb"],
            a["border"], len(cams)]
    body = [v for c in cams for v in (c["src"], c["uv"], c["h"], c["w"], c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"], c["frac"], c["xy_fs"], c["xy_rs"], c["fr_fs"],
                                      c["fr_rs"], c["map_count"])]
    return kind + " " + " ".join(str(v) for v in head + body)


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_call_descriptions_under_sanitizers(driver):
    single, stitch = _single_cases(), _stitch_cases()
    got = hostplan.run_driver(driver, [_single_line(kind, a) for kind, a, _ in single] + [_stitch_line(kind, cams, a) for kind, cams, a, _ in stitch], "remap_nv12_out")
    for (kind, a, want), g in zip(single, got):
        assert g == want, (_single_line(kind, a), g, want)
    for (kind, cams, a, want), g in zip(stitch, got[len(single):]):
        assert g[0] == want and (want == OK or g[1:] == [0, 0]), (_stitch_line(kind, cams, a), g, want)
    # the grid of a stitch that goes on to a launch: 256 x 4 tiles over the canvas, one frame per item whatever the map count
    for kind, k in (("sbgr", CAM), ("snv12", NVCAM)):
        lines = [_stitch_line(kind, [k] * n_, dict(CALL, border=1, **kw)) for n_, kw in ((1, {}), (8, {}), (3, dict(batch=5)), (1, dict(batch=0)))]
        assert hostplan.run_driver(driver, lines, "remap_nv12_out") == [[OK, OK, 2], [OK, OK, 2], [OK, OK, 10], [OK, OK, 0]]


def _through_the_library(lib, kind, a, border):
    P = ctypes.c_void_p
    head = (P(a["src"]),) + ((P(a["uv"]),) if kind == "nv12" else ()) + (P(a["dy"]), P(a["duv"]), a["batch"], a["src_h"], a["src_w"], a["dst_h"], a["dst_w"], a["src_fs"], a["src_rs"])
    head += ((a["uv_fs"], a["uv_rs"]) if kind == "nv12" else ()) + (a["y_fs"], a["y_rs"], a["duv_fs"], a["duv_rs"], P(a["xy"]), P(a["frac"]), a["map_count"], a["xy_fs"], a["xy_rs"],
                                                                   a["frac_fs"], a["frac_rs"], a["interp"], a["mode"])
    if kind == "nv12":
        return lib.bevwarp_remap_nv12_to_nv12(*head, border, None)
    return lib.bevwarp_remap_to_nv12(*head, a["rgb"], border, None)


def _stitch_through_the_library(lib, kind, cams, a):
    arr = (_lib.MapCamera * max(len(cams), 1))(*[_lib.MapCamera(c["src"] or None, c["uv"] or None, c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"] or None, c["frac"] or None,
                                                                c["xy_fs"], c["xy_rs"], c["fr_fs"], c["fr_rs"], c["h"], c["w"], c["map_count"], 0) for c in cams])
    bv = [1.0, 2.0, float("nan") if a["border"] == 2 else 3.0]
    border = ctypes.cast((ctypes.c_double * 3)(*bv), ctypes.c_void_p) if a["border"] else None
    head = (None if a["cams_null"] else ctypes.addressof(arr), len(cams) if a["n"] is None else a["n"], a["dy"] or None, a["duv"] or None, a["batch"], a["dh"], a["dw"], a["y_fs"],
            a["y_rs"], a["duv_fs"], a["duv_rs"], a["interp"], a["blend"], a["feather"])
    if kind == "snv12":
        return lib.bevwarp_stitch_maps_nv12_to_nv12(*head, border, None)
    return lib.bevwarp_stitch_maps_to_nv12(*head, a["rgb"], border, None)


def test_status_order_through_the_library():
    """Every call either fails a check or has nothing to launch: an empty batch, or -- after every other check -- a NaN in the border value."""
    lib = hostplan.built_lib()
    nan3 = ctypes.cast((ctypes.c_double * 3)(1.0, float("nan"), 1.0), ctypes.c_void_p)
    for kind, a, (st, plan, _, _) in _single_cases():
        # (the checks, then the launch plan's limit, then the border value -- read by the constant border only: the other modes would launch)
        want = st if st != OK or a["batch"] == 0 else (plan if plan != OK else NOT_FINITE)
        if want == NOT_FINITE and a["mode"] != 0:
            assert _through_the_library(lib, kind, dict(a, batch=0), nan3) == OK, _single_line(kind, a)
            continue
        assert _through_the_library(lib, kind, a, nan3) == want, (_single_line(kind, a), want)
    for kind, a in (("bgr", BGR), ("nv12", NV12)):
        assert _through_the_library(lib, kind, dict(a, batch=0), None) == OK and _through_the_library(lib, kind, dict(a, batch=0), nan3) == OK
        inf3 = ctypes.cast((ctypes.c_double * 3)(0.0, 0.0, float("inf")), ctypes.c_void_p)
        assert _through_the_library(lib, kind, a, inf3) == NOT_FINITE
    for kind, cams, a, want in _stitch_cases():
        assert want != OK or a["batch"] == 0
        assert _stitch_through_the_library(lib, kind, cams, a) == want, (_stitch_line(kind, cams, a), want)


def test_abi_surface():
    lib = hostplan.built_lib()
    assert lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "#define BEVWARP_ABI_VERSION 7" in header
    for name, nargs, n64 in zip(NAMES, (26, 28, 17, 16), (10, 12, 4, 4)):
        decl = checked_declaration(name, nargs, n64)
        for arg in ("dst_y", "dst_uv", "uv_row_stride", "interp", "border_value"):
            assert arg in decl, (name, arg)
    assert ", ".join(NAMES) in header.split("Conventions")[0]
    from bev import warp as dropin
    from bev_amd import warp
    for name in ("remap_to_nv12", "remap_nv12_to_nv12", "remap_stitch_to_nv12", "remap_stitch_nv12_to_nv12"):
        assert getattr(dropin, name) is getattr(warp, name)


# ---- the Python entries: every refusal is a ValueError before any device work ----

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
    singles = ((lambda mp, **kw: warp.remap_to_nv12(img2, mp, **kw)), (lambda mp, **kw: warp.remap_nv12_to_nv12(y2, uv2, mp, **kw)))
    stitches = ((lambda mps, **kw: warp.remap_stitch_to_nv12([img2] * len(mps), mps, **kw)), (lambda mps, **kw: warp.remap_stitch_nv12_to_nv12([y2] * len(mps), [uv2] * len(mps), mps, **kw)))
    for f in singles:
        with pytest.raises(ValueError, match="needs a WarpMap"):
            f((torch.zeros((1, 6, 8, 2), dtype=torch.int16), None))
        with pytest.raises(ValueError, match="BORDER_TRANSPARENT"):
            f(m, border_mode=warp.BORDER_TRANSPARENT)
        with pytest.raises(ValueError, match="border mode"):
            f(m, border_mode=6)
        for dh, dw in ((5, 8), (6, 7), (5, 7)):
            with pytest.raises(ValueError, match="even sides"):
                f(_cpu_map(dh=dh, dw=dw))
        with pytest.raises(ValueError, match="holds 3 frames for a batch of 2"):
            f(_cpu_map(n=3))
        with pytest.raises(ValueError, match="the map is on"):
            f(_cpu_map(device="meta"))
        for out, text in ((torch.zeros((2, 9, 7), dtype=torch.uint8), "joined out"), (torch.zeros((2, 9, 8), dtype=torch.int16), "joined out"),
                          (torch.zeros((3, 9, 8), dtype=torch.uint8), "out planes must be"), ((torch.zeros((2, 6, 8), dtype=torch.uint8),), "joined .* or a \\(y, uv\\) pair"),
                          ((torch.zeros((2, 6, 8), dtype=torch.uint8), torch.zeros((2, 3, 4), dtype=torch.uint8)), "out planes must be"),
                          ((torch.zeros((2, 6, 8), dtype=torch.uint8), torch.zeros((2, 3, 8, 2), dtype=torch.uint8)), "out planes must be"),
                          ((torch.zeros((2, 6, 16), dtype=torch.uint8)[:, :, ::2], torch.zeros((2, 3, 4, 2), dtype=torch.uint8)), "contiguous")):
            with pytest.raises(ValueError, match=text):
                f(m, out=out)
    for f in stitches:
        for maps, kw, text in (([], {}, "1..8 cameras"), ([m] * 9, {}, "1..8 cameras"), ([m], dict(blend="mean"), "blend"), ([m], dict(blend="feather", feather=0), "1..4096"),
                               ([m], dict(blend="feather", feather=4097), "1..4096"), ([np.eye(3)], {}, "WarpMap per camera"), ([m, _cpu_map(dh=4)], {}, "map of camera 1 has dsize"),
                               ([m, _cpu_map(interp=0)], {}, "map of camera 1 .* interpolation 0"), ([_cpu_map(dh=5)], {}, "even sides"), ([_cpu_map(dw=6, dh=5)], {}, "even sides"),
                               ([m, _cpu_map(n=3)], {}, "holds 3 frames for a batch of 2"), ([_cpu_map(device="meta")], {}, "the map is on"),
                               ([m], dict(out=torch.zeros((2, 9, 7), dtype=torch.uint8)), "joined out")):
            with pytest.raises(ValueError, match=text):
                f(maps, **kw)
    with pytest.raises(ValueError, match="1 warp maps for 2 cameras"):
        warp.remap_stitch_to_nv12([img2, img2], [m])
    with pytest.raises(ValueError, match="1 uv planes for 2 cameras"):
        warp.remap_stitch_nv12_to_nv12([y2, y2], [uv2], [m, m])
    # the sources: 8-bit, 3 channels, on a device
    for src, text in ((torch.zeros((8, 8, 3), dtype=torch.uint8), "CUDA"), (img.numpy(), "CUDA"), (fake(8, 8, 3).float().as_subclass(_ClaimsCuda), "uint8"),
                      (fake(8, 8, 4), "\\(H, W, 3\\)"), (fake(8, 8), "\\(H, W, 3\\)"), (fake(8, 8, 1), "\\(H, W, 3\\)")):
        with pytest.raises(ValueError, match=text):
            warp.remap_to_nv12(src, m)
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch_to_nv12([src], [m])
    with pytest.raises(ValueError, match="camera 1 has 1 frames"):
        warp.remap_stitch_to_nv12([img2, img], [m, m])
    for ys, uvs, text in (((7, 8), (3, 4, 2), "even sides"), ((8, 8), (4, 8, 2), "uv of shape")):
        with pytest.raises(ValueError, match=text):
            warp.remap_nv12_to_nv12(fake(*ys), fake(*uvs), m)
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch_nv12_to_nv12([fake(*ys)], [fake(*uvs)], [m])
    with pytest.raises(ValueError, match="CUDA"):
        warp.remap_nv12_to_nv12(torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8), m)
    with pytest.raises(ValueError, match="camera 1 has 1 frames"):
        warp.remap_stitch_nv12_to_nv12([y2, fake(8, 8)], [uv2, fake(4, 4, 2)], [m, m])


def test_frame_pipeline_refusals_that_remain():
    from bev_amd.pipeline import FramePipeline
    with pytest.raises(ValueError, match="warp_map .*planar"):
        FramePipeline((8, 8), 3, None, (8, 6), warp_map=_cpu_map(), planar=True)
    for kw in (dict(dst_format="nv12"), dict(src_format="nv12", dst_format="nv12")):
        with pytest.raises(ValueError, match="planar"):
            FramePipeline((8, 8), 3, None, (8, 6), warp_map=_cpu_map(), planar=True, **kw)
    # the map's own checks stand ahead of the format checks: a host map for a "cuda" pipeline is refused as such, whatever the slots
    for kw in (dict(src_format="nv12"), dict(dst_format="nv12"), dict(src_format="nv12", dst_format="nv12")):
        with pytest.raises(ValueError, match="warp_map is on"):
            FramePipeline((8, 8), 3, None, (8, 6), warp_map=_cpu_map(), **kw)
        with pytest.raises(ValueError, match="warp_map was built for dsize"):
            FramePipeline((8, 8), 3, None, (6, 8), warp_map=_cpu_map(), **kw)
    # NV12 slots keep their rules (a map that passes its own checks: the pipeline's device is the map's)
    odd = _cpu_map(dh=5, dw=7)
    with pytest.raises(ValueError, match="dst_format=\"nv12\" needs an even dsize"):
        FramePipeline((8, 8), 3, None, (7, 5), warp_map=odd, dst_format="nv12", device="cpu")
    with pytest.raises(ValueError, match="src_format=\"nv12\" needs even frame sides"):
        FramePipeline((7, 8), 3, None, (8, 6), warp_map=_cpu_map(), src_format="nv12", device="cpu")
    with pytest.raises(ValueError, match="channels=3 and dtype=torch.uint8"):
        FramePipeline((8, 8), 4, None, (8, 6), warp_map=_cpu_map(), dst_format="nv12", device="cpu")
    assert "bevwarp_remap_to_nv12" in FramePipeline.__init__.__doc__ and "bevwarp_remap_nv12_to_nv12" in FramePipeline.__init__.__doc__


# ---- the code objects: the expected instances, no scratch, no LDS, at most 128 VGPRs ----

def test_single_camera_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_map_nv12_out.hip", tmp_path, "warp_map_nv12_out.h")
    frames = {n: k for n, k in found.items() if "remap_to_nv12_kernel" in n}
    nv12 = {n: k for n, k in found.items() if "remap_nv12_to_nv12_kernel" in n}
    assert len(frames) == 2 * 5 * 2, len(frames)  # interpolation x border mode x channel order
    assert len(nv12) == 2 * 5, len(nv12)          # interpolation x border mode
    assert len(found) == len(frames) + len(nv12)
    codeobj.assert_lean(found)
    flags = codeobj.makefile_flags("warp_map_nv12_out.hip", "nv12_store.h")
    assert "-fno-fast-math" in flags and "-ffp-contract=off" in flags
    for header in ("remap_sample_u8x3.h", "remap_taps_u8x3.inc", "remap_frame_u8x3.inc", "remap_sample_nv12.h", "remap_taps_nv12.inc", "tap_load.h", "nv12_sample.h"):
        codeobj.makefile_flags("warp_map_nv12_out.hip", header)  # (both shared samplers rebuild the unit)


def test_stitch_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_stitch_maps_nv12_out.hip", tmp_path, "warp_stitch_maps_nv12_out.h")
    assert all("stitch_maps_nv12_out_kernel" in n for n in found)
    assert len(found) == 3 * 2 * 2, len(found)    # {B, G, R; R, G, B; NV12} x interpolation x blend
    codeobj.assert_lean(found)
    assert "-fno-fast-math" in codeobj.makefile_flags("warp_stitch_maps_nv12_out.hip", "nv12_store.h")
    for header in ("stitch_sample.h", "stitch_maps_u8x3.inc", "tap_load.h", "nv12_sample.h"):  # (the shared stitch samplers and camera loop rebuild the unit)
        codeobj.makefile_flags("warp_stitch_maps_nv12_out.hip", header)
