"""NV12 frames through a fixed camera's warp map (bevwarp_remap_nv12, bevwarp_remap_nv12_planes; remap_nv12, remap_nv12_to_planar) without
a device: the numpy definition (tests/remap_nv12_ref.py) tied to the oracle by bits, the C ABI's host checks under the sanitizers
(tests/host_plan_driver.cpp, family `remap_nv12`), the same statuses through the built library, the ABI surface, the Python entries' own refusals and
the kernels' code object."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import codeobj
from tests import hostplan
from tests import nv12_ref as NR
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests.test_abi import checked_declaration
from tests.test_lens_cpu import GEOMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
NAMES = ("bevwarp_remap_nv12", "bevwarp_remap_nv12_planes")


# ---- the definition tied to the oracle, by bits ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
@pytest.mark.parametrize("rgb", [False, True])
def test_pinhole_maps_reproduce_the_nv12_oracle(geom, interp, rgb):
    """remap of the converted frame through remap_ref.build's pinhole map IS the oracle's warp of the converted frame (CONSTANT)."""
    sw, sh, dw, dh, M = GEOMS[geom]
    xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
    for kind in ("uniform", "phase"):
        y, uv = NR.frame(kind, 3, sh, sw)
        for bv in (None, (7.0, 200.0, 31.0)):
            got = RN.remap_nv12(y, uv, xy, frac, interp, RR.CONSTANT, 0.0 if bv is None else bv, rgb=rgb)
            np.testing.assert_array_equal(got, NR.warp_nv12(y, uv, M, (dw, dh), interp, border_value=bv, rgb=rgb), err_msg="%s %s" % (kind, bv))


def test_plane_stage_is_planes16_refs():
    """remap_nv12_ref.planes_f32 restates planes16_ref.planes_f32's stage: equal on the oracle's own warp of a converted frame."""
    from tests import planes16_ref as P16
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    y, uv = NR.frame("uniform", 4, sh, sw)
    bgr = NR.nv12_to_bgr(y, uv)
    scale, bias = (1 / 255.0, 0.017, 3.0), (-0.4, 0.0, 11.5)
    xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, wn.LINEAR)
    got = RN.remap_nv12_planes(y, uv, xy, frac, wn.LINEAR, RR.CONSTANT, scale, bias, (9.0, 8.0, 7.0))
    np.testing.assert_array_equal(got.view(np.uint32), P16.planes_f32(bgr, M, (dw, dh), wn.LINEAR, scale, bias, (9.0, 8.0, 7.0)).view(np.uint32))


# ---- the host checks under the sanitizers ----

# an 8 x 8 frame: Y 64 bytes at 4096, four rows of four pairs at 8192; an 8 x 8 x 3 destination at 2^20 (planes: three float16 planes, rows
# 16 bytes, planes 128, frames 384); the maps at 2^24 and 2^26; never dereferenced
PIX = dict(y=4096, uv=8192, dst=1 << 20, xy=1 << 24, frac=1 << 26, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, y_fs=64, y_rs=8, uv_fs=32, uv_rs=8, dst_fs=192, dst_rs=24,
           map_count=1, xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16, interp=1, mode=0, rgb=0)
PLANES = dict(y=4096, uv=8192, dst=1 << 20, xy=1 << 24, frac=1 << 26, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, y_fs=64, y_rs=8, uv_fs=32, uv_rs=8, dst_fs=384, dst_ps=128,
              dst_rs=16, map_count=1, xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16, interp=1, mode=0, rgb=0, plane_dtype=_lib.F16)
NONE = [0, 0, 0]


def _pix(**kw):
    a = dict(PIX, **kw)
    return "pix " + " ".join(str(a[k]) for k in PIX)


def _planes(**kw):
    a = dict(PLANES, **kw)
    return "planes " + " ".join(str(a[k]) for k in PLANES)


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def _common_cases(call, dst_bytes, wide):
    """Cases both entries share.  call: _pix or _planes; dst_bytes: one frame of the destination (its bounding range); wide: keywords of
    a destination 2^20 + 1 rows high."""
    ok = [OK, OK, 1, 2]  # (an 8 x 8 destination: 2 tiles)
    D = 1 << 20
    three = dict(batch=3, y_fs=64, uv_fs=32)
    cases = [(call(), ok), (call(interp=0), ok), (call(interp=0, frac=0), ok), (call(rgb=1), ok), (call(batch=0), [OK] + NONE), (call(batch=0, map_count=7), [BAD_ARG] + NONE)]
    # 1. BEVWARP_ERR_BAD_ARG: null pointers (the frac plane under linear only), sizes, odd sides, layouts, an odd uv base or stride
    cases += [(call(**{k: 0}), [BAD_ARG] + NONE) for k in ("y", "uv", "dst", "xy", "frac", "src_h", "src_w", "dst_h", "dst_w")]
    cases += [(call(xy=0, interp=0), [BAD_ARG] + NONE), (call(batch=-1), [BAD_ARG] + NONE), (call(src_h=-8), [BAD_ARG] + NONE)]
    cases += [(call(src_h=7), [BAD_ARG] + NONE), (call(src_w=7), [BAD_ARG] + NONE), (call(src_h=6, src_w=6), ok), (call(dst_h=7, dst_w=5), ok)]
    cases += [(call(y_rs=7), [BAD_ARG] + NONE), (call(uv_rs=6), [BAD_ARG] + NONE), (call(uv=8193), [BAD_ARG] + NONE), (call(uv_rs=9), [BAD_ARG] + NONE),
              (call(uv_fs=33), [BAD_ARG] + NONE), (call(y=4097, y_rs=9, y_fs=73), ok),                                     # (the Y plane takes any base and stride)
              (call(batch=2, map_count=1, y_fs=63), [BAD_ARG] + NONE), (call(batch=2, map_count=1, uv_fs=30), [BAD_ARG] + NONE)]
    cases += [(call(xy=(1 << 24) + 2), [BAD_ARG] + NONE), (call(xy_rs=34), [BAD_ARG] + NONE), (call(xy_rs=28), [BAD_ARG] + NONE), (call(frac=(1 << 26) + 1), [BAD_ARG] + NONE),
              (call(frac_rs=17), [BAD_ARG] + NONE), (call(frac_rs=14), [BAD_ARG] + NONE), (call(xy=(1 << 24) + 4, frac=(1 << 26) + 2), ok),
              (call(frac=(1 << 26) + 1, frac_rs=3, interp=0), ok)]                                                          # (nearest: the frac plane is not looked at)
    # ... the map count: 1 or the batch; a shared map's frame strides are not looked at, per-frame maps must not overlap their successors
    cases += [(call(map_count=0), [BAD_ARG] + NONE), (call(map_count=2), [BAD_ARG] + NONE), (call(map_count=2, **three), [BAD_ARG] + NONE),
              (call(map_count=0, **three), [BAD_ARG] + NONE), (call(map_count=3, **three), [OK, OK, 1, 6]), (call(map_count=1, **three), [OK, OK, 1, 6]),
              (call(map_count=1, xy_fs=1, frac_fs=1, **three), [OK, OK, 1, 6]), (call(map_count=3, xy_fs=255, **three), [BAD_ARG] + NONE),
              (call(map_count=3, xy_fs=258, **three), [BAD_ARG] + NONE), (call(map_count=3, frac_fs=127, **three), [BAD_ARG] + NONE)]
    # 2. BEVWARP_ERR_UNSUPPORTED, after every bad argument and before the size limits
    cases += [(call(interp=i), [UNSUPPORTED] + NONE) for i in (2, 3, -1)] + [(call(rgb=r), [UNSUPPORTED] + NONE) for r in (2, -1)]
    cases += [(call(mode=m), [UNSUPPORTED] + NONE) for m in (6, 16, -1, 100)]
    cases += [(call(mode=6, map_count=2), [BAD_ARG] + NONE), (call(interp=2, xy_rs=28), [BAD_ARG] + NONE), (call(mode=6, src_h=7), [BAD_ARG] + NONE),
              (call(interp=2, frac=0), [UNSUPPORTED] + NONE),                                                              # (no frac plane is asked of an interpolation that has none)
              (call(mode=6, src_w=32768, y_rs=32768, uv_rs=32768), [UNSUPPORTED] + NONE)]
    # 3. BEVWARP_ERR_TOO_LARGE, per source plane; the map planes have no such limit
    cases += [(call(src_w=32768, y_rs=32768, uv_rs=32768), [TOO_LARGE] + NONE), (call(src_h=32768), [TOO_LARGE] + NONE), (call(y_rs=1 << 24), [TOO_LARGE] + NONE),
              (call(uv_rs=1 << 24), [TOO_LARGE] + NONE), (call(y_rs=(1 << 24) - 1, dst=1 << 40), ok), (call(uv_rs=(1 << 24) - 2, dst=1 << 40), ok),
              (call(src_w=32768, y_rs=32768, uv_rs=32768, dst=4096), [TOO_LARGE] + NONE)]                                   # ... before the overlap
    # 4. BEVWARP_ERR_OVERLAP: dst against each of the four read images
    cases += [(call(dst=4096), [OVERLAP] + NONE), (call(dst=4096 + 62), [OVERLAP] + NONE), (call(dst=4096 + 64), ok), (call(dst=4096 - dst_bytes), ok),
              (call(dst=4096 - dst_bytes + 2), [OVERLAP] + NONE),
              (call(dst=8192), [OVERLAP] + NONE), (call(dst=8192 + 30), [OVERLAP] + NONE), (call(dst=8192 + 32), ok), (call(dst=8192 - dst_bytes + 2), [OVERLAP] + NONE),
              (call(xy=D), [OVERLAP] + NONE), (call(xy=D + dst_bytes - 4), [OVERLAP] + NONE), (call(xy=D + dst_bytes), ok), (call(xy=D - 252), [OVERLAP] + NONE),
              (call(xy=D - 256), ok),
              (call(frac=D + dst_bytes - 2), [OVERLAP] + NONE), (call(frac=D + dst_bytes), ok), (call(frac=D - 126), [OVERLAP] + NONE), (call(frac=D - 128), ok),
              (call(frac=D + 100, interp=0), ok),                                                                           # (nearest: not read)
              (call(xy=4096, frac=4096 + 64), ok), (call(uv=4096 + 8, y=4096), ok)]                                          # the read images may overlap each other
    # 5. BEVWARP_ERR_TOO_LARGE from the launch plan, after the overlap
    cases += [(call(**wide), [OK, TOO_LARGE, 0, 0]), (call(**dict(wide, dst=4096)), [OVERLAP] + NONE)]
    return cases


def test_remap_nv12_call_under_sanitizers(driver):
    huge = (1 << 63) - 1
    w20 = 1 << 20
    cases = _common_cases(_pix, 192, dict(dst_h=w20 + 1, dst_fs=1 << 26, dst=1 << 40, xy=1 << 44, frac=1 << 48))
    cases += [(_pix(mode=m, interp=i, rgb=r), [OK, OK, 1, 2]) for m in range(6) for i in (0, 1) for r in (0, 1)]      # all six borders
    cases += [(_pix(dst_rs=23), [BAD_ARG] + NONE), (_pix(batch=2, dst_fs=191, y_fs=64, uv_fs=32), [BAD_ARG] + NONE)]
    # the frames-per-item plan: 32 frames through a shared 1024^2 map, and through per-frame maps
    big = dict(batch=32, dst_h=1024, dst_w=1024, dst_rs=3072, dst_fs=3072 * 1024, dst=1 << 40, xy=1 << 44, frac=1 << 48, xy_rs=4096, xy_fs=1 << 22, frac_rs=2048, frac_fs=1 << 21)
    cases += [(_pix(map_count=1, **big), [OK, OK, 2, 16 * 1024]), (_pix(map_count=32, **big), [OK, OK, 1, 32 * 1024])]
    # destination sides at 2^20
    one = dict(dst=1 << 40, xy=1 << 44, frac=1 << 48)
    cases += [(_pix(dst_w=w20, dst_h=1, dst_rs=3 * w20, dst_fs=3 * w20, xy_rs=4 * w20, frac_rs=2 * w20, **one), [OK, OK, 1, 4096]),
              (_pix(dst_w=w20 + 1, dst_h=1, dst_rs=4 * w20, dst_fs=4 * w20, xy_rs=8 * w20, frac_rs=4 * w20, **one), [OK, TOO_LARGE, 0, 0])]
    # strides next to 2^63: bad arguments or size limits, not overflows (one row, or two frames: the images' last bytes stay below 2^64)
    cases += [(_pix(dst_h=1, xy_rs=huge - 3, frac_rs=huge - 1, dst_rs=huge), [OK, OK, 1, 1]),
              (_pix(batch=2, map_count=2, dst_h=1, xy_fs=huge - 3, frac_fs=huge - 1, dst_fs=192), [OK, OK, 1, 2]),
              (_pix(batch=2, map_count=2, xy_rs=huge - 3, xy_fs=huge - 3), [BAD_ARG] + NONE), (_pix(batch=2, map_count=2, frac_rs=huge - 1, frac_fs=huge - 1), [BAD_ARG] + NONE),
              (_pix(batch=3, dst_rs=huge, dst_fs=huge), [BAD_ARG] + NONE), (_pix(y_rs=huge), [TOO_LARGE] + NONE), (_pix(uv_rs=huge - 1), [TOO_LARGE] + NONE),
              (_pix(uv_rs=huge), [BAD_ARG] + NONE), (_pix(batch=2, y_rs=huge, y_fs=huge), [BAD_ARG] + NONE), (_pix(batch=2, uv_fs=huge - 1, y_fs=huge, dst=16), [OK, OK, 1, 4])]
    hostplan.check_cases(driver, cases, "remap_nv12")


def test_remap_nv12_planes_call_under_sanitizers(driver):
    huge = (1 << 63) - 1
    w20 = 1 << 20
    cases = _common_cases(_planes, 384, dict(dst_h=w20 + 1, dst_ps=16 * (w20 + 1), dst_fs=48 * (w20 + 1), dst=1 << 40, xy=1 << 44, frac=1 << 48))
    ok = [OK, OK, 1, 2]
    f32 = dict(plane_dtype=_lib.F32, dst_rs=32, dst_ps=256, dst_fs=768)
    # the five writing borders; TRANSPARENT joins the unsupported formats
    cases += [(_planes(mode=m, interp=i, plane_dtype=pd), ok) for m in range(5) for i in (0, 1) for pd in (_lib.F16, _lib.BF16)]
    cases += [(_planes(mode=m, **f32), ok) for m in range(5)]
    cases += [(_planes(mode=5), [UNSUPPORTED] + NONE), (_planes(mode=5, **f32), [UNSUPPORTED] + NONE), (_planes(mode=5, map_count=2), [BAD_ARG] + NONE),
              (_planes(mode=5, src_h=32768), [UNSUPPORTED] + NONE)]
    cases += [(_planes(plane_dtype=pd), [UNSUPPORTED] + NONE) for pd in (_lib.U8, _lib.F64, 5, -1)]
    # the destination's layout: element-size alignment, rows, planes and frames that hold their contents
    cases += [(_planes(dst_rs=17), [BAD_ARG] + NONE), (_planes(dst_ps=129), [BAD_ARG] + NONE), (_planes(dst_fs=385), [BAD_ARG] + NONE), (_planes(dst=(1 << 20) + 1), [BAD_ARG] + NONE),
              (_planes(dst_rs=14), [BAD_ARG] + NONE), (_planes(dst_ps=126), [BAD_ARG] + NONE), (_planes(batch=2, y_fs=64, uv_fs=32, dst_fs=382), [BAD_ARG] + NONE),
              (_planes(dst_rs=18, dst_ps=144, dst_fs=432), ok), (_planes(**dict(f32, dst_rs=34)), [BAD_ARG] + NONE), (_planes(**dict(f32, dst_rs=28)), [BAD_ARG] + NONE),
              (_planes(dst_rs=14, plane_dtype=7), [UNSUPPORTED] + NONE), (_planes(dst_rs=7, plane_dtype=7), [BAD_ARG] + NONE)]   # (an unknown plane type: 1-byte elements)
    cases += [(_planes(dst_h=1, xy_rs=huge - 3, frac_rs=huge - 1, dst_rs=1 << 62, dst_ps=1 << 62, xy=256, frac=512), [OK, OK, 1, 1]), (_planes(dst_ps=huge - 1, dst_fs=huge - 1, batch=2), [BAD_ARG] + NONE),
              (_planes(y_rs=huge), [TOO_LARGE] + NONE), (_planes(batch=2, map_count=2, xy_rs=huge - 3, xy_fs=huge - 3), [BAD_ARG] + NONE)]
    hostplan.check_cases(driver, cases, "remap_nv12")


# ---- the same statuses through the built library (fake pointers, never dereferenced: every call below fails validation or launches nothing) ----

def test_abi_surface_and_statuses_through_the_library():
    lib = hostplan.built_lib()
    assert lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "#define BEVWARP_ABI_VERSION 7" in header
    for name, nargs, n64 in zip(NAMES, (26, 30), (10, 11)):
        decl = checked_declaration(name, nargs, n64)
        for arg in ("map_xy", "map_frac", "map_count", "border_mode", "rgb_order", "uv_row_stride"):
            assert arg in decl, (name, arg)
    assert "bevwarp_remap_nv12, bevwarp_remap_nv12_planes" in header.split("Conventions")[0]
    from bev import warp as dropin
    from bev_amd import warp
    assert dropin.remap_nv12 is warp.remap_nv12 and dropin.remap_nv12_to_planar is warp.remap_nv12_to_planar

    P = ctypes.c_void_p
    vec = lambda *v: ctypes.cast((ctypes.c_double * 3)(*v), P)  # noqa: E731
    nan3 = vec(1.0, float("nan"), 1.0)

    def pix(**kw):
        a = dict(PIX, bv=nan3, **kw) if "bv" not in kw else dict(PIX, **kw)
        return lib.bevwarp_remap_nv12(P(a["y"]), P(a["uv"]), P(a["dst"]), a["batch"], a["src_h"], a["src_w"], a["dst_h"], a["dst_w"], a["y_fs"], a["y_rs"], a["uv_fs"],
                                      a["uv_rs"], a["dst_fs"], a["dst_rs"], P(a["xy"]), P(a["frac"]), a["map_count"], a["xy_fs"], a["xy_rs"], a["frac_fs"], a["frac_rs"],
                                      a["interp"], a["mode"], a["rgb"], a["bv"], None)

    def planes(scale=None, bias=None, **kw):
        a = dict(PLANES, bv=nan3, **kw) if "bv" not in kw else dict(PLANES, **kw)
        return lib.bevwarp_remap_nv12_planes(P(a["y"]), P(a["uv"]), P(a["dst"]), a["batch"], a["src_h"], a["src_w"], a["dst_h"], a["dst_w"], a["y_fs"], a["y_rs"],
                                             a["uv_fs"], a["uv_rs"], a["dst_fs"], a["dst_ps"], a["dst_rs"], P(a["xy"]), P(a["frac"]), a["map_count"], a["xy_fs"],
                                             a["xy_rs"], a["frac_fs"], a["frac_rs"], a["interp"], a["mode"], a["rgb"], a["bv"], scale, bias, a["plane_dtype"], None)

    for call in (pix, planes):
        # (P(0) is a null pointer.)  Otherwise valid: refused on the border value alone, after every other check and before any launch
        assert call() == NOT_FINITE and call(interp=0, frac=0) == NOT_FINITE and call(rgb=1) == NOT_FINITE
        assert call(batch=0) == OK and call(batch=0, bv=None) == OK
        # 1. BAD_ARG
        for k in ("y", "uv", "dst", "xy", "frac", "src_h", "dst_w"):
            assert call(**{k: 0}) == BAD_ARG, k
        assert call(src_h=7) == BAD_ARG and call(src_w=7) == BAD_ARG and call(uv=8193) == BAD_ARG and call(uv_rs=9) == BAD_ARG and call(uv_fs=33) == BAD_ARG
        assert call(y_rs=7) == BAD_ARG and call(xy=(1 << 24) + 2) == BAD_ARG and call(frac=(1 << 26) + 1) == BAD_ARG and call(xy_rs=28) == BAD_ARG
        assert call(map_count=0) == BAD_ARG and call(map_count=2) == BAD_ARG and call(batch=3, map_count=2) == BAD_ARG
        assert call(map_count=2, interp=2) == BAD_ARG and call(xy_rs=28, mode=6) == BAD_ARG          # bad arguments come before unsupported ones ...
        # 2. UNSUPPORTED
        assert call(interp=2) == UNSUPPORTED and call(rgb=2) == UNSUPPORTED and call(mode=6) == UNSUPPORTED and call(mode=-1) == UNSUPPORTED
        assert call(mode=6, src_w=32768, y_rs=32768, uv_rs=32768) == UNSUPPORTED                       # ... which come before the size limits
        # 3. TOO_LARGE, per source plane, before the overlap
        assert call(src_w=32768, y_rs=32768, uv_rs=32768) == TOO_LARGE and call(src_h=32768) == TOO_LARGE and call(uv_rs=1 << 24) == TOO_LARGE
        assert call(src_h=32768, dst=4096) == TOO_LARGE
        # 4. OVERLAP with each of the four read images, before the launch plan's limit and the border value
        assert call(dst=4096 + 62) == OVERLAP and call(dst=8192 + 30) == OVERLAP and call(xy=1 << 20) == OVERLAP and call(frac=(1 << 20) + 100) == OVERLAP
        assert call(frac=(1 << 20) + 100, interp=0) == NOT_FINITE                                      # (nearest: the frac plane is not read)
        # 6. NOT_FINITE for border_value under CONSTANT only (the other modes launch -- not without a device: an empty batch stands in)
        assert call(bv=vec(0.0, 0.0, float("inf"))) == NOT_FINITE and call(mode=1, batch=0) == OK
    for m in range(1, 6):
        assert pix(mode=m, batch=0) == OK
    assert planes(mode=5) == UNSUPPORTED and planes(mode=4, batch=0) == OK and planes(plane_dtype=_lib.U8) == UNSUPPORTED
    assert planes(dst_rs=17) == BAD_ARG and planes(dst_ps=126) == BAD_ARG
    w20 = 1 << 20
    assert pix(dst_h=w20 + 1, dst_fs=1 << 26, dst=1 << 40, xy=1 << 44, frac=1 << 48) == TOO_LARGE    # 5. the launch plan, before the border value
    assert planes(dst_h=w20 + 1, dst_ps=16 * (w20 + 1), dst_fs=48 * (w20 + 1), dst=1 << 40, xy=1 << 44, frac=1 << 48, scale=vec(1.0, float("inf"), 1.0)) == TOO_LARGE
    good = vec(1.0, 2.0, 3.0)
    for slot in ("scale", "bias"):
        for i in range(3):
            v = [1.0, 2.0, 3.0]
            v[i] = float("inf") if i else float("nan")
            assert planes(bv=good, **{slot: vec(*v)}) == NOT_FINITE
            assert planes(bv=good, mode=2, **{slot: vec(*v)}) == NOT_FINITE   # (scale and bias are looked at under every border)


# ---- the Python entries ----

class _ClaimsCuda(torch.Tensor):
    """A host tensor that answers is_cuda: the shape checks run without a device (nothing after them is reached)."""
    is_cuda = property(lambda self: True)


def _cpu_map(n=1, dh=6, dw=5, interp=1, device="cpu"):
    from bev_amd import warp
    return warp.WarpMap(torch.zeros((n, dh, dw, 2), dtype=torch.int16, device=device), torch.zeros((n, dh, dw), dtype=torch.int16, device=device) if interp else None,
                        interp, (dw, dh))


def test_python_entries_validate_before_the_device():
    from bev_amd import warp
    from bev_amd.pipeline import FramePipeline
    fake = lambda *shape: torch.zeros(shape, dtype=torch.uint8).as_subclass(_ClaimsCuda)  # noqa: E731
    y2, uv2 = fake(2, 8, 8), fake(2, 4, 4, 2)
    for f in (warp.remap_nv12, warp.remap_nv12_to_planar):
        with pytest.raises(ValueError, match="needs a WarpMap"):
            f(y2, uv2, (torch.zeros((1, 6, 5, 2), dtype=torch.int16), None))
        with pytest.raises(ValueError, match="border mode"):
            f(y2, uv2, _cpu_map(), border_mode=6)
        with pytest.raises(ValueError, match="CUDA"):
            f(torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8), _cpu_map())
        for ys, uvs in (((7, 8), (3, 4, 2)), ((8, 7), (4, 3, 2)), ((2, 7, 8), (2, 3, 4, 2))):   # odd source sides
            with pytest.raises(ValueError, match="even sides"):
                f(fake(*ys), fake(*uvs), _cpu_map())
        with pytest.raises(ValueError, match="uv of shape"):
            f(fake(8, 8), fake(4, 8, 2), _cpu_map())
        with pytest.raises(ValueError, match="contiguous"):
            f(fake(8, 16)[:, ::2], fake(4, 4, 2), _cpu_map())
        with pytest.raises(ValueError, match="holds 3 frames for a batch of 2"):
            f(y2, uv2, _cpu_map(n=3))
        with pytest.raises(ValueError, match="holds 2 frames for a batch of 1"):
            f(fake(8, 8), fake(4, 4, 2), _cpu_map(n=2))
        with pytest.raises(ValueError, match="the map is on"):
            f(y2, uv2, _cpu_map(device="meta"))
        assert "FramePipeline" in f.__doc__ and "out=" in f.__doc__ and "stream of its own" in f.__doc__
    with pytest.raises(ValueError, match="dsize is"):
        warp.remap_nv12(y2, uv2, _cpu_map(), out=torch.zeros((2 * 6 * 5 * 3 + 1,), dtype=torch.uint8))
    with pytest.raises(ValueError, match="dsize is"):  # an `out` of the result's rank with height and width swapped: the element count fits, the shape does not
        warp.remap_nv12(y2, uv2, _cpu_map(), out=torch.zeros((2, 5, 6, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="dsize is"):
        warp.remap_nv12(fake(8, 8), fake(4, 4, 2), _cpu_map(), out=torch.zeros((5, 6, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="dsize is"):
        warp.remap_nv12_to_planar(y2, uv2, _cpu_map(), out=torch.zeros((2, 3, 5, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="BORDER_TRANSPARENT"):
        warp.remap_nv12_to_planar(y2, uv2, _cpu_map(), border_mode=warp.BORDER_TRANSPARENT)
    with pytest.raises(ValueError, match="out_dtype"):
        warp.remap_nv12_to_planar(y2, uv2, _cpu_map(), out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out must be"):
        warp.remap_nv12_to_planar(y2, uv2, _cpu_map(), out_dtype=torch.float16, out=torch.zeros((2, 3, 6, 5), dtype=torch.float32))
    # the pipeline keeps refusing a map together with NV12 slots: streaming callers call the two functions with out=
    with pytest.raises(ValueError, match="warp_map"):
        FramePipeline((8, 8), 3, None, (5, 6), warp_map=_cpu_map(), src_format="nv12")


def test_nv12_planes_helper_takes_no_matrix():
    from bev_amd import warp
    fake = lambda *shape: torch.zeros(shape, dtype=torch.uint8).as_subclass(_ClaimsCuda)  # noqa: E731
    y3, uv4 = warp._nv12_planes("f", fake(8, 8), fake(4, 4, 2))
    assert y3.shape == (1, 8, 8) and uv4.shape == (1, 4, 4, 2)
    frame = fake(2, 12, 8)
    y, uv = warp.split_nv12(frame)
    y3, uv4 = warp._nv12_planes("f", y, uv)  # split_nv12's views are passed through
    assert y3.data_ptr() == frame.data_ptr() and y3.stride() == (96, 8, 1) and uv4.stride() == (96, 8, 2, 1) and uv4.data_ptr() == frame.data_ptr() + 64


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_nv12_map_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_map_nv12.hip", tmp_path, header="warp_map_nv12.h")
    pixels = {n: k for n, k in found.items() if "remap_nv12_kernel" in n}
    planes = {n: k for n, k in found.items() if "remap_nv12_planes_kernel" in n}
    assert len(pixels) == 2 * 6 * 2, len(pixels)  # interpolation x border x channel order
    assert len(planes) == 2 * 5 * 2, len(planes)  # interpolation x writing border x (float32 | 16-bit planes)
    assert len(found) == len(pixels) + len(planes)
    codeobj.assert_lean(found)
    for header in ("map_entry.h", "map_entry_taps.inc", "plane_store.inc", "nv12_sample.h"):  # (the shared stages rebuild both of their users)
        codeobj.makefile_flags("warp_map.hip" if header.startswith("map_entry") else "warp_nv12_planes.hip", header)
    for header in ("remap_sample_nv12.h", "remap_taps_nv12.inc", "nv12_sample.h"):  # (the NV12 map sampler, shared with the NV12-out unit)
        for unit in ("warp_map_nv12.hip", "warp_map_nv12_out.hip"):
            codeobj.makefile_flags(unit, header)
