"""The multi-camera warp (bevwarp_warp_stitch, warp_stitch) without a device: the numpy reference (tests/stitch_ref.py) against the
one-call-per-camera route of tests/border_ref.py and against hand-computed weights, the C ABI's host checks through the loaded library
and under the sanitizers (tests/host_plan_driver.cpp, the `stitch` family), the kernels' code object, the ABI surface and the Python entry's own checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle.warp_numpy import LINEAR, NEAREST
from tests import border_ref as BR
from tests import codeobj
from tests import hostplan
from tests import stitch_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the scene of tests/test_gpu_stitch.py: (w, h, inverse map) per camera, canvas 260 x 22
SCENE = [(40, 24, np.array([[0.30, 0.20, -4], [0.01, 0.90, -1], [0.0004, 0, 1]])),
         (64, 18, np.array([[0.38, 0, -36], [0.02, 0.80, -3], [0, 0, 1]])),
         (31, 33, np.array([[-0.35, 0, 80], [0, 1.40, -2], [0, 0.001, 1]]))]
DSIZE = (260, 22)


def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


def _scene(dtype, c=3):
    return [_src((h, w, c), dtype, seed=30 + k) for k, (w, h, _) in enumerate(SCENE)], [M for _, _, M in SCENE]


# ---- the reference against the route that exists ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_over_is_the_chain_of_transparent_warps(dtype, interp):
    srcs, Ms = _scene(dtype)
    canvas = np.full((DSIZE[1], DSIZE[0], 3), 77, dtype)
    chain = canvas
    for s, M in zip(srcs, Ms):
        chain = BR.warp(s, M, DSIZE, interp, BR.TRANSPARENT, m_is_inverse=True, canvas=chain)
    got, count = SR.stitch(srcs, Ms, DSIZE, interp, SR.OVER, mode=SR.TRANSPARENT, canvas=canvas)
    np.testing.assert_array_equal(got, chain)
    assert (got[count == 0] == 77).all()
    const, _ = SR.stitch(srcs, Ms, DSIZE, interp, SR.OVER, mode=SR.CONSTANT, border_value=(3, 200, 41))
    np.testing.assert_array_equal(const[count > 0], chain[count > 0])
    assert (const[count == 0] == np.array([3, 200, 41], dtype)).all()
    back, _ = SR.stitch(srcs[::-1], Ms[::-1], DSIZE, interp, SR.OVER, mode=SR.TRANSPARENT, canvas=canvas)
    assert not np.array_equal(back, got)  # (the order of the list decides the overlaps)


def test_scene_holds_every_cover_class():
    """What the GPU tests rely on: the counts of pixels covered by 0 / 1 / 2 / 3 cameras, and covered pixels in the second tile column."""
    srcs, Ms = _scene(np.uint8)
    for interp, want in ((NEAREST, [210, 2736, 2681, 93]), (LINEAR, [314, 2802, 2561, 43])):
        _, count = SR.stitch(srcs, Ms, DSIZE, interp)
        assert [int((count == n).sum()) for n in range(4)] == want
        assert (count[:, 256:] > 0).any()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_feather_single_cover_is_the_cameras_own_warp(dtype, interp):
    srcs, Ms = _scene(dtype)
    for F in (1, 3, 64):
        got, count = SR.stitch(srcs, Ms, DSIZE, interp, SR.FEATHER, F, mode=SR.TRANSPARENT)
        over, _ = SR.stitch(srcs, Ms, DSIZE, interp, SR.OVER, mode=SR.TRANSPARENT)
        np.testing.assert_array_equal(got[count <= 1], over[count <= 1])
        for s, (w, h, M) in zip(srcs, SCENE):
            mine = BR.written_mask((h, w), M, DSIZE, interp, m_is_inverse=True) & (count == 1)
            assert mine.any()
            np.testing.assert_array_equal(got[mine], BR.warp(s, M, DSIZE, interp, BR.TRANSPARENT, m_is_inverse=True)[mine])
        assert not np.array_equal(got[count >= 2], over[count >= 2])


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_two_identical_cameras_give_that_camera(interp):
    """(w p + w p + ((2 w) >> 1)) / (2 w) = p + 1 / 2, truncated: p."""
    w, h, M = SCENE[0]
    s = _src((h, w, 3), np.uint8, seed=5)
    for F in (1, 7, 4096):
        got, count = SR.stitch([s, s], [M, M], DSIZE, interp, SR.FEATHER, F, mode=SR.TRANSPARENT)
        assert set(np.unique(count)) == {0, 2}
        np.testing.assert_array_equal(got, BR.warp(s, M, DSIZE, interp, BR.TRANSPARENT, m_is_inverse=True))


def test_feather_is_the_weighted_mean_by_hand():
    """Two 1-channel cameras under the identity: camera 0 is 6 x 5 of 10s, camera 1 is 6 x 5 of 200s shifted two pixels to the right."""
    a, b = np.full((5, 6), 10, np.uint8), np.full((5, 6), 200, np.uint8)
    shift = np.array([[1.0, 0, -2], [0, 1, 0], [0, 0, 1]])  # canvas x -> camera x - 2
    got, count = SR.stitch([a, b], [np.eye(3), shift], (8, 5), NEAREST, SR.FEATHER, 64, mode=SR.CONSTANT, border_value=7)
    assert count[2].tolist() == [1, 1, 2, 2, 2, 2, 1, 1]
    # row 2 (sy = 2: d_y = 3): camera 0 at x = 2..5 has d = min(x + 1, 6 - x, 3) = 3, 3, 2, 1; camera 1 at sx = 0..3 has 1, 2, 3, 3
    want = [(3 * 10 + 1 * 200 + 2) // 4, (3 * 10 + 2 * 200 + 2) // 5, (2 * 10 + 3 * 200 + 2) // 5, (1 * 10 + 3 * 200 + 2) // 4]
    assert got[2].tolist() == [10, 10] + want + [200, 200]
    # F = 1: the plain mean, rounded half up
    mean, _ = SR.stitch([a, b], [np.eye(3), shift], (8, 5), NEAREST, SR.FEATHER, 1)
    assert mean[2].tolist() == [10, 10, 105, 105, 105, 105, 200, 200]
    # float32: acc = (0 + w0 p0) + w1 p1 in float32, then one division
    fa, fb = np.full((5, 6), 0.1, np.float32), np.full((5, 6), 0.7, np.float32)
    gotf, _ = SR.stitch([fa, fb], [np.eye(3), shift], (8, 5), NEAREST, SR.FEATHER, 64)
    f = np.float32
    assert gotf[2, 3] == (f(0) + f(3) * f(0.1) + f(2) * f(0.7)) / f(5)
    assert gotf[2, 0] == f(0.1) and gotf[2, 7] == f(0.7)


def test_edge_distance_by_hand():
    w, h = 40, 24
    d = SR.edge_distance
    assert d(0, 0, w, h) == 1 and d(w - 1, 0, w, h) == 1 and d(0, h - 1, w, h) == 1 and d(w - 1, h - 1, w, h) == 1  # corners
    assert d(5, 0, w, h) == 1 and d(0, 7, w, h) == 1 and d(5, h - 1, w, h) == 1 and d(w - 1, 7, w, h) == 1          # edges
    assert d(5, 7, w, h) == 6 and d(36, 7, w, h) == 4 and d(20, 20, w, h) == 4 and d(20, 11, w, h) == 12 and d(20, 12, w, h) == 12
    # through the maps, under the identity: nearest covers the whole frame, bilinear all but the last column and row (whose d is 2)
    s = _src((h, w), np.uint8, seed=1)
    for interp, last in ((NEAREST, 1), (LINEAR, 2)):
        (cover, _, wk), = SR.cameras([s], [np.eye(3)], (w, h), interp, 4096)
        assert cover.sum() == (w * h if interp == NEAREST else (w - 1) * (h - 1))
        assert wk[0, 0] == 1 and wk[7, 5] == 6 and wk[11, 20] == 12
        assert wk[h - last, 20] == last and wk[7, w - last] == last
        if interp == LINEAR:
            assert not cover[h - 1].any() and not cover[:, w - 1].any() and not wk[h - 1].any()
        (_, _, cut), = SR.cameras([s], [np.eye(3)], (w, h), interp, 5)
        assert cut.max() == 5 and cut[7, 5] == 5 and cut[2, 20] == 3


# ---- the ABI surface, without a device (fake pointers, never dereferenced: every call below fails validation first or has no frame) ----

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
DST = 1 << 20


def _cam(src=16, m=16, fs=192, rs=24, h=8, w=8, m_count=1):
    return _lib.Camera(src, m, fs, rs, h, w, m_count, 0)


def _call(lib, cams, n=None, cams_null=False, dst=DST, batch=1, dh=8, dw=8, ch=3, dfs=192, drs=24, dtype=_lib.U8, interp=1, blend=0, feather=64, mode=0, bv=None):
    arr = (_lib.Camera * max(len(cams), 1))(*cams)
    border = None if bv is None else ctypes.cast((ctypes.c_double * len(bv))(*bv), ctypes.c_void_p)
    return lib.bevwarp_warp_stitch(None if cams_null else ctypes.addressof(arr), len(cams) if n is None else n, dst, batch, dh, dw, ch, dfs, drs, dtype, interp,
                                   blend, feather, mode, border, None)


def test_abi_surface():
    lib = hostplan.built_lib()
    assert "bevwarp_warp_stitch" in _lib.SYMBOLS and lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), "bevwarp_warp_stitch") is not None
    assert ctypes.sizeof(_lib.Camera) == 48
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "int bevwarp_warp_stitch(const bevwarp_camera *cams /*HOST*/, int n_cams, void *dst, int batch," in header
    assert "#define BEVWARP_STITCH_MAX_CAMERAS 8" in header and "#define BEVWARP_STITCH_OVER 0" in header and "#define BEVWARP_STITCH_FEATHER 1" in header
    assert "bev/constructor/homo_constr.py:19-25" in header.split("Conventions")[0]  # (in the table of entries)
    assert "warping several cameras into one canvas, one call each" in header.split("typedef struct bevwarp_camera")[0].split("bevwarp_warp_lens(")[-1]
    import bev.warp as bev_warp
    from bev_amd import warp
    assert bev_warp.warp_stitch is warp.warp_stitch


def test_status_order_through_the_library():
    lib = hostplan.built_lib()
    nan = [0.0, float("nan"), 0.0]  # a call that passes every check of the cameras fails on this: nothing is launched
    good = _cam()
    assert _call(lib, [good], batch=0) == OK and _call(lib, [good] * 8, batch=0) == OK
    assert _call(lib, [good], bv=nan) == NOT_FINITE and _call(lib, [good] * 8, bv=nan) == NOT_FINITE
    # 1. the call's own arguments, before any camera or format is looked at
    assert _call(lib, [good], cams_null=True) == BAD_ARG and _call(lib, [], n=0) == BAD_ARG and _call(lib, [good] * 9) == BAD_ARG and _call(lib, [good], n=-1) == BAD_ARG
    assert _call(lib, [good] * 9, interp=2) == BAD_ARG and _call(lib, [_cam(src=None)] * 9) == BAD_ARG
    for f, want in ((0, BAD_ARG), (4097, BAD_ARG), (-1, BAD_ARG), (1, NOT_FINITE), (4096, NOT_FINITE)):
        assert _call(lib, [good], blend=1, feather=f, bv=nan) == want, f
        assert _call(lib, [good], blend=0, feather=f, bv=nan) == NOT_FINITE, f  # OVER ignores it
    assert _call(lib, [good], blend=1, feather=0, interp=2) == BAD_ARG
    # 2. per camera: the format (blend and border mode are part of it), then the rest in bevwarp_warp's order
    assert _call(lib, [good], blend=2, feather=0) == UNSUPPORTED and _call(lib, [good], blend=-1) == UNSUPPORTED
    for mode in (1, 2, 3, 4, 6, 16):
        assert _call(lib, [good], mode=mode) == UNSUPPORTED, mode
    assert _call(lib, [good], interp=2) == UNSUPPORTED and _call(lib, [good], dtype=_lib.F16) == UNSUPPORTED and _call(lib, [good], ch=5) == UNSUPPORTED
    assert _call(lib, [good], dst=None) == BAD_ARG and _call(lib, [_cam(m=None)]) == BAD_ARG and _call(lib, [good], batch=-1) == BAD_ARG
    assert _call(lib, [_cam(m_count=2)]) == BAD_ARG and _call(lib, [_cam(rs=23)]) == BAD_ARG and _call(lib, [good], drs=23) == BAD_ARG
    wide = _cam(w=40000, rs=120000, fs=960000)
    assert _call(lib, [wide], dst=1 << 30) == TOO_LARGE
    # a bad third camera is reported while the first two are fine; the first bad camera decides, not the first phase
    assert _call(lib, [good, good, _cam(src=None)]) == BAD_ARG
    assert _call(lib, [good, good, _cam(m_count=3)], batch=2, dfs=192) == BAD_ARG
    assert _call(lib, [good, good, wide], dst=1 << 30) == TOO_LARGE
    assert _call(lib, [good, good, _cam(h=0)]) == BAD_ARG
    assert _call(lib, [wide, _cam(src=None)], dst=1 << 30) == TOO_LARGE and _call(lib, [_cam(src=None), wide], dst=1 << 30) == BAD_ARG
    # dst against every camera; the cameras may share bytes
    assert _call(lib, [good, _cam(src=4096), _cam(src=DST)]) == OVERLAP
    assert _call(lib, [good, _cam(src=4096), _cam(src=DST + 191)]) == OVERLAP and _call(lib, [good, _cam(src=4096), _cam(src=DST - 191)]) == OVERLAP
    assert _call(lib, [good, _cam(src=4096), _cam(src=DST + 192)], bv=nan) == NOT_FINITE  # adjacent is fine
    assert _call(lib, [_cam(src=DST), good, good]) == OVERLAP
    assert _call(lib, [good, good, _cam(src=20)], bv=nan) == NOT_FINITE  # the same frames twice, and a third that straddles them
    assert _call(lib, [good, _cam(src=DST)], batch=0) == OK  # (an empty batch has no bytes to share)
    # 3. the destination's sides, 4. the border value (the constant border's only), 5. the empty batch
    one = dict(ch=1, dst=1 << 30)
    cam1 = _cam(rs=8, fs=64)
    assert _call(lib, [cam1], dw=(1 << 20) + 1, drs=1 << 21, dfs=1 << 24, bv=[float("nan")], **one) == TOO_LARGE
    assert _call(lib, [cam1], dh=(1 << 20) + 1, drs=8, dfs=1 << 24, batch=0, **one) == TOO_LARGE
    assert _call(lib, [cam1], dw=1 << 20, drs=1 << 20, dfs=1 << 23, bv=[float("nan")], **one) == NOT_FINITE
    assert _call(lib, [good], bv=nan, batch=0) == NOT_FINITE and _call(lib, [good], bv=[float("inf"), 0, 0], batch=0) == NOT_FINITE
    assert _call(lib, [good], bv=nan, mode=5, batch=0) == OK
    assert _call(lib, [good], bv=[1.0, 2.0, 3.0], batch=0) == OK


# ---- the host checks under the sanitizers ----

@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


CAM = dict(src=16, h=8, w=8, fs=192, rs=24, m_count=1, m_null=0)
CALL = dict(n=None, cams_null=0, dst=1 << 30, batch=1, dh=8, dw=8, ch=3, dfs=192, drs=24, dtype=0, interp=1, blend=0, feather=64, mode=0, border=0)


def _c(**kw):
    return dict(CAM, **kw)


def _line(cams, **kw):
    a = dict(CALL, **kw)
    n = len(cams) if a["n"] is None else a["n"]
    head = [n, a["cams_null"], a["dst"], a["batch"], a["dh"], a["dw"], a["ch"], a["dfs"], a["drs"], a["dtype"], a["interp"], a["blend"], a["feather"], a["mode"],
            a["border"], len(cams)]
    body = [v for c in cams for v in (c["src"], c["h"], c["w"], c["fs"], c["rs"], c["m_count"], c["m_null"])]
    return "stitch " + " ".join(str(v) for v in head + body)


def test_stitch_status_under_sanitizers(driver):
    big, top = 2147483647, (1 << 63) - 1
    g = _c()
    ok2 = [OK, OK, 2]  # an 8 x 8 canvas: one tile column, two tile rows
    bad, unsup, large, nonfinite, overlap = [BAD_ARG, 0, 0], [UNSUPPORTED, 0, 0], [TOO_LARGE, 0, 0], [NOT_FINITE, 0, 0], [OVERLAP, 0, 0]
    # camera counts
    cases = [(_line([], n=0), bad), (_line([g]), ok2), (_line([g] * 8), ok2), (_line([g] * 9), bad), (_line([g], n=-1), bad), (_line([g], n=big), bad),
             (_line([g], cams_null=1), bad), (_line([g] * 7 + [_c(w=32768, rs=3 * 32768, fs=24 * 32768)]), large), (_line([g] * 7 + [_c(m_null=1)]), bad)]
    # feather
    cases += [(_line([g], blend=1, feather=f), want) for f, want in ((0, bad), (1, ok2), (4096, ok2), (4097, bad), (-big, bad), (big, bad))]
    cases += [(_line([g], blend=0, feather=f), ok2) for f in (0, 4097, -big, big)]
    # formats
    cases += [(_line([g], blend=b), unsup) for b in (2, -1, big)] + [(_line([g], mode=m), unsup) for m in (1, 2, 3, 4, 6, 16, 21, -1)]
    cases += [(_line([g], mode=5), ok2), (_line([g], interp=0), ok2), (_line([g], interp=2), unsup), (_line([g], dtype=3), unsup), (_line([g], ch=0), unsup),
              (_line([g], ch=5, border=2), unsup), (_line([_c(rs=96, fs=768)], dtype=1, drs=96, dfs=768), ok2)]
    cases += [(_line([_c(rs=8 * c, fs=64 * c)], ch=c, drs=8 * c, dfs=64 * c), ok2) for c in (1, 2, 4)]
    # strides next to 2^63
    cases += [(_line([_c(rs=top)]), large),                                   # holds the rows; no 24-bit multiply reaches it
              (_line([_c(rs=-1)]), bad), (_line([_c(rs=-top - 1)]), bad), (_line([g], drs=-top - 1), bad),
              (_line([_c(fs=top)], batch=2), overlap),                        # frame 1 lies 2^63 bytes on: the canvas is inside the bounding range
              (_line([_c(fs=-top - 1)], batch=2), bad), (_line([g], dfs=-top - 1, batch=2), bad),
              (_line([g], dfs=top, batch=2), [OK, OK, 4]),                    # canvases 2^63 bytes apart, the camera below both
              (_line([_c(fs=top)], batch=1), ok2)]                            # (one frame: its stride is not looked at)
    # sides next to 2^31 and 32767 / 32768
    one = dict(ch=1)
    c1 = _c(rs=8, fs=64)
    cases += [(_line([_c(w=32767, rs=3 * 32767, fs=24 * 32767)]), ok2), (_line([_c(w=32768, rs=3 * 32768, fs=24 * 32768)]), large),
              (_line([_c(h=32767, fs=24 * 32767)]), ok2), (_line([_c(h=32768, fs=24 * 32768)]), large),
              (_line([_c(w=big)]), bad), (_line([_c(w=big, rs=3 * big, fs=24 * big)]), large), (_line([_c(h=big, fs=24 * big)]), large),
              (_line([_c(w=0)]), bad), (_line([_c(h=-1)]), bad), (_line([g], dw=0), bad), (_line([g], dh=-big - 1), bad),
              (_line([c1], dw=big, dh=1, drs=big, dfs=big, **one), large), (_line([c1], dw=8, dh=big, drs=8, dfs=8 * big, **one), large),
              (_line([c1], dw=big, dh=big, drs=big, dfs=big * big, **one), large),
              (_line([c1], dw=1 << 20, dh=1, drs=1 << 20, dfs=1 << 20, **one), [OK, OK, 4096]),
              (_line([c1], dw=(1 << 20) + 1, dh=1, drs=1 << 21, dfs=1 << 21, **one), large),
              (_line([c1], dw=8, dh=(1 << 20) + 1, drs=8, dfs=1 << 24, **one), large),
              (_line([c1], batch=big, dst=1 << 40, drs=8, dfs=64, **one), large)]  # (2 tiles per frame: the grid passes 2^31 - 1 items)
    # order: the first bad camera, then the sides, then the border value, then the empty batch
    wide = _c(w=32768, rs=3 * 32768, fs=24 * 32768)
    cases += [(_line([g, g, _c(src=0)]), bad), (_line([g, g, wide]), large), (_line([wide, _c(src=0)]), large), (_line([_c(src=0), wide]), bad),
              (_line([g, _c(src=4096), _c(src=1 << 30)]), overlap), (_line([g, g, _c(src=20)]), ok2), (_line([g, _c(src=(1 << 30) + 192)]), ok2),
              (_line([g], border=2), nonfinite), (_line([g], border=2, mode=5), ok2), (_line([g], border=1), ok2),
              (_line([c1], dw=(1 << 20) + 1, dh=1, drs=1 << 21, dfs=1 << 21, border=2, **one), large),
              (_line([g], batch=0), [OK, OK, 0]), (_line([g], batch=0, border=2), nonfinite), (_line([g, _c(src=1 << 30)], batch=0), [OK, OK, 0]),
              (_line([c1], batch=0, dh=(1 << 20) + 1, drs=8, dfs=1 << 24, **one), large), (_line([g], batch=-1), bad)]
    hostplan.check_cases(driver, cases, "stitch")


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_stitch_kernels_code_object(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("warp_stitch.hip", tmp_path, "flat_frame.h").items() if "warp_stitch_kernel" in n}
    assert len(kernels) == 2 * 4 * 2 * 2, len(kernels)  # dtype x channels x interpolation x blend
    codeobj.assert_lean(kernels)
    codeobj.makefile_flags("warp_stitch.hip", "warp_stitch.h")
    assert "-fno-fast-math" in codeobj.makefile_flags("warp_stitch.hip")


# ---- the Python entry's own checks, all before a device is needed ----

def test_python_entry_validates_before_the_device():
    from bev_amd import warp
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)
    eye = np.eye(3)
    for srcs, Ms, kw, text in (([], [], {}, "1..8 cameras"), ([img] * 9, [eye] * 9, {}, "1..8 cameras"), ([img, img], [eye], {}, "2 cameras"),
                               ([img], [eye], dict(blend="mean"), "blend"), ([img], [eye], dict(blend="feather", feather=0), "1..4096"),
                               ([img], [eye], dict(blend="feather", feather=4097), "1..4096"), ([img], [eye], dict(border_mode=warp.BORDER_REPLICATE), "border mode"),
                               ([img], [eye], dict(border_mode=warp.BORDER_REFLECT_101), "border mode"), ([img], [eye], dict(flags=warp.INTER_CUBIC), "interpolation"),
                               ([img, img.float()], [eye] * 2, {}, "camera 1 has dtype torch.float32"), ([img, img[:, :, :2]], [eye] * 2, {}, "camera 1 .* 2 channels"),
                               ([img[None], img, img[None].expand(2, 8, 8, 3)], [eye] * 3, {}, "camera 2 .* batch 2"), ([img[:, :, 0], img], [eye] * 2, {}, "camera 1 .* 3 channels"),
                               ([img], [eye], {}, "CUDA"), ([img.numpy()], [eye], {}, "CUDA")):
        with pytest.raises(ValueError, match=text):
            warp.warp_stitch(srcs, Ms, (8, 8), **kw)
