"""Bicubic sampling through a bilinear warp map (bevwarp_remap | BEVWARP_MAP_BICUBIC; bev_amd.warp.remap(interpolation=INTER_CUBIC)) without a
GPU: the numpy reference (tests/remap_cubic_ref.py) tied to tests/cubic_ref.warp by bits and its properties, the host checks under the
sanitizers and through the library, the Python refusals, and the code object of the kernel unit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from tests import codeobj
from tests import cubic_ref as CR
from tests import hostplan
from tests import remap_cubic_ref as RC
from tests import remap_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
FLAG = 0x200
SH, SW, DH, DW = 23, 37, 40, 52
# a keystone whose destination reaches past the source on every side (dst -> src)
KEYSTONE = np.array([[0.9, 0.15, -6.0], [0.05, 0.8, -5.0], [0.0015, 0.001, 1.0]])
BORDER = (7.0, 200.0, 31.0, 99.0)
CANARY = 77


def _src(h, w, c, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8) if dtype == np.uint8 else (rng.random((h, w, c), dtype=np.float32) * 4 - 2).astype(np.float32)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- the reference against the matrix warp's reference, from pinhole maps ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_reference_equals_the_matrix_reference_on_pinhole_maps(dtype, c):
    xy, frac = RR.build((DW, DH), KEYSTONE, interp=RR.LINEAR)
    inl, partial, all_out, written = CR.classes((SH, SW), KEYSTONE, (DW, DH), m_is_inverse=True)
    assert inl.any() and partial.any() and all_out.any() and (~written).any() and (written & ~inl).any()
    for got, want in zip(RC.classes(xy, SW, SH), (inl, partial, all_out, written)):
        np.testing.assert_array_equal(got, want)
    src = _src(SH, SW, c, dtype, 10 + c)
    canvas = np.full((DH, DW, c), CANARY, dtype)
    for mode in RC.MODES:
        bv = BORDER[:c] if mode == RC.CONSTANT else 0.0
        got = RC.remap_cubic(src, xy, frac, mode, bv, canvas)
        want = CR.warp(src, KEYSTONE, (DW, DH), mode, m_is_inverse=True, border_value=bv, canvas=canvas)
        assert got.dtype == want.dtype == dtype
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg="mode %d" % mode)
    # (H, W) frames
    np.testing.assert_array_equal(RC.remap_cubic(src[..., 0], xy, frac, RC.REFLECT), CR.warp(src[..., 0], KEYSTONE, (DW, DH), RC.REFLECT, m_is_inverse=True))


# ---- the reference's own properties ----

def test_sentinel_entries_and_high_frac_bits():
    xy, frac = RR.build((DW, DH), KEYSTONE, interp=RR.LINEAR)
    xy, frac = xy.copy(), frac.copy()
    xy[3:9, 5:30] = RR.SENTINEL
    frac[3:9, 5:30] = 0
    for dtype in (np.uint8, np.float32):
        src = _src(SH, SW, 3, dtype, 20)
        out = RC.remap_cubic(src, xy, frac, RC.CONSTANT, BORDER[:3])
        want = np.array(BORDER[:3]).astype(dtype)
        assert (out[3:9, 5:30] == want).all()  # the border value itself
        canvas = np.full((DH, DW, 3), CANARY, dtype)
        out = RC.remap_cubic(src, xy, frac, RC.TRANSPARENT, canvas=canvas)
        assert (out[3:9, 5:30] == CANARY).all()  # not written
        assert (RC.remap_cubic(src, xy, frac, RC.TRANSPARENT)[3:9, 5:30] == 0).all()
        # bits 10..15 of frac are ignored
        noisy = frac | (np.random.default_rng(21).integers(0, 64, frac.shape).astype(np.uint16) << 10)
        assert (noisy != frac).any()
        for mode in RC.MODES:
            np.testing.assert_array_equal(_bits(RC.remap_cubic(src, xy, noisy, mode, BORDER[:3], canvas)), _bits(RC.remap_cubic(src, xy, frac, mode, BORDER[:3], canvas)))
        # ... and so is the sign of an int16 view of the plane
        np.testing.assert_array_equal(_bits(RC.remap_cubic(src, xy, noisy.view(np.int16), RC.WRAP)), _bits(RC.remap_cubic(src, xy, frac, RC.WRAP)))


def checkerboard():
    """A 0 / 255 checkerboard of 2 x 2 squares and a map that magnifies it: bicubic overshoots below 0 and above 255."""
    yy, xx = np.mgrid[0:24, 0:24]
    src = (((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)[:, :, None]
    Minv = np.array([[0.31, 0.02, 1.3], [-0.01, 0.29, 2.1], [0, 0, 1.0]])
    xy, frac = RR.build((64, 48), Minv, interp=RR.LINEAR)
    return src, xy, frac


def test_checkerboard_overshoots_into_both_clamps():
    src, xy, frac = checkerboard()
    pre = RC.presums(src, xy, frac, RC.REPLICATE)
    v = (pre + 16384) >> 15
    assert (v < 0).any() and (v > 255).any(), (int(v.min()), int(v.max()))
    out = RC.remap_cubic(src, xy, frac, RC.REPLICATE)
    assert out.min() == 0 and out.max() == 255
    np.testing.assert_array_equal(out, np.clip(v, 0, 255).astype(np.uint8))


# ---- the host checks under the sanitizers, and the same lists through the library ----

CALL = dict(src=16, dst=1 << 20, xy=1 << 24, frac=1 << 26, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, channels=3, src_fs=192, src_rs=24, dst_fs=192, dst_rs=24,
            map_count=1, xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16, dtype=0, interp=1 | FLAG, mode=0)
OTHERS = ("build", "nv12", "nv12_planes", "to_nv12", "nv12_to_nv12", "planes", "stitch", "stitch_nv12")


def _call(**kw):
    a = dict(CALL, **kw)
    return "call " + " ".join(str(a[k]) for k in CALL)


def _status_cases():
    """[(arguments of a bevwarp_remap call over CALL, the status of its checks)]: every status the entry documents, with the flag set."""
    three = dict(batch=3)
    cases = [(dict(mode=m, dtype=d, channels=c, src_rs=8 * c * e, src_fs=64 * c * e, dst_rs=8 * c * e, dst_fs=64 * c * e), OK)
             for m in range(6) for d, e in ((0, 1), (1, 4)) for c in (1, 2, 3, 4)]
    cases += [(dict(interp=i), UNSUPPORTED) for i in (FLAG, FLAG | 2, FLAG | 3, FLAG | 1 | 0x100, -1, FLAG | 4, FLAG | 1 | 0x400)]  # nearest, cubic, ... | flag
    cases += [(dict(interp=i), UNSUPPORTED) for i in (2, 3)] + [(dict(interp=0), OK), (dict(interp=1), OK)]  # without the flag: as it was
    cases += [(dict(interp=FLAG, frac=0), UNSUPPORTED)]                  # (nearest | flag: refused for its word, not served without a frac plane)
    cases += [(dict(mode=m), UNSUPPORTED) for m in (6, 16, -1)] + [(dict(dtype=d), UNSUPPORTED) for d in (2, 3, 4, -1)] + [(dict(channels=c), UNSUPPORTED) for c in (0, 5)]
    cases += [(dict(src=0), BAD_ARG), (dict(dst=0), BAD_ARG), (dict(xy=0), BAD_ARG), (dict(frac=0), BAD_ARG)]  # a NULL frac plane: BAD_ARG, as for a bilinear call
    cases += [(dict(src_h=0), BAD_ARG), (dict(dst_w=0), BAD_ARG), (dict(batch=-1), BAD_ARG)]
    cases += [(dict(map_count=0), BAD_ARG), (dict(map_count=2), BAD_ARG), (dict(map_count=3, **three), OK), (dict(map_count=1, **three), OK),
              (dict(map_count=3, xy_fs=255, **three), BAD_ARG), (dict(map_count=3, frac_fs=127, **three), BAD_ARG)]
    cases += [(dict(xy=(1 << 24) + 2), BAD_ARG), (dict(frac=(1 << 26) + 1), BAD_ARG), (dict(xy_rs=28), BAD_ARG), (dict(frac_rs=14), BAD_ARG), (dict(src_rs=23), BAD_ARG)]
    cases += [(dict(src_w=32768, src_rs=3 * 32768, src_fs=24 * 32768), TOO_LARGE), (dict(src_h=32768, src_fs=24 * 32768), TOO_LARGE)]
    cases += [(dict(dst=16), OVERLAP), (dict(xy=1 << 20), OVERLAP), (dict(frac=(1 << 20) + 190), OVERLAP), (dict(frac=(1 << 20) + 192), OK)]
    # the order: NULL and sides, the format, the map count, the layouts, the source's size, the overlap
    cases += [(dict(src=0, interp=FLAG), BAD_ARG), (dict(interp=FLAG, map_count=2), UNSUPPORTED), (dict(map_count=2, xy_rs=28), BAD_ARG),
              (dict(xy_rs=28, src_w=32768, src_rs=3 * 32768, src_fs=24 * 32768), BAD_ARG), (dict(src_h=32768, src_fs=24 * 32768, dst=16), TOO_LARGE)]
    return cases


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_host_checks_under_sanitizers(driver):
    flags = [("flag %d" % w, [f, left]) for w, f, left in ((0, 0, 0), (1, 0, 1), (FLAG, 1, 0), (FLAG | 1, 1, 1), (FLAG | 2, 1, 2), (0x100, 0, 0x100), (0x301, 1, 0x101),
                                                         (-1, 1, -1 & ~FLAG))]
    got = hostplan.run_driver(driver, [ln for ln, _ in flags], "remap_cubic")
    for (ln, want), g in zip(flags, got):
        assert g == want, (ln, g, want)
    cases = _status_cases()
    lines = [_call(**kw) for kw, _ in cases]
    got = hostplan.run_driver(driver, lines, "remap_cubic")
    for (kw, want), ln, g in zip(cases, lines, got):
        a = dict(CALL, **kw)
        flagged = int(bool(a["interp"] & FLAG))
        if want == OK:
            tiles = 2 * a["batch"]  # (an 8 x 8 destination: 2 tiles a frame, one frame per item at this size)
            assert g == [flagged, OK, OK, 1, tiles], (ln, g)
        else:
            assert g == [flagged, want, 0, 0, 0], (ln, g, want)
    # an empty batch: the checks pass, nothing is planned; destination sides past 2^20: the plan refuses
    w20 = 1 << 20
    one = dict(channels=1, src_rs=8, src_fs=64, dst=1 << 40, xy=1 << 44, frac=1 << 48)
    more = [(_call(batch=0), [1, OK, 0, 0, 0]),
            (_call(dst_w=w20, dst_h=1, dst_rs=w20, dst_fs=w20, xy_rs=4 * w20, frac_rs=2 * w20, **one), [1, OK, OK, 1, 4096]),
            (_call(dst_w=w20 + 1, dst_h=1, dst_rs=2 * w20, dst_fs=2 * w20, xy_rs=8 * w20, frac_rs=4 * w20, **one), [1, OK, TOO_LARGE, 0, 0])]
    got = hostplan.run_driver(driver, [ln for ln, _ in more], "remap_cubic")
    for (ln, want), g in zip(more, got):
        assert g == want, (ln, g, want)
    # no other entry takes the flag out of its word
    others = [("other %s %d" % (e, w), [want]) for e in OTHERS for w, want in ((1, OK), (0, OK), (FLAG | 1, UNSUPPORTED), (FLAG, UNSUPPORTED), (2, UNSUPPORTED))]
    got = hostplan.run_driver(driver, [ln for ln, _ in others], "remap_cubic")
    for (ln, want), g in zip(others, got):
        assert g == want, (ln, g, want)


def _p(v):
    return ctypes.c_void_p(v) if v else None


def test_the_same_statuses_through_the_library():
    """Fake addresses, never dereferenced: a call whose checks pass is stopped by a NaN border value, which is looked at last
    (BEVWARP_BORDER_CONSTANT only: under every other mode such a call would launch, so those are left to the driver and to the GPU)."""
    lib = hostplan.built_lib()
    assert lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    nan4 = (ctypes.c_double * 4)(*[float("nan")] * 4)  # (every channel: no call below may pass its checks and launch on these addresses)
    nan_border = ctypes.cast(nan4, ctypes.c_void_p)

    def remap(bv=nan_border, **kw):
        a = dict(CALL, **kw)
        return lib.bevwarp_remap(_p(a["src"]), _p(a["dst"]), a["batch"], a["src_h"], a["src_w"], a["dst_h"], a["dst_w"], a["channels"], a["src_fs"], a["src_rs"], a["dst_fs"],
                                 a["dst_rs"], _p(a["xy"]), _p(a["frac"]), a["map_count"], a["xy_fs"], a["xy_rs"], a["frac_fs"], a["frac_rs"], a["dtype"], a["interp"], a["mode"], bv,
                                 None)

    for kw, want in _status_cases():
        if dict(CALL, **kw)["mode"] != 0:
            continue
        assert remap(**kw) == (NOT_FINITE if want == OK else want), (kw, want)
    assert remap(batch=0) == OK and remap(batch=0, bv=None) == OK  # nothing to do: no launch, the border value is not looked at
    # the other entries judge the whole word
    mxy, mfr, src, dst = _p(1 << 24), _p(1 << 26), _p(16), _p(1 << 20)
    cam = _lib.MapCamera(src=16, uv=4096, frame_stride=192, row_stride=24, uv_frame_stride=32, uv_row_stride=8, map_xy=1 << 24, map_frac=1 << 26, xy_frame_stride=256,
                         xy_row_stride=32, frac_frame_stride=128, frac_row_stride=16, src_h=8, src_w=8, map_count=1, reserved=0)
    entries = {
        "bevwarp_remap_nv12": lambda w: lib.bevwarp_remap_nv12(src, _p(4096), dst, 1, 8, 8, 8, 8, 64, 8, 32, 8, 192, 24, mxy, mfr, 1, 256, 32, 128, 16, w, 0, 0, nan_border, None),
        "bevwarp_remap_planes": lambda w: lib.bevwarp_remap_planes(src, dst, 1, 8, 8, 8, 8, 192, 24, 768, 256, 32, mxy, mfr, 1, 256, 32, 128, 16, w, 0, nan_border, None, None,
                                                                   _lib.F32, None),
        "bevwarp_remap_to_nv12": lambda w: lib.bevwarp_remap_to_nv12(src, dst, _p(1 << 21), 1, 8, 8, 8, 8, 192, 24, 64, 8, 32, 8, mxy, mfr, 1, 256, 32, 128, 16, w, 0, 0, nan_border,
                                                                     None),
        "bevwarp_stitch_maps": lambda w: lib.bevwarp_stitch_maps(ctypes.cast(ctypes.pointer(cam), ctypes.c_void_p), 1, dst, 1, 8, 8, 3, 192, 24, _lib.U8, w, 0, 0, 0, nan_border, None),
    }
    for name, fn in entries.items():
        assert fn(1) == NOT_FINITE, name  # (the call is good: only the border value stops it)
        assert fn(1 | FLAG) == UNSUPPORTED and fn(FLAG) == UNSUPPORTED, name
    build = lambda w: lib.bevwarp_build_map(None, 1, None, 1.0, w, mxy, mfr, 8, 8, 256, 32, 128, 16, None)  # noqa: E731
    assert build(1) == BAD_ARG  # (M is NULL: the first check -- the interpolation is judged right after it)
    build = lambda w: lib.bevwarp_build_map(src, 1, None, 1.0, w, mxy, _p((1 << 24) + 64), 8, 8, 256, 32, 128, 16, None)  # noqa: E731
    assert build(1) == OVERLAP and build(1 | FLAG) == UNSUPPORTED and build(FLAG) == UNSUPPORTED and build(FLAG | 0x101) == UNSUPPORTED


def test_header_and_constants():
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "#define BEVWARP_MAP_BICUBIC 0x200\n" in header and "#define BEVWARP_ABI_VERSION 7\n" in header
    assert _lib.MAP_BICUBIC == FLAG and _lib.ABI_VERSION == 7
    text = header.split("BEVWARP_MAP_BICUBIC: bicubic sampling")[1].split("#define BEVWARP_MAP_BICUBIC")[0]
    for cite in ("wx = sx - 1, wy = sy - 1", "[-32769, 32769]", "No other entry takes the flag", "(-32768, -32768)", "bevwarp_warp_border's BEVWARP_CUBIC text"):
        assert cite in text, cite


# ---- the Python entries, before any device is touched ----

def _cpu_map(interp=1, device="cpu", dh=6, dw=5):
    from bev_amd import warp
    return warp.WarpMap(torch.zeros((1, dh, dw, 2), dtype=torch.int16, device=device), torch.zeros((1, dh, dw), dtype=torch.int16, device=device) if interp else None,
                        interp, (dw, dh))


def test_python_entries_refuse_before_the_device():
    from bev_amd import warp
    from bev_amd.pipeline import FramePipeline
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="bicubic samples a bilinear map"):
        warp.remap(None, _cpu_map(interp=0), interpolation=warp.INTER_CUBIC)  # (judged before the tensor is looked at)
    with pytest.raises(ValueError, match="bicubic samples a bilinear map"):
        warp.remap(src.to("meta"), _cpu_map(interp=0, device="meta"), interpolation=warp.INTER_CUBIC)
    for bad in (3, 4, -1, 0x201, 0x200, "cubic", 2.0, True):
        with pytest.raises(ValueError, match="interpolation"):
            warp.remap(None, _cpu_map(), interpolation=bad)
    with pytest.raises(ValueError, match="interpolation"):
        warp.remap(None, _cpu_map(interp=1), interpolation=warp.INTER_NEAREST)  # (another map's interpolation is no request either)
    with pytest.raises(ValueError, match="interpolation"):
        warp.remap(None, _cpu_map(interp=0), interpolation=warp.INTER_LINEAR)
    # what passes the word's check goes on to the checks it always met: no CUDA tensor
    for m, interp in ((_cpu_map(), warp.INTER_CUBIC), (_cpu_map(), warp.INTER_LINEAR), (_cpu_map(), None), (_cpu_map(interp=0), warp.INTER_NEAREST), (_cpu_map(), np.int64(2))):
        with pytest.raises(ValueError, match="CUDA"):
            warp.remap(src, m, interpolation=interp)
    assert warp._map_interpolation("t", _cpu_map(), warp.INTER_CUBIC) == 0x201 and warp._map_interpolation("t", _cpu_map(), None) == 1
    # the unchanged refusals
    with pytest.raises(ValueError):
        warp.WarpMap(torch.zeros((1, 6, 5, 2), dtype=torch.int16), torch.zeros((1, 6, 5), dtype=torch.int16), 2, (5, 6))
    with pytest.raises(ValueError):
        warp.build_warp_map(np.eye(3), (8, 8), flags=warp.INTER_CUBIC)
    # FramePipeline(map_interpolation=...)
    with pytest.raises(ValueError, match="bicubic samples a bilinear map"):
        FramePipeline((8, 8), 3, None, (5, 6), warp_map=_cpu_map(interp=0), map_interpolation=warp.INTER_CUBIC)
    for kw in (dict(src_format="nv12"), dict(dst_format="nv12"), dict(src_format="nv12", dst_format="nv12")):
        with pytest.raises(ValueError, match="NV12"):
            FramePipeline((8, 8), 3, None, (6, 6), warp_map=_cpu_map(dh=6, dw=6), map_interpolation=warp.INTER_CUBIC, **kw)
    with pytest.raises(ValueError, match="interpolation"):
        FramePipeline((8, 8), 3, None, (5, 6), warp_map=_cpu_map(), map_interpolation=3)
    with pytest.raises(ValueError, match="needs a warp_map"):
        FramePipeline((8, 8), 3, np.eye(3), (5, 6), map_interpolation=warp.INTER_CUBIC)
    with pytest.raises(ValueError, match="warp_map is on"):  # (the word is good: the next check refuses the CPU map)
        FramePipeline((8, 8), 3, None, (5, 6), warp_map=_cpu_map(), map_interpolation=warp.INTER_CUBIC)
    import inspect
    assert list(inspect.signature(FramePipeline.__init__).parameters)[-1] == "map_interpolation"
    assert list(inspect.signature(warp.remap).parameters) == ["src", "warp_map", "border_mode", "border_value", "out", "interpolation"]


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_map_cubic_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_map_cubic.hip", tmp_path, "cubic_sample.h")
    assert len(found) == 2 * 4 * 6 and all("remap_cubic_kernel" in n for n in found), sorted(found)  # dtype x channels x mode
    codeobj.assert_lean(found)
    codeobj.makefile_flags("warp_map_cubic.hip", "map_entry.h")
    codeobj.makefile_flags("warp_cubic.hip", "cubic_sample.h")  # (the shared sampler rebuilds both of its users)


def test_matrix_cubic_kernels_are_still_48(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("warp_cubic.hip", tmp_path).items() if "warp_cubic_kernel" in n}
    assert len(kernels) == 2 * 4 * 6, len(kernels)
    codeobj.assert_lean(kernels)
