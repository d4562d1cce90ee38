"""Per-camera exposure gains in the stitches through warp maps (BEVWARP_STITCH_GAIN, bev_amd.warp.remap_stitch*(..., gains=),
bev_amd.exposure) without a device: the gain step over its whole domain, the six entries' host checks under the flag -- through
tests/host_plan_driver.cpp, family `stitch_gain` under the sanitizers and through the loaded library -- the header, the gained units' code objects, the
Python entries' and SitePipeline's refusals, and the gain solver."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bev_amd import _lib
from bev_amd import exposure
from tests import codeobj
from tests import hostplan
from tests import remap_ref as RR
from tests import stitch_gain_ref as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN = 0x100


# ---- the gain step ----

def test_gain_over_its_whole_domain():
    p, G = np.arange(256)[:, None], np.arange(1024)[None, :]
    t = SG.gain(p, G)
    assert t.shape == (256, 1024) and t.min() == 0 and t.max() == 255
    assert (t[:, 256] == np.arange(256)).all()                     # 256 is the identity for every p
    assert (t[:, 0] == 0).all() and (t[0, :] == 0).all()           # a gain of 0, and black, give 0
    assert (np.diff(t, axis=0) >= 0).all() and (np.diff(t, axis=1) >= 0).all()  # monotone in p and in G
    exact = (p * G + 128) >> 8
    assert (t == np.minimum(exact, 255)).all() and (exact > 255).any() and (t[exact > 255] == 255).all()  # saturating, never wrapping
    assert (p * G).max() == 255 * 1023 == 260865                  # (what a 16-bit multiply would not hold)
    # by hand: (p, G) -> (p G + 128) >> 8, cut off at 255
    for pv, Gv, want in ((100, 384, 150), (200, 384, 255), (1, 128, 1), (1, 127, 0), (255, 255, 254), (3, 1023, 12), (63, 1023, 252), (64, 1023, 255), (255, 1023, 255),
                         (255, 257, 255), (254, 257, 255), (253, 257, 254), (77, 256, 77), (77, 0, 0), (2, 64, 1), (1, 64, 0)):
        assert t[pv, Gv] == want, (pv, Gv, t[pv, Gv], want)


def test_apply_gains_and_quantize_are_the_definition():
    frames = torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3).contiguous()
    for G3 in ((256, 256, 256), (0, 1023, 300), (255, 257, 512), (1, 128, 127)):
        got = exposure.apply_gains(frames, G3).numpy()
        np.testing.assert_array_equal(got, SG.apply_gain(frames.numpy(), G3))
    np.testing.assert_array_equal(exposure.apply_gains(frames, (256, 256, 256)).numpy(), frames.numpy())
    G = exposure.quantize_gains([1.0, 0.5, 1023 / 256], 3)
    assert G.dtype == np.int64 and G.tolist() == [[256] * 3, [128] * 3, [1023] * 3]
    G = exposure.quantize_gains([[1.001, 0.998, 0.0], [2.0, 3.99, 1.5]], 2)
    assert G.tolist() == [[256, 255, 0], [512, 1021, 384]] == SG.quantize([[1.001, 0.998, 0.0], [2.0, 3.99, 1.5]], 2).tolist()
    assert exposure.gain_words(G) == [256 | 255 << 10, 512 | 1021 << 10 | 384 << 20] == [SG.word(g) for g in G]
    assert all(w >> 30 == 0 for w in exposure.gain_words(exposure.quantize_gains([1023 / 256], 1)))
    for bad in (frames.float(), frames[:, :2], torch.zeros(3, dtype=torch.uint8)[..., None]):
        with pytest.raises(ValueError):
            exposure.apply_gains(bad, (256, 256, 256))
    for bad in ((256, 256), (256, 256, 1024), (-1, 0, 0)):
        with pytest.raises(ValueError):
            exposure.apply_gains(frames, bad)


# ---- the header ----

def test_header_defines_the_flag():
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert re.search(r"^#define BEVWARP_STITCH_GAIN 0x100$", header, re.M) and _lib.STITCH_GAIN == GAIN
    assert re.search(r"^#define BEVWARP_ABI_VERSION 7$", header, re.M) and _lib.ABI_VERSION == 7
    assert "gain(p, Gc) = min(255, (p * Gc + 128) >> 8)" in header and "G0 | G1 << 10 | G2 << 20" in header
    assert re.search(r"int reserved;\s*/\* 0; under BEVWARP_STITCH_GAIN", header)      # the member keeps its name
    assert "gain" not in " ".join(_lib.SYMBOLS)                                         # no new exported symbol
    assert ctypes.sizeof(_lib.MapCamera) == 112


# ---- the six entries' statuses under the flag (fake pointers, never dereferenced: every call fails a check or has nothing to launch) ----

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE = 0, -1, -2, -3, -4
PASSES = NOT_FINITE  # a call that passes every check of its cameras and of the canvas ends on the NaN border value: nothing is launched
KINDS = ("maps", "nv12", "to_nv12", "nv12_to_nv12", "planes", "nv12_planes")
DST, XY, FR = 1 << 20, 1 << 24, 1 << 26
WORD = 300 | 256 << 10 | 1023 << 20  # a valid gain word
CAM = dict(src=4096, uv=0, h=8, w=8, fs=192, rs=24, uv_fs=0, uv_rs=0, xy=XY, frac=FR, xy_fs=256, xy_rs=32, fr_fs=128, fr_rs=16, map_count=1, reserved=WORD)
NVCAM = dict(CAM, uv=8192, fs=64, rs=8, uv_fs=32, uv_rs=8)
CALL = dict(n=None, cams_null=0, dst=DST, batch=1, dh=8, dw=8, ch=3, dfs=192, drs=24, dtype=0, interp=1, blend=GAIN, feather=64, rgb=0, mode=0, border=2, dst2=0, d2fs=0,
            d2rs=0, plane=1)
# the destinations of the other four: a Y plane with the pairs behind it; three float32 planes
DEST = {"to_nv12": dict(dfs=96, drs=8, dst2=DST + 64, d2fs=96, d2rs=8), "planes": dict(dfs=768, drs=32, d2fs=256)}
DEST["nv12_to_nv12"], DEST["nv12_planes"] = DEST["to_nv12"], DEST["planes"]


def _cam(kind, **kw):
    return dict(NVCAM if kind.startswith("nv12") else CAM, **kw)


def _case(kind, cams, want, **kw):
    return kind, cams, dict(dict(CALL, **DEST.get(kind, {})), **kw), want


def _cases():
    big = 2147483647
    out = []
    for kind in KINDS:
        k = _cam(kind)
        wide = dict(k, w=32768, rs=(1 if kind.startswith("nv12") else 3) * 32768, fs=24 * 32768, uv_rs=32768, uv_fs=4 * 32768)
        # the flag is taken out of the word: what is left is judged as without it
        out += [_case(kind, [k], PASSES), _case(kind, [k] * 8, PASSES), _case(kind, [k], PASSES, blend=GAIN | 1), _case(kind, [k], PASSES, blend=GAIN | 1, feather=4096),
                _case(kind, [k], BAD_ARG, blend=GAIN | 1, feather=0), _case(kind, [k], BAD_ARG, blend=GAIN | 1, feather=4097), _case(kind, [k], PASSES, feather=0),
                _case(kind, [k], OK, batch=0, border=1), _case(kind, [k], PASSES, interp=0), _case(kind, [k], UNSUPPORTED, interp=2)]
        out += [_case(kind, [dict(k, reserved=0)], UNSUPPORTED, blend=b) for b in (0x102, 0x200, -1, 0x300, GAIN | 0x400, 2)]
        out += [_case(kind, [], BAD_ARG, n=0), _case(kind, [k] * 9, BAD_ARG), _case(kind, [k], BAD_ARG, cams_null=1), _case(kind, [k], BAD_ARG, n=-1)]
        # the gain word: bits 30 and 31 (a negative `reserved`) are refused, in camera order, after the feather and before any camera's own checks
        for bad in (1 << 30, -(1 << 31), -1, (1 << 30) | WORD, -(1 << 30)):
            out += [_case(kind, [dict(k, reserved=bad)], BAD_ARG), _case(kind, [k, k, dict(k, reserved=bad)], BAD_ARG), _case(kind, [dict(k, reserved=bad), k], BAD_ARG),
                    _case(kind, [wide, dict(k, reserved=bad)], BAD_ARG), _case(kind, [dict(k, reserved=bad)], BAD_ARG, blend=0x102),
                    _case(kind, [dict(k, reserved=bad)], BAD_ARG, interp=2), _case(kind, [dict(k, reserved=bad)], BAD_ARG, batch=0, border=1)]
        out += [_case(kind, [dict(k, reserved=g)], PASSES) for g in (0, (1 << 30) - 1, 256 | 256 << 10 | 256 << 20, 1023)]
        out += [_case(kind, [wide, k], TOO_LARGE), _case(kind, [k, dict(k, src=0)], BAD_ARG), _case(kind, [k], BAD_ARG, dst=0), _case(kind, [dict(k, map_count=2)], BAD_ARG)]
        # without the flag `reserved` is not looked at: a garbage word changes no status
        for g in (-1, 1 << 30, -(1 << 31), big, WORD):
            out += [_case(kind, [dict(k, reserved=g)], PASSES, blend=0), _case(kind, [dict(k, reserved=g)] * 8, PASSES, blend=1),
                    _case(kind, [dict(k, reserved=g)], UNSUPPORTED, blend=2), _case(kind, [dict(wide, reserved=g)], TOO_LARGE, blend=0),
                    _case(kind, [dict(k, reserved=g)], BAD_ARG, blend=1, feather=0), _case(kind, [dict(k, reserved=g)], OK, blend=0, batch=0, border=1)]
    # bevwarp_stitch_maps under the flag: 8 bits and 3 channels only, refused where the format is judged (before the layouts) ...
    g = _cam("maps")
    out += [_case("maps", [dict(g, rs=96, fs=768)], UNSUPPORTED, dtype=1, drs=96, dfs=768)]
    out += [_case("maps", [dict(g, rs=8 * c, fs=64 * c)], UNSUPPORTED, ch=c, drs=8 * c, dfs=64 * c) for c in (1, 2, 4)]
    out += [_case("maps", [dict(g, rs=8 * c, fs=64 * c)], UNSUPPORTED, ch=c, drs=8 * c, dfs=64 * c, dtype=1) for c in (1, 3)]
    out += [_case("maps", [dict(g, rs=7)], UNSUPPORTED, ch=4), _case("maps", [dict(g, rs=7)], UNSUPPORTED, dtype=1), _case("maps", [dict(g, rs=23)], BAD_ARG),
            _case("maps", [dict(g, src=0)], BAD_ARG, ch=4)]                                                       # (NULL before the format, as ever)
    # ... and what it takes without the flag, garbage words and all
    out += [_case("maps", [dict(g, rs=96, fs=768, reserved=-1)], PASSES, blend=0, dtype=1, drs=96, dfs=768)]
    out += [_case("maps", [dict(g, rs=8 * c, fs=64 * c, reserved=1 << 30)], PASSES, blend=1, ch=c, drs=8 * c, dfs=64 * c) for c in (1, 2, 4)]
    return out


def _line(kind, cams, a):
    n = len(cams) if a["n"] is None else a["n"]
    head = [n, a["cams_null"], a["dst"], a["batch"], a["dh"], a["dw"], a["ch"], a["dfs"], a["drs"], a["dtype"], a["interp"], a["blend"], a["feather"], a["rgb"], a["mode"],
            a["border"], a["dst2"], a["d2fs"], a["d2rs"], a["plane"], len(cams)]
    body = [v for c in cams for v in (c["src"], c["uv"], c["h"], c["w"], c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"], c["frac"], c["xy_fs"], c["xy_rs"], c["fr_fs"],
                                      c["fr_rs"], c["map_count"], c["reserved"])]
    return kind + " " + " ".join(str(v) for v in head + body)


def _through_the_library(lib, kind, cams, a):
    arr = (_lib.MapCamera * max(len(cams), 1))(*[_lib.MapCamera(c["src"] or None, c["uv"] or None, c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"] or None, c["frac"] or None,
                                                                c["xy_fs"], c["xy_rs"], c["fr_fs"], c["fr_rs"], c["h"], c["w"], c["map_count"], c["reserved"]) for c in cams])
    nb = a["ch"] if kind == "maps" else 3
    bv = [1.0, 2.0, 3.0, 4.0]
    if a["border"] == 2 and 1 <= nb <= 4:
        bv[nb - 1] = float("nan")
    border = ctypes.cast((ctypes.c_double * 4)(*bv), ctypes.c_void_p) if a["border"] else None
    head = (None if a["cams_null"] else ctypes.addressof(arr), len(cams) if a["n"] is None else a["n"], a["dst"] or None)
    size = (a["batch"], a["dh"], a["dw"])
    ibf = (a["interp"], a["blend"], a["feather"])
    if kind == "maps":
        return lib.bevwarp_stitch_maps(*head, *size, a["ch"], a["dfs"], a["drs"], a["dtype"], *ibf, a["mode"], border, None)
    if kind == "nv12":
        return lib.bevwarp_stitch_maps_nv12(*head, *size, a["dfs"], a["drs"], *ibf, a["rgb"], a["mode"], border, None)
    if kind == "to_nv12":
        return lib.bevwarp_stitch_maps_to_nv12(*head, a["dst2"] or None, *size, a["dfs"], a["drs"], a["d2fs"], a["d2rs"], *ibf, a["rgb"], border, None)
    if kind == "nv12_to_nv12":
        return lib.bevwarp_stitch_maps_nv12_to_nv12(*head, a["dst2"] or None, *size, a["dfs"], a["drs"], a["d2fs"], a["d2rs"], *ibf, border, None)
    one = ctypes.cast((ctypes.c_double * 3)(1.0, 1.0, 1.0), ctypes.c_void_p)
    if kind == "planes":
        return lib.bevwarp_stitch_maps_planes(*head, *size, a["dfs"], a["d2fs"], a["drs"], *ibf, border, one, one, a["plane"], None)
    return lib.bevwarp_stitch_maps_nv12_planes(*head, *size, a["dfs"], a["d2fs"], a["drs"], *ibf, a["rgb"], border, one, one, a["plane"], None)


def test_status_through_the_library():
    """Every case either fails a check or has nothing to launch (an empty batch, or a NaN border value after every other check)."""
    lib = hostplan.built_lib()
    cases = _cases()
    assert len(cases) > 500 and {kind for kind, _, _, _ in cases} == set(KINDS)
    for kind, cams, a, want in cases:
        assert want != OK or a["batch"] == 0
        assert _through_the_library(lib, kind, cams, a) == want, (_line(kind, cams, a), want)
    # bevwarp_warp_stitch does not know the flag: it is an unsupported blend there, as it was
    cam = (_lib.Camera * 1)(_lib.Camera(4096, 8192, 192, 24, 8, 8, 1, 0))
    for blend in (GAIN, GAIN | 1):
        assert lib.bevwarp_warp_stitch(ctypes.addressof(cam), 1, DST, 1, 8, 8, 3, 192, 24, 0, 1, blend, 64, 0, None, None) == UNSUPPORTED


def test_status_under_sanitizers():
    driver = hostplan.build_driver()
    cases = _cases()
    got = hostplan.run_driver(driver, [_line(kind, cams, a) for kind, cams, a, _ in cases], "stitch_gain")
    for (kind, cams, a, want), out in zip(cases, got):
        flagged = int(a["blend"] & GAIN != 0)
        assert out[0] == want and out[3] == flagged and (want == OK or out[1:3] == [0, 0]), (_line(kind, cams, a), out, want)
    # the grid of a call that goes on to a launch, and the gain words as they were checked: what is launched is filled from these
    words = [WORD, 0, (1 << 30) - 1, 256 | 256 << 10 | 256 << 20, 1, 1023 << 20, 77 << 10, 5]
    for kind in KINDS:
        cams = [_cam(kind, reserved=w) for w in words]
        lines = [_line(kind, cams[:n], dict(dict(CALL, border=1, **DEST.get(kind, {})), **kw)) for n, kw in ((1, {}), (8, {}), (3, dict(batch=0)), (2, dict(blend=GAIN | 1)))]
        assert hostplan.run_driver(driver, lines, "stitch_gain") == [[OK, OK, 2, 1] + words[:1], [OK, OK, 2, 1] + words, [OK, OK, 0, 1] + words[:3], [OK, OK, 2, 1] + words[:2]], kind
        plain = _line(kind, cams[:2], dict(dict(CALL, border=1, blend=1, **DEST.get(kind, {}))))
        assert hostplan.run_driver(driver, [plain], "stitch_gain") == [[OK, OK, 2, 0]]
    wide = dict(dw=260, dh=22, drs=780, dfs=780 * 22, dst=1 << 40, batch=3, border=1)
    cam = _cam("maps", xy=1 << 44, frac=1 << 48, xy_rs=1040, fr_rs=520, xy_fs=1040 * 22, fr_fs=520 * 22, map_count=3)
    assert hostplan.run_driver(driver, [_line("maps", [cam], dict(CALL, **wide))], "stitch_gain") == [[OK, OK, 2 * 6 * 3, 1, WORD]]


# ---- the code objects of the gained units ----

UNITS = {"warp_stitch_gain.hip": "warp_stitch_maps.hip", "warp_stitch_gain_nv12_out.hip": "warp_stitch_maps_nv12_out.hip",
         "warp_stitch_gain_planes.hip": "warp_stitch_maps_planes.hip"}


def _template_args(name, stem):
    """The integer and bool template arguments of a mangled kernel name, in order (the pixel type `h` is skipped)."""
    tail = name.split(stem, 1)[1]
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", tail))


def test_gained_kernels_code_objects(tmp_path):
    found = codeobj.kernels("warp_stitch_gain.hip", tmp_path, "warp_stitch_maps.h")
    frames = {n: k for n, k in found.items() if "stitch_gain_kernel" in n}
    nv12 = {n: k for n, k in found.items() if "stitch_gain_nv12_kernel" in n}
    # source (B, G, R frames; NV12 frames in two orders) x interpolation x blend: 8-bit pixels of 3 channels only
    assert {_template_args(n, "stitch_gain_kernel") for n in frames} == {(3, i, b) for i in (0, 1) for b in (0, 1)} and all("IhLi3E" in n for n in frames)
    assert {_template_args(n, "stitch_gain_nv12_kernel") for n in nv12} == {(i, b, o) for i in (0, 1) for b in (0, 1) for o in (0, 1)}
    assert len(frames) == 4 and len(nv12) == 8 and len(found) == 12
    codeobj.assert_lean(found)

    found = codeobj.kernels("warp_stitch_gain_nv12_out.hip", tmp_path, "warp_stitch_maps_nv12_out.h")
    sources = {(0, 0), (0, 1), (1, 0)}  # (NV12, RGB): B, G, R frames; R, G, B frames; NV12 frames
    assert {_template_args(n, "stitch_gain_nv12_out_kernel") for n in found} == {(i, b) + s for i in (0, 1) for b in (0, 1) for s in sources}
    assert len(found) == 12 and all("stitch_gain_nv12_out_kernel" in n for n in found)
    codeobj.assert_lean(found)

    found = codeobj.kernels("warp_stitch_gain_planes.hip", tmp_path, "warp_stitch_maps_planes.h")
    sources = {(0, 0), (1, 0), (1, 1)}  # (NV12, RGB): interleaved frames; NV12 frames as B, G, R; as R, G, B
    assert {_template_args(n, "stitch_gain_planes_kernel") for n in found} == {(i, b) + s + (w,) for i in (0, 1) for b in (0, 1) for s in sources for w in (0, 1)}
    assert len(found) == 24 and all("stitch_gain_planes_kernel" in n for n in found)
    codeobj.assert_lean(found)

    with open(os.path.join(codeobj.CSRC, "Makefile")) as f:
        make = f.read()
    for unit, shadowed in UNITS.items():
        assert "-fno-fast-math" in codeobj.makefile_flags(unit)
        for header in ("warp_stitch_maps.h", "stitch_sample.h", "stitch_maps_u8x3.inc", "tap_load.h", "nv12_sample.h", "nv12_store.h", "plane_store.inc", "flat_frame.h"):
            codeobj.makefile_flags(unit, header)
        # a gained unit is the text of the unit it shadows: an edit to that unit rebuilds it
        assert re.search(r"^%s .*: %s$" % (re.escape(unit.replace(".hip", ".o")), re.escape(shadowed)), make, re.M), unit
        with open(os.path.join(codeobj.CSRC, unit)) as f:
            text = re.sub(r"//[^\n]*", "", f.read()).split()
        assert text == ["#define", "BEVWARP_STITCH_GAIN_UNIT", "#include", '"%s"' % shadowed], unit


# ---- the Python entries' and SitePipeline's refusals, all before a device is needed ----

def _cpu_map(dsize=(8, 8)):
    from bev_amd import warp
    dw, dh = dsize
    return warp.WarpMap(torch.zeros((1, dh, dw, 2), dtype=torch.int16), torch.zeros((1, dh, dw), dtype=torch.int16), 1, dsize)


BAD_GAINS = (([1.0, 1.0], "2 gains for 1 cameras"), ([], "0 gains for 1 cameras"), ([[1.0, 1.0]], "shape"), ([[1.0] * 4], "shape"), ([[[1.0] * 3]], "shape"), (1.0, "shape"),
             ([float("nan")], "finite"), ([float("inf")], "finite"), ([[1.0, -0.001, 1.0]], r"\[0, 1023/256\]"), ([4.0], r"\[0, 1023/256\]"), (["bright"], "gains"))


def test_python_entries_refuse_bad_gains_before_the_device():
    from bev_amd import warp
    img, m = torch.zeros((8, 8, 3), dtype=torch.uint8), _cpu_map()
    y, uv = torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8)
    entries = ((warp.remap_stitch, ([img], [m])), (warp.remap_stitch_to_nv12, ([img], [m])), (warp.remap_stitch_to_planar, ([img], [m])),
               (warp.remap_stitch_nv12, ([y], [uv], [m])), (warp.remap_stitch_nv12_to_nv12, ([y], [uv], [m])), (warp.remap_stitch_nv12_to_planar, ([y], [uv], [m])))
    for fn, args in entries:
        for gains, text in BAD_GAINS:
            with pytest.raises(ValueError, match=text):
                fn(*args, gains=gains)
        for gains in ([1023 / 256], [[0.0, 1.0, 2.5]], np.ones(1), torch.ones((1, 3)), None):  # good gains pass on to the device check
            with pytest.raises(ValueError, match="CUDA"):
                fn(*args, gains=gains)
    with pytest.raises(ValueError, match="2 gains for 3 cameras"):
        warp.remap_stitch([img] * 3, [m] * 3, gains=[1.0, 1.0])
    # remap_stitch under gains: uint8 frames of 3 channels only
    for src, text in ((img.float(), "gains apply to uint8 frames of 3 channels; camera 0 is torch.float32"), (img[:, :, :2], "camera 0 .*\\(8, 8, 2\\)"),
                      (img[:, :, :1], "camera 0"), (torch.zeros((8, 8, 4), dtype=torch.uint8), "camera 0"), (img[:, :, 0], "camera 0")):
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch([src], [m], gains=[1.0])
        with pytest.raises(ValueError, match="CUDA"):  # (and what they are without gains)
            warp.remap_stitch([src], [m])
    with pytest.raises(ValueError, match="camera 1 is torch.float32"):
        warp.remap_stitch([img, img.float()], [m, m], gains=[1.0, 1.0])


def test_site_pipeline_refuses_bad_gains():
    from bev_amd import pipeline
    import inspect
    m = _cpu_map()
    for src_format, dst_format in (("bgr", "bgr"), ("nv12", "bgr"), ("bgr", "nv12"), ("nv12", "nv12"), ("bgr", "planes"), ("nv12", "planes")):
        for gains, text in BAD_GAINS:
            with pytest.raises(ValueError, match=text):
                pipeline.SitePipeline([(8, 8)], [m], (8, 8), src_format=src_format, dst_format=dst_format, device="cpu", gains=gains)
    with pytest.raises(ValueError, match="1 gains for 2 cameras"):
        pipeline.SitePipeline([(8, 8)] * 2, [m, m], (8, 8), device="cpu", gains=[1.0])
    assert inspect.signature(pipeline.SitePipeline.__init__).parameters["gains"].default is None
    doc = pipeline.SitePipeline.set_gains.__doc__
    assert "during the call" in doc and "next commit()" in doc


# ---- the solver ----

def test_solve_gains_two_cameras_by_hand():
    """N = [[1000, 400], [400, 1000]], I01 = 100, I10 = 50, alpha = 0.01, beta = 100:
    b = (140000, 140000), A = [[140000 + 2 * 0.01 * 100^2 * 400, -2 * 0.01 * 100 * 50 * 400], [-40000, 140000 + 2 * 0.01 * 50^2 * 400]]
      = [[220000, -40000], [-40000, 160000]], so g = (5 / 6, 13 / 12)."""
    N = np.array([[1000, 400], [400, 1000]])
    S = np.zeros((2, 2, 3))
    S[0, 1], S[1, 0] = 100 * 400, 50 * 400
    S[0, 0], S[1, 1] = 7 * 1000, 9 * 1000  # (a camera's own mean enters nowhere)
    for per_channel in (True, False):
        g = exposure.solve_gains(N, S, per_channel=per_channel)
        assert g.shape == (2, 3) and g.dtype == np.float64
        np.testing.assert_allclose(g, [[5 / 6] * 3, [13 / 12] * 3], rtol=0, atol=1e-12)
    # per channel: channel 1 of both cameras agrees already, channel 2 is the pair the other way round
    S[0, 1], S[1, 0] = (100 * 400, 80 * 400, 50 * 400), (50 * 400, 80 * 400, 100 * 400)
    g = exposure.solve_gains(N, S)
    np.testing.assert_allclose(g[:, 0], [5 / 6, 13 / 12], rtol=0, atol=1e-12)
    np.testing.assert_allclose(g[:, 2], [13 / 12, 5 / 6], rtol=0, atol=1e-12)
    np.testing.assert_allclose(g[:, 1], [1.0, 1.0], rtol=0, atol=1e-12)
    assert abs(g[0, 0] * 100 - g[1, 0] * 50) < abs(100 - 50)  # the gained means are closer than the raw ones
    one = exposure.solve_gains(N, S, per_channel=False)           # the channel means agree (230 / 3 both ways): one solve, all ones
    np.testing.assert_allclose(one, np.ones((2, 3)), rtol=0, atol=1e-12)


def test_solve_gains_equal_means_give_ones():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 8):
        N = rng.integers(1, 5000, (n, n))
        N = N + N.T
        S = np.empty((n, n, 3))
        S[:] = (64.0 * N)[..., None] * np.array([1.0, 2.0, 0.5])  # every overlap mean is (64, 128, 32) in both cameras
        for per_channel in (True, False):
            np.testing.assert_allclose(exposure.solve_gains(N, S, per_channel=per_channel), np.ones((n, 3)), rtol=0, atol=1e-12)
    # a camera that covers nothing keeps 1, and takes no part
    N = np.array([[1000, 400, 0], [400, 1000, 0], [0, 0, 0]])
    S = np.zeros((3, 3, 3))
    S[0, 1], S[1, 0] = 100 * 400, 50 * 400
    np.testing.assert_allclose(exposure.solve_gains(N, S), [[5 / 6] * 3, [13 / 12] * 3, [1.0] * 3], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        exposure.solve_gains(np.ones((2, 3)), np.ones((2, 3, 3)))


def test_overlap_stats_twin_on_hand_made_maps():
    """Two cameras of 6 x 5 px on a 1-row canvas of 8 px through nearest maps: camera 0 under the identity (covers px 0..5), camera 1 two
    pixels to the right (covers px 2..7); a third entry row-wise outside.  Their overlap is px 2..5."""
    from bev_amd import warp
    a = np.zeros((5, 6, 3), np.uint8)
    a[..., 0], a[..., 1], a[..., 2] = np.arange(6) * 10, 20, 30          # camera 0's channel 0 is 10 sx
    b = np.full((5, 6, 3), (100, 110, 120), np.uint8)
    xy0 = np.stack([np.arange(8), np.full(8, 2)], axis=-1).astype(np.int16)[None]
    xy1 = np.stack([np.arange(8) - 2, np.full(8, 2)], axis=-1).astype(np.int16)[None]
    bevs = [RR.remap(s, xy, None, 0, RR.TRANSPARENT, canvas=np.zeros((1, 8, 3), np.uint8))[None] for s, xy in ((a, xy0), (b, xy1))]
    masks = [RR.written(xy, 6, 5, 0)[None] for xy in (xy0, xy1)]
    assert masks[0][0, 0].tolist() == [True] * 6 + [False] * 2 and masks[1][0, 0].tolist() == [False] * 2 + [True] * 6
    N, S = SG.overlap_stats(bevs, masks)
    assert N.dtype == np.int64 and S.dtype == np.int64
    assert N.tolist() == [[6, 4], [4, 6]]
    assert S[0, 0].tolist() == [150, 120, 180] and S[0, 1].tolist() == [20 + 30 + 40 + 50, 80, 120]
    assert S[1, 1].tolist() == [600, 660, 720] and S[1, 0].tolist() == [400, 440, 480]
    # the module's cover test is the definition's, for both interpolations
    for interp in (0, 1):
        for xy in (xy0, xy1, np.array([[[-1, 0], [0, -1], [5, 4], [4, 3], [6, 0], [0, 5], [-32768, -32768], [32767, 32767]]], np.int16)):
            m = warp.WarpMap(torch.from_numpy(xy[None].copy()), torch.zeros((1, 1, 8), dtype=torch.int16) if interp else None, interp, (8, 1))
            np.testing.assert_array_equal(exposure.cover_mask(m, (5, 6))[0].numpy(), RR.written(xy, 6, 5, interp))
    g = exposure.solve_gains(N, S)
    assert g.shape == (2, 3) and (g[0] > 1).all() and (g[1] < 1).all()  # the darker camera is raised, the brighter one lowered


# ---- the launch-context cases of tests/test_gpu_stitch_gain.py: what they need in order to show anything ----

def _context_cases():
    from tests import test_gpu_stitch_gain as TG
    return TG.CONTEXT_CASES


def test_the_context_cases_cover_the_six_gained_entries():
    from tests import launch_contexts as LC
    from tests import test_gpu_stitch_gain as TG
    cases = _context_cases()
    assert sorted({c.symbol for c in cases}) == sorted(s for s in _lib.SYMBOLS if s.startswith("bevwarp_stitch_maps"))
    assert len({c.symbol for c in cases}) == 6 and len({c.name for c in cases}) == len(cases)
    assert [c.name for c in cases if c.no_out] == ["gains-remap_stitch-no_out"]
    assert sorted(c.symbol for c in cases if c.sliceable and not c.no_out) == ["bevwarp_stitch_maps", "bevwarp_stitch_maps_planes", "bevwarp_stitch_maps_to_nv12"]
    plain = {c.name: c for c in LC.CASES}
    for c in cases:  # each stands beside the ungained case of the table: the same symbol, inputs and destination
        other = plain[TG.UNGAINED[c.name]]
        assert other.symbol == c.symbol and other.inputs is c.inputs and other.out_shapes == c.out_shapes and other.sliceable == c.sliceable
    G = SG.quantize(TG.CONTEXT_GAINS, 2)
    assert G.shape == (2, 3) and (G != 256).all() and len({int(g) for g in G.ravel()}) == 6 and G.min() > 0 and G.max() <= 1023


@pytest.mark.parametrize("case", _context_cases(), ids=repr)
def test_the_context_cases_preconditions_hold_on_the_host(case):
    """The two sets give different results under the gains, and each differs from the ungained expectation of the same set (a launch that
    dropped the gain words would pass neither); cover counts 0, 1 and 2; the gains travel as a host value the replay check overwrites."""
    from tests import launch_contexts as LC
    from tests import test_gpu_stitch_gain as TG
    case.assert_preconditions()
    plain = {c.name: c for c in LC.CASES}[TG.UNGAINED[case.name]]
    exp = {which: case.expected(which, which) for which in LC.SETS}
    assert LC.differ(exp["A"], exp["B"])
    for which in LC.SETS:
        ungained = plain.expected(which, which)
        assert [e.shape for e in exp[which]] == [e.shape for e in ungained] and LC.differ(exp[which], ungained)
        for e, u in zip(exp[which], ungained):
            assert not (e == LC.POISON).all()
            if case.cover is not None and e.shape[-1] == 3 and e.dtype == np.uint8:  # interleaved: what no camera covers is not gained
                uncovered = case.cover() == 0
                np.testing.assert_array_equal(e[uncovered], u[uncovered])
    host = case.host("A")
    assert set(host) >= {"gains", "border"} and all(a.dtype == np.float64 and np.isfinite(a).all() for a in host.values())
    np.testing.assert_array_equal(host["gains"], TG.CONTEXT_GAINS)
    assert host["gains"] is not case.host("A")["gains"]  # (fresh arrays per call: the check overwrites its own)
    for count in case.cover():
        assert set(np.unique(count)) == {0, 1, 2}
    if case.no_out:
        for w, e in zip(case.written(), exp["A"][0]):
            assert w.any() and not w.all() and (e[~w] == 0).all() and (e[w] != 0).any()
