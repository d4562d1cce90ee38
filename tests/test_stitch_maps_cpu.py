"""The multi-camera stitch through warp maps (bevwarp_stitch_maps / bevwarp_stitch_maps_nv12, remap_stitch / remap_stitch_nv12) without a
device: the numpy definition (tests/stitch_maps_ref.py) against the routes that exist -- tests/stitch_ref.py's stitch for pinhole maps,
chained tests/remap_ref.py remaps for OVER -- and against hand-computed weights; the C ABI's host checks through the loaded library and
under the sanitizers (tests/host_plan_driver.cpp, family `stitch_maps`); the kernels' code object, the ABI surface and the Python entries' own checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle.warp_numpy import LINEAR, NEAREST
from tests import codeobj
from tests import hostplan
from tests import nv12_ref as NR
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
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


# ---- the definition against the routes that exist ----

@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_pinhole_maps_give_the_matrix_stitch(dtype, interp):
    """Identity (i): with maps built from the matrices, every blend and border of the map stitch is stitch_ref.stitch's, by bits."""
    srcs, Ms = _scene(dtype)
    maps = [RR.build(DSIZE, M, interp=interp) for M in Ms]
    canvas = np.full((DSIZE[1], DSIZE[0], 3), 77, dtype)
    for blend, F in ((SM.OVER, 64), (SM.FEATHER, 1), (SM.FEATHER, 3), (SM.FEATHER, 64)):
        for mode in (SM.CONSTANT, SM.TRANSPARENT):
            got, count = SM.stitch(srcs, maps, interp, blend, F, mode, (3, 200, 41), canvas)
            exp, count_m = SR.stitch(srcs, Ms, DSIZE, interp, blend, F, mode, (3, 200, 41), canvas)
            np.testing.assert_array_equal(got.view(np.uint8), exp.view(np.uint8), err_msg="blend %d F %d mode %d" % (blend, F, mode))
            np.testing.assert_array_equal(count, count_m)
    assert all((count == n).sum() >= 40 for n in range(4))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_over_is_the_chain_of_transparent_remaps(dtype, interp):
    """Identity (ii), for frames and for NV12 planes."""
    srcs, Ms = _scene(dtype)
    maps = [RR.build(DSIZE, M, interp=interp) for M in Ms]
    canvas = np.full((DSIZE[1], DSIZE[0], 3), 77, dtype)
    chain = canvas
    for s, (xy, frac) in zip(srcs, maps):
        chain = RR.remap(s, xy, frac, interp, RR.TRANSPARENT, canvas=chain)
    got, count = SM.stitch(srcs, maps, interp, SM.OVER, mode=SM.TRANSPARENT, canvas=canvas)
    np.testing.assert_array_equal(got, chain)
    assert (got[count == 0] == 77).all() and (count == 0).any()
    back, _ = SM.stitch(srcs[::-1], maps[::-1], interp, SM.OVER, mode=SM.TRANSPARENT, canvas=canvas)
    assert not np.array_equal(back, got)  # (the order of the list decides the overlaps)
    if dtype == np.uint8:
        frames = [NR.frame("uniform", 7 + k, h + (h & 1), w + (w & 1)) for k, (w, h, _) in enumerate(SCENE)]
        chain = canvas
        for (y, uv), (xy, frac) in zip(frames, maps):
            chain = RR.remap(NR.nv12_to_bgr(y, uv, True), xy, frac, interp, RR.TRANSPARENT, canvas=chain)
        got, _ = SM.stitch_nv12([y for y, _ in frames], [uv for _, uv in frames], maps, interp, SM.OVER, mode=SM.TRANSPARENT, canvas=canvas, rgb=True)
        np.testing.assert_array_equal(got, chain)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_feather_single_cover_is_the_cameras_own_remap(dtype, interp):
    srcs, Ms = _scene(dtype)
    srcs = [s * np.float32(1e37) for s in srcs] if dtype == np.float32 else srcs  # ((w p) / w gives p back neither where w p overflows nor where it rounds)
    maps = [RR.build(DSIZE, M, interp=interp) for M in Ms]
    for F in (1, 3, 64):
        got, count = SM.stitch(srcs, maps, interp, SM.FEATHER, F, mode=SM.TRANSPARENT)
        over, _ = SM.stitch(srcs, maps, interp, SM.OVER, mode=SM.TRANSPARENT)
        np.testing.assert_array_equal(got[count <= 1], over[count <= 1])
        for s, (xy, frac) in zip(srcs, maps):
            mine = RR.written(xy, s.shape[1], s.shape[0], interp) & (count == 1)
            assert mine.any()
            np.testing.assert_array_equal(got[mine], RR.remap(s, xy, frac, interp, RR.TRANSPARENT)[mine])
        assert not np.array_equal(got[count >= 2], over[count >= 2])


def _row_map(sx, sy=2):
    """A 1-row nearest map whose entries are (sx[i], sy)."""
    sx = np.asarray(sx)
    return np.stack([sx, np.full_like(sx, sy)], axis=-1).astype(np.int16)[None], None


def test_feather_is_the_weighted_mean_by_hand():
    """Two 1-channel cameras on a 1-row canvas of 8 px, both 6 x 5: camera 0 (10s) under the identity, camera 1 (200s) two pixels to the right."""
    a, b = np.full((5, 6), 10, np.uint8), np.full((5, 6), 200, np.uint8)
    maps = [_row_map(np.arange(8)), _row_map(np.arange(8) - 2)]
    got, count = SM.stitch([a, b], maps, NEAREST, SM.FEATHER, 64, SM.CONSTANT, 7)
    assert count[0].tolist() == [1, 1, 2, 2, 2, 2, 1, 1]
    # sy = 2: d_y = 3.  camera 0 at sx = 2..5 has d = min(sx + 1, 6 - sx, 3) = 3, 3, 2, 1; camera 1 at sx = 0..3 has 1, 2, 3, 3
    want = [(3 * 10 + 1 * 200 + 2) // 4, (3 * 10 + 2 * 200 + 2) // 5, (2 * 10 + 3 * 200 + 2) // 5, (1 * 10 + 3 * 200 + 2) // 4]
    assert got[0].tolist() == [10, 10] + want + [200, 200]
    cut, _ = SM.stitch([a, b], maps, NEAREST, SM.FEATHER, 2, SM.CONSTANT, 7)  # F = 2: weights 2, 2, 2, 1 and 1, 2, 2, 2
    assert cut[0].tolist() == [10, 10, (2 * 10 + 200 + 1) // 3, (20 + 400 + 2) // 4, (20 + 400 + 2) // 4, (10 + 400 + 1) // 3, 200, 200]
    mean, _ = SM.stitch([a, b], maps, NEAREST, SM.FEATHER, 1)  # F = 1: the plain mean, rounded half up
    assert mean[0].tolist() == [10, 10, 105, 105, 105, 105, 200, 200]
    # float32: acc = (0 + w0 p0) + w1 p1 in float32, then one division
    f = np.float32
    gotf, _ = SM.stitch([np.full((5, 6), 0.1, f), np.full((5, 6), 0.7, f)], maps, NEAREST, SM.FEATHER, 64)
    assert gotf[0, 3] == (f(0) + f(3) * f(0.1) + f(2) * f(0.7)) / f(5)
    assert gotf[0, 0] == f(0.1) and gotf[0, 7] == f(0.7)


def test_single_cover_rule_and_uncovered_pixels():
    a, b = np.full((5, 6, 2), 10, np.uint8), np.full((5, 6, 2), 200, np.uint8)
    maps = [_row_map([0, 1, 9, -1]), _row_map([-3, 2, 9, 6])]  # px 0: camera 0 alone; px 1: both; px 2, 3: neither
    canvas = np.full((1, 4, 2), 77, np.uint8)
    for blend in (SM.OVER, SM.FEATHER):
        got, count = SM.stitch([a, b], maps, NEAREST, blend, 64, SM.TRANSPARENT, canvas=canvas)
        assert count[0].tolist() == [1, 1 + 1, 0, 0] and got[0, 0].tolist() == [10, 10] and got[0, 2:].tolist() == [[77, 77]] * 2
        got, _ = SM.stitch([a, b], maps, NEAREST, blend, 64, SM.CONSTANT, (3, 250.5))
        assert got[0, 2:].tolist() == [[3, 250]] * 2  # (250.5 rounds half to even)
    assert SM.stitch([a, b], maps, NEAREST, SM.OVER)[0][0, 1].tolist() == [200, 200]
    assert SM.stitch([a, b], maps, NEAREST, SM.FEATHER)[0][0, 1].tolist() == [(2 * 10 + 3 * 200 + 2) // 5] * 2


@pytest.mark.parametrize("interp", [NEAREST, LINEAR])
def test_sentinel_never_covers(interp):
    """(-32768, -32768) is outside every admissible source, the largest included; so is (32767, 32767)."""
    xy = np.array([[[-32768, -32768], [32767, 32767], [0, 0], [32766, 32766]]], np.int16)
    frac = None if interp == NEAREST else np.array([[0, 1023, 0xffff, 0]], np.uint16)
    for w, h in ((1, 1), (2, 2), (8, 8), (32767, 32767), (32767, 1), (1, 32767)):
        cover = RR.written(xy, w, h, interp)[0]
        assert not cover[0] and not cover[1]
        assert cover[2] == (interp == NEAREST or (w >= 2 and h >= 2))
        assert cover[3] == (interp == NEAREST and (w, h) == (32767, 32767))
    s = np.full((3, 3), 9, np.uint8)
    got, count = SM.stitch([s, s], [(xy, frac), (xy, frac)], interp, SM.FEATHER, 4096, SM.CONSTANT, 5)
    assert count[0].tolist() == [0, 0, 2, 0] and got[0].tolist() == [5, 5, 9, 5]


# ---- the ABI surface, without a device (fake pointers, never dereferenced: every call below fails validation first or has no frame) ----

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
PASSES = NOT_FINITE  # a call that passes every check of its cameras and of the canvas ends on the NaN border value: nothing is launched
DST, XY, FR = 1 << 20, 1 << 24, 1 << 26
# an 8 x 8 source of 8-bit B, G, R pixels, and its NV12 twin; one shared bilinear map of an 8 x 8 canvas
CAM = dict(src=4096, uv=0, h=8, w=8, fs=192, rs=24, uv_fs=0, uv_rs=0, xy=XY, frac=FR, xy_fs=256, xy_rs=32, fr_fs=128, fr_rs=16, map_count=1)
NVCAM = dict(CAM, uv=8192, fs=64, rs=8, uv_fs=32, uv_rs=8)
CALL = dict(n=None, cams_null=0, dst=DST, batch=1, dh=8, dw=8, ch=3, dfs=192, drs=24, dtype=0, interp=1, blend=0, feather=64, rgb=0, mode=0, border=2)


def _c(**kw):
    return dict(CAM, **kw)


def _n(**kw):
    return dict(NVCAM, **kw)


def _case(kind, cams, want, **kw):
    return kind, cams, dict(CALL, **kw), want


def _cases():
    big, top = 2147483647, (1 << 63) - 1
    g, v = _c(), _n()
    out = []
    for kind, k in (("maps", g), ("nv12", v)):
        # 1. the call's own arguments, before any camera or format is looked at
        out += [_case(kind, [], BAD_ARG, n=0), _case(kind, [k], PASSES), _case(kind, [k] * 8, PASSES), _case(kind, [k] * 9, BAD_ARG), _case(kind, [k], BAD_ARG, n=-1),
                _case(kind, [k], BAD_ARG, n=big), _case(kind, [k], BAD_ARG, cams_null=1), _case(kind, [k] * 9, BAD_ARG, interp=2), _case(kind, [dict(k, src=0)] * 9, BAD_ARG)]
        out += [_case(kind, [k], want, blend=1, feather=f) for f, want in ((0, BAD_ARG), (1, PASSES), (4096, PASSES), (4097, BAD_ARG), (-big, BAD_ARG), (big, BAD_ARG))]
        out += [_case(kind, [k], PASSES, blend=0, feather=f) for f in (0, 4097, -big, big)]  # OVER ignores it
        out += [_case(kind, [k], BAD_ARG, blend=1, feather=0, interp=2)]
        # 2. per camera: the formats (blend and border mode are part of them)
        out += [_case(kind, [k], UNSUPPORTED, blend=b) for b in (2, -1, big)] + [_case(kind, [k], UNSUPPORTED, mode=m) for m in (1, 2, 3, 4, 6, 16, 21, -1)]
        out += [_case(kind, [k], UNSUPPORTED, interp=i) for i in (2, 3, -1)] + [_case(kind, [k], PASSES, interp=0), _case(kind, [k], OK, mode=5, batch=0)]
        # NULL images, sides, the map count, layouts
        out += [_case(kind, [dict(k, src=0)], BAD_ARG), _case(kind, [dict(k, xy=0)], BAD_ARG), _case(kind, [dict(k, frac=0)], BAD_ARG),
                _case(kind, [dict(k, frac=0)], PASSES, interp=0), _case(kind, [dict(k, xy=0)], BAD_ARG, interp=0), _case(kind, [k], BAD_ARG, dst=0),
                _case(kind, [dict(k, h=0)], BAD_ARG), _case(kind, [dict(k, w=-1)], BAD_ARG), _case(kind, [k], BAD_ARG, dw=0), _case(kind, [k], BAD_ARG, dh=-big - 1),
                _case(kind, [k], BAD_ARG, batch=-1)]
        two = dict(batch=2)
        out += [_case(kind, [dict(k, map_count=m)], BAD_ARG) for m in (0, 2, -1)] + [_case(kind, [dict(k, map_count=m)], BAD_ARG, **two) for m in (0, 3)]
        out += [_case(kind, [dict(k, map_count=2)], PASSES, **two), _case(kind, [dict(k, map_count=1)], PASSES, **two),
                _case(kind, [k, dict(k, map_count=2)], PASSES, **two),                                   # shared and per-frame maps in one call
                _case(kind, [dict(k, map_count=2, xy_fs=255)], BAD_ARG, **two), _case(kind, [dict(k, map_count=2, fr_fs=127)], BAD_ARG, **two),
                _case(kind, [dict(k, map_count=1, xy_fs=1, fr_fs=1)], PASSES, **two)]                    # a shared map's frame strides are not looked at
        out += [_case(kind, [dict(k, xy=XY + 2)], BAD_ARG), _case(kind, [dict(k, xy_rs=34)], BAD_ARG), _case(kind, [dict(k, xy_rs=28)], BAD_ARG),
                _case(kind, [dict(k, frac=FR + 1)], BAD_ARG), _case(kind, [dict(k, fr_rs=17)], BAD_ARG), _case(kind, [dict(k, fr_rs=14)], BAD_ARG),
                _case(kind, [dict(k, xy=XY + 4, frac=FR + 2)], PASSES), _case(kind, [k], BAD_ARG, drs=23), _case(kind, [k], BAD_ARG, dfs=191, **two)]
        # the first failing camera decides, not the first phase
        wide = dict(k, w=32768, rs=(3 if kind == "maps" else 1) * 32768, fs=24 * 32768, uv_rs=32768, uv_fs=4 * 32768)
        out += [_case(kind, [wide], TOO_LARGE), _case(kind, [k, k, dict(k, src=0)], BAD_ARG), _case(kind, [k, k, wide], TOO_LARGE),
                _case(kind, [wide, dict(k, src=0)], TOO_LARGE), _case(kind, [dict(k, src=0), wide], BAD_ARG), _case(kind, [k, dict(k, map_count=2)], BAD_ARG),
                _case(kind, [k] * 7 + [dict(k, frac=0)], BAD_ARG), _case(kind, [k] * 7 + [wide], TOO_LARGE), _case(kind, [wide, k], UNSUPPORTED, blend=2, ch=3),
                _case(kind, [dict(k, xy_rs=1 << 24, fr_rs=1 << 24)], PASSES)]                             # the maps have no source limits
        # dst against each read image of a later camera; the cameras may share every byte they read, and a map
        out += [_case(kind, [k, dict(k, src=DST)], OVERLAP), _case(kind, [k, dict(k, src=DST + 191)], OVERLAP), _case(kind, [k, dict(k, src=DST + 192)], PASSES),
                _case(kind, [k, dict(k, xy=DST)], OVERLAP), _case(kind, [k, dict(k, xy=DST + 188)], OVERLAP), _case(kind, [k, dict(k, xy=DST + 192)], PASSES),
                _case(kind, [k, dict(k, xy=DST - 252)], OVERLAP), _case(kind, [k, dict(k, xy=DST - 256)], PASSES),
                _case(kind, [k, k, dict(k, frac=DST + 190)], OVERLAP), _case(kind, [k, k, dict(k, frac=DST + 192)], PASSES),
                _case(kind, [k, dict(k, frac=DST + 100)], PASSES, interp=0),                              # (nearest: not read)
                _case(kind, [dict(k, src=DST), k], OVERLAP), _case(kind, [k, dict(k, src=DST)], OK, batch=0, border=1),  # (an empty batch has no bytes to share)
                _case(kind, [k, k, k], PASSES), _case(kind, [k, dict(k, src=4100), dict(k, src=12288, uv=12288 + 64)], PASSES),
                _case(kind, [dict(k, xy=4096, frac=4096 + 64), k], PASSES)]
        # strides next to 2^63: bad arguments or size limits, not overflows (one row, or two frames: the images' last bytes stay below 2^64)
        out += [_case(kind, [dict(k, xy_rs=top - 3, fr_rs=top - 1)], PASSES, dh=1, drs=top), _case(kind, [dict(k, map_count=2, xy_fs=top - 3, fr_fs=top - 1)], PASSES, dh=1, **two),
                _case(kind, [dict(k, map_count=2, xy_rs=top - 3, xy_fs=top - 3)], BAD_ARG, **two), _case(kind, [dict(k, map_count=2, fr_rs=top - 1, fr_fs=top - 1)], BAD_ARG, **two),
                _case(kind, [k], BAD_ARG, batch=3, drs=top, dfs=top), _case(kind, [dict(k, rs=top)], TOO_LARGE), _case(kind, [dict(k, rs=-1)], BAD_ARG),
                _case(kind, [dict(k, rs=-top - 1)], BAD_ARG), _case(kind, [k], BAD_ARG, drs=-top - 1), _case(kind, [dict(k, xy_rs=top)], BAD_ARG),
                _case(kind, [dict(k, fs=-top - 1)], BAD_ARG, **two), _case(kind, [dict(k, fs=top)], PASSES)]  # (one frame: its stride is not looked at)
        # 3. the destination's sides, 4. the border value (the constant border's only), 5. the empty batch
        w20 = 1 << 20
        far = dict(k, xy=1 << 44, frac=1 << 48)
        ch = 1 if kind == "maps" else 3
        one = dict(ch=1, dst=1 << 40)
        f1 = dict(far, rs=8, fs=64) if kind == "maps" else far
        out += [_case(kind, [dict(f1, xy_rs=4 * w20, fr_rs=2 * w20)], PASSES, dw=w20, dh=1, drs=ch * w20, dfs=ch * w20, **one),
                _case(kind, [dict(f1, xy_rs=8 * w20, fr_rs=4 * w20)], TOO_LARGE, dw=w20 + 1, dh=1, drs=4 * w20, dfs=4 * w20, **one),
                _case(kind, [f1], TOO_LARGE, dw=8, dh=w20 + 1, drs=8 * ch, dfs=1 << 26, **one),
                _case(kind, [f1], TOO_LARGE, dw=8, dh=w20 + 1, drs=8 * ch, dfs=1 << 26, batch=0, **one),
                _case(kind, [f1], TOO_LARGE, batch=big, drs=8 * ch, dfs=64 * ch, **one),                 # (2 tiles per frame: the grid passes 2^31 - 1 items)
                _case(kind, [k], OK, border=0, batch=0), _case(kind, [k], OK, border=1, batch=0), _case(kind, [k], NOT_FINITE, border=2, batch=0),
                _case(kind, [k], OK, border=2, mode=5, batch=0), _case(kind, [k, dict(k, src=0)], BAD_ARG, batch=0)]
    # the formats and the order of checks that differ between the two entries
    out += [_case("maps", [g], UNSUPPORTED, dtype=d) for d in (2, 3, 4, -1)] + [_case("maps", [g], UNSUPPORTED, ch=c) for c in (0, 5)]
    out += [_case("maps", [_c(rs=8 * c, fs=64 * c)], PASSES, ch=c, drs=8 * c, dfs=64 * c) for c in (1, 2, 4)]
    out += [_case("maps", [_c(rs=96, fs=768)], PASSES, dtype=1, drs=96, dfs=768), _case("maps", [_c(rs=98, fs=784)], BAD_ARG, dtype=1, drs=96, dfs=768),
            _case("maps", [_c(uv=0, uv_rs=-5, uv_fs=3)], PASSES),                                        # uv and its strides are not looked at
            _case("maps", [_c(map_count=2)], UNSUPPORTED, dtype=3), _case("maps", [_c(rs=23)], UNSUPPORTED, ch=5),      # bevwarp_remap: the format first
            _case("maps", [_c(h=7, w=7, rs=21, fs=147)], PASSES)]                                         # odd sides are fine for interleaved frames
    out += [_case("nv12", [v], UNSUPPORTED, rgb=r) for r in (2, -1)] + [_case("nv12", [v], PASSES, rgb=1), _case("nv12", [v], PASSES, dtype=9, ch=7)]
    out += [_case("nv12", [_n(map_count=2)], BAD_ARG, rgb=2), _case("nv12", [_n(uv_rs=6)], BAD_ARG, rgb=2),             # bevwarp_remap_nv12: the format last
            _case("nv12", [_n(uv=0)], BAD_ARG), _case("nv12", [_n(h=7)], BAD_ARG), _case("nv12", [_n(w=7)], BAD_ARG), _case("nv12", [_n(h=6, w=6)], PASSES),
            _case("nv12", [_n(uv=8193)], BAD_ARG), _case("nv12", [_n(uv_rs=9)], BAD_ARG), _case("nv12", [_n(uv_rs=10)], PASSES),
            _case("nv12", [_n(uv_fs=33)], BAD_ARG, batch=2), _case("nv12", [_n(uv_fs=30)], BAD_ARG, batch=2), _case("nv12", [_n(uv_fs=34)], PASSES, batch=2),
            _case("nv12", [v, _n(uv=DST)], OVERLAP), _case("nv12", [v, _n(uv=DST + 190)], OVERLAP), _case("nv12", [v, _n(uv=DST + 192)], PASSES),
            _case("nv12", [v, _n(uv=DST - 30)], OVERLAP), _case("nv12", [v, _n(uv=DST - 32)], PASSES),
            _case("nv12", [_n(uv_rs=(1 << 63) - 2)], TOO_LARGE), _case("nv12", [_n(uv_rs=(1 << 63) - 1)], BAD_ARG)]
    return out


def _line(kind, cams, a):
    n = len(cams) if a["n"] is None else a["n"]
    head = [n, a["cams_null"], a["dst"], a["batch"], a["dh"], a["dw"], a["ch"], a["dfs"], a["drs"], a["dtype"], a["interp"], a["blend"], a["feather"], a["rgb"], a["mode"],
            a["border"], len(cams)]
    body = [v for c in cams for v in (c["src"], c["uv"], c["h"], c["w"], c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"], c["frac"], c["xy_fs"], c["xy_rs"], c["fr_fs"],
                                      c["fr_rs"], c["map_count"])]
    return kind + " " + " ".join(str(v) for v in head + body)


def _through_the_library(lib, kind, cams, a):
    arr = (_lib.MapCamera * max(len(cams), 1))(*[_lib.MapCamera(c["src"] or None, c["uv"] or None, c["fs"], c["rs"], c["uv_fs"], c["uv_rs"], c["xy"] or None, c["frac"] or None,
                                                                c["xy_fs"], c["xy_rs"], c["fr_fs"], c["fr_rs"], c["h"], c["w"], c["map_count"], 0) for c in cams])
    nb = 3 if kind == "nv12" else a["ch"]
    bv = [1.0, 2.0, 3.0, 4.0]
    if a["border"] == 2 and 1 <= nb <= 4:
        bv[nb - 1] = float("nan")
    border = ctypes.cast((ctypes.c_double * 4)(*bv), ctypes.c_void_p) if a["border"] else None
    head = (None if a["cams_null"] else ctypes.addressof(arr), len(cams) if a["n"] is None else a["n"], a["dst"] or None, a["batch"], a["dh"], a["dw"])
    if kind == "nv12":
        return lib.bevwarp_stitch_maps_nv12(*head, a["dfs"], a["drs"], a["interp"], a["blend"], a["feather"], a["rgb"], a["mode"], border, None)
    return lib.bevwarp_stitch_maps(*head, a["ch"], a["dfs"], a["drs"], a["dtype"], a["interp"], a["blend"], a["feather"], a["mode"], border, None)


def test_abi_surface():
    lib = hostplan.built_lib()
    for name in ("bevwarp_stitch_maps", "bevwarp_stitch_maps_nv12"):
        assert name in _lib.SYMBOLS and getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None
    assert lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.MapCamera) == 112
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "int bevwarp_stitch_maps(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w, int channels," in header
    assert "int bevwarp_stitch_maps_nv12(const bevwarp_map_camera *cams /*HOST*/, int n_cams, void *dst, int batch, int dst_h, int dst_w," in header
    assert "typedef struct bevwarp_map_camera {" in header and "bevwarp_stitch_maps, bevwarp_stitch_maps_nv12" in header.split("Conventions")[0]
    import bev.warp as bev_warp
    from bev_amd import warp
    assert bev_warp.remap_stitch is warp.remap_stitch and bev_warp.remap_stitch_nv12 is warp.remap_stitch_nv12


def test_status_order_through_the_library():
    """Every case either fails a check or has nothing to launch (an empty batch, or a NaN border value after every other check)."""
    lib = hostplan.built_lib()
    for kind, cams, a, want in _cases():
        assert want != OK or a["batch"] == 0
        assert _through_the_library(lib, kind, cams, a) == want, (_line(kind, cams, a), want)


# ---- the host checks under the sanitizers ----

@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_status_under_sanitizers(driver):
    cases = _cases()
    got = hostplan.run_driver(driver, [_line(kind, cams, a) for kind, cams, a, _ in cases], "stitch_maps")
    for (kind, cams, a, want), out in zip(cases, got):
        assert out[0] == want and (want == OK or out[1:] == [0, 0]), (_line(kind, cams, a), out, want)
    # the grid of a call that goes on to a launch: kBorderTileW x kBorderTileH tiles over the canvas, one frame per item whatever the map count
    for kind, k in (("maps", _c()), ("nv12", _n())):
        lines = [_line(kind, [k] * n, dict(dict(CALL, border=1), **kw)) for n, kw in ((1, {}), (8, {}), (3, dict(batch=5, dfs=192)), (1, dict(batch=0)), (1, dict(mode=5, border=2)))]
        assert hostplan.run_driver(driver, lines, "stitch_maps") == [[OK, OK, 2], [OK, OK, 2], [OK, OK, 10], [OK, OK, 0], [OK, OK, 2]]
        wide = dict(dw=260, dh=22, drs=780, dfs=780 * 22, dst=1 << 40)
        lines = [_line(kind, [dict(k, xy=1 << 44, frac=1 << 48, xy_rs=1040, fr_rs=520, xy_fs=1040 * 22, fr_fs=520 * 22, map_count=m)], dict(CALL, border=0, batch=3, **wide)) for m in (1, 3)]
        assert hostplan.run_driver(driver, lines, "stitch_maps") == [[OK, OK, 2 * 6 * 3]] * 2


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_stitch_maps_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_stitch_maps.hip", tmp_path, "warp_stitch_maps.h")
    frames = {n: k for n, k in found.items() if "stitch_maps_kernel" in n}
    nv12 = {n: k for n, k in found.items() if "stitch_maps_nv12_kernel" in n}
    assert len(frames) == 2 * 4 * 2 * 2, len(frames)  # dtype x channels x interpolation x blend
    assert len(nv12) == 2 * 2 * 2, len(nv12)          # interpolation x blend x channel order
    assert len(found) == len(frames) + len(nv12)
    codeobj.assert_lean(found)
    assert "-fno-fast-math" in codeobj.makefile_flags("warp_stitch_maps.hip", "warp_stitch_maps.h")
    for unit in ("warp_stitch_maps.hip", "warp_stitch.hip"):  # (the shared stitch samplers rebuild every user, FEATHER's division the matrix stitch too)
        for header in ("stitch_sample.h", "tap_load.h", "nv12_sample.h"):
            codeobj.makefile_flags(unit, header)


# ---- the map samplers' helpers are defined once ----

def test_map_sampler_helpers_have_one_definition():
    """The units that sample through warp maps share their helpers through headers and included text: a unit that
    brings a copy of one back -- above all of convert_packed, whose value barrier keeps wrong pixels off the MI355X -- fails here."""
    import glob
    import re
    csrc = os.path.join(ROOT, "bev_amd", "csrc")
    code = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.inc"))):
        with open(path) as f:
            code[os.path.basename(path)] = re.sub(r"//[^\n]*", "", f.read())  # (comments may name them)
    assert len(code) > 60

    def where(pattern):
        return sorted((name, len(re.findall(pattern, text))) for name, text in code.items() if re.search(pattern, text))

    once = {r"\bint\s+div_byte_mean\s*\(": "stitch_sample.h",
            r"\bvoid\s+load_camera_entries\s*\(": "stitch_sample.h",
            r"\buint32_t\s+sample_inlier_nv12\s*\(": "stitch_sample.h",
            r"\buint32_t\s+sample_entry_nv12\s*\(": "remap_sample_nv12.h",
            r"\bstruct\s+NvTaps\b": "remap_sample_nv12.h",
            r"\buint32_t\s+pair_at\s*\(": "remap_sample_nv12.h",
            r"\buint32_t\s+convert_packed\s*\(": "nv12_sample.h",
            r'\basm\s*\(\s*""\s*:\s*"\+v"\s*\(\s*g\s*\)\s*\)': "nv12_sample.h",                 # the value barrier
            r"\bvoid\s+load_pair\s*\(": "tap_load.h",                                             # the packed 6-byte pair load
            r"\bvoid\s+load_pair_u8x3\s*\(": "tap_load.h",
            r"\bPixel<T, C>\s+load_at\s*\(": "tap_load.h",
            r"\buint32_t\s+load_at\s*\(": "tap_load.h",
            r"\buint32_t\s+sample_entry\s*\(": "remap_sample_u8x3.h",                             # the packed sampler
            r"\bPixel<T, C>\s+sample_entry\s*\(": "warp_map.hip"}                                 # the generic one
    for pattern, home in once.items():
        assert where(pattern) == [(home, 1)], (pattern, where(pattern))
    # (the bicubic unit has a sample_inlier of its own, for its 16 taps)
    for pattern in (r"\buint32_t\s+sample_inlier\s*\(", r"\bPixel<T, C>\s+sample_inlier\s*\("):
        assert [w for w in where(pattern) if w[0] != "warp_cubic.hip"] == [("stitch_sample.h", 1)], (pattern, where(pattern))
    # two structs are called Taps: remap_kernel's, for every pixel type, and the packed one
    assert where(r"\bstruct\s+Taps\b") == [("remap_sample_u8x3.h", 1), ("warp_map.hip", 1)]
    # the 8-bit 3-channel camera loop is text that both of its kernels include, and the feather weight is written there and in the two generic loops only
    assert where(r'#include "stitch_maps_u8x3\.inc"') == [("warp_stitch_maps_nv12_out.hip", 1), ("warp_stitch_maps_planes.hip", 1)]
    assert where(r",\s*a\.feather\s*\)") ==[("stitch_maps_u8x3.inc", 1), ("warp_stitch.hip", 1), ("warp_stitch_maps.hip", 1)]


# ---- the Python entries' own checks, all before a device is needed ----

def _cpu_map(n=1, dsize=(8, 8), interp=1):
    from bev_amd import warp
    dw, dh = dsize
    return warp.WarpMap(torch.zeros((n, dh, dw, 2), dtype=torch.int16), torch.zeros((n, dh, dw), dtype=torch.int16) if interp == 1 else None, interp, dsize)


def test_python_entries_validate_before_the_device():
    from bev_amd import warp
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)
    m = _cpu_map()
    for srcs, maps, kw, text in (([], [], {}, "1..8 cameras"), ([img] * 9, [m] * 9, {}, "1..8 cameras"), ([img, img], [m], {}, "1 warp maps for 2 cameras"),
                                 ([img], [m], dict(blend="mean"), "blend"), ([img], [m], dict(blend="feather", feather=0), "1..4096"),
                                 ([img], [m], dict(blend="feather", feather=4097), "1..4096"), ([img], [m], dict(border_mode=warp.BORDER_REPLICATE), "border mode"),
                                 ([img], [m], dict(border_mode=warp.BORDER_REFLECT_101), "border mode"), ([img], [np.eye(3)], {}, "WarpMap per camera .*camera 0 has ndarray"),
                                 ([img, img], [m, _cpu_map(dsize=(8, 6))], {}, "map of camera 1 has dsize"), ([img, img], [m, _cpu_map(interp=0)], {}, "map of camera 1 .* interpolation 0"),
                                 ([img, img.float()], [m] * 2, {}, "camera 1 has dtype torch.float32"), ([img, img[:, :, :2]], [m] * 2, {}, "camera 1 .* 2 channels"),
                                 ([img[None], img, img[None].expand(2, 8, 8, 3)], [m] * 3, {}, "camera 2 .* batch 2"), ([img[:, :, 0], img], [m] * 2, {}, "camera 1 .* 3 channels"),
                                 ([img, img.double()], [m] * 2, {}, "camera 1 is torch.float64"), ([img.numpy()], [m], {}, "camera 0 is"),
                                 ([img], [_cpu_map(n=2)], {}, "2 frames for a batch of 1"), ([img[None].expand(3, 8, 8, 3)], [_cpu_map(n=2)], {}, "2 frames for a batch of 3"),
                                 ([img], [m], dict(out=torch.zeros((6, 8, 3), dtype=torch.uint8)), "dsize is \\(8, 8\\), out is"),
                                 ([img], [m], dict(out=torch.zeros((8 * 8 * 3 + 1,), dtype=torch.uint8)), "out has 193 elements"),
                                 ([img], [m], {}, "CUDA")):
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch(srcs, maps, **kw)
    y, uv = torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((4, 4, 2), dtype=torch.uint8)
    for ys, uvs, maps, kw, text in (([], [], [], {}, "1..8 cameras"), ([y] * 9, [uv] * 9, [m] * 9, {}, "1..8 cameras"), ([y, y], [uv, uv], [m], {}, "1 warp maps for 2 cameras"),
                                    ([y, y], [uv], [m, m], {}, "1 uv planes for 2 cameras"), ([y], [uv], [m], dict(blend="mean"), "blend"),
                                    ([y], [uv], [m], dict(blend="feather", feather=4097), "1..4096"), ([y], [uv], [m], dict(border_mode=warp.BORDER_WRAP), "border mode"),
                                    ([y], [uv], [np.eye(3)], {}, "WarpMap per camera"), ([y, y], [uv, uv], [m, _cpu_map(interp=0)], {}, "map of camera 1"),
                                    ([y], [uv], [m], {}, "CUDA"), ([y.numpy()], [uv], [m], {}, "CUDA")):
        with pytest.raises(ValueError, match=text):
            warp.remap_stitch_nv12(ys, uvs, maps, **kw)
