"""The fixed-camera warp maps (bevwarp_build_map, bevwarp_remap; build_warp_map, remap, convert_maps) without a device: the numpy
definition (tests/remap_ref.py) tied to the trusted references by bits, convertMaps' known answers, the C ABI's host checks and the
frames-per-item plan under the sanitizers (tests/host_plan_driver.cpp, family `remap`), the kernels' code object, the ABI surface and the Python
entries' own refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import border_ref as BR
from tests import codeobj
from tests import hostplan
from tests import lens_ref as LR
from tests import remap_ref as RR
from tests.test_lens_cpu import GEOMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
LENSES = {"A": LR.LENS_A, "B": LR.LENS_B}
BV = (7.0, 200.0, 31.0)


def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


# ---- the definition tied to the trusted references, by bits ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_pinhole_maps_reproduce_the_oracle_and_the_border_reference(geom, interp, dtype):
    sw, sh, dw, dh, M = GEOMS[geom]
    xy, frac = RR.build((dw, dh), wn.invert3x3(M), None, INF, interp)
    assert xy.shape == (dh, dw, 2) and xy.dtype == np.int16 and (frac is None) == (interp == wn.NEAREST)
    for c in (1, 3):
        src = _src((sh, sw, c), dtype, seed=40 + c)
        canvas = _src((dh, dw, c), dtype, seed=50 + c)
        got = RR.remap(src, xy, frac, interp, RR.CONSTANT, border_value=BV[:c])
        np.testing.assert_array_equal(got, wn.warp_perspective(src, M, (dw, dh), interp, border_value=BV[:c]))
        for mode in RR.MODES[1:]:
            got = RR.remap(src, xy, frac, interp, mode, canvas=canvas)
            np.testing.assert_array_equal(got, BR.warp(src, M, (dw, dh), interp, mode, canvas=canvas), err_msg=BR.NAMES[mode])


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("lens_name", sorted(LENSES))
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_lens_maps_reproduce_the_lens_reference(geom, lens_name, interp, dtype):
    """... and the sentinel argument of include/bevwarp.h under test: with invalid pixels stored as (-32768, -32768), frac 0, a sampler that
    knows nothing of validity gives lens_ref.warp's pixels for CONSTANT and TRANSPARENT."""
    sw, sh, dw, dh, M = GEOMS[geom]
    K = LR.camera_K(sw, sh)
    R, lens, r2_max = LR.ray_matrix(M, K), LR.lens12(K, LENSES[lens_name]), LR.lens_valid_r2(LENSES[lens_name])
    xy, frac = RR.build((dw, dh), R, lens, r2_max, interp)
    for c in (1, 3):
        src = _src((sh, sw, c), dtype, seed=60 + c)
        canvas = _src((dh, dw, c), dtype, seed=70 + c)
        np.testing.assert_array_equal(RR.remap(src, xy, frac, interp, RR.CONSTANT, border_value=BV[:c]),
                                      LR.warp(src, R, lens, r2_max, (dw, dh), interp, LR.CONSTANT, border_value=BV[:c]))
        np.testing.assert_array_equal(RR.remap(src, xy, frac, interp, RR.TRANSPARENT, canvas=canvas),
                                      LR.warp(src, R, lens, r2_max, (dw, dh), interp, LR.TRANSPARENT, canvas=canvas))


@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_sentinel_sits_exactly_on_the_invalid_pixels(interp):
    """brno with lens A has invalid pixels, some of which would land inside the frame (test_lens_cpu's ghosts)."""
    sw, sh, dw, dh, M = GEOMS["brno"]
    K = LR.camera_K(sw, sh)
    R, lens, r2_max = LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A), LR.lens_valid_r2(LR.LENS_A)
    xy, frac = RR.build((dw, dh), R, lens, r2_max, interp)
    sx, sy, _, _, valid = LR.maps((dw, dh), R, lens, r2_max, interp)
    sentinel = (xy[..., 0] == -32768) & (xy[..., 1] == -32768)
    assert (~valid).sum() > 0 and valid.sum() > 0
    np.testing.assert_array_equal(sentinel, ~valid)
    if frac is not None:
        assert not frac[~valid].any()
    ghosts = LR.inliers(sx, sy, np.ones_like(valid), sw, sh, interp) & ~valid
    assert ghosts.sum() > 0 and not RR.written(xy, sw, sh, interp)[ghosts].any()


# ---- convertMaps ----

def test_convert_maps_known_answers():
    from bev_amd import warp
    f = np.float32
    xs = np.array([[0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, 1e6, -1e6, np.nan, 3.25, -0.25]], f)
    ys = np.zeros_like(xs)
    # X = rint(32 x): ties to even 0, 2, 2, -0 -> 0, -2; +-1e6 * 32 = +-3.2e7 -> sx saturates; NaN -> INT_MAX; 104; -8
    want_X = [0, 2, 2, 0, -2, 32000000, -32000000, 2147483647, 104, -8]
    xy, frac = warp.convert_maps(xs, ys)
    assert xy.dtype == np.int16 and frac.dtype == np.uint16 and xy.shape == (1, 10, 2) and frac.shape == (1, 10)
    np.testing.assert_array_equal(xy[0, :, 0], [max(min(X >> 5, 32767), -32768) for X in want_X])
    np.testing.assert_array_equal(frac[0], [X & 31 for X in want_X])
    assert list(xy[0, 4]) == [-1, 0] and frac[0, 4] == 30          # -1.5 / 32 -> X = -2: sx = -1, fx = 30
    assert xy[0, 5, 0] == 32767 and xy[0, 6, 0] == -32768 and xy[0, 7, 0] == 32767
    xy2, frac2 = warp.convert_maps(np.stack([ys, xs], axis=-1))       # (H, W, 2): x first
    np.testing.assert_array_equal(xy2[..., 1], xy[..., 0])
    np.testing.assert_array_equal(frac2, (frac.astype(np.int64) << 5).astype(np.uint16))
    # nearest: the coordinate itself is rounded, half to even, and there is no frac plane
    xn = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, 1e6, -1e6, np.nan]], f)
    xyn, fn = warp.convert_maps(xn, np.zeros_like(xn), nearest=True)
    assert fn is None
    np.testing.assert_array_equal(xyn[0, :, 0], [0, 2, 2, 0, -2, 32767, -32768, 32767])
    # against the scalar restatement, on seeded coordinates of every magnitude
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((6, 40)) * 10.0 ** rng.integers(-3, 7, (6, 40))).astype(f)
    y = (rng.standard_normal((6, 40)) * 10.0 ** rng.integers(-3, 7, (6, 40))).astype(f)
    for nearest in (False, True):
        got, want = warp.convert_maps(x, y, nearest=nearest), RR.convert_maps(x, y, nearest=nearest)
        np.testing.assert_array_equal(got[0], want[0])
        assert (got[1] is None and want[1] is None) if nearest else (got[1] == want[1]).all()
    for bad in (dict(map1=np.zeros((4, 4), f)), dict(map1=np.zeros((4, 4, 2), np.float64)), dict(map1=np.zeros((4, 4), f), map2=np.zeros((4, 5), f))):
        with pytest.raises(ValueError):
            warp.convert_maps(**bad)


@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_convert_maps_equals_build_where_the_float32_cast_is_exact(interp):
    """lens_ref.chain's (u, v) cast to float32 and converted equal build()'s entries wherever the cast is exact: there float32(u) * 32 is
    exact too (a power of two), so both round the same number."""
    from bev_amd import warp
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    K = LR.camera_K(sw, sh)
    R, lens = LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_B)
    u, v, _ = LR.chain((dw, dh), R, lens)
    # (coordinates on a 1/64-px grid: exact in float32, with ties among them)
    u, v = np.rint(u * 64.0) / 64.0, np.rint(v * 64.0) / 64.0
    assert (u.astype(np.float32) == u).all() and (v.astype(np.float32) == v).all()
    xy, frac = warp.convert_maps(u.astype(np.float32), v.astype(np.float32), nearest=interp == wn.NEAREST)
    scale = 32.0 if interp == wn.LINEAR else 1.0
    X, Y = wn._round_clamped(u * scale), wn._round_clamped(v * scale)
    if interp == wn.NEAREST:
        np.testing.assert_array_equal(xy, np.stack([X, Y], -1).astype(np.int16))
    else:
        np.testing.assert_array_equal(xy, np.stack([X >> 5, Y >> 5], -1).astype(np.int16))
        np.testing.assert_array_equal(frac, (((Y & 31) << 5) | (X & 31)).astype(np.uint16))
    # ... and on the chain's own float64 values the two agree wherever the float32 cast is exact
    u0, v0, _ = LR.chain((dw, dh), R, lens)
    exact = (u0.astype(np.float32) == u0) & (v0.astype(np.float32) == v0)
    bx, bf = RR.build((dw, dh), R, lens, INF, interp)
    cx, cf = warp.convert_maps(u0.astype(np.float32), v0.astype(np.float32), nearest=interp == wn.NEAREST)
    np.testing.assert_array_equal(cx[exact], bx[exact])
    if bf is not None:
        np.testing.assert_array_equal(cf[exact], bf[exact])


# ---- the host checks and the frames-per-item plan under the sanitizers ----

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
CALL = dict(src=16, dst=1 << 20, xy=1 << 24, frac=1 << 26, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, channels=3, src_fs=192, src_rs=24, dst_fs=192, dst_rs=24,
            map_count=1, xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16, dtype=0, interp=1, mode=0)


def _call(**kw):
    a = dict(CALL, **kw)
    return "call " + " ".join(str(a[k]) for k in CALL)


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_call_checks_under_sanitizers(driver):
    big = 2147483647
    ok = [OK, OK, 1, 2]  # (an 8 x 8 destination: 2 tiles)
    cases = [(_call(mode=m, dtype=d, channels=c, interp=i, src_rs=8 * c * e, src_fs=64 * c * e, dst_rs=8 * c * e, dst_fs=64 * c * e), ok)
             for m in range(6) for d, e in ((0, 1), (1, 4)) for c in (1, 2, 3, 4) for i in (0, 1)]
    cases += [(_call(batch=0), [OK, 0, 0, 0])]
    cases += [(_call(mode=m), [UNSUPPORTED, 0, 0, 0]) for m in (6, 16, 16 + 5, -1, 100)]
    cases += [(_call(interp=i), [UNSUPPORTED, 0, 0, 0]) for i in (2, 3, -1)]                # BEVWARP_CUBIC included
    cases += [(_call(interp=2, frac=0), [UNSUPPORTED, 0, 0, 0])]
    cases += [(_call(dtype=d), [UNSUPPORTED, 0, 0, 0]) for d in (2, 3, 4, -1)]             # the 16-bit types included
    cases += [(_call(channels=c), [UNSUPPORTED, 0, 0, 0]) for c in (0, 5)]
    # the map count: 1 or the batch
    three = dict(batch=3, dst=1 << 20)
    cases += [(_call(map_count=0), [BAD_ARG, 0, 0, 0]), (_call(map_count=2), [BAD_ARG, 0, 0, 0]), (_call(map_count=2, **three), [BAD_ARG, 0, 0, 0]),
              (_call(map_count=0, **three), [BAD_ARG, 0, 0, 0]), (_call(map_count=3, **three), [OK, OK, 1, 6]), (_call(map_count=1, **three), [OK, OK, 1, 6]),
              (_call(map_count=3, xy_fs=255, **three), [BAD_ARG, 0, 0, 0]),      # per-frame maps that overlap their successors
              (_call(map_count=3, frac_fs=127, **three), [BAD_ARG, 0, 0, 0]),
              (_call(map_count=1, xy_fs=1, frac_fs=1, **three), [OK, OK, 1, 6])]  # a shared map's frame strides are not looked at
    # NULL planes; frac may be NULL for nearest only
    cases += [(_call(src=0), [BAD_ARG, 0, 0, 0]), (_call(dst=0), [BAD_ARG, 0, 0, 0]), (_call(xy=0), [BAD_ARG, 0, 0, 0]), (_call(frac=0), [BAD_ARG, 0, 0, 0]),
              (_call(frac=0, interp=0), ok), (_call(xy=0, interp=0), [BAD_ARG, 0, 0, 0])]
    # misaligned planes and short rows
    cases += [(_call(xy=(1 << 24) + 2), [BAD_ARG, 0, 0, 0]), (_call(xy_rs=34), [BAD_ARG, 0, 0, 0]), (_call(frac=(1 << 26) + 1), [BAD_ARG, 0, 0, 0]),
              (_call(frac_rs=17), [BAD_ARG, 0, 0, 0]), (_call(xy_rs=28), [BAD_ARG, 0, 0, 0]), (_call(frac_rs=14), [BAD_ARG, 0, 0, 0]),
              (_call(xy=(1 << 24) + 4, frac=(1 << 26) + 2), ok), (_call(map_count=3, xy_fs=258, **three), [BAD_ARG, 0, 0, 0])]
    # the destination against the source and against either map plane
    cases += [(_call(dst=16), [OVERLAP, 0, 0, 0]), (_call(dst=16 + 192), ok),
              (_call(xy=1 << 20), [OVERLAP, 0, 0, 0]), (_call(xy=(1 << 20) + 188), [OVERLAP, 0, 0, 0]), (_call(xy=(1 << 20) + 192), ok),
              (_call(xy=(1 << 20) - 252), [OVERLAP, 0, 0, 0]), (_call(xy=(1 << 20) - 256), ok),
              (_call(frac=(1 << 20) + 190), [OVERLAP, 0, 0, 0]), (_call(frac=(1 << 20) + 192), ok), (_call(frac=(1 << 20) + 100, interp=0), ok),  # (nearest: not read)
              (_call(xy=(1 << 20) + 3 * 192 - 4, **three), [OVERLAP, 0, 0, 0]),                 # a shared map inside the third destination frame
              (_call(xy=16, frac=16 + 64), ok)]                                               # the maps may overlap the source and each other: all are read
    # source sides 32767 / 32768; the maps have no such limit
    cases += [(_call(src_w=32768, src_rs=3 * 32768, src_fs=24 * 32768), [TOO_LARGE, 0, 0, 0]), (_call(src_h=32768, src_fs=24 * 32768), [TOO_LARGE, 0, 0, 0]),
              (_call(src_w=32767, src_rs=3 * 32767, src_fs=24 * 32767, dst=1 << 28), ok), (_call(src_h=32767, src_fs=24 * 32767, dst=1 << 28), ok)]
    # destination sides around 2^20 and 2^31: the checks pass, the plan refuses
    one = dict(channels=1, src_rs=8, src_fs=64, dst=1 << 40, xy=1 << 44, frac=1 << 48)
    w20 = 1 << 20
    cases += [(_call(dst_w=w20, dst_h=1, dst_rs=w20, dst_fs=w20, xy_rs=4 * w20, frac_rs=2 * w20, **one), [OK, OK, 1, 4096]),
              (_call(dst_w=w20 + 1, dst_h=1, dst_rs=2 * w20, dst_fs=2 * w20, xy_rs=8 * w20, frac_rs=4 * w20, **one), [OK, TOO_LARGE, 0, 0]),
              (_call(dst_w=8, dst_h=w20 + 1, dst_rs=8, dst_fs=1 << 24, **one), [OK, TOO_LARGE, 0, 0]),
              (_call(dst_w=8, dst_h=w20, dst_rs=8, dst_fs=1 << 24, **one), [OK, OK, 1, w20 // 4]),
              (_call(dst_w=big, dst_h=1, dst_rs=big, dst_fs=big, xy_rs=4 * big, frac_rs=2 * big, **one), [OK, TOO_LARGE, 0, 0]),
              (_call(batch=big, map_count=big, xy_fs=256, frac_fs=128, dst_rs=8, dst_fs=64, **one), [OK, TOO_LARGE, 0, 0]),  # 2 tiles per frame: past 2^31 - 1 items
              (_call(batch=big, map_count=1, dst_rs=8, dst_fs=64, **one), [OK, OK, 8, 2 * ((big + 7) // 8)])]                # ... which groups of 8 frames bring back in range
    # strides next to 2^63: bad arguments, not overflows
    huge = (1 << 63) - 1
    # (one row, or two frames: the images' last bytes stay below 2^64 and the answers are determinate)
    cases += [(_call(dst_h=1, xy_rs=huge - 3, frac_rs=huge - 1, dst_rs=huge), [OK, OK, 1, 1]),
              (_call(batch=2, map_count=2, dst_h=1, xy_fs=huge - 3, frac_fs=huge - 1), [OK, OK, 1, 2]),
              (_call(batch=2, map_count=2, xy_rs=huge - 3, xy_fs=huge - 3), [BAD_ARG, 0, 0, 0]), (_call(batch=2, map_count=2, frac_rs=huge - 1, frac_fs=huge - 1), [BAD_ARG, 0, 0, 0]),
              (_call(batch=3, dst_rs=huge, dst_fs=huge), [BAD_ARG, 0, 0, 0]), (_call(src_rs=huge), [TOO_LARGE, 0, 0, 0])]
    hostplan.check_cases(driver, cases, "remap")


def test_frames_per_item_plan_under_sanitizers(driver):
    """The grid covers every (frame, tile) exactly once, whatever the plan chose; a shared map gets the largest power of two that leaves
    `fill` items, per-frame maps one frame per item; the benchmark shape takes 8 frames per item and still has 4096 items."""
    lines, want = [], []
    for batch in (1, 2, 7, 33):
        for shared in (True, False):
            for dst_h, dst_w in ((20, 36), (5, 515), (1, 1)):
                for max_fpi, fill in ((8, 1), (8, 4096), (1, 1), (4, 12)):
                    lines.append("plan %d %d %d %d %d %d" % (batch, 1 if shared else batch, dst_h, dst_w, max_fpi, fill))
                    tiles = -(-dst_w // 256) * -(-dst_h // 4)
                    fpi = 1
                    while shared and batch > 1 and fpi * 2 <= max_fpi and fpi * 2 <= batch and -(-batch // (fpi * 2)) * tiles >= fill:
                        fpi *= 2
                    groups = -(-batch // fpi)
                    want.append([OK, fpi, groups, groups * tiles, 1])
    # (the launches of tests/test_gpu_remap.py::test_frame_loop_groups_of_frames: 2 and 8 frames per item, a short last group; and 4)
    lines += ["plan 33 1 256 1024 8 4096", "plan 33 1 1024 1024 8 4096", "plan 7 1 1024 1024 8 4096", "plan 33 1 257 515 8 1024"]
    want += [[OK, 2, 17, 17 * 256, 1], [OK, 8, 5, 5 * 1024, 1], [OK, 2, 4, 4 * 1024, 1], [OK, 4, 9, 9 * 195, 1]]
    lines += ["plan 32 1 1024 1024 8 4096", "plan 32 32 1024 1024 8 4096", "plan 32 1 1024 1024 1 4096", "plan 1 1 1024 1024 8 4096",
              "plan 2147483647 2147483647 8 8 8 4096", "plan 2147483647 1 8 8 8 4096", "plan 2 1 1048577 8 8 1"]
    want += [[OK, 8, 4, 4096, 1], [OK, 1, 32, 32768, 1], [OK, 1, 32, 32768, 1], [OK, 1, 1, 1024, 1], [TOO_LARGE, 0, 0, 0, 0], [OK, 8, 268435456, 536870912, 0],
             [TOO_LARGE, 0, 0, 0, 0]]
    got = hostplan.run_driver(driver, lines, "remap")
    for ln, w, g in zip(lines, want, got):
        assert g == w, (ln, g, w)
        assert g[3] <= 2147483647


def test_build_map_status_under_sanitizers(driver):
    B = dict(m_null=0, m_count=1, lens=0, r2_max="1.5", interp=1, xy=1 << 24, frac=1 << 26, dst_h=8, dst_w=8, xy_fs=256, xy_rs=32, frac_fs=128, frac_rs=16)

    def line(**kw):
        a = dict(B, **kw)
        return "build " + " ".join(str(a[k]) for k in B)

    w20 = 1 << 20
    cases = [(line(), [OK, 2]), (line(interp=0), [OK, 2]), (line(interp=0, frac=0), [OK, 2]), (line(lens=1), [OK, 2]), (line(lens=1, r2_max="inf"), [OK, 2]),
             (line(m_count=3), [OK, 6]), (line(m_count=1, xy_fs=1, frac_fs=1), [OK, 2]),
             (line(m_null=1), [BAD_ARG, 0]), (line(xy=0), [BAD_ARG, 0]), (line(frac=0), [BAD_ARG, 0]), (line(m_count=0), [BAD_ARG, 0]), (line(m_count=-1), [BAD_ARG, 0]),
             (line(dst_h=0), [BAD_ARG, 0]), (line(dst_w=-1), [BAD_ARG, 0]),
             (line(interp=2), [UNSUPPORTED, 0]), (line(interp=2, frac=0), [UNSUPPORTED, 0]), (line(interp=-1), [UNSUPPORTED, 0]),
             (line(xy=(1 << 24) + 2), [BAD_ARG, 0]), (line(frac=(1 << 26) + 1), [BAD_ARG, 0]), (line(xy_rs=30), [BAD_ARG, 0]), (line(xy_rs=28), [BAD_ARG, 0]),
             (line(frac_rs=15), [BAD_ARG, 0]), (line(frac_rs=14), [BAD_ARG, 0]), (line(m_count=3, xy_fs=252), [BAD_ARG, 0]), (line(m_count=3, frac_fs=126), [BAD_ARG, 0]),
             (line(frac=(1 << 26) + 1, interp=0), [OK, 2]),                         # (nearest: the frac plane is not looked at)
             (line(dst_w=w20, dst_h=1, xy_rs=4 * w20, frac_rs=2 * w20), [OK, 4096]), (line(dst_w=w20 + 1, dst_h=1, xy_rs=8 * w20, frac_rs=4 * w20), [TOO_LARGE, 0]),
             (line(dst_h=w20 + 1), [TOO_LARGE, 0]), (line(m_count=2147483647, xy=1 << 44, frac=1 << 20), [TOO_LARGE, 0]),
             (line(frac=(1 << 24) + 128), [OVERLAP, 0]), (line(frac=(1 << 24) + 256), [OK, 2]), (line(frac=(1 << 24) - 126), [OVERLAP, 0]), (line(frac=(1 << 24) - 128), [OK, 2]),
             (line(frac=(1 << 24) + 128, interp=0), [OK, 2]),
             (line(lens=2), [NOT_FINITE, 0]), (line(lens=1, r2_max="-1"), [BAD_ARG, 0]), (line(lens=1, r2_max="nan"), [BAD_ARG, 0]), (line(lens=0, r2_max="nan"), [OK, 2])]
    hostplan.check_cases(driver, cases, "remap")


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_map_kernels_code_object(tmp_path):
    found = codeobj.kernels("warp_map.hip", tmp_path, "warp_map.h")
    remap = {n: k for n, k in found.items() if "remap_kernel" in n}
    build = {n: k for n, k in found.items() if "build_map_kernel" in n}
    assert len(remap) == 2 * 4 * 2 * 6, len(remap)  # dtype x channels x interpolation x border
    assert len(build) == 2 * 2, len(build)          # interpolation x (pinhole, lens)
    assert len(found) == len(remap) + len(build)
    codeobj.assert_lean(found)
    codeobj.makefile_flags("warp_lens.hip", "lens_pixel.h")  # (the shared lens step rebuilds both of its users)
    for unit in ("warp_map.hip", "warp_stitch_maps.hip"):  # (so do the shared tap loads)
        codeobj.makefile_flags(unit, "tap_load.h")


# ---- the ABI surface, without a device (fake pointers, never dereferenced: every call below fails validation first) ----

def test_abi_surface():
    lib = hostplan.built_lib()
    assert "bevwarp_remap" in _lib.SYMBOLS and "bevwarp_build_map" in _lib.SYMBOLS and lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    assert len(_lib.SYMBOLS["bevwarp_remap"][1]) == 24 and len(_lib.SYMBOLS["bevwarp_build_map"][1]) == 14
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "int bevwarp_remap(const void *src, void *dst, int batch," in header and "int bevwarp_build_map(const double *M, int m_count," in header
    table = header.split("Conventions")[0]
    assert "bevwarp_build_map, bevwarp_remap" in table
    for cite in ("vis_homo.py:85-91", "bev/calib.py:25"):
        assert cite in table.split("bevwarp_build_map, bevwarp_remap")[1].split("bevwarp_warp_stitch")[0], cite
    assert "(-32768, -32768)" in header and "CV_16SC2" in header and "CV_16UC1" in header
    one, far, mxy, mfr = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p(1 << 26)
    nan_border = ctypes.cast((ctypes.c_double * 3)(0.0, float("nan"), 0.0), ctypes.c_void_p)

    def call(src=one, dst=far, batch=1, xy=mxy, frac=mfr, map_count=1, xy_rs=32, frac_rs=16, dtype=_lib.U8, interp=1, mode=0, bv=None):
        return lib.bevwarp_remap(src, dst, batch, 8, 8, 8, 8, 3, 192, 24, 192, 24, xy, frac, map_count, 256, xy_rs, 128, frac_rs, dtype, interp, mode, bv, None)

    assert call(batch=0) == OK  # nothing to do: no launch
    assert call(bv=nan_border) == NOT_FINITE                       # every check passed: the border value is looked at last
    assert call(mode=6) == UNSUPPORTED and call(interp=2) == UNSUPPORTED and call(dtype=_lib.F16) == UNSUPPORTED and call(dtype=_lib.BF16) == UNSUPPORTED
    assert call(src=None) == BAD_ARG and call(xy=None) == BAD_ARG and call(frac=None) == BAD_ARG and call(frac=None, interp=0, bv=nan_border) == NOT_FINITE
    assert call(map_count=0) == BAD_ARG and call(map_count=2) == BAD_ARG and call(batch=3, map_count=2) == BAD_ARG
    assert call(xy=ctypes.c_void_p((1 << 24) + 2)) == BAD_ARG and call(frac=ctypes.c_void_p((1 << 26) + 1)) == BAD_ARG and call(xy_rs=28) == BAD_ARG
    assert call(xy=far) == OVERLAP and call(frac=ctypes.c_void_p((1 << 20) + 100)) == OVERLAP and call(dst=one) == OVERLAP

    lens = (ctypes.c_double * 12)(800.0, 810.0, 319.5, 239.5, -0.3, 0.1, 0.001, -0.0005, -0.01, 0, 0, 0)
    nan_lens = (ctypes.c_double * 12)(800.0, 810.0, 319.5, 239.5, float("nan"), 0, 0, 0, 0, 0, 0, 0)

    def build(M=one, m_count=1, lens=None, r2_max=1.0, interp=1, xy=mxy, frac=mfr, dst_h=8, xy_rs=32):
        return lib.bevwarp_build_map(M, m_count, lens, r2_max, interp, xy, frac, dst_h, 8, 256, xy_rs, 128, 16, None)

    assert build(M=None) == BAD_ARG and build(xy=None) == BAD_ARG and build(frac=None) == BAD_ARG and build(m_count=0) == BAD_ARG and build(dst_h=0) == BAD_ARG
    assert build(interp=2) == UNSUPPORTED and build(xy_rs=30) == BAD_ARG and build(dst_h=(1 << 20) + 1) == TOO_LARGE
    assert build(frac=ctypes.c_void_p((1 << 24) + 64)) == OVERLAP
    assert build(lens=nan_lens) == NOT_FINITE and build(lens=lens, r2_max=-1.0) == BAD_ARG and build(lens=lens, r2_max=float("nan")) == BAD_ARG


# ---- the Python entries ----

def test_bev_warp_reexports_the_new_names():
    import bev.cv2_compat as bev_cv2
    import bev.warp as bev_warp
    from bev_amd import cv2_compat, warp
    assert bev_warp.remap is warp.remap and bev_warp.build_warp_map is warp.build_warp_map and bev_warp.WarpMap is warp.WarpMap
    assert bev_warp.convert_maps is warp.convert_maps
    assert bev_cv2.remap is cv2_compat.remap and bev_cv2.convertMaps is cv2_compat.convertMaps


def _cpu_map(n=1, dh=6, dw=5, interp=1):
    from bev_amd import warp
    return warp.WarpMap(torch.zeros((n, dh, dw, 2), dtype=torch.int16), torch.zeros((n, dh, dw), dtype=torch.int16) if interp else None, interp, (dw, dh))


def test_python_entries_validate_before_the_device():
    from bev_amd import cv2_compat, warp
    from bev_amd.pipeline import FramePipeline
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)  # (CPU tensors: a call that passed these checks would be refused for its device next)
    with pytest.raises(ValueError, match="holds 3 frames for a batch of 2"):
        warp.remap(src, _cpu_map(n=3))
    with pytest.raises(ValueError, match="dsize is"):
        warp.remap(src, _cpu_map(), out=torch.zeros((2, 7, 5, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="dsize is"):
        warp.remap(src, _cpu_map(), out=torch.zeros((2 * 6 * 5 * 3 + 1,), dtype=torch.uint8))
    with pytest.raises(ValueError, match="the map is on"):
        warp.remap(src, warp.WarpMap(torch.zeros((1, 6, 5, 2), dtype=torch.int16, device="meta"), torch.zeros((1, 6, 5), dtype=torch.int16, device="meta"), 1, (5, 6)))
    with pytest.raises(ValueError, match="needs a WarpMap"):
        warp.remap(src, (torch.zeros((1, 6, 5, 2), dtype=torch.int16), None))
    with pytest.raises(ValueError, match="border mode"):
        warp.remap(src, _cpu_map(), border_mode=6)
    with pytest.raises(ValueError, match="uint8 or float32"):
        warp.remap(src.to(torch.int32), _cpu_map())
    with pytest.raises(ValueError, match="CUDA"):
        warp.remap(src, _cpu_map())  # everything else is in order: no CUDA tensor
    # WarpMap itself
    for bad in (dict(xy=torch.zeros((1, 6, 5, 2), dtype=torch.int32)), dict(xy=torch.zeros((1, 6, 4, 2), dtype=torch.int16)), dict(frac=None),
                dict(frac=torch.zeros((2, 6, 5), dtype=torch.int16)), dict(frac=torch.zeros((1, 6, 5), dtype=torch.uint8)), dict(interp=2),
                dict(xy=torch.zeros((1, 6, 5, 4), dtype=torch.int16)[..., ::2])):
        a = dict(xy=torch.zeros((1, 6, 5, 2), dtype=torch.int16), frac=torch.zeros((1, 6, 5), dtype=torch.int16), interp=1, dsize=(5, 6))
        a.update(bad)
        with pytest.raises(ValueError):
            warp.WarpMap(**a)
    assert warp.WarpMap(torch.zeros((1, 6, 5, 2), dtype=torch.int16), None, 0, (5, 6)).frac is None
    # build_warp_map
    K = LR.camera_K(8, 8)
    with pytest.raises(ValueError):
        warp.build_warp_map(np.eye(3), (8, 8), flags=warp.INTER_CUBIC)
    with pytest.raises(ValueError):
        warp.build_warp_map(np.eye(3), (0, 8))
    with pytest.raises(ValueError):
        warp.build_warp_map(np.eye(4), (8, 8))
    with pytest.raises(ValueError):
        warp.build_warp_map(np.eye(3), (8, 8), K=K, dist_coeff=[0.1, 0.2])
    with pytest.raises(ValueError, match="needs the camera matrix"):
        warp.build_warp_map(np.eye(3), (8, 8), dist_coeff=LR.LENS_A)
    with pytest.raises(ValueError, match="out must be a WarpMap"):
        warp.build_warp_map(np.eye(3), (8, 8), out=_cpu_map())  # another dsize
    with pytest.raises(ValueError, match="CUDA"):
        warp.build_warp_map(np.eye(3), (8, 8), device="cpu")
    # cv2_compat.remap: numpy in; the maps are judged before anything is uploaded
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        cv2_compat.remap(img, np.zeros((6, 5, 2), np.int16), None, cv2_compat.INTER_LINEAR)      # no frac plane for bilinear
    with pytest.raises(ValueError):
        cv2_compat.remap(img, np.zeros((6, 5, 2), np.int16), np.zeros((6, 4), np.uint16), cv2_compat.INTER_LINEAR)
    with pytest.raises(ValueError):
        cv2_compat.remap(img, np.zeros((6, 5), np.float64), np.zeros((6, 5), np.float64), cv2_compat.INTER_LINEAR)
    with pytest.raises(ValueError):
        cv2_compat.remap(img, np.zeros((6, 5), np.float32), np.zeros((6, 5), np.float32), cv2_compat.INTER_CUBIC)
    with pytest.raises(ValueError):
        cv2_compat.remap(img.astype(np.int16), np.zeros((6, 5), np.float32), np.zeros((6, 5), np.float32), cv2_compat.INTER_LINEAR)
    # FramePipeline(warp_map=...): interleaved frames in and out only; the map is one camera's
    for kw in (dict(planar=True), dict(src_format="nv12"), dict(dst_format="nv12")):
        with pytest.raises(ValueError, match="warp_map"):
            FramePipeline((8, 8), 3, None, (5, 6), warp_map=_cpu_map(), **kw)
    with pytest.raises(ValueError, match="warp_map"):
        FramePipeline((8, 8), 3, None, (5, 6), warp_map=_cpu_map(n=2))
    with pytest.raises(ValueError, match="warp_map"):
        FramePipeline((8, 8), 3, None, (7, 6), warp_map=_cpu_map())
    with pytest.raises(ValueError, match="warp_map"):
        FramePipeline((8, 8), 3, None, (5, 6), warp_map="map")
