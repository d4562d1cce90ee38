"""CPU companion of tests/test_gpu_limits.py: the expected values of the limit tests are only as good as the oracle at those shapes, so on
the compact copies of the widest, tallest and widest-stride sources (tests/limits_cases.py) the C oracle must equal its numpy restatement,
the border reference its C twin (the constant border; the other modes and the bicubic reference have no C twin of their warps -- the bicubic
tables' twin is tests/test_cubic_cpu.py's), and the maps must reach what the cases promise.  Also on the CPU: every layout the GPU module
builds lies inside its backing buffer, the ABI admits exactly the sizes the cases claim, and the fast tiles' 24-bit tap address equals the
plain product at the admitted extremes."""
import numpy as np
import pytest

from bev_amd import _lib
from oracle import cpu_oracle as co
from oracle import warp_numpy as wn
from oracle.warp_numpy import fixed_point_maps
from tests import border_ref as br
from tests import cubic_ref as cr
from tests import hostplan
from tests import lens_ref as LR
from tests import limits_cases as lc
from tests import nv12_ref as NR
from tests import remap_nv12_ref as RN
from tests import remap_ref as RR
from tests import stitch_maps_ref as SM
from tests import stitch_ref as SR

CASES = [(name, hw, dsize, key, Minv) for name, hw, dsize, maps in lc.compact_cases() for key, Minv in sorted(maps.items())]
IDS = ["%s-%s" % (c[0], c[3]) for c in CASES]


@pytest.mark.parametrize("dtype,c", [(np.uint8, 1), (np.uint8, 3), (np.uint8, 4), (np.float32, 1), (np.float32, 4)], ids=lambda v: getattr(v, "__name__", str(v)))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_its_numpy_restatement(case, dtype, c):
    _, (h, w), dsize, _, Minv = case
    src = lc.pixels(1, h, w, c, dtype)
    for interp in (co.NEAREST, co.LINEAR):
        exp = wn.warp_perspective(src, Minv, dsize, interp, m_is_inverse=True, border_value=lc.BORDER[:c])
        got = co.warp_perspective(src, Minv, dsize, interp, m_is_inverse=True, border_value=lc.BORDER[:c])
        np.testing.assert_array_equal(got.view(np.uint32) if dtype == np.float32 else got, exp.view(np.uint32) if dtype == np.float32 else exp)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_border_reference_equals_its_c_twin_and_the_bicubic_one_agrees_on_integer_maps(case):
    """border_ref's CONSTANT is the oracle's warp (its C twin).  cubic_ref has no C twin of its warp: on these shapes it is held to the
    property that pins its indexing -- at integer coordinates (fx = fy = 0) the bicubic weights are (0, 1, 0, 0), so the warp through the
    case's map rounded to integers is the nearest-neighbour warp of the oracle."""
    _, (h, w), dsize, _, Minv = case
    for dtype, c in ((np.uint8, 3), (np.float32, 1)):
        src = lc.pixels(2, h, w, c, dtype)
        for interp in (br.NEAREST, br.LINEAR):
            got = br.warp(src, Minv, dsize, interp, br.CONSTANT, m_is_inverse=True, border_value=lc.BORDER[:c])
            np.testing.assert_array_equal(got, co.warp_perspective(src, Minv, dsize, interp, m_is_inverse=True, border_value=lc.BORDER[:c]))
    Mi = np.rint(Minv)
    src = lc.pixels(3, h, w, 3, np.uint8)
    inl, _, _, _ = cr.classes((h, w), Mi, dsize, m_is_inverse=True)
    got = cr.warp(src, Mi, dsize, br.REPLICATE, m_is_inverse=True)
    near = br.warp(src, Mi, dsize, br.NEAREST, br.REPLICATE, m_is_inverse=True)
    np.testing.assert_array_equal(got, near)
    assert inl.any() and not inl.all()


def test_maps_reach_what_the_cases_promise():
    """From the oracle's maps: in-frame and border pixels, the last column (row) with two valid taps and the first saturated one."""
    for name, (h, w), dsize, maps in lc.compact_cases()[:2]:
        for key, Minv in maps.items():
            for interp in (co.NEAREST, co.LINEAR):
                sxy, _ = co.warp_maps(dsize, Minv, interp)
                s = sxy[..., 0] if name == "wide" else sxy[..., 1]
                assert (s == lc.MAX_SIDE - 2).any() and (s == 32767).any(), (name, key, interp)
                assert ((sxy[..., 0] >= 0) & (sxy[..., 0] < w - 1) & (sxy[..., 1] >= 0) & (sxy[..., 1] < h - 1)).any()
    rows = lc.max_rows(lc.STRIDE_ALIGNED)
    sxy, _ = co.warp_maps(lc.STRIDE_DSIZE, lc.stride_map(rows), co.LINEAR)
    assert sxy[0, 0, 1] == 0 and sxy[-1, 0, 1] == rows - 1           # first and last source row
    assert rows - 20 <= sxy[56, 0, 1] and sxy[59, 0, 1] + 1 <= rows - 4  # the tile of rows 56 .. 59: inside the frame, within its last 20 rows


def test_every_layout_lies_inside_its_backing_buffer():
    """The largest byte offset each kernel forms from its arguments -- source (h - 1) rs + row bytes with the frame term, the destination's
    last store with the frame and plane terms -- against the bytes the GPU module allocates for the view (extent_bytes)."""
    for dtype, c, rs in lc.STRIDE_FORMATS:
        esz, rows = np.dtype(dtype).itemsize, lc.max_rows(rs)
        assert rows * rs < lc.FRAME_LIMIT <= (rows + 1) * rs and rs < lc.ROW_LIMIT and rs % esz == 0
        assert lc.source_reach(rows, lc.STRIDE_W, c, esz, rs) == lc.extent_bytes((rows, lc.STRIDE_W, c), (rs, c * esz, esz), esz) < lc.FRAME_LIMIT
    h, w = lc.BIG_SRC_HW
    dw, dh = lc.BIG_DSIZE
    for esz in (1, 4):
        c, fs = 3, lc.BEYOND_4G
        assert lc.source_reach(h, w, c, esz, w * c * esz, lc.BIG_BATCH, fs) == lc.extent_bytes((lc.BIG_BATCH, h, w, c), (fs, w * c * esz, c * esz, esz), esz)
        assert lc.dest_reach(dh, dw, c, esz, dw * c * esz, lc.BIG_BATCH, fs) == lc.extent_bytes((lc.BIG_BATCH, dh, dw, c), (fs, dw * c * esz, c * esz, esz), esz)
        assert fs % 16 == 0 and 2 * fs > 1 << 33
        rows = lc.ROWS_PAST_4G5
        assert (rows - 1) * lc.ROW_64M > 4.5 * (1 << 30) >= (rows - 2) * lc.ROW_64M
        assert lc.dest_reach(rows, dw, c, esz, lc.ROW_64M) == lc.extent_bytes((rows, dw, c), (lc.ROW_64M, c * esz, esz), esz) < 6 * (1 << 30)
    assert lc.dest_reach(dh, dw, 2, 4, dw * 4, planes=2, ps=lc.BEYOND_4G) == lc.extent_bytes((2, dh, dw), (lc.BEYOND_4G, dw * 4, 4), 4)
    assert lc.dest_reach(lc.ROWS_PAST_4G5, dw, 1, 4, lc.ROW_64M, planes=1) == lc.extent_bytes((1, lc.ROWS_PAST_4G5, dw), (0, lc.ROW_64M, 4), 4)


def test_fast_tile_tap_address_equals_the_plain_product_at_the_limits():
    """rows_coords.inc / rows_run.inc: S0 = umul24(hy, rs) + umul24(hx, PBs) + kOff with hy = kHiBias + sy, hx = kHiBias + sx and
    kOff = fa - 0x380000 (rs + PBs), all modulo 2^32, must be sy rs + sx PBs + fa for every source the host admits -- and the second tap
    row's S0 + rs must not wrap either.  Restated in integers at the extremes of cases A to C and at the limits' corners."""
    k_hi_bias = 0x43380000

    def umul24(a, b):
        return ((a & 0xffffff) * (b & 0xffffff)) & 0xffffffff

    def s0(sy, sx, rs, pbs, fa):
        k_off = (fa - 0x380000 * ((rs + pbs) & 0xffffffff)) & 0xffffffff
        return (umul24(k_hi_bias + sy, rs) + ((umul24(k_hi_bias + sx, pbs) + k_off) & 0xffffffff)) & 0xffffffff

    assert (k_hi_bias & 0xffffff) == 0x380000 and 0x380000 + lc.MAX_SIDE < 1 << 24  # a 15-bit index never carries out of the low 24 bits
    shapes = [(40, lc.MAX_SIDE, lc.MAX_SIDE * pbs, pbs) for pbs in (1, 3, 4, 16)] + [(lc.MAX_SIDE, 40, 40 * pbs, pbs) for pbs in (1, 3, 4, 16)]
    shapes += [(lc.max_rows(rs), lc.STRIDE_W, rs, np.dtype(dt).itemsize * c) for dt, c, rs in lc.STRIDE_FORMATS]
    shapes += [(lc.MAX_SIDE, 4095, 65535, 16), (lc.MAX_SIDE, 16383, 65537, 4), (127, 32, lc.ROW_LIMIT - 1, 16)]
    for h, w, rs, pbs in shapes:
        assert h * rs < lc.FRAME_LIMIT and rs < lc.ROW_LIMIT and w * pbs <= rs
        for fa in (0, 1, 3):
            for sy in (0, 1, h - 2, h - 1):
                for sx in (0, 1, w - 2, w - 1):
                    exact = sy * rs + sx * pbs + fa
                    assert s0(sy, sx, rs, pbs, fa) == exact and (s0(sy, sx, rs, pbs, fa) + rs) & 0xffffffff == exact + rs, (h, w, rs, pbs, fa, sy, sx)


def test_abi_admits_the_limits_and_refuses_one_past_them():
    """Sizes only (bevwarp_tile_classes_bytes takes no pointer): the sides of cases A and B and the destination of case F are admitted."""
    lib = _lib.load()
    for dtype in (_lib.U8, _lib.F32):
        assert lib.bevwarp_tile_classes_bytes(1, 40, lc.MAX_SIDE, 40, 600, 4, dtype, 1) > 0
        assert lib.bevwarp_tile_classes_bytes(1, lc.MAX_SIDE, 40, 600, 40, 4, dtype, 1) > 0
        assert lib.bevwarp_tile_classes_bytes(1, 40, lc.MAX_SIDE + 1, 40, 600, 1, dtype, 1) == -3
        assert lib.bevwarp_tile_classes_bytes(1, lc.MAX_SIDE + 1, 40, 600, 40, 1, dtype, 1) == -3


def test_decode_case_straddles_the_exactness_bound():
    """Case F's numbers: with d tiles per frame, 3 frames keep the multiply-high exact (and get a magic from the host's rule), 4 do not --
    and for 4 the multiply-high really is wrong somewhere, so a kernel without the fallback would be caught."""
    d = lc.DECODE_TILES
    lo, hi = (b * d for b in lc.DECODE_BATCHES)
    assert -(-lo // 8) * 8 * d < 1 << 32 <= hi * d  # (the row kernel rounds its item count up to a multiple of 8)
    assert (1 << 32) - -(-lo // 8) * 8 * d < (1 << 32) // 100
    assert lc.multiply_high_is_exact(lo, d) and not lc.multiply_high_is_exact(hi, d)
    assert d * 24 <= 1 << 20 and d * 4 <= 1 << 20  # the destination heights that give d tiles (24-row tiles of the 8-bit kernel, 4-row border tiles)


# ---- the companions of tests/test_gpu_limits_entries.py: the lens, NV12, map and stitch entries on the same shapes ---------------------------
ENTRY_CASES = [(name, key) for name in ("wide", "tall") for key in sorted(lc.WIDE_ENTRY_MAPS)]
ENTRY_IDS = ["%s-%s" % c for c in ENTRY_CASES]
WRITING_MODES = (RR.CONSTANT, RR.REPLICATE, RR.REFLECT, RR.WRAP, RR.REFLECT_101)


def lens_chain(name, key):
    """(ray matrix, the lens' 12 values, r2_max) of a lens run of case A / B."""
    hw = lc.entry_case(name)[0]
    K, dist, r2_max = lc.mild_lens(hw, key)
    Minv = (lc.WIDE_LENS_MAPS if name == "wide" else lc.TALL_LENS_MAPS)[key]
    return LR.ray_matrix(Minv, K, inverse_given=True), LR.lens12(K, dist), r2_max


def test_entry_maps_reach_what_the_cases_promise():
    """On the long axis, from the references' own coordinates: the last index with two valid taps (side - 2), for `right_end` the last
    column too, the saturated 32767, and for `left_end` pixels before the frame down to -1 (one valid tap); with the lens, among the valid
    pixels, and both valid pixels and pixels beyond r2_max occur."""
    for name in ("wide", "tall"):
        for nv12 in (False, True):
            (h, w), dsize, maps, axis = lc.entry_case(name, nv12)
            side = (w, h)[axis]
            assert side == (lc.MAX_EVEN if nv12 else lc.MAX_SIDE) and set(maps) == {"right_end", "minify64", "left_end"}
            for key, Minv in maps.items():
                for interp in (co.NEAREST, co.LINEAR):
                    s = fixed_point_maps(dsize, Minv, interp)[axis]
                    what = (name, nv12, key, interp)
                    if key == "left_end":
                        assert (s == -1).any() and (s < -1).any() and (s == 0).any() and s.max() < side - 2, what
                    else:
                        assert (s == side - 2).any() and (s == 32767).any() and s.min() >= 0, what
                        assert (s == side - 1).any() == (key == "right_end"), what
        (h, w), dsize, _, axis = lc.entry_case(name)
        side = (w, h)[axis]
        assert set(lc.WIDE_LENS_MAPS) == set(lc.TALL_LENS_MAPS) == set(lc.WIDE_ENTRY_MAPS)  # every map runs through the lens as well
        for interp in (co.NEAREST, co.LINEAR):
            for key in ("right_end", "minify64"):
                R, lens, r2_max = lens_chain(name, key)
                m = LR.maps(dsize, R, lens, r2_max, interp)
                s, valid = m[axis][m[4]], m[4]
                assert valid.any() and (~valid).any() and (s == side - 2).any() and (s == 32767).any() and s.min() >= 0, (name, key, interp)
                assert (s == side - 1).any() == (key == "right_end"), (name, key, interp)
            R, lens, r2_max = lens_chain(name, "left_end")
            m = LR.maps(dsize, R, lens, r2_max, interp)
            s = m[axis][m[4]]
            assert (s == -1).any() and (s < -1).any() and (s == 0).any(), (name, interp)
    # case C's NV12 frame: the first and the last row of both planes
    y_rows, uv_rows = lc.STRIDE_NV12["y"][1], lc.STRIDE_NV12["uv"][1]
    assert y_rows == 2 * uv_rows == lc.max_rows(lc.STRIDE_NV12["y"][0])
    sy = fixed_point_maps(lc.STRIDE_DSIZE, lc.stride_map(y_rows), co.LINEAR)[1]
    assert sy[0, 0] == 0 and sy[-1, 0] == y_rows - 1
    # the stitch: all three cameras cover a common part of the canvas, and each has pixels it does not cover
    for nv12 in (False, True):
        covers = [br.inliers(*fixed_point_maps(lc.STITCH_DSIZE, M, co.LINEAR)[:2], hw[1], hw[0], co.LINEAR) for hw, M in lc.stitch_cameras(nv12)]
        assert np.logical_and.reduce(covers).sum() > 1000 and all(not c.all() for c in covers)


@pytest.mark.parametrize("case", ENTRY_CASES, ids=ENTRY_IDS)
def test_map_reference_equals_the_border_and_the_lens_reference(case):
    """remap_ref.remap through remap_ref.build is border_ref.warp in the five modes that write every pixel, and lens_ref.warp for CONSTANT
    and TRANSPARENT, bit for bit on cases A and B: the expected values of the map entries are as good as those of the entries they stand
    in for."""
    name, key = case
    (h, w), dsize, maps, _ = lc.entry_case(name)
    for dtype, c in ((np.uint8, 3), (np.float32, 1)):
        src = lc.pixels(4, h, w, c, dtype)
        for interp in (co.NEAREST, co.LINEAR):
            xy, frac = RR.build(dsize, maps[key], interp=interp)
            for mode in WRITING_MODES:
                got = RR.remap(src, xy, frac, interp, mode, border_value=lc.BORDER[:c])
                exp = br.warp(src, maps[key], dsize, interp, mode, m_is_inverse=True, border_value=lc.BORDER[:c])
                np.testing.assert_array_equal(got.view(np.uint32) if dtype == np.float32 else got, exp.view(np.uint32) if dtype == np.float32 else exp)
            R, lens, r2_max = lens_chain(name, key)
            xy, frac = RR.build(dsize, R, lens, r2_max, interp)
            canvas = lc.pixels(5, dsize[1], dsize[0], c, dtype)
            for mode in (RR.CONSTANT, RR.TRANSPARENT):
                got = RR.remap(src, xy, frac, interp, mode, border_value=lc.BORDER[:c], canvas=canvas)
                exp = LR.warp(src, R, lens, r2_max, dsize, interp, mode, border_value=lc.BORDER[:c], canvas=canvas)
                np.testing.assert_array_equal(got.view(np.uint32) if dtype == np.float32 else got, exp.view(np.uint32) if dtype == np.float32 else exp)


@pytest.mark.parametrize("case", ENTRY_CASES, ids=ENTRY_IDS)
def test_nv12_map_reference_equals_the_nv12_warp_reference(case):
    name, key = case
    (h, w), dsize, maps, _ = lc.entry_case(name, nv12=True)
    y, uv = NR.frame("phase", 6, h, w)
    for interp in (co.NEAREST, co.LINEAR):
        xy, frac = RR.build(dsize, maps[key], interp=interp)
        np.testing.assert_array_equal(RN.remap_nv12(y, uv, xy, frac, interp, RR.CONSTANT, lc.BORDER[:3]),
                                      NR.warp_nv12(y, uv, maps[key], dsize, interp, border_value=lc.BORDER[:3], m_is_inverse=True))


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.float32, 1)], ids=["uint8x3", "float32x1"])
def test_stitch_through_pinhole_maps_equals_the_stitch_reference(dtype, c):
    cams = lc.stitch_cameras()
    srcs = [lc.pixels(7 + i, h, w, c, dtype) for i, ((h, w), _) in enumerate(cams)]
    Minvs = [M for _, M in cams]
    for interp in (co.NEAREST, co.LINEAR):
        maps = [RR.build(lc.STITCH_DSIZE, M, interp=interp) for M in Minvs]
        for blend in (SR.OVER, SR.FEATHER):
            got, n_got = SM.stitch(srcs, maps, interp, blend, 64, SM.CONSTANT, lc.BORDER[:c])
            exp, n_exp = SR.stitch(srcs, Minvs, lc.STITCH_DSIZE, interp, blend, 64, SR.CONSTANT, lc.BORDER[:c])
            np.testing.assert_array_equal(got.view(np.uint32) if dtype == np.float32 else got, exp.view(np.uint32) if dtype == np.float32 else exp)
            np.testing.assert_array_equal(n_got, n_exp)
            assert (n_exp == 3).any() and (n_exp == 0).any()


def _disjoint(rows_a, rows_b):
    ivs = sorted(rows_a + rows_b)
    return all(a[1] <= b[0] for a, b in zip(ivs, ivs[1:]))


def test_nv12_layouts_lie_inside_their_holder_and_the_abi_admits_them():
    """The two NV12 layouts of cases D and E: every row inside the bytes the helper asks for, Y and pair rows disjoint, frames 2^32 + 4096
    bytes apart -- and written_planes_overlap (bevwarp_warp_to_nv12's checks, from the plan driver) admits both as DESTINATIONS, while a
    pair plane moved onto the Y rows is refused."""
    dw, dh = lc.BIG_DSIZE
    joined = lc.nv12_joined(lc.BIG_BATCH, dh, dw, lc.BEYOND_4G)
    beside = lc.nv12_beside(lc.ROWS_PAST_4G5, dw, lc.ROW_64M, 1024)
    assert lc.ROWS_PAST_4G5 % 2 == 0
    for lay, n_y, n_uv in ((joined, lc.BIG_BATCH * dh, lc.BIG_BATCH * dh // 2), (beside, lc.ROWS_PAST_4G5, lc.ROWS_PAST_4G5 // 2)):
        ry, ruv = lc.spec_rows(lay["y"]), lc.spec_rows(lay["uv"])
        assert len(ry) == n_y and len(ruv) == n_uv and all(e - b == dw for b, e in ry + ruv)
        assert _disjoint(ry, ruv) and max(e for _, e in ry + ruv) == lay["bytes"] and min(b for b, _ in ry + ruv) == 0
    assert joined["bytes"] == 2 * lc.BEYOND_4G + dh * 3 // 2 * dw and joined["uv"][1][0] == joined["y"][1][0] == lc.BEYOND_4G
    assert (lc.ROWS_PAST_4G5 - 1) * lc.ROW_64M + dw == lc.dest_reach(lc.ROWS_PAST_4G5, dw, 1, 1, lc.ROW_64M) <= beside["bytes"] < 6 * (1 << 30)
    sources = lc.nv12_joined(lc.BIG_BATCH, lc.BIG_SRC_HW[0], lc.BIG_SRC_HW[1], lc.BEYOND_4G)
    assert _disjoint(lc.spec_rows(sources["y"]), lc.spec_rows(sources["uv"])) and sources["bytes"] < 9 * (1 << 30)
    base, src = 1 << 40, 1 << 30  # (no pointer is dereferenced)

    def status(lay, batch, rows, fs, rs, uv_off=None):
        uv = lay["uv"][2] if uv_off is None else uv_off
        line = "to_nv12 %d %d %d %d 96 700 %d %d %d %d %d %d %d %d %d 1 0" % (src, base, base + uv, batch, rows, dw, 96 * 2100, 2100, fs, rs, fs, rs, 1)
        return hostplan.run_driver(hostplan.build_driver(), [line], "plan")[0][0]
    assert status(joined, lc.BIG_BATCH, dh, lc.BEYOND_4G, dw) == 0
    assert status(beside, 1, lc.ROWS_PAST_4G5, 0, lc.ROW_64M) == 0
    overlap = -6  # BEVWARP_ERR_OVERLAP
    assert status(joined, lc.BIG_BATCH, dh, lc.BEYOND_4G, dw, uv_off=dh * dw - 2) == overlap    # the first pair row on the last Y row
    assert status(beside, 1, lc.ROWS_PAST_4G5, 0, lc.ROW_64M, uv_off=dw - 2) == overlap
