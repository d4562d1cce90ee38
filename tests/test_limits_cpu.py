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
from tests import border_ref as br
from tests import cubic_ref as cr
from tests import limits_cases as lc

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
