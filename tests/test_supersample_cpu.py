"""The supersampled warp without a device: the numpy reference (tests/supersample_ref.py) against hand answers, the host checks of
BEVWARP_SUPERSAMPLE_* through tests/host_plan_driver.cpp, family `supersample` (under the sanitizers) and through the built library with pointers that
are never dereferenced, the header's text, the Python entry's refusals, and the new kernels' code object."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import border_ref as BR
from tests import codeobj
from tests import hostplan
from tests import supersample_ref as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
S2, S4, S8 = 0x1000, 0x2000, 0x3000
INT_MAX = 2 ** 31 - 1


# ---- the reference against hand answers -----------------------------------------------------------------------------------------------

def test_identity_is_not_the_identity_image():
    """The property the header states: the ramp 0, 32, ..., 224 under k = 2, bilinear, REPLICATE."""
    ramp = np.arange(0, 256, 32, dtype=np.uint8)[None, :]
    got = SS.warp(ramp, np.eye(3), (8, 1), 2, wn.LINEAR, BR.REPLICATE)
    np.testing.assert_array_equal(got, np.array([[4, 32, 64, 96, 128, 160, 192, 220]], np.uint8))
    np.testing.assert_array_equal(SS.warp(ramp, np.eye(3), (8, 1), 1, wn.LINEAR, BR.REPLICATE), ramp)  # k = 1 is the plain warp


@pytest.mark.parametrize("k", SS.FACTORS)
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_constant_image_stays_constant(k, interp):
    """Every mode, both pixel types, bit for bit (CONSTANT: with the image's value as the border value).  0.75 has two mantissa bits: its
    products with the blend's weights (multiples of 1 / 1024) and all their sums are exact."""
    Minv = np.array([[3.7, 0.4, -9.0], [-0.3, 4.1, -6.0], [0.001, 0.003, 1.0]])  # minifies 4x and leaves the 13 x 9 source on every side
    for value, dtype in ((93, np.uint8), (0.75, np.float32)):
        src = np.full((9, 13, 2), value, dtype)
        for mode in SS.MODES:
            got = SS.warp(src, Minv, (11, 7), k, interp, mode, m_is_inverse=True, border_value=value)
            assert got.dtype == dtype and got.shape == (7, 11, 2)
            assert (got == dtype(value)).all(), (BR.NAMES[mode], dtype)


def test_float32_reduce_order_by_hand():
    """k = 2 on a 2 x 2 fine grid whose pixels ARE the source's four: Minv = [[2, 0, .5], [0, 2, .5], [0, 0, 1]] has the identity as its
    fine matrix.  ((1e8 + 1) + -1e8) + 1 is 1 in float32 (the first sum rounds back to 1e8); columns first, or pairwise, gives 2."""
    Minv = np.array([[2.0, 0, 0.5], [0, 2.0, 0.5], [0, 0, 1.0]])
    np.testing.assert_array_equal(SS.fine_matrix(Minv, 2), np.eye(3))
    src = np.array([[1e8, 1.0], [-1e8, 1.0]], np.float32)
    got = SS.warp(src, Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)
    assert got.dtype == np.float32 and got.shape == (1, 1)
    assert got[0, 0] == np.float32(0.25)
    f = np.float32
    assert f(f(f(f(1e8) + f(1.0)) + f(-1e8)) + f(1.0)) * f(0.25) == f(0.25)  # the stated order, spelt out
    assert f(f(f(1e8) + f(-1e8)) + f(f(1.0) + f(1.0))) * f(0.25) == f(0.5)   # another order is another number
    # 8-bit: (1 + 2 + 3 + 4 + 2) >> 2 = 3, and (0 + 0 + 0 + 1 + 2) >> 2 = 0: round half up
    assert SS.warp(np.array([[1, 2], [3, 4]], np.uint8), Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)[0, 0] == 3
    assert SS.warp(np.array([[0, 0], [0, 1]], np.uint8), Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)[0, 0] == 0
    assert SS.warp(np.array([[0, 0], [1, 1]], np.uint8), Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)[0, 0] == 1


def test_nan_propagates_and_denormals_stay():
    Minv = np.array([[2.0, 0, 0.5], [0, 2.0, 0.5], [0, 0, 1.0]])
    tiny = np.float32(1e-45)  # the smallest denormal: 4 of them times 1 / 4 is itself
    got = SS.warp(np.full((2, 2), tiny, np.float32), Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)
    assert got[0, 0] == tiny and got[0, 0] != 0
    src = np.array([[1.0, np.nan], [2.0, 3.0]], np.float32)
    assert np.isnan(SS.warp(src, Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)[0, 0])
    src = np.array([[1.0, np.inf], [2.0, -np.inf]], np.float32)
    assert np.isnan(SS.warp(src, Minv, (1, 1), 2, wn.NEAREST, BR.REPLICATE, m_is_inverse=True)[0, 0])


def test_fine_matrix_entries():
    np.testing.assert_array_equal(SS.fine_matrix(np.eye(3), 2), [[0.5, 0, -0.25], [0, 0.5, -0.25], [0, 0, 1.0]])
    np.testing.assert_array_equal(SS.fine_matrix(np.eye(3), 4), [[0.25, 0, -0.375], [0, 0.25, -0.375], [0, 0, 1.0]])
    np.testing.assert_array_equal(SS.fine_matrix(np.eye(3), 8), [[0.125, 0, -0.4375], [0, 0.125, -0.4375], [0, 0, 1.0]])
    # a matrix whose products round: every line one float64 operation (Python's floats have no FMA either)
    M = np.array([[0.1, 0.3, 0.7], [-1.1, 2.3, 1e-3], [1e-5, -3e-5, 0.9]])
    for k, c in ((2, -0.25), (4, -0.375), (8, -0.4375)):
        F = SS.fine_matrix(M, k)
        for r in range(3):
            m0, m1, m2 = (float(v) for v in M[r])
            assert F[r, 0] == m0 / k and F[r, 1] == m1 / k
            assert F[r, 2] == (m0 * c + m1 * c) + m2
    assert Fraction(0.1) * Fraction(-0.375) != Fraction(0.1 * -0.375)  # (the product does round)
    assert Fraction(0.1 * -0.375 + 0.3 * -0.375) + Fraction(0.7) != Fraction((0.1 * -0.375 + 0.3 * -0.375) + 0.7)  # (and so does the last sum)


def test_straddling_shapes_straddle():
    """The fine grids of the GPU test's straddling shapes have evaluation blocks whose width is no multiple of k."""
    for (dw, dh), k, bw in (((50, 7), 2, 73), ((30, 3), 4, 85)):
        assert SS.block_width(k * dw, k * dh) == bw and bw % k != 0 and bw < k * dw


# ---- the host checks: the driver under the sanitizers ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_take_supersample(driver):
    words = [0, 1, 2, 0x100, 0x200, S2 | 1, S8 | 0, S4 | 2, -1]
    want = [[1, 0], [1, 1], [1, 2], [1, 0x100], [1, 0x200], [2, 1], [8, 0], [4, 2], [8, -1 & ~0x3000]]
    assert hostplan.run_driver(driver, ["field %d" % w for w in words], "supersample") == want
    assert want[-1][1] == -12289


def _call(src=16, dst=1 << 20, minv=16, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, channels=3, src_fs=192, src_rs=24, dst_fs=192, dst_rs=24, m_count=1,
          dtype=_lib.U8, interp=1 | S2, mode=1):
    return "call %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (src, dst, minv, batch, src_h, src_w, dst_h, dst_w, channels, src_fs, src_rs, dst_fs, dst_rs,
                                                                      m_count, dtype, interp, mode)


# test_border_cpu.py's list of bad arguments, by name, with the status each has today
BAD_ARGUMENTS = [
    (dict(src=0), BAD_ARG), (dict(dst=0), BAD_ARG), (dict(minv=0), BAD_ARG), (dict(batch=-1), BAD_ARG), (dict(channels=5), UNSUPPORTED),
    (dict(channels=0), UNSUPPORTED), (dict(dtype=7), UNSUPPORTED), (dict(interp=3), UNSUPPORTED), (dict(src_rs=23), BAD_ARG), (dict(m_count=2), BAD_ARG),
    (dict(src_w=40000, src_rs=120000, src_fs=960000), TOO_LARGE), (dict(dst=16), OVERLAP), (dict(dst=16 + 191), OVERLAP),
    (dict(batch=4, dst=16 + 3 * 192 + 100), OVERLAP), (dict(dtype=_lib.F32, src_rs=26), BAD_ARG), (dict(src_h=0), BAD_ARG),
]


def test_call_statuses_in_their_documented_order(driver):
    cases, want = [], []

    def add(expected, **kw):
        cases.append(_call(**kw))
        want.append(expected)

    for k, field in ((2, S2), (4, S4), (8, S8)):
        for mode in SS.MODES:  # a good call: the destination's grid, the fine grid's blocks
            add([k, OK, OK, 8 * k, 2], interp=1 | field, mode=mode)
            add([k, OK, OK, 8 * k, 2], interp=0 | field, mode=mode, dtype=_lib.F32, src_rs=96, src_fs=768, dst_rs=96, dst_fs=768)
        add([k, UNSUPPORTED, 0, 0, 0], interp=2 | field)                       # bicubic under the field
        add([k, UNSUPPORTED, 0, 0, 0], interp=1 | field, mode=5)               # TRANSPARENT under the field
        for mode in (6, 16, 17, -1, 100):                                      # an unknown mode: before everything else
            add([k, UNSUPPORTED, 0, 0, 0], interp=1 | field, mode=mode)
            add([k, UNSUPPORTED, 0, 0, 0], interp=1 | field, mode=mode, src=0)
        add([k, BAD_ARG, 0, 0, 0], interp=2 | field, src=0)                    # NULLs and sides before the format ...
        add([k, BAD_ARG, 0, 0, 0], interp=1 | field, mode=5, dst_h=0)
        add([k, UNSUPPORTED, 0, 0, 0], interp=1 | field, mode=5, m_count=2)    # ... the format before the matrix count and the strides
        add([k, UNSUPPORTED, 0, 0, 0], interp=2 | field, src_rs=23)
        for patch, status in BAD_ARGUMENTS:
            kw = dict(patch)
            kw["interp"] = kw.get("interp", 1) | field
            for mode in SS.MODES:
                add([k, status, 0, 0, 0], mode=mode, **kw)
        add([k, OK, 0, 0, 0], interp=1 | field, batch=0)                       # an empty batch: OK, nothing planned
        # k dst_w just past INT_MAX: where the source's size is judged -- after the strides, before the overlap
        w = INT_MAX // k + 1
        add([k, TOO_LARGE, 0, 0, 0], interp=1 | field, dst_w=w, channels=1, dst_rs=w, dst_fs=8 * w, src_rs=8, src_fs=64)
        add([k, TOO_LARGE, 0, 0, 0], interp=1 | field, dst_h=w, dst_w=1, channels=1, dst_rs=1, dst_fs=w, src_rs=8, src_fs=64)
        add([k, TOO_LARGE, 0, 0, 0], interp=1 | field, dst_w=w, channels=1, dst_rs=w, dst_fs=8 * w, src_rs=8, src_fs=64, dst=16)  # (not OVERLAP)
        add([k, BAD_ARG, 0, 0, 0], interp=1 | field, dst_w=w, channels=1, dst_rs=w - 1, dst_fs=8 * w, src_rs=8, src_fs=64)      # (the stride first)
        add([k, TOO_LARGE, 0, 0, 0], interp=1 | field, dst_w=w, channels=1, dst_rs=w, dst_fs=8 * w, src_rs=8, src_fs=64, batch=0)
        # one column fewer: the checks pass, and the plan refuses a side beyond 2^20 as it does without the field
        add([k, OK, TOO_LARGE, 0, 0], interp=1 | field, dst_w=w - 1, channels=1, dst_rs=w, dst_fs=8 * w, src_rs=8, src_fs=64)
        # strides next to 2^63: bad arguments like any other, no overflow
        big = 2 ** 63 - 1
        add([k, BAD_ARG, 0, 0, 0], interp=1 | field, batch=2, src_fs=big, src_rs=big - 7)
        add([k, BAD_ARG, 0, 0, 0], interp=1 | field, batch=2, dst_fs=big, dst_rs=big)
        add([k, OK, OK, 8 * k, 4], interp=1 | field, batch=2, m_count=2, src_fs=1 << 61, dst=1 << 62, dst_fs=1 << 60)
    # the fine grid's blocks: widths that are no multiple of k, and the destination's tiles
    add([2, OK, OK, 73, 4], interp=1 | S2, batch=2, dst_w=50, dst_h=7, dst_rs=150, dst_fs=1050)
    add([4, OK, OK, 85, 1], interp=1 | S4, dst_w=30, dst_h=3, dst_rs=90, dst_fs=270)
    add([8, OK, OK, 64, 2 * 3], interp=1 | S8, dst_w=257, dst_h=9, dst_rs=771, dst_fs=6939)
    got = hostplan.run_driver(driver, cases, "supersample")
    for line, g, w in zip(cases, got, want):
        assert g == w, (line, g, w)


def test_other_entries_judge_the_whole_word(driver):
    lines, want = [], []
    for entry in ("warp", "lens", "remap", "build"):
        for interp in (0, 1):
            lines.append("other %s %d" % (entry, interp))
            want.append([OK])
            for field in (S2, S4, S8):
                lines.append("other %s %d" % (entry, interp | field))
                want.append([UNSUPPORTED])
    for field in (S2, S4, S8):
        lines += ["other lens %d" % (1 | 0x100 | field), "other build %d" % (1 | 0x100 | field), "other remap %d" % (1 | 0x200 | field)]
        want += [[UNSUPPORTED]] * 3
    assert hostplan.run_driver(driver, lines, "supersample") == want


# ---- the same statuses through the built library (fake pointers, never dereferenced: every call ends before a launch) ---------------------

@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


def _border_args(one, far, **patch):
    a = dict(src=one, dst=far, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, channels=3, src_fs=192, src_rs=24, dst_fs=192, dst_rs=24, minv=one, m_count=1,
             dtype=_lib.U8, interp=1, mode=1, border=None, stream=None)
    a.update(patch)
    return list(a.values())


def test_library_statuses(lib):
    assert lib.bevwarp_version() == 7 and "bevwarp_warp_border" in _lib.SYMBOLS
    one, far = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)
    ptr = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    for patch, status in BAD_ARGUMENTS:
        kw = {k: (ptr(v) if k in ("src", "dst", "minv") else v) for k, v in patch.items()}
        for mode in range(6):
            plain = lib.bevwarp_warp_border(*_border_args(one, far, **dict(kw, mode=mode)))
            assert plain == status, (patch, mode)  # field 0: today's answers
        for field in (S2, S4, S8):
            flagged = dict(kw, interp=kw.get("interp", 1) | field)
            for mode in SS.MODES:
                assert lib.bevwarp_warp_border(*_border_args(one, far, **dict(flagged, mode=mode))) == status, (patch, field, mode)
    for field in (S2, S4, S8):
        assert lib.bevwarp_warp_border(*_border_args(one, far, interp=2 | field)) == UNSUPPORTED
        assert lib.bevwarp_warp_border(*_border_args(one, far, interp=1 | field, mode=5)) == UNSUPPORTED
        for mode in (6, 16, 17, -1, 100):
            assert lib.bevwarp_warp_border(*_border_args(None, far, interp=1 | field, mode=mode)) == UNSUPPORTED
        assert lib.bevwarp_warp_border(*_border_args(one, far, interp=1 | field, batch=0)) == OK
        w = INT_MAX // (1 << (field >> 12)) + 1
        assert lib.bevwarp_warp_border(*_border_args(one, far, interp=1 | field, dst_w=w, channels=1, dst_rs=w, dst_fs=8 * w, src_rs=8, src_fs=64)) == TOO_LARGE
        # a non-finite border value: last, and read by the constant border only
        nan = (ctypes.c_double * 3)(1.0, float("nan"), 2.0)
        bad_border = ctypes.cast(nan, ctypes.c_void_p)
        assert lib.bevwarp_warp_border(*_border_args(one, far, interp=1 | field, mode=0, border=bad_border)) == NOT_FINITE
        assert lib.bevwarp_warp_border(*_border_args(one, one, interp=1 | field, mode=0, border=bad_border)) == OVERLAP
    # with the field 0 the unknown modes and the empty batch answer as they always did
    for mode in (6, 16, 17, -1, 100):
        assert lib.bevwarp_warp_border(*_border_args(one, far, mode=mode)) == UNSUPPORTED
    assert lib.bevwarp_warp_border(*_border_args(one, far, batch=0)) == OK


def test_library_other_entries_refuse_the_field(lib):
    one, far = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)
    xy, fr = ctypes.c_void_p(1 << 24), ctypes.c_void_p(1 << 26)
    for word in (S2, S4, S8, 0x4000):  # (0x4000: a bit no entry knows -- the field's bits are answered like it)
        for interp in (0, 1):
            w = interp | word
            assert lib.bevwarp_warp(one, far, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, _lib.U8, w, None, None) == UNSUPPORTED
            assert lib.bevwarp_warp_lens(one, far, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, None, 1.0, _lib.U8, w, 0, None, None) == UNSUPPORTED
            assert lib.bevwarp_warp_lens(one, far, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, None, 1.0, _lib.U8, w | 0x100, 0, None, None) == UNSUPPORTED
            assert lib.bevwarp_remap(one, far, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, xy, fr, 1, 256, 32, 128, 16, _lib.U8, w, 0, None, None) == UNSUPPORTED
            assert lib.bevwarp_build_map(one, 1, None, 0.0, w, xy, fr, 8, 8, 256, 32, 128, 16, None) == UNSUPPORTED


def test_header_defines_and_abi_version():
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        text = f.read()
    for name, value in (("BEVWARP_SUPERSAMPLE_2", "0x1000"), ("BEVWARP_SUPERSAMPLE_4", "0x2000"), ("BEVWARP_SUPERSAMPLE_8", "0x3000"),
                        ("BEVWARP_SUPERSAMPLE_MASK", "0x3000"), ("BEVWARP_ABI_VERSION", "7")):
        assert re.search(r"^#define %s\s+%s\b" % (name, value), text, re.M), name
    assert (_lib.SUPERSAMPLE_2, _lib.SUPERSAMPLE_4, _lib.SUPERSAMPLE_8) == (S2, S4, S8) and SS.FIELD == {1: 0, 2: S2, 4: S4, 8: S8}
    assert _lib.ABI_VERSION == 7


# ---- the Python entry refuses before it touches a device ------------------------------------------------------------------------------

def test_python_refusals_without_a_device():
    import bev.warp as bev_warp
    from bev_amd import warp as W
    assert bev_warp.warp_perspective_supersampled is W.warp_perspective_supersampled
    img = torch.zeros((8, 8, 3), dtype=torch.uint8)  # a CPU tensor: anything that got as far as the frames would say so
    for bad in (0, 3, 16, -2, 2.5, True, None, "2"):
        with pytest.raises(ValueError, match="supersample must be"):
            W.warp_perspective_supersampled(img, np.eye(3), (8, 8), supersample=bad)
    for k in (2, 4, 8):
        with pytest.raises(ValueError, match="interpolation"):
            W.warp_perspective_supersampled(img, np.eye(3), (8, 8), supersample=k, flags=W.INTER_CUBIC)
        for mode in (W.BORDER_TRANSPARENT, 6, 16, -1):
            with pytest.raises(ValueError, match="border mode"):
                W.warp_perspective_supersampled(img, np.eye(3), (8, 8), supersample=k, border_mode=mode)
        with pytest.raises(ValueError, match="fine grid"):
            W.warp_perspective_supersampled(img, np.eye(3), (INT_MAX // k + 1, 8), supersample=k)
        with pytest.raises(ValueError, match="fine grid"):
            W.warp_perspective_supersampled(img, np.eye(3), (8, INT_MAX // k + 1), supersample=k)
        with pytest.raises(ValueError, match="CUDA"):
            W.warp_perspective_supersampled(img, np.eye(3), (8, 8), supersample=k)
    with pytest.raises(ValueError, match="CUDA"):  # supersample = 1 is warp_perspective, refusals included
        W.warp_perspective_supersampled(img, np.eye(3), (8, 8), supersample=1)


# ---- the code object of the new kernels: no scratch, no LDS, at most 128 VGPRs each ----------------------------------------------------------

def test_supersample_kernels_code_object(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("warp_supersample.hip", tmp_path, "warp_supersample.h").items() if "warp_supersample_kernel" in n}
    assert len(kernels) == 2 * 2 * 4 * 5, len(kernels)  # dtype x interpolation x channels x mode (k is a loop bound)
    codeobj.assert_lean(kernels)
