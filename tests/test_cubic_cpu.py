"""The bicubic warp without a device: the numpy reference's tables against known answers, bev_amd/csrc/cubic_tab.h under the sanitizers
(tests/cubic_tab_driver.cpp, g++) against the reference bit for bit, the reference on images with known results, the C ABI's argument
checks, the cv2-compatible constant, and the kernels' code object.  OpenCV's remapBicubic restated from memory: parity unpinned."""
import ctypes
import subprocess

import numpy as np
import pytest

from bev_amd import _lib
from tests import border_ref as BR
from tests import codeobj
from tests import cubic_ref as CR
from tests import hostplan


# ---- the tables of the reference ----

def test_reference_tables_meet_the_anchors():
    wi, adjusted, diffs, saturated = CR.fixed_table(True)
    wf = CR.float_table()
    assert wi.shape == wf.shape == (32, 32, 16) and wi.dtype == np.int16 and wf.dtype == np.float32
    assert (wi.astype(np.int64).sum(axis=2) == 32768).all()
    assert adjusted == 657 and min(diffs) == -2 and max(diffs) == 4
    assert saturated == 1
    e00 = np.zeros(16, np.int16)
    e00[5], e00[10] = 32767, 1  # 32768 saturates at [1][1]; the missing 1 goes to [2][2]
    np.testing.assert_array_equal(wi[0, 0], e00)
    np.testing.assert_array_equal(wi[16, 16], [288, -1824, -1824, 288, -1824, 11552, 11552, -1824, -1824, 11552, 11552, -1824, 288, -1824, -1824, 288])
    np.testing.assert_array_equal(wi[5, 27], [42, -407, -2597, 228, -481, 4639, 29563, -2597, -75, 728, 4639, -407, 8, -75, -482, 42])
    assert CR.table_crc32(wi) == 0x690308d7
    assert CR.table_crc32(wf) == 0x4285e4f7
    assert np.abs(wi.astype(np.int64)).sum(axis=2).max() == 61952  # (an int32 accumulator is ample: 255 * 61952 < 2^24)


# ---- cubic_tab.h under the sanitizers ----

N_LIST = (1, 2, 3, 4, 5, 37, 640, 32767)
REACH = 32769


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    """(float entries, fixed entries, remapped indices [mode][n][p]) as cubic_tab.h computes them.
    (-ffp-contract=off: the definition rounds after every multiply and add.)"""
    tmp = tmp_path_factory.mktemp("cubic_tab")
    tables, remap = (str(tmp / n) for n in ("tables.bin", "remap.bin"))
    exe = hostplan.build_driver(source="cubic_tab_driver.cpp", extra_flags=("-ffp-contract=off",))
    r = subprocess.run([exe, tables, remap], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(tables, "rb").read()
    assert len(raw) == 1024 * 16 * (4 + 2)
    wf = np.frombuffer(raw[:1024 * 16 * 4], "<f4").reshape(32, 32, 16)
    wi = np.frombuffer(raw[1024 * 16 * 4:], "<i2").reshape(32, 32, 16)
    idx = np.fromfile(remap, "<i4").reshape(4, len(N_LIST), 2 * REACH + 1)
    return wf, wi, idx


def test_header_tables_equal_the_reference_bit_for_bit(driver_output):
    wf, wi, _ = driver_output
    np.testing.assert_array_equal(wf.view(np.uint32), CR.float_table().view(np.uint32))
    np.testing.assert_array_equal(wi, CR.fixed_table())


def test_header_index_remap_over_the_whole_window_range(driver_output):
    """window_index(window_period(mode, n)) for every p in [-32769, 32769].  The whole range is compared with numpy.pad's twin of each
    mode (tests/test_border_cpu.py ties that to border_interpolate's loop, which takes |p| / n trips per call); the range's ends and
    the neighbourhood of the image are compared with border_interpolate itself."""
    _, _, idx = driver_output
    p_all = np.arange(-REACH, REACH + 1)
    for mi, mode in enumerate(BR.SOURCE_READING):
        for ni, n in enumerate(N_LIST):
            padded = np.pad(np.arange(n), REACH, mode=BR.PAD_MODE[mode])
            np.testing.assert_array_equal(idx[mi, ni], padded[p_all + REACH], err_msg="%s n=%d" % (BR.NAMES[mode], n))
            near = list(range(-min(3 * n + 8, REACH), min(4 * n + 8, REACH) + 1, max(1, n // 50)))
            for p in near + [-REACH, -REACH + 1, -32768, 32767, 32768, REACH]:
                assert idx[mi, ni, p + REACH] == BR.border_interpolate(p, n, mode), (BR.NAMES[mode], n, p)


# ---- the reference on images with known answers (uint8) ----

def _src(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def test_identity_returns_the_source():
    src = _src(9, 13, 2, 1)
    np.testing.assert_array_equal(CR.warp(src, np.eye(3), (13, 9), BR.REPLICATE), src)
    # TRANSPARENT writes every pixel whose integer position lies in the source: all of them, edge rows and columns included
    # (the bilinear rule leaves the last row and column alone, tests/test_border_cpu.py)
    got = CR.warp(src, np.eye(3), (13, 9), BR.TRANSPARENT, canvas=np.full_like(src, 77))
    np.testing.assert_array_equal(got, src)
    assert CR.written_mask((9, 13), np.eye(3), (13, 9)).all()


def test_integer_translation_is_an_exact_shift():
    src = _src(7, 11, 3, 2)
    K = 40
    for mode in BR.SOURCE_READING:
        padded = np.pad(src, ((K, K), (K, K), (0, 0)), mode=BR.PAD_MODE[mode])
        for tx, ty in ((5, -3), (-20, 14), (13, 9)):
            Minv = np.array([[1.0, 0, -tx], [0, 1.0, -ty], [0, 0, 1.0]])
            got = CR.warp(src, Minv, (24, 19), mode, m_is_inverse=True)
            np.testing.assert_array_equal(got, padded[K - ty:K - ty + 19, K - tx:K - tx + 24], err_msg="%s t=(%d, %d)" % (BR.NAMES[mode], tx, ty))
    Minv = np.array([[1.0, 0, -5], [0, 1.0, 3], [0, 0, 1.0]])
    got = CR.warp(src, Minv, (24, 19), BR.CONSTANT, m_is_inverse=True, border_value=(9, 8, 7))
    exp = np.empty((19, 24, 3), np.uint8)
    exp[...] = (9, 8, 7)
    exp[0:4, 5:16] = src[3:7]
    np.testing.assert_array_equal(got, exp)


def test_constant_image_stays_constant():
    src = np.full((12, 17, 3), 201, np.uint8)
    Minv = np.array([[0.37, -0.21, -3.0], [0.18, 0.41, -2.5], [0.0005, 0.0, 1.0]])
    for mode in BR.SOURCE_READING:
        assert (CR.warp(src, Minv, (40, 30), mode, m_is_inverse=True) == 201).all(), BR.NAMES[mode]
    assert (CR.warp(src.astype(np.float32), Minv, (40, 30), BR.REPLICATE, m_is_inverse=True) > 200.99).all()


def test_checkerboard_overshoots_into_both_clamps():
    yy, xx = np.mgrid[0:24, 0:24]
    src = (((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)[:, :, None]
    Minv = np.array([[0.31, 0.02, 1.3], [-0.01, 0.29, 2.1], [0, 0, 1.0]])
    sx, sy, fx, fy = CR.window((60, 60), Minv)
    W = CR.fixed_table()[fy, fx].astype(np.int64)
    inl = CR.classes((24, 24), Minv, (60, 60), m_is_inverse=True)[0]
    taps = np.stack([src[np.clip(sy + i, 0, 23), np.clip(sx + j, 0, 23), 0].astype(np.int64) for i in range(4) for j in range(4)], axis=-1)
    raw = ((taps * W).sum(axis=-1) + 16384) >> 15
    assert (raw[inl] < 0).any() and (raw[inl] > 255).any()  # the sums leave [0, 255] on both sides ...
    got = CR.warp(src, Minv, (60, 60), BR.REPLICATE, m_is_inverse=True)[..., 0]
    np.testing.assert_array_equal(got[inl], np.clip(raw[inl], 0, 255))  # ... and the result is their clamp
    assert (got[inl & (raw < 0)] == 0).all() and (got[inl & (raw > 255)] == 255).all()


def test_float_inlier_and_general_orders_differ():
    """Both association orders are part of the definition; they give different float32 results, so neither path may stand in for the other."""
    rng = np.random.default_rng(3)
    src = rng.random((20, 20, 1), dtype=np.float32)
    Minv = np.array([[0.9, 0.1, 2.2], [-0.1, 0.95, 3.1], [0, 0, 1.0]])
    sx, sy, fx, fy = CR.window((12, 12), Minv)
    assert CR.classes((20, 20), Minv, (12, 12), m_is_inverse=True)[0].all()
    W = CR.float_table()[fy, fx]
    seq = np.zeros((12, 12), np.float32)
    for i in range(4):
        for j in range(4):
            seq = seq + src[sy + i, sx + j, 0] * W[..., 4 * i + j]
    got = CR.warp(src, Minv, (12, 12), BR.REPLICATE, m_is_inverse=True)[..., 0]
    assert got.dtype == np.float32 and (got != seq).any() and np.allclose(got, seq, rtol=0, atol=1e-5)


# ---- the C ABI, without a device (fake pointers, never dereferenced: every call below fails validation first) ----

@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


CUBIC = 2
ONE, FAR = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)
OK_ARGS = [ONE, FAR, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, ONE, 1, _lib.U8, CUBIC, None, None]
# the list of tests/test_border_cpu.py::test_abi_entry_validates_like_bevwarp_warp
BAD = [dict(a0=None), dict(a1=None), dict(a12=None), dict(a2=-1), dict(a7=5), dict(a7=0), dict(a14=7), dict(a15=3), dict(a9=23),
       dict(a13=2), dict(a4=40000, a9=120000, a8=960000), dict(a1=ONE), dict(a1=ctypes.c_void_p(16 + 191)),
       dict(a2=4, a1=ctypes.c_void_p(16 + 3 * 192 + 100)), dict(a14=_lib.F32, a9=26), dict(a3=0)]


def _patched(patch):
    a = list(OK_ARGS)
    for k, v in patch.items():
        a[int(k[1:])] = v
    return a


def test_abi_cubic_validates_like_every_other_interpolation(lib):
    assert _lib.INTER_CUBIC == CUBIC and lib.bevwarp_version() == 7
    for patch in BAD:
        a = _patched(patch)
        want = lib.bevwarp_warp(*a)
        assert want < 0, patch
        linear = list(a)
        linear[15] = 1 if "a15" not in patch else a[15]
        assert lib.bevwarp_warp(*linear) == want, patch  # the status bilinear gets for the same mistake
        for mode in range(6):
            assert lib.bevwarp_warp_border(*(a[:16] + [mode] + a[16:])) == want, (patch, mode)


def test_abi_cubic_empty_batch_is_a_no_op(lib):
    a = _patched(dict(a2=0))
    assert lib.bevwarp_warp(*a) == 0
    for mode in range(6):
        assert lib.bevwarp_warp_border(*(a[:16] + [mode] + a[16:])) == 0, mode


def test_abi_other_interpolations_and_entry_points_stay_unsupported(lib):
    for interp in (3, 4, 5, 7, -1):
        a = _patched(dict(a15=interp))
        assert lib.bevwarp_warp(*a) == -2, interp
        for mode in range(6):
            assert lib.bevwarp_warp_border(*(a[:16] + [mode] + a[16:])) == -2, (interp, mode)
    for mode in (6, 16, 17, -1, 100):  # an unknown border mode is refused with bicubic as with bilinear
        assert lib.bevwarp_warp_border(*(OK_ARGS[:16] + [mode, None, None])) == -2, mode
    a = OK_ARGS
    assert lib.bevwarp_warp_classes(*(a[:17] + [FAR, 0, None])) == -2
    assert lib.bevwarp_warp_classes(*(a[:17] + [FAR, 1, None])) == -2
    assert lib.bevwarp_tile_classes_bytes(1, 8, 8, 8, 8, 3, _lib.U8, CUBIC) == -2
    assert lib.bevwarp_warp_planar(ONE, FAR, 1, 8, 8, 8, 8, 3, 192, 24, 768, 256, 32, ONE, 1, _lib.U8, CUBIC, None, None, None, None) == -2
    assert lib.bevwarp_resize(ONE, FAR, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, _lib.U8, CUBIC, None) == -2
    assert lib.bevwarp_footprint(FAR, 1, 8, 8, 8, 8, ONE, 1, CUBIC, None) == -2


# ---- Python ----

def test_inter_cubic_constant():
    import bev.cv2_compat as bev_cv2
    import bev.warp as bev_warp
    from bev_amd import cv2_compat as cv2, warp
    for mod in (cv2, warp, bev_cv2, bev_warp):
        assert mod.INTER_CUBIC == 2, mod.__name__


def test_python_rejects_before_the_device():
    from bev_amd import cv2_compat as cv2, warp
    img = np.zeros((8, 8, 3), np.uint8)
    for mode in (16, 6, -1):  # an unknown border mode with flags=INTER_CUBIC
        with pytest.raises(ValueError):
            cv2.warpPerspective(img, np.eye(3), (8, 8), flags=cv2.INTER_CUBIC, borderMode=mode)
        with pytest.raises(ValueError):
            warp.warp_perspective(img, np.eye(3), (8, 8), flags=warp.INTER_CUBIC, border_mode=mode)


def test_warp_to_planar_keeps_rejecting_cubic():
    """The planar warp has no bicubic kernel; its interpolation check comes before anything that needs a device."""
    from bev_amd import warp
    with pytest.raises(ValueError, match="interpolation"):
        warp.warp_to_planar(np.zeros((8, 8, 3), np.uint8), np.eye(3), (8, 8), flags=warp.INTER_CUBIC)


# ---- the code object: at least one kernel, no scratch, at most 128 VGPRs (4 waves per SIMD, the border kernels' bound) ----

def test_cubic_kernels_code_object(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("warp_cubic.hip", tmp_path).items() if "warp_cubic_kernel" in n}
    assert len(kernels) == 2 * 4 * 6, len(kernels)  # dtype x channels x mode
    codeobj.assert_lean(kernels)
