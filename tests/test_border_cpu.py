"""The warp's border modes without a device: the numpy reference (tests/border_ref.py) against the trusted constant-border
oracle and against known answers, the C ABI's argument checks, the cv2-compatible constants, and the new kernels' code objects."""
import ctypes
import os

import numpy as np
import pytest

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import border_ref as BR
from tests import codeobj
from tests import hostplan
from tests import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(h, w, c, dtype, seed=0):
    rng = np.random.default_rng(seed)
    shape = (h, w) if c == 0 else (h, w, c)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


CONSTANT_CASES = [  # (src h, w, channels (0 = 2-D), dst w, h, homography kind)
    (72, 128, 3, 64, 48, "brno"), (60, 100, 1, 90, 30, "keystone"), (36, 64, 4, 70, 20, "rot"), (108, 192, 2, 37, 53, "brno"),
    (20, 30, 0, 33, 9, "rot"),
]


def _H(kind, sw, sh, dw, dh):
    if kind == "brno":
        return wl.synth_brno_H(sw, sh, dw, dh)
    if kind == "keystone":
        return wl.keystone_H(sw, sh, dw, dh)
    return wl.rotated_H(sw, sh, dw, dh, 30.0, zoom=2.5)


@pytest.mark.parametrize("case", CONSTANT_CASES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
def test_constant_equals_the_oracle(case, dtype, interp):
    """The reference differs from the trusted constant-border oracle only in tap selection: with CONSTANT they agree bit for bit."""
    sh, sw, c, dw, dh, kind = case
    src = _src(sh, sw, c, dtype, seed=sw)
    M = _H(kind, sw, sh, dw, dh)
    bv = (7.0, 200.0, 31.0, 99.0)[:max(c, 1)]
    got = BR.warp(src, M, (dw, dh), interp, BR.CONSTANT, border_value=bv)
    np.testing.assert_array_equal(got, wn.warp_perspective(src, M, (dw, dh), interp, border_value=bv))


@pytest.mark.parametrize("n", range(1, 10))
def test_border_interpolate_loop_equals_numpy_pad(n):
    lo, hi = -(3 * n + 40), 4 * n + 40
    ps = list(range(lo, hi + 1)) + list(range(-32770, -32760)) + list(range(32760, 32770))
    K = 32771
    for mode in BR.SOURCE_READING:
        padded = np.pad(np.arange(n), K, mode=BR.PAD_MODE[mode])
        for p in ps:
            assert BR.border_interpolate(p, n, mode) == padded[p + K], (BR.NAMES[mode], n, p)
    assert BR.border_interpolate(-1, n, BR.CONSTANT) == -1 and BR.border_interpolate(n, n, BR.CONSTANT) == -1


@pytest.mark.parametrize("mode", BR.SOURCE_READING)
@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_integer_translation_is_a_window_of_numpy_pad(mode, interp, dtype):
    """A translation by whole pixels (fx = fy = 0) reads the source at (x - tx, y - ty): the window of the padded image."""
    src = _src(7, 11, 3, dtype, seed=3)
    K = 64
    padded = np.pad(src, ((K, K), (K, K), (0, 0)), mode=BR.PAD_MODE[mode])
    for tx, ty in ((5, -3), (-20, 14), (13, 9), (-30, -25)):
        Minv = np.array([[1.0, 0, -tx], [0, 1.0, -ty], [0, 0, 1.0]])
        got = BR.warp(src, Minv, (24, 19), interp, mode, m_is_inverse=True)
        np.testing.assert_array_equal(got, padded[K - ty:K - ty + 19, K - tx:K - tx + 24], err_msg="%s t=(%d, %d)" % (BR.NAMES[mode], tx, ty))


@pytest.mark.parametrize("interp", [wn.NEAREST, wn.LINEAR])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_identity_and_transparent_identity(interp, dtype):
    src = _src(9, 13, 2, dtype, seed=4)
    for mode in BR.SOURCE_READING:
        np.testing.assert_array_equal(BR.warp(src, np.eye(3), (13, 9), interp, mode), src)
    canvas = np.full_like(src, 77)
    got = BR.warp(src, np.eye(3), (13, 9), interp, BR.TRANSPARENT, canvas=canvas)
    if interp == wn.NEAREST:
        np.testing.assert_array_equal(got, src)
    else:  # remapBilinear's inlier test is sx <= w - 2: exactly the last row and column stay untouched
        np.testing.assert_array_equal(got[:-1, :-1], src[:-1, :-1])
        assert (got[-1] == 77).all() and (got[:, -1] == 77).all()


def test_int16_saturation_and_nan_coordinates():
    """Indices saturate to int16 before borderInterpolate, and a NaN coordinate maps to INT_MAX (-> 32767)."""
    src = _src(5, 7, 1, np.uint8, seed=5)
    Minv = np.array([[1.0, 0, 40000.0], [0, 1.0, -50000.0], [0, 0, 1.0]])
    got = BR.warp(src, Minv, (3, 2), wn.NEAREST, BR.WRAP, m_is_inverse=True)
    assert got[0, 0, 0] == src[(-32768) % 5, 32767 % 7, 0]
    # W denormal with a zero numerator: 32 / W overflows, 0 * inf is NaN -> X = Y = INT_MAX -> sx = sy = 32767
    Minv = np.array([[0.0, 0, 0], [0, 0.0, 0], [0, 0, 5e-324]])
    got = BR.warp(src, Minv, (2, 2), wn.LINEAR, BR.REPLICATE, m_is_inverse=True)
    assert (got[..., 0] == src[4, 6, 0]).all()


# ---- the C ABI, without a device (fake pointers, never dereferenced: every call below fails validation first) ----

@pytest.fixture(scope="module")
def lib():
    return hostplan.built_lib()


def test_abi_entry_validates_like_bevwarp_warp(lib):
    assert "bevwarp_warp_border" in _lib.SYMBOLS and lib.bevwarp_version() == 7
    one = ctypes.c_void_p(16)
    far = ctypes.c_void_p(1 << 20)
    ok_args = [one, far, 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, _lib.U8, 1, None, None]
    bad = [dict(a0=None), dict(a1=None), dict(a12=None), dict(a2=-1), dict(a7=5), dict(a7=0), dict(a14=7), dict(a15=3), dict(a9=23),
           dict(a13=2), dict(a4=40000, a9=120000, a8=960000), dict(a1=one), dict(a1=ctypes.c_void_p(16 + 191)),
           dict(a2=4, a1=ctypes.c_void_p(16 + 3 * 192 + 100)), dict(a14=_lib.F32, a9=26), dict(a3=0)]

    def patched(patch):
        a = list(ok_args)
        for k, v in patch.items():
            a[int(k[1:])] = v
        return a

    for patch in bad:
        a = patched(patch)
        want = lib.bevwarp_warp(*a)
        assert want < 0, patch
        for mode in range(6):
            assert lib.bevwarp_warp_border(*(a[:16] + [mode] + a[16:])) == want, (patch, mode)
    assert lib.bevwarp_warp_border(*(patched(dict(a2=0))[:16] + [1, None, None])) == 0  # empty batch: a no-op


def test_abi_unknown_modes_are_unsupported(lib):
    one = ctypes.c_void_p(16)
    args = [one, ctypes.c_void_p(1 << 20), 1, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, _lib.U8, 1]
    for mode in (6, 16, 16 + 1, -1, 100):  # (16 = OpenCV's BORDER_ISOLATED bit)
        assert lib.bevwarp_warp_border(*(args + [mode, None, None])) == -2, mode


def test_cv2_compat_border_constants():
    import bev.cv2_compat as bev_cv2
    import bev.warp as bev_warp
    from bev_amd import cv2_compat as cv2, warp
    expect = dict(BORDER_CONSTANT=0, BORDER_REPLICATE=1, BORDER_REFLECT=2, BORDER_WRAP=3, BORDER_REFLECT_101=4, BORDER_REFLECT101=4,
                  BORDER_DEFAULT=4, BORDER_TRANSPARENT=5)
    for mod in (cv2, warp, bev_cv2, bev_warp):
        for name, v in expect.items():
            assert getattr(mod, name) == v, (mod.__name__, name)


def test_cv2_compat_rejects_unknown_border_before_the_device():
    from bev_amd import cv2_compat as cv2, warp
    img = np.zeros((8, 8, 3), np.uint8)
    for mode in (16, 6, -1):
        with pytest.raises(ValueError):
            cv2.warpPerspective(img, np.eye(3), (8, 8), borderMode=mode)
    with pytest.raises(ValueError):  # the batched entry validates the mode first too
        warp.warp_perspective(img, np.eye(3), (8, 8), border_mode=16)


# ---- the code objects of the new kernels: no scratch, at most 128 VGPRs each ----

def test_border_kernels_code_object(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("warp_border.hip", tmp_path).items() if "warp_border_kernel" in n}
    assert len(kernels) == 2 * 2 * 4 * 5, len(kernels)  # dtype x interpolation x channels x mode
    codeobj.assert_lean(kernels)
