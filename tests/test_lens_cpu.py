"""The lens warp (bevwarp_warp_lens, warp_perspective_lens) without a device: the numpy reference (tests/lens_ref.py) against an
independent 50-digit evaluation and against the trusted pinhole oracle, the host helpers, the C ABI's host checks under the
sanitizers (tests/host_plan_driver.cpp, family `lens`), the kernels' code object and the ABI surface."""
import ctypes
import decimal
import os

import numpy as np
import pytest

from bev_amd import _lib
from oracle import warp_numpy as wn
from tests import codeobj
from tests import hostplan
from tests import lens_ref as LR
from tests import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
GEOMS = {  # (src w, h, dst w, h, forward matrix): tests/test_gpu_border.py's
    "rotated_zoom_out": (160, 96, 120, 100, wl.rotated_H(160, 96, 120, 100, 30.0, zoom=2.5)),
    "brno": (640, 360, 160, 120, wl.synth_brno_H(640, 360, 160, 120)),
}


def _src(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)


# ---- the reference's maps against the same formulas in 50-digit decimal ----

def _exact_uv(R, lens, x, y):
    """(u, v) of destination pixel (x, y): the definition's formulas on the float64 inputs, evaluated in 50-digit decimal."""
    D = decimal.Decimal
    r = [D(float(v)) for v in np.asarray(R, np.float64).ravel()]
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = [D(float(v)) for v in lens]
    x, y = D(int(x)), D(int(y))
    W = r[6] * x + r[7] * y + r[8]
    xn, yn = (r[0] * x + r[1] * y + r[2]) / W, (r[3] * x + r[4] * y + r[5]) / W
    x2, y2 = xn * xn, yn * yn
    r2, xy2 = x2 + y2, 2 * xn * yn
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = xn * kr + p1 * xy2 + p2 * (r2 + 2 * x2)
    yd = yn * kr + p1 * (r2 + 2 * y2) + p2 * xy2
    return fx * xd + cx, fy * yd + cy


def test_maps_against_50_digit_evaluation():
    """|32 u_exact - X| <= 0.5 + 1e-6 at 400 seeded pixels of rotated_zoom_out with lens B: 0.5 is the rounding to 1/32 px, and 1e-6
    bounds the float64 chain's own error -- about 25 operations of relative error 2^-53 each on 32 u < 2^13 (and on intermediate
    values of the same order: r2 < 1, kr ~ 1) is below 25 * 2^-53 * 2^13 * 4 < 1e-10, four orders inside the allowance."""
    sw, sh, dw, dh, M = GEOMS["rotated_zoom_out"]
    K = LR.camera_K(sw, sh)
    R, lens = LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_B)
    sx, sy, fx, fy, valid = LR.maps((dw, dh), R, lens, INF, wn.LINEAR)
    assert valid.all()
    X, Y = sx * 32 + fx, sy * 32 + fy
    rng = np.random.default_rng(2024)
    worst = decimal.Decimal(0)
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for x, y in zip(rng.integers(0, dw, 400), rng.integers(0, dh, 400)):
            u, v = _exact_uv(R, lens, x, y)
            worst = max(worst, abs(32 * u - int(X[y, x])), abs(32 * v - int(Y[y, x])))
    print("worst |32 u_exact - X| = %s" % worst)
    assert worst <= decimal.Decimal("0.500001"), worst


# ---- identity lens: the chains coincide for nearest ----

@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_identity_lens_nearest_equals_the_pinhole_oracle(geom, dtype):
    """fx = fy = 1, cx = cy = 0, no distortion, R = Minv: xn * 1 + 0 is xn, so the nearest maps are the pinhole oracle's, bit for bit.
    (Bilinear differs by construction -- (Xn / W) * 32 against Xn * (32 / W) -- and is not compared.)"""
    sw, sh, dw, dh, M = GEOMS[geom]
    lens = np.array([1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    for c in (1, 3):
        src = _src((sh, sw, c), dtype, seed=20 + c)
        bv = (7.0, 200.0, 31.0)[:c]
        got = LR.warp(src, wn.invert3x3(M), lens, INF, (dw, dh), wn.NEAREST, LR.CONSTANT, border_value=bv)
        np.testing.assert_array_equal(got, wn.warp_perspective(src, M, (dw, dh), wn.NEAREST, border_value=bv))


def test_reference_geometries_hold_every_kind_of_pixel():
    """What the GPU tests rely on: both geometries have interior, edge-cut and outside pixels under both lenses, and brno with lens A
    has invalid pixels of which some would land inside the frame (ghosts)."""
    for geom, (sw, sh, dw, dh, M) in GEOMS.items():
        K = LR.camera_K(sw, sh)
        R = LR.ray_matrix(M, K)
        for dist in (LR.LENS_A, LR.LENS_B):
            sx, sy, _, _, valid = LR.maps((dw, dh), R, LR.lens12(K, dist), LR.lens_valid_r2(dist), wn.LINEAR)
            inl = LR.inliers(sx, sy, valid, sw, sh, wn.LINEAR)
            touch = valid & (sx >= -1) & (sx < sw) & (sy >= -1) & (sy < sh)
            assert inl.any() and (touch & ~inl).any() and (~touch).any(), (geom, dist)
    sw, sh, dw, dh, M = GEOMS["brno"]
    K = LR.camera_K(sw, sh)
    R, lens = LR.ray_matrix(M, K), LR.lens12(K, LR.LENS_A)
    sx, sy, _, _, _ = LR.maps((dw, dh), R, lens, INF, wn.LINEAR)
    _, _, r2 = LR.chain((dw, dh), R, lens)
    ghosts = LR.inliers(sx, sy, np.ones_like(sx, bool), sw, sh, wn.LINEAR) & ~(r2 <= LR.lens_valid_r2(LR.LENS_A))
    assert ghosts.sum() > 0


# ---- the host helpers ----

def test_lens_valid_r2_known_answers():
    from bev_amd import warp
    for fn in (warp.lens_valid_r2, LR.lens_valid_r2):
        assert fn([-0.25, 0, 0, 0]) == pytest.approx(4.0 / 3.0, rel=1e-12)  # d/dr [r (1 - r^2 / 4)] = 1 - 3 r^2 / 4
        assert fn([0.0, 0, 0, 0]) == INF and fn(None) == INF
        assert fn([0, 0, 0, 0, 0, -0.5, 0, 0]) == pytest.approx(2.0, rel=1e-12)  # the pole of 1 / (1 - r^2 / 2)
    for dist in (LR.LENS_A, LR.LENS_B):
        assert warp.lens_valid_r2(dist) == pytest.approx(LR.lens_valid_r2(dist), rel=1e-9)
    with pytest.raises(ValueError):
        warp.lens_valid_r2([0.1, 0.2, 0.3])


def test_ray_matrix():
    import bev.warp as bev_warp
    from bev_amd import warp
    assert bev_warp.ray_matrix is warp.ray_matrix and bev_warp.warp_perspective_lens is warp.warp_perspective_lens
    assert bev_warp.lens_valid_r2 is warp.lens_valid_r2 and bev_warp.lens_from_calib is warp.lens_from_calib
    for geom, (sw, sh, dw, dh, M) in GEOMS.items():
        K = LR.camera_K(sw, sh)
        want = np.linalg.inv(K) @ np.linalg.inv(M)
        scale = np.abs(want).max(axis=1, keepdims=True)  # (per row: the rows differ by orders of magnitude)
        for got in (warp.ray_matrix(M, K), warp.ray_matrix(np.linalg.inv(M), K, inverse_given=True), warp.ray_matrix(M, np.hstack([K, np.zeros((3, 1))])),
                    LR.ray_matrix(M, K)):
            assert (np.abs(got - want) <= 1e-12 * scale).all(), geom
        np.testing.assert_array_equal(warp.ray_matrix(np.stack([M, M]), K)[1], warp.ray_matrix(M, K))
    K = LR.camera_K(160, 96)
    K[0, 1] = 0.01
    with pytest.raises(ValueError):
        warp.ray_matrix(np.eye(3), K)


def test_lens_from_calib():
    import bev
    from bev_amd import warp
    T = np.eye(4, dtype=np.float32)
    K, d = warp.lens_from_calib(bev.Calib(fx=800.0, fy=810.0, cx=319.5, cy=239.5, T=T))
    assert K.dtype == np.float64 and K[0, 0] == 800.0 and K[1, 2] == 239.5 and d.shape == (5,) and not d.any()
    _, d = warp.lens_from_calib(bev.Calib(fx=800.0, fy=810.0, cx=319.5, cy=239.5, T=T, dist_coeff=list(LR.LENS_B)))
    np.testing.assert_array_equal(d, LR.LENS_B)
    pts = np.array([[0.0, 0], [10, 0], [10, 10], [0, 10]])
    with pytest.raises(ValueError):
        warp.lens_from_calib(bev.Calib(pts_image=pts, pts_world=np.hstack([pts, np.zeros((4, 1))])))


def test_python_entry_validates_before_the_device():
    from bev_amd import warp
    img = np.zeros((8, 8, 3), np.uint8)
    K = LR.camera_K(8, 8)
    with pytest.raises(ValueError):
        warp.warp_perspective_lens(img, np.eye(3), (8, 8), K, [0.1, 0.2])  # 2 coefficients
    with pytest.raises(ValueError):
        warp.warp_perspective_lens(img, np.eye(3), (8, 8), K, LR.LENS_A, border_mode=warp.BORDER_REPLICATE)
    with pytest.raises(ValueError):
        warp.warp_perspective_lens(img, np.eye(3), (8, 8), K, LR.LENS_A, flags=warp.INTER_CUBIC)
    with pytest.raises(ValueError):
        warp.warp_perspective_lens(img, np.eye(3), (8, 8), K, LR.LENS_A)  # a numpy image: no CUDA tensor


# ---- the host checks under the sanitizers ----

OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
CALL = dict(src=16, dst=1 << 20, batch=1, src_h=8, src_w=8, dst_h=8, dst_w=8, channels=3, src_fs=192, src_rs=24, dst_fs=192, dst_rs=24, m_count=1, m_null=0,
            dtype=0, interp=1, mode=0)


def _call(**kw):
    a = dict(CALL, **kw)
    return "call " + " ".join(str(a[k]) for k in CALL)


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_call_checks_under_sanitizers(driver):
    big = 2147483647
    cases = [(_call(), [OK, OK, 2]), (_call(mode=5), [OK, OK, 2]), (_call(interp=0), [OK, OK, 2]),
             (_call(dtype=1, src_rs=96, src_fs=768, dst_rs=96, dst_fs=768), [OK, OK, 2]), (_call(batch=0), [OK, 0, 0])]
    cases += [(_call(channels=c, src_rs=8 * c, dst_rs=8 * c), [OK, OK, 2]) for c in (1, 2, 4)]
    cases += [(_call(mode=m), [UNSUPPORTED, 0, 0]) for m in (1, 2, 3, 4, 6, 16, 16 + 5, -1, 100)]
    cases += [(_call(interp=i), [UNSUPPORTED, 0, 0]) for i in (2, 3, -1)]
    cases += [(_call(dtype=d), [UNSUPPORTED, 0, 0]) for d in (2, 3, 4, -1)]
    cases += [(_call(channels=c), [UNSUPPORTED, 0, 0]) for c in (0, 5)]
    cases += [(_call(m_count=2), [BAD_ARG, 0, 0]), (_call(m_count=0), [BAD_ARG, 0, 0]), (_call(batch=3, m_count=2), [BAD_ARG, 0, 0]),
              (_call(batch=3, m_count=3), [OK, OK, 6]), (_call(batch=3, m_count=1), [OK, OK, 6])]
    cases += [(_call(src=0), [BAD_ARG, 0, 0]), (_call(dst=0), [BAD_ARG, 0, 0]), (_call(m_null=1), [BAD_ARG, 0, 0])]
    cases += [(_call(dst=16), [OVERLAP, 0, 0]), (_call(dst=16 + 100), [OVERLAP, 0, 0]), (_call(dst=16 + 7 * 24 + 23), [OVERLAP, 0, 0]),
              (_call(dst=16 + 192), [OK, OK, 2]), (_call(src_rs=48, dst_rs=48, src_fs=384, dst_fs=384, dst=16 + 24), [OK, OK, 2])]  # (side by side)
    cases += [(_call(src_w=32768, src_rs=3 * 32768, src_fs=24 * 32768), [TOO_LARGE, 0, 0]), (_call(src_h=32768, src_fs=24 * 32768), [TOO_LARGE, 0, 0]),
              (_call(src_w=32767, src_rs=3 * 32767, src_fs=24 * 32767, dst=1 << 24), [OK, OK, 2]), (_call(src_h=32767, src_fs=24 * 32767, dst=1 << 24), [OK, OK, 2])]
    one = dict(channels=1, src_rs=8, src_fs=64)  # destination sides next to 2^31 and 2^20: the checks pass, the launch plan refuses
    cases += [(_call(dst_w=big, dst_h=1, dst_rs=big, dst_fs=big, **one), [OK, TOO_LARGE, 0]), (_call(dst_w=8, dst_h=big, dst_rs=8, dst_fs=8 * big, **one), [OK, TOO_LARGE, 0]),
              (_call(dst_w=big, dst_h=big, dst_rs=big, dst_fs=big * big, **one), [OK, TOO_LARGE, 0]),
              (_call(dst_w=1 << 20, dst_h=1, dst_rs=1 << 20, dst_fs=1 << 20, **one), [OK, OK, 4096]),
              (_call(dst_w=(1 << 20) + 1, dst_h=1, dst_rs=1 << 21, dst_fs=1 << 21, **one), [OK, TOO_LARGE, 0]),
              (_call(dst_w=8, dst_h=(1 << 20) + 1, dst_rs=8, dst_fs=1 << 24, **one), [OK, TOO_LARGE, 0]),
              (_call(batch=big, dst=1 << 40, dst_rs=8, dst_fs=64, **one), [OK, TOO_LARGE, 0])]  # (2 tiles per frame: the grid passes 2^31 - 1 items)
    hostplan.check_cases(driver, cases, "lens")


def test_lens_status_under_sanitizers(driver):
    good = [800.0, 810.0, 319.5, 239.5, -0.3, 0.1, 0.001, -0.0005, -0.01, 0.9, -0.3, 0.02]

    def line(lens, r2_max):
        return "lens " + " ".join(repr(float(v)) for v in list(lens) + [r2_max])

    cases = [(line(good, 1.5), OK), (line(good, INF), OK), (line(good, 0.0), OK), (line(good, -0.0), OK), (line([1.0, 1.0] + [0.0] * 10, INF), OK),
             (line(good, float("nan")), BAD_ARG), (line(good, -1.0), BAD_ARG), (line(good, -INF), BAD_ARG), (line(good, -5e-324), BAD_ARG),
             (line([0.0] + good[1:], 1.0), BAD_ARG), (line([-0.0] + good[1:], 1.0), BAD_ARG), (line(good[:1] + [0.0] + good[2:], 1.0), BAD_ARG), ("lens_null", BAD_ARG)]
    for i in range(12):
        for bad in (float("nan"), INF, -INF):
            cases.append((line(good[:i] + [bad] + good[i + 1:], 1.0), NOT_FINITE))
    cases.append((line([0.0, float("nan")] + good[2:], -1.0), NOT_FINITE))  # (a non-finite entry is reported before a zero focal length)
    got = hostplan.run_driver(driver, [c for c, _ in cases], "lens")
    for (c, want), g in zip(cases, got):
        assert g == [want], (c, g, want)


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_lens_kernels_code_object(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("warp_lens.hip", tmp_path, "warp_lens.h").items() if "warp_lens_kernel" in n}
    assert len(kernels) == 2 * 4 * 2 * 2, len(kernels)  # dtype x channels x interpolation x border
    codeobj.assert_lean(kernels)


# ---- the ABI surface, without a device (fake pointers, never dereferenced: every call below fails validation first) ----

def test_abi_surface():
    lib = hostplan.built_lib()
    assert "bevwarp_warp_lens" in _lib.SYMBOLS and lib.bevwarp_version() == 7
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "int bevwarp_warp_lens(const void *src, void *dst, int batch," in header
    for cite in ("bev/calib.py:25", "bev/homo.py:130-135", "vis_homo.py:30-31"):
        assert cite in header.split("Conventions")[0], cite  # (in the table of entries)
    assert "parity with OpenCV is unpinned" in header
    one, far = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)
    lens = (ctypes.c_double * 12)(800.0, 810.0, 319.5, 239.5, -0.3, 0.1, 0.001, -0.0005, -0.01, 0, 0, 0)
    nan_lens = (ctypes.c_double * 12)(800.0, 810.0, 319.5, 239.5, float("nan"), 0, 0, 0, 0, 0, 0, 0)

    def call(lens=lens, r2_max=1.0, batch=1, interp=1, mode=0, dtype=_lib.U8, src=one, m=one):
        return lib.bevwarp_warp_lens(src, far, batch, 8, 8, 8, 8, 3, 192, 24, 192, 24, m, 1, lens, r2_max, dtype, interp, mode, None, None)

    assert call(batch=0) == OK  # nothing to do: no launch
    assert call(mode=1) == UNSUPPORTED and call(interp=2) == UNSUPPORTED and call(dtype=_lib.F16) == UNSUPPORTED
    assert call(src=None) == BAD_ARG and call(m=None) == BAD_ARG
    assert call(lens=None) == BAD_ARG and call(lens=nan_lens) == NOT_FINITE
    assert call(r2_max=-1.0) == BAD_ARG and call(r2_max=float("nan")) == BAD_ARG
