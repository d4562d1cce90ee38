"""The lens point projection (bevwarp_project_points_lens, bev_amd.points.distort_points / undistort_points) without a device: the
numpy reference (tests/points_lens_ref.py) against a 50-digit evaluation, against the plain homography and against the lens warp's
chain, the convergence of the inverse, the C ABI's host checks under the sanitizers (tests/host_plan_driver.cpp, family `points_lens`), the ABI
surface, the kernels' code object and the Python entries' argument errors."""
import ctypes
import os

import mpmath
import numpy as np
import pytest

from bev_amd import _lib
from tests import codeobj
from tests import hostplan
from tests import lens_ref as LR
from tests import points_lens_ref as PR
from tests import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SW, SH = 640, 360
K = LR.camera_K(SW, SH)
LENSES = {"A": LR.LENS_A, "B": LR.LENS_B}
K3 = np.array([[K[0, 0], 0, K[0, 2]], [0, K[1, 1], K[1, 2]], [0, 0, 1.0]])


def _frame_pixels():
    u, v = np.meshgrid(np.arange(float(SW)), np.arange(float(SH)))
    return np.stack([u.ravel(), v.ravel()], axis=1)


def _far_grid():
    u, v = np.meshgrid(np.arange(-2000.0, 2640.0, 16.0), np.arange(-2000.0, 2360.0, 16.0))
    return np.stack([u.ravel(), v.ravel()], axis=1)


# ---- the reference against the same formulas in 50-digit arithmetic ----

def _mp_plane(H, x, y):
    h = [mpmath.mpf(float(v)) for v in np.asarray(H, np.float64).ravel()]
    W = h[6] * x + h[7] * y + h[8]
    return (h[0] * x + h[1] * y + h[2]) / W, (h[3] * x + h[4] * y + h[5]) / W


def _mp_lens(lens, xn, yn):
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = [mpmath.mpf(float(v)) for v in lens]
    x2, y2 = xn * xn, yn * yn
    r2, xy2 = x2 + y2, 2 * xn * yn
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    return fx * (xn * kr + p1 * xy2 + p2 * (r2 + 2 * x2)) + cx, fy * (yn * kr + p1 * (r2 + 2 * y2) + p2 * xy2) + cy


def _mp_undistort(lens, u, v, iters):
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = [mpmath.mpf(float(t)) for t in lens]
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd, yd
    for _ in range(iters):
        x2, y2 = x * x, y * y
        r2, xy2 = x2 + y2, 2 * x * y
        ic = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        x, y = (xd - (p1 * xy2 + p2 * (r2 + 2 * x2))) * ic, (yd - (p1 * (r2 + 2 * y2) + p2 * xy2)) * ic
    return x, y


@pytest.mark.parametrize("name", sorted(LENSES))
def test_reference_against_50_digit_evaluation(name):
    """200 seeded points per direction.  DISTORT: |u - u_exact| <= 1e-9 px -- about 35 float64 operations of relative error 2^-53
    each on values below 2^11 px (the plane coordinates below 2, kr ~ 1) stay below 35 * 2^-53 * 2^11 * 4 < 4e-11.  UNDISTORT: the
    fixed-point step is a contraction inside the frame (its error shrinks from step to step: 0.1 px after 5 steps, 2e-9 after 20), so
    rounding errors do not accumulate beyond a few ulp of coordinates below 2: |x - x_exact| <= 1e-12; the residual, a difference of
    pixel coordinates below 2^11 with errors of that size, <= 1e-9 px."""
    lens = LR.lens12(K, LENSES[name])
    M = wl.synth_brno_H(SW, SH, 160, 120)
    R = LR.ray_matrix(M, K)
    rng = np.random.default_rng(77)
    with mpmath.workdps(50):
        bev = np.stack([rng.uniform(0, 160, 200), rng.uniform(0, 120, 200)], axis=1)
        u, v, r2 = PR.distort_chain(bev, R, lens)
        keep = r2 <= LR.lens_valid_r2(LENSES[name])
        assert keep.sum() > 50
        worst = mpmath.mpf(0)
        for i in np.flatnonzero(keep):
            xn, yn = _mp_plane(R, mpmath.mpf(float(bev[i, 0])), mpmath.mpf(float(bev[i, 1])))
            ue, ve = _mp_lens(lens, xn, yn)
            worst = max(worst, abs(ue - float(u[i])), abs(ve - float(v[i])))
        print("lens %s distort: worst |u - u_exact| = %s px" % (name, mpmath.nstr(worst, 5)))
        assert worst <= mpmath.mpf("1e-9")

        raw = np.stack([rng.uniform(0, SW, 200), rng.uniform(0, SH, 200)], axis=1)
        out, e = PR.undistort(raw, np.eye(3), lens, INF, 20, INF)
        worst_x, worst_e = mpmath.mpf(0), mpmath.mpf(0)
        for i in range(200):
            x, y = _mp_undistort(lens, mpmath.mpf(float(raw[i, 0])), mpmath.mpf(float(raw[i, 1])), 20)
            u2, v2 = _mp_lens(lens, x, y)
            worst_x = max(worst_x, abs(x - float(out[i, 0])), abs(y - float(out[i, 1])))
            worst_e = max(worst_e, abs(max(abs(u2 - float(raw[i, 0])), abs(v2 - float(raw[i, 1]))) - float(e[i])))
        print("lens %s undistort: worst |x - x_exact| = %s, worst |e - e_exact| = %s px" % (name, mpmath.nstr(worst_x, 5), mpmath.nstr(worst_e, 5)))
        assert worst_x <= mpmath.mpf("1e-12") and worst_e <= mpmath.mpf("1e-9")


# ---- zero distortion: the plain homography ----

def test_zero_distortion_is_the_plain_homography():
    """k = p = 0: kr = 1 / 1 and every tangential term is a product with 0, so DISTORT is K applied to plane(H, p) and UNDISTORT's
    steps leave (xd, yd) where they are.  Against H @ (x, y, 1) dehomogenised in plain numpy: 1e-12 relative, project_points' own bar
    against its oracle -- the two evaluations round K @ R differently, and towards the horizon of this matrix the sum W cancels by up
    to three digits, which a few ulp of its terms turn into 1e3 ulp of the quotient."""
    lens = LR.lens12(K, None)
    M = wl.synth_brno_H(SW, SH, 160, 120)
    R = LR.ray_matrix(M, K)
    rng = np.random.default_rng(5)
    bev = np.stack([rng.uniform(0, 160, 500), rng.uniform(0, 120, 500)], axis=1)
    got = PR.distort(bev, R, lens, INF)
    p = np.concatenate([bev, np.ones((500, 1))], axis=1) @ (K3 @ R).T
    np.testing.assert_allclose(got, p[:, :2] / p[:, 2:], rtol=1e-12, atol=1e-10)  # (atol: a pixel coordinate that crosses 0)
    xn, yn = PR.plane(R, bev[:, 0], bev[:, 1])
    u, v, _ = PR.distort_chain(bev, R, lens)
    np.testing.assert_array_equal(u, K[0, 0] * xn + K[0, 2])
    np.testing.assert_array_equal(v, K[1, 1] * yn + K[1, 2])
    raw = np.stack([rng.uniform(0, SW, 500), rng.uniform(0, SH, 500)], axis=1)
    for iters in (1, 20):
        out, e = PR.undistort(raw, M @ K3, lens, INF, iters, 1e-9)  # (M: undistorted pixel -> BEV pixel)
        q = np.concatenate([raw, np.ones((500, 1))], axis=1) @ M.T
        np.testing.assert_allclose(out, q[:, :2] / q[:, 2:], rtol=1e-12, atol=1e-10)
        assert (e <= 1e-12).all()  # (u - cx) / fx * fx + cx: an ulp of a pixel coordinate


# ---- the warp tie-in: one evaluation block ----

def test_one_block_identity_with_the_lens_warp_chain():
    """At the integer pixels of a 64 x 48 destination (one evaluation block: bx = 0) DISTORT's u, v, r2 are lens_ref.chain's, bit for bit."""
    dw, dh = 64, 48
    R = LR.ray_matrix(wl.synth_brno_H(SW, SH, dw, dh), K)
    x, y = np.meshgrid(np.arange(float(dw)), np.arange(float(dh)))
    pix = np.stack([x.ravel(), y.ravel()], axis=1)
    for dist in LENSES.values():
        lens = LR.lens12(K, dist)
        want = LR.chain((dw, dh), R, lens)
        got = PR.distort_chain(pix, R, lens)
        for g, w in zip(got, want):
            assert PR.same_bits(g, w.ravel())


# ---- convergence of the inverse ----

@pytest.mark.parametrize("name", sorted(LENSES))
def test_every_frame_pixel_converges_in_20_steps(name):
    lens, r2_max = LR.lens12(K, LENSES[name]), LR.lens_valid_r2(LENSES[name])
    out, e = PR.undistort(_frame_pixels(), np.eye(3), lens, r2_max, 20, 1e-3)
    print("lens %s, 20 steps: max residual %.3g px" % (name, e.max()))
    assert (e <= 1e-6).all() and not np.isnan(out).any()


def test_five_steps_are_not_enough():
    """Why the default is not OpenCV's 5."""
    lens = LR.lens12(K, LR.LENS_A)
    _, e = PR.undistort(_frame_pixels(), np.eye(3), lens, INF, 5, INF)
    print("lens A, 5 steps: max residual %.3g px" % e.max())
    assert e.max() > 1e-2


@pytest.mark.parametrize("name", sorted(LENSES))
def test_far_grid_has_both_verdicts_and_invalid_points_are_nan(name):
    lens, r2_max = LR.lens12(K, LENSES[name]), LR.lens_valid_r2(LENSES[name])
    tol = 1e-3
    raw = _far_grid()
    out, e = PR.undistort(raw, np.eye(3), lens, r2_max, 20, tol)
    nan = np.isnan(out).any(axis=1)
    assert nan.any() and (~nan).any()
    # the verdict's two conditions, recomputed from the accepted output itself: H is the identity, so out is the plane point (x, y)
    _, _, r2 = PR.lens_steps([np.float64(t) for t in lens], out[:, 0], out[:, 1])
    with np.errstate(invalid="ignore"):
        assert (r2[~nan] <= r2_max).all() and (e[~nan] <= tol).all()
        assert nan[~(e <= tol)].all()
    # ... and without the radius limit the points beyond it are back: they were NaN because of it
    free, e2 = PR.undistort(raw, np.eye(3), lens, INF, 20, tol)
    np.testing.assert_array_equal(e2, e)
    _, _, r2_free = PR.lens_steps([np.float64(t) for t in lens], free[:, 0], free[:, 1])
    beyond = ~np.isnan(free).any(axis=1) & (r2_free > r2_max)
    assert nan[beyond].all()
    assert np.isnan(out).all(axis=1)[nan].all()  # both coordinates


# ---- the host checks under the sanitizers ----

OK, BAD_ARG, UNSUPPORTED, NOT_FINITE, OVERLAP = 0, -1, -2, -4, -6
GOOD = [800.0, 810.0, 319.5, 239.5, -0.3, 0.1, 0.001, -0.0005, -0.01, 0.9, -0.3, 0.02]
CALL = dict(src=1 << 20, dst=1 << 21, res=0, n=1000, h=1, direction=1, iters=20, tol_px=1e-3, dtype=2, has_lens=1, r2_max=1.5)


def _status(lens=GOOD, **kw):
    a = dict(CALL, **kw)
    return "status " + " ".join(repr(float(a[k])) if k in ("tol_px", "r2_max") else str(a[k]) for k in CALL) + "".join(" %r" % float(v) for v in lens)


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def test_status_under_sanitizers(driver):
    nan = float("nan")
    src, dst, n = CALL["src"], CALL["dst"], CALL["n"]
    cases = [(_status(), OK), (_status(direction=0), OK), (_status(dtype=1), OK), (_status(res=1 << 22), OK), (_status(src=dst), OK), (_status(n=0), OK),
             (_status(n=0, res=src), OK)]
    # 1. BAD_ARG
    cases += [(_status(src=0), BAD_ARG), (_status(dst=0), BAD_ARG), (_status(h=0), BAD_ARG), (_status(n=-1), BAD_ARG), (_status(n=-(1 << 62)), BAD_ARG),
              (_status(src=0, n=0), BAD_ARG), (_status(direction=2), BAD_ARG), (_status(direction=-1), BAD_ARG), (_status(direction=0, res=1 << 22), BAD_ARG)]
    cases += [(_status(iters=0), BAD_ARG), (_status(iters=1), OK), (_status(iters=100), OK), (_status(iters=101), BAD_ARG), (_status(iters=-5), BAD_ARG),
              (_status(tol_px=-0.0), OK), (_status(tol_px=0.0), OK), (_status(tol_px=nan), BAD_ARG), (_status(tol_px=INF), OK), (_status(tol_px=-1e-300), BAD_ARG),
              (_status(tol_px=-INF), BAD_ARG)]
    cases += [(_status(direction=0, iters=0, tol_px=nan), OK), (_status(direction=0, iters=1000, tol_px=-1.0), OK)]  # (DISTORT ignores both)
    # ... before 2. UNSUPPORTED, before 3. NOT_FINITE (H), before 4. the lens, before 5. OVERLAP
    cases += [(_status(dtype=d), UNSUPPORTED) for d in (0, 3, 4, -1, 7)]
    cases += [(_status(src=0, dtype=0), BAD_ARG), (_status(iters=0, dtype=0, h=2), BAD_ARG), (_status(dtype=0, h=2), UNSUPPORTED), (_status(h=2), NOT_FINITE),
              (_status(h=3), NOT_FINITE), (_status(h=2, has_lens=0), NOT_FINITE), (_status(has_lens=0), BAD_ARG), (_status(has_lens=0, res=src), BAD_ARG),
              (_status(lens=GOOD[:4] + [nan] + GOOD[5:], res=src), NOT_FINITE), (_status(lens=[INF] + GOOD[1:]), NOT_FINITE),
              (_status(lens=[0.0] + GOOD[1:], res=src), BAD_ARG), (_status(lens=GOOD[:1] + [-0.0] + GOOD[2:]), BAD_ARG),
              (_status(r2_max=nan, res=src), BAD_ARG), (_status(r2_max=-1.0), BAD_ARG), (_status(r2_max=INF), OK), (_status(r2_max=0.0), OK)]
    # 5. OVERLAP: residual (n values) against in and out (n points each), to the byte.  float64: 16000-byte points, 8000-byte residual
    for base in (src, dst):
        cases += [(_status(res=base), OVERLAP), (_status(res=base + 16 * n - 1), OVERLAP), (_status(res=base + 16 * n), OK), (_status(res=base - 8 * n), OK),
                  (_status(res=base - 8 * n + 1), OVERLAP), (_status(res=base + 8), OVERLAP)]
        cases += [(_status(dtype=1, res=base + 8 * n - 1), OVERLAP), (_status(dtype=1, res=base + 8 * n), OK), (_status(dtype=1, res=base - 4 * n), OK),
                  (_status(dtype=1, res=base - 4 * n + 1), OVERLAP)]
    cases += [(_status(src=dst, res=dst + 64), OVERLAP)]
    # n next to 2^62: the ranges are compared in 128 bits -- 16 n bytes pass 2^64
    for big in ((1 << 62) - 1, 1 << 62, (1 << 62) + 1, (1 << 63) - 1):
        cases += [(_status(n=big), OK), (_status(n=big, res=8), OVERLAP), (_status(n=big, res=1 << 40), OVERLAP), (_status(n=big, dtype=1, res=1 << 40), OVERLAP),
                  (_status(n=big, direction=0), OK)]
    # last: alignment (a point moves as one unit)
    cases += [(_status(src=src + 8), BAD_ARG), (_status(dst=dst + 8), BAD_ARG), (_status(dtype=1, src=src + 8), OK), (_status(dtype=1, src=src + 4), BAD_ARG),
              (_status(res=(1 << 22) + 4), BAD_ARG), (_status(dtype=1, res=(1 << 22) + 4), OK), (_status(dtype=1, res=(1 << 22) + 2), BAD_ARG)]
    got = hostplan.run_driver(driver, [c for c, _ in cases], "points_lens")
    for (c, want), g in zip(cases, got):
        assert g == [want], (c, g, want)


# ---- the ABI surface, without a device (fake pointers, never dereferenced: every call below ends before a launch) ----

def test_abi_surface():
    lib = hostplan.built_lib()
    assert "bevwarp_project_points_lens" in _lib.SYMBOLS and lib.bevwarp_version() == 7
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "int bevwarp_project_points_lens(const void *in, void *out, void *residual /*device, may be NULL*/, int64_t n," in header
    assert "#define BEVWARP_LENS_DISTORT 0" in header and "#define BEVWARP_LENS_UNDISTORT 1" in header
    entry = header.split("Conventions")[0].split("bevwarp_project_points_lens")[1].split("bevwarp_rbox_iou")[0]  # (its row in the table of entries)
    for cite in ("rbox_world_img, bev/rbox.py:221-226", "Calib.gen_center_in_world, bev/calib.py:135-138", "bev/homo.py:130-135", "bev/calib.py:25"):
        assert cite in entry, cite
    assert "parity with OpenCV is unpinned" in header.split("bevwarp_project_points(const void *in")[1]
    a, b, r = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21), ctypes.c_void_p(1 << 22)
    H = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    H_nan = (ctypes.c_double * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)
    lens = (ctypes.c_double * 12)(*GOOD)
    nan_lens = (ctypes.c_double * 12)(*([float("nan")] + GOOD[1:]))

    def call(src=a, dst=b, res=None, n=0, H=H, lens=lens, r2_max=1.5, direction=1, iters=20, tol_px=1e-3, dtype=_lib.F64):
        return lib.bevwarp_project_points_lens(src, dst, res, n, H, lens, r2_max, direction, iters, tol_px, dtype, None)

    assert call() == OK and call(direction=0) == OK and call(res=r) == OK  # n == 0: nothing to do, no launch
    assert call(src=None) == BAD_ARG and call(dst=None) == BAD_ARG and call(H=None) == BAD_ARG and call(n=-1) == BAD_ARG
    assert call(direction=2) == BAD_ARG and call(direction=0, res=r) == BAD_ARG
    assert call(iters=0) == BAD_ARG and call(iters=101) == BAD_ARG and call(iters=1) == OK and call(iters=100) == OK
    assert call(tol_px=float("nan")) == BAD_ARG and call(tol_px=-1.0) == BAD_ARG and call(tol_px=-0.0) == OK and call(tol_px=INF) == OK
    assert call(dtype=_lib.U8) == UNSUPPORTED and call(dtype=_lib.F16) == UNSUPPORTED and call(dtype=_lib.U8, H=H_nan) == UNSUPPORTED
    assert call(H=H_nan) == NOT_FINITE and call(H=H_nan, lens=None) == NOT_FINITE
    assert call(lens=None) == BAD_ARG and call(lens=nan_lens) == NOT_FINITE and call(r2_max=-1.0) == BAD_ARG
    assert call(n=1000, res=a) == OVERLAP and call(n=1000, res=ctypes.c_void_p((1 << 21) + 15999)) == OVERLAP and call(n=1000, lens=None, res=a) == BAD_ARG
    assert call(n=1000, src=ctypes.c_void_p((1 << 20) + 8)) == BAD_ARG  # (a misaligned point: refused before the launch)


# ---- the code object: no scratch, no LDS, at most 128 VGPRs ----

def test_points_lens_kernels_code_object(tmp_path):
    kernels = {n: k for n, k in codeobj.kernels("points_lens.hip", tmp_path, "points_lens.h").items() if "points_lens_kernel" in n}
    assert len(kernels) == 2 * 2, sorted(kernels)  # dtype x direction
    codeobj.assert_lean(kernels)


# ---- the Python entries: argument errors before any device is asked for ----

def test_python_entries_validate_before_the_device():
    import torch

    import bev
    from bev_amd import points
    pts = torch.zeros((4, 2), dtype=torch.float64)  # a host tensor: the last thing the entries look at
    for fn in (points.distort_points, points.undistort_points):
        with pytest.raises(ValueError, match="dist_coeff must hold"):
            fn(pts, K, [0.1, 0.2])
        with pytest.raises(ValueError, match="skew"):
            fn(pts, np.array([[800.0, 0.1, 320], [0, 800, 180], [0, 0, 1]]), LR.LENS_A)
        with pytest.raises(ValueError, match="finite"):
            fn(pts, K, [float("nan"), 0, 0, 0])
        with pytest.raises(ValueError, match="finite"):
            fn(pts, np.array([[0.0, 0, 320], [0, 800, 180], [0, 0, 1]]), LR.LENS_A)
        with pytest.raises(ValueError, match="r2_max"):
            fn(pts, K, LR.LENS_A, r2_max=-1.0)
        with pytest.raises(ValueError, match="r2_max"):
            fn(pts, K, LR.LENS_A, r2_max=float("nan"))
        with pytest.raises(ValueError, match="H must be 3x3"):
            fn(pts, K, LR.LENS_A, H=np.eye(4))
        with pytest.raises(ValueError, match="CUDA"):
            fn(pts, K, LR.LENS_A)
        with pytest.raises(ValueError, match="CUDA"):
            fn(pts.numpy(), K, LR.LENS_A)
    for iters in (0, 101, -1, 2.5, True):
        with pytest.raises(ValueError, match="iters"):
            points.undistort_points(pts, K, LR.LENS_A, iters=iters)
    for tol in (-1.0, float("nan"), -1e-300):
        with pytest.raises(ValueError, match="tol_px"):
            points.undistort_points(pts, K, LR.LENS_A, tol_px=tol)
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = 10.0
    calib = bev.Calib(fx=800.0, fy=810.0, cx=319.5, cy=239.5, T=T, dist_coeff=list(LR.LENS_A))
    with pytest.raises(ValueError, match="CUDA"):
        points.world_to_raw(calib, pts)
    with pytest.raises(ValueError, match="iters"):
        points.raw_to_world(calib, pts, iters=0)
    flat = np.array([[0.0, 0], [10, 0], [10, 10], [0, 10]])
    with pytest.raises(ValueError, match="no K"):
        points.world_to_raw(bev.Calib(pts_image=flat, pts_world=np.hstack([flat, np.zeros((4, 1))])), pts)
