"""The equidistant (fisheye) lens model (include/bevwarp.h, BEVWARP_LENS_FISHEYE) without a device: the definition's arctangent and the
numpy reference (tests/fisheye_ref.py) against 40-digit arithmetic, the convergence of the inverse, the host helpers, the C ABI's host
checks under the sanitizers (tests/host_plan_driver.cpp, family `fisheye`) and through the built library, the Python entries' refusals, and the code
objects of the three new kernel units."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

from bev_amd import _lib
from tests import codeobj
from tests import fisheye_ref as FR
from tests import hostplan
from tests import lens_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
OK, BAD_ARG, UNSUPPORTED, TOO_LARGE, NOT_FINITE, OVERLAP = 0, -1, -2, -3, -4, -6
FISHEYE = 0x100
K = np.array([[200.0, 0, 319.5], [0, 200.0, 179.5], [0, 0, 1.0]])  # a 640 x 360 frame, the centre at its middle
GOOD = [200.0, 204.0, 319.5, 179.5, -0.02, 0.004, -0.001, 0.0002, 0.0, 0.0, 0.0, 0.0]


def _ulps(got, exact):
    """|got - exact| in units of the last place of the double nearest to `exact`."""
    return abs((mpmath.mpf(float(got)) - exact) / mpmath.mpf(float(np.spacing(abs(float(exact))))))


# ---- atan_pos ----

def test_constants_by_derivation():
    """The reference's constants, and the same literals in fisheye_pixel.h, are the doubles nearest to what they stand for."""
    with open(os.path.join(ROOT, "bev_amd", "csrc", "fisheye_pixel.h")) as f:
        header = f.read()
    literals = {float.fromhex(h) for h in re.findall(r"-?0x[0-9a-f]+\.[0-9a-f]+p[+-]\d+", header)}
    with mpmath.workdps(40):
        want = [float(mpmath.atan(mpmath.mpf(i) / 8)) for i in range(9)]
        assert FR.A == want
        pio2, pi = mpmath.pi / 2, +mpmath.pi
        assert FR.PIO2_HI == float(pio2) and FR.PIO2_LO == float(pio2 - mpmath.mpf(FR.PIO2_HI))
        assert FR.PI_HI == float(pi) and FR.PI_LO == float(pi - mpmath.mpf(FR.PI_HI))
    assert literals == set(want) | {FR.PIO2_HI, FR.PIO2_LO, FR.PI_HI, FR.PI_LO}
    assert [FR.C3, FR.C5, FR.C7, FR.C9, FR.C11, FR.C13, FR.C15] == [1.0 / n for n in (3, 5, 7, 9, 11, 13, 15)]
    for n in (3, 5, 7, 9, 11, 13, 15):
        assert "c%d = 1.0 / %d.0" % (n, n) in header


def test_atan_pos_within_2_ulp():
    """Uniform in [0, 1] and in [1, 50], log-uniform over 1e-12..1e12, the breakpoints and the midpoints between them: at most 2 ulp from
    the 40-digit arctangent; 0 and +inf exact; NaN is NaN."""
    rng = np.random.default_rng(7)
    t = np.concatenate([rng.uniform(0, 1, 19000), rng.uniform(1, 50, 19000), 10.0 ** rng.uniform(-12, 12, 19000), np.arange(9) / 8.0, (np.arange(8) + 0.5) / 8.0])
    got = FR.atan_pos(t)
    with mpmath.workdps(40):
        worst = max(_ulps(g, mpmath.atan(mpmath.mpf(float(x)))) for x, g in zip(t, got))
    print("worst error of atan_pos over %d samples: %.3f ulp" % (t.size, float(worst)))
    assert worst <= 2
    assert FR.atan_pos(0.0) == 0.0 and FR.atan_pos(INF) == FR.PIO2_HI and np.isnan(FR.atan_pos(NAN))
    assert FR.atan_pos(1.0) == FR.A[8] and FR.atan_pos(np.float64(0.125)) == FR.A[1]


# ---- the forward chain ----

def _mp_forward(lens, X, Y, W):
    fx, fy, cx, cy, k1, k2, k3, k4 = [mpmath.mpf(float(v)) for v in lens[:8]]
    X, Y, W = mpmath.mpf(float(X)), mpmath.mpf(float(Y)), mpmath.mpf(float(W))
    rho = mpmath.sqrt(X * X + Y * Y)
    theta = mpmath.atan2(rho, W)
    t2 = theta * theta
    thd = theta * (1 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2)
    g = thd / rho if rho != 0 else mpmath.mpf(0)
    return fx * X * g + cx, fy * Y * g + cy, theta


def test_forward_chain_against_40_digits():
    rng = np.random.default_rng(3)
    lens = FR.lens12(K, FR.K_TEST)
    X, Y = rng.uniform(-3, 3, 600), rng.uniform(-3, 3, 600)
    Wd = np.concatenate([rng.uniform(0.05, 2, 300), rng.uniform(-2, -0.05, 250), np.zeros(50)])  # in front, behind, and at 90 degrees
    u, v, theta = FR.steps(lens, X, Y, Wd)
    with mpmath.workdps(40):
        for i in range(X.size):
            eu, ev, et = _mp_forward(lens, X[i], Y[i], Wd[i])
            assert abs(u[i] - eu) < 1e-9 and abs(v[i] - ev) < 1e-9 and abs(theta[i] - et) < 1e-14, (X[i], Y[i], Wd[i])
    assert (theta[-50:] == FR.PIO2_HI).all() and (theta[300:550] > FR.PIO2_HI).all()


def test_special_rays():
    lens = FR.lens12(K, FR.K_TEST)
    u, v, theta = FR.steps(lens, [0.0, 0.0, 0.0, 1.0, NAN], [0.0, 0.0, 0.0, 0.0, 1.0], [1.0, -1.0, 0.0, 0.0, 1.0])
    assert (u[0], v[0], theta[0]) == (319.5, 179.5, 0.0)           # the optical axis
    assert theta[1] == FR.PI_HI and (u[1], v[1]) == (319.5, 179.5)  # straight back: g = 0 by definition
    assert np.isnan(theta[2]) and (u[2], v[2]) == (319.5, 179.5)    # 0 / 0: invalid under every theta_max
    assert theta[3] == FR.PIO2_HI and np.isnan(theta[4]) and np.isnan(u[4])
    valid = FR.maps((1, 1), np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0.0]]), lens, INF, 1)[4]
    assert not valid.any()  # NaN <= inf is false


def test_equidistant_without_coefficients():
    """k = 0: the image radius is f theta, and along the optical axis' neighbourhood the rational chain with k = 0 agrees to first order."""
    rng = np.random.default_rng(5)
    lens = FR.lens12(K, None)
    ang, phi = rng.uniform(0, np.pi / 3, 500), rng.uniform(0, 2 * np.pi, 500)
    X, Y, Wd = np.sin(ang) * np.cos(phi), np.sin(ang) * np.sin(phi), np.cos(ang)
    scale = rng.uniform(0.1, 10, 500)
    u, v, theta = FR.steps(lens, X * scale, Y * scale, Wd * scale)
    assert np.abs(np.hypot(u - 319.5, v - 179.5) - 200.0 * ang).max() < 1e-9 and np.abs(theta - ang).max() < 1e-14
    # the optical axis: both models send it to the principal point, exactly
    R = np.array([[0.01, 0, -0.05], [0, 0.01, -0.03], [0, 0, 1.0]])
    uf, vf, _ = FR.chain((8, 4), R, lens)
    ur, vr, _ = LR.chain((8, 4), R, LR.lens12(K, None))
    assert (uf[3, 5], vf[3, 5]) == (ur[3, 5], vr[3, 5]) == (319.5, 179.5)
    assert np.abs(uf - ur).max() < 200.0 * 0.06 ** 3 and np.abs(uf - ur).max() > 0  # tan(theta) - theta < theta^3 (theta <= 0.06 here)


# ---- the inverse ----

def test_inverse_converges_in_10_steps_on_a_frame_and_not_in_3():
    """Every pixel of a 640 x 360 frame (fx = fy = 200, centre at the middle, K_TEST, theta_max = valid_theta): within 1e-9 px after 10
    steps; 3 steps are not enough."""
    lens = FR.lens12(K, FR.K_TEST)
    theta_max = FR.valid_theta(FR.K_TEST)
    v, u = np.mgrid[0:360, 0:640]
    pts = np.stack([u.ravel(), v.ravel()], axis=1).astype(np.float64)
    out, e = FR.undistort(pts, np.eye(3), lens, theta_max, 10, INF)
    print("worst reprojection error after 10 steps: %.3g px" % e.max())
    assert e.max() <= 1e-9 and not np.isnan(out).any()
    _, e3 = FR.undistort(pts, np.eye(3), lens, theta_max, 3, INF)
    print("worst reprojection error after 3 steps: %.3g px" % e3.max())
    assert e3.max() > 1e-9
    # ... and the rays are unit-free directions on both sides of 90 degrees: the frame's corners lie at 105 degrees
    rx, ry, rz = FR.undistort_ray(pts, lens, 10)
    assert rz[0] < 0 < rz[180 * 640 + 320] and (rz < 0).sum() > 1000
    u2, v2, _ = FR.steps(lens, 3.0 * rx, 3.0 * ry, 3.0 * rz)
    assert np.abs(u2 - pts[:, 0]).max() < 1e-9 and np.abs(v2 - pts[:, 1]).max() < 1e-9


# ---- host helpers ----

def test_ray_matrix_oriented():
    from bev_amd import warp
    rng = np.random.default_rng(11)
    Kc = np.array([[210.0, 0, 300.5], [0, 190.0, 170.25], [0, 0, 1.0]])
    for _ in range(20):
        M = np.eye(3) + rng.uniform(-0.3, 0.3, (3, 3))
        M[2, :2] *= 1e-3
        for sign in (1.0, -1.0):
            for inverse in (False, True):
                A = sign * (np.linalg.inv(M) if inverse else M)
                R = warp.ray_matrix(A, Kc, inverse_given=inverse, oriented=True)
                assert np.array_equal(R, warp.ray_matrix(-A, Kc, inverse_given=inverse, oriented=True))  # the same rays for M and -M
                assert np.array_equal(R, FR.ray_matrix(A, Kc, inverse_given=inverse))
                plain = warp.ray_matrix(A, Kc, inverse_given=inverse)
                assert np.array_equal(plain, LR.ray_matrix(A, Kc, inverse_given=inverse))  # oriented=False: today's result
                assert np.array_equal(R, plain) or np.array_equal(R, -plain)
                # the destination pixel of the optical axis looks forward
                p = M @ np.array([Kc[0, 2], Kc[1, 2], 1.0])
                ray = R @ np.array([p[0] / p[2], p[1] / p[2], 1.0])
                assert ray[2] > 0 and abs(ray[0]) < 1e-9 * ray[2] and abs(ray[1]) < 1e-9 * ray[2]
    batch = np.stack([np.eye(3), -np.eye(3)])
    assert np.array_equal(warp.ray_matrix(batch, Kc, oriented=True)[0], warp.ray_matrix(batch, Kc, oriented=True)[1])


def test_fisheye_valid_theta():
    import bev.warp
    from bev_amd import warp
    assert bev.warp.fisheye_valid_theta is warp.fisheye_valid_theta
    assert warp.fisheye_valid_theta(None) == np.pi == warp.fisheye_valid_theta([0, 0, 0, 0]) == warp.fisheye_valid_theta(FR.K_TEST)
    # a known fold: theta (1 + k1 theta^2) stops growing where 1 + 3 k1 theta^2 = 0
    assert warp.fisheye_valid_theta([-1.0 / 3.0, 0, 0, 0]) == pytest.approx(1.0, abs=1e-12)
    assert warp.fisheye_valid_theta([-1.0 / 12.0, 0, 0, 0]) == pytest.approx(2.0, abs=1e-12)
    assert warp.fisheye_valid_theta([-1.0 / 48.0, 0, 0, 0]) == np.pi  # the fold lies at 4 radians: capped
    k = (0.1, -0.2, 0.01, 0.002)
    t = warp.fisheye_valid_theta(k)
    assert t == pytest.approx(FR.valid_theta(k), abs=1e-12) and 0 < t < np.pi
    t2 = t * t
    assert abs(1 + (((9 * k[3] * t2 + 7 * k[2]) * t2 + 5 * k[1]) * t2 + 3 * k[0]) * t2) < 1e-9


# ---- the host checks under the sanitizers ----

@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver()


def _lens_line(lens=GOOD, theta_max=1.5):
    return "lens " + " ".join(repr(float(v)) for v in list(lens) + [theta_max])


def _with(i, v):
    return GOOD[:i] + [v] + GOOD[i + 1:]


def test_lens_status_under_sanitizers(driver):
    cases = [(_lens_line(), OK), (_lens_line(theta_max=INF), OK), (_lens_line(theta_max=0.0), OK), (_lens_line(theta_max=-0.0), OK), ("lens_null", BAD_ARG)]
    cases += [(_lens_line(_with(i, bad)), NOT_FINITE) for i in range(12) for bad in (NAN, INF, -INF)]
    cases += [(_lens_line(_with(0, 0.0)), BAD_ARG), (_lens_line(_with(1, -0.0)), BAD_ARG)]
    cases += [(_lens_line(_with(i, 1e-300)), BAD_ARG) for i in (8, 9, 10, 11)]  # the four reserved entries
    cases += [(_lens_line(theta_max=NAN), BAD_ARG), (_lens_line(theta_max=-1e-300), BAD_ARG), (_lens_line(theta_max=-INF), BAD_ARG)]
    # the order: NOT_FINITE before the BAD_ARGs of the values
    cases += [(_lens_line(_with(0, 0.0)[:5] + [NAN] + GOOD[6:]), NOT_FINITE), (_lens_line(_with(8, NAN), theta_max=-1.0), NOT_FINITE)]
    got = hostplan.run_driver(driver, [c for c, _ in cases], "fisheye")
    for (c, want), g in zip(cases, got):
        assert g == [want], (c, g, want)


def test_flag_and_calls_under_sanitizers(driver):
    flags = [("flag %d" % w, [f, left]) for w, f, left in ((0, 0, 0), (1, 0, 1), (0x100, 1, 0), (0x101, 1, 1), (0x102, 1, 2), (0x200, 0, 0x200), (0x300, 1, 0x200),
                                                           (-1, 1, -257), (16 | 0x100, 1, 16))]
    # bevwarp_warp_lens: the flag is no part of the format; what is left of the word is judged as it always was, before the lens
    warps = [("warp %d %d %s" % (interp, lens, th), want) for interp, lens, th, want in (
        (0x100, 1, "1.5", [OK, OK]), (0x101, 1, "inf", [OK, OK]), (1, 1, "1.5", [OK, OK]), (0x102, 1, "1.5", [UNSUPPORTED, 0]), (0x200, 1, "1.5", [UNSUPPORTED, 0]),
        (0x300, 1, "1.5", [UNSUPPORTED, 0]), (0x102, 0, "nan", [UNSUPPORTED, 0]), (0x101, 0, "1.5", [OK, BAD_ARG]), (0x101, 2, "-1", [OK, NOT_FINITE]),
        (0x101, 3, "1.5", [OK, BAD_ARG]), (0x101, 4, "1.5", [OK, BAD_ARG]), (0x101, 1, "nan", [OK, BAD_ARG]), (0x101, 1, "-1", [OK, BAD_ARG]),
        (1, 4, "1.5", [OK, OK]))]  # (without the flag entry 10 is k5 of the rational model)
    src, dst, res = 1 << 20, 1 << 21, 1 << 22

    def points(direction=0x101, lens=1, th="1.5", h=1, n=1000, res=0, iters=10, tol="0.001", dtype=2, src=src):
        return "points %d %d %d %d %d %d %s %d %d %s %d" % (src, dst, res, n, h, lens, th, direction, iters, tol, dtype)

    F64 = _lib.F64
    pts = [(points(dtype=F64), [OK]), (points(direction=0x100, dtype=F64), [OK]), (points(dtype=F64, res=res), [OK]), (points(dtype=_lib.F32), [OK]),
           # a direction outside the two, with or without the flag: BAD_ARG, before everything the lens could say
           (points(direction=0x102, dtype=F64, lens=0), [BAD_ARG]), (points(direction=0x200, dtype=F64), [BAD_ARG]), (points(direction=0x300, dtype=F64), [BAD_ARG]),
           (points(direction=-1, dtype=F64), [BAD_ARG]), (points(direction=0x100, res=res, dtype=F64), [BAD_ARG]), (points(iters=0, dtype=F64), [BAD_ARG]),
           (points(iters=101, dtype=F64), [BAD_ARG]), (points(tol="nan", dtype=F64), [BAD_ARG]), (points(direction=0x100, iters=0, tol="nan", dtype=F64), [OK]),
           (points(dtype=0, lens=0), [UNSUPPORTED]), (points(dtype=F64, h=2, lens=0), [NOT_FINITE]), (points(dtype=F64, h=0), [BAD_ARG]),
           # the lens, at the place of the lens checks: NULL, a NaN entry, fx == 0, a reserved entry, theta_max
           (points(dtype=F64, lens=0, res=src), [BAD_ARG]), (points(dtype=F64, lens=2, res=src, th="-1"), [NOT_FINITE]), (points(dtype=F64, lens=3, res=src), [BAD_ARG]),
           (points(dtype=F64, lens=4, res=src), [BAD_ARG]), (points(dtype=F64, th="nan", res=src), [BAD_ARG]), (points(dtype=F64, th="-0.5"), [BAD_ARG]),
           (points(dtype=F64, th="inf"), [OK]), (points(direction=1, dtype=F64, lens=4), [OK]),
           # ... before OVERLAP, before the alignment
           (points(dtype=F64, res=src), [OVERLAP]), (points(dtype=F64, src=src + 8), [BAD_ARG]), (points(dtype=F64, res=src, src=src + 8), [OVERLAP])]
    mp, xy, fr = 4096, 1 << 24, 1 << 26

    def build(interp=0x101, lens=1, th="1.5", m=mp, xy=xy, frac=fr, m_count=1, dst_h=8, dst_w=8, xy_rs=32, frac_rs=16):
        return "build %d %d %d %d %d %s %d %d %d %d %d" % (m, xy, frac, m_count, lens, th, interp, dst_h, dst_w, xy_rs, frac_rs)

    builds = [(build(), [OK, 2]), (build(interp=0x100, frac=0), [OK, 2]), (build(m_count=3), [OK, 6]), (build(interp=1, lens=0), [OK, 2]), (build(interp=1), [OK, 2]),
              (build(m=0), [BAD_ARG, 0]), (build(xy=0), [BAD_ARG, 0]), (build(m_count=0, lens=0), [BAD_ARG, 0]), (build(dst_h=0), [BAD_ARG, 0]),
              (build(interp=0x102, lens=0), [UNSUPPORTED, 0]), (build(interp=0x200), [UNSUPPORTED, 0]), (build(interp=0x300), [UNSUPPORTED, 0]),
              (build(frac=0, lens=0), [BAD_ARG, 0]), (build(xy_rs=30, lens=0), [BAD_ARG, 0]), (build(dst_h=(1 << 20) + 1, lens=0), [TOO_LARGE, 0]),
              (build(frac=xy + 64, lens=0), [OVERLAP, 0]),
              # the lens last: a fisheye map has no pinhole chain, so a NULL lens is refused
              (build(lens=0), [BAD_ARG, 0]), (build(lens=2, th="-1"), [NOT_FINITE, 0]), (build(lens=3), [BAD_ARG, 0]), (build(lens=4), [BAD_ARG, 0]),
              (build(th="nan"), [BAD_ARG, 0]), (build(th="-1"), [BAD_ARG, 0]), (build(th="inf"), [OK, 2]), (build(interp=1, lens=4), [OK, 2])]
    cases = flags + warps + pts + builds
    hostplan.check_cases(driver, cases, "fisheye")


# ---- the same statuses through the built library (fake pointers, never dereferenced: every call ends before a launch) ----

def test_abi_surface():
    lib = hostplan.built_lib()
    assert lib.bevwarp_version() == 7 == _lib.ABI_VERSION
    with open(os.path.join(ROOT, "include", "bevwarp.h")) as f:
        header = f.read()
    assert "#define BEVWARP_LENS_FISHEYE 0x100" in header
    for text in ("atan_pos", "0x1.921fb54442d18p+0", "0x1.1a62633145c07p-54", "theta_max", "sign of M_ray"):
        assert text in header, text
    one, far, mxy, mfr = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24), ctypes.c_void_p(1 << 26)
    arr = lambda v: (ctypes.c_double * 12)(*v)  # noqa: E731
    good, nan_lens, zero_fx = arr(GOOD), arr(_with(5, NAN)), arr(_with(0, 0.0))
    reserved = [arr(_with(i, 0.5)) for i in (8, 9, 10, 11)]

    def warp(lens=good, theta_max=1.5, batch=1, interp=0x101, mode=0, src=one):
        return lib.bevwarp_warp_lens(src, far, batch, 8, 8, 8, 8, 3, 192, 24, 192, 24, one, 1, lens, theta_max, _lib.U8, interp, mode, None, None)

    assert warp(batch=0) == OK and warp(batch=0, lens=None) == OK  # nothing to do: no launch, the lens is not looked at
    assert warp(interp=0x102) == UNSUPPORTED and warp(interp=0x200) == UNSUPPORTED and warp(interp=0x300) == UNSUPPORTED and warp(mode=1) == UNSUPPORTED
    assert warp(src=None) == BAD_ARG and warp(src=None, lens=None) == BAD_ARG and warp(interp=0x102, lens=None) == UNSUPPORTED
    assert warp(lens=None) == BAD_ARG and warp(lens=nan_lens, theta_max=-1.0) == NOT_FINITE and warp(lens=zero_fx) == BAD_ARG
    assert all(warp(lens=r) == BAD_ARG for r in reserved) and all(warp(lens=r, interp=0x100) == BAD_ARG for r in reserved)
    assert warp(theta_max=NAN) == BAD_ARG and warp(theta_max=-1.0) == BAD_ARG

    def build(M=one, m_count=1, lens=good, theta_max=1.5, interp=0x101, xy=mxy, frac=mfr, dst_h=8, xy_rs=32):
        return lib.bevwarp_build_map(M, m_count, lens, theta_max, interp, xy, frac, dst_h, 8, 256, xy_rs, 128, 16, None)

    assert build(M=None) == BAD_ARG and build(xy=None) == BAD_ARG and build(frac=None) == BAD_ARG and build(m_count=0) == BAD_ARG and build(dst_h=0) == BAD_ARG
    assert build(interp=0x102) == UNSUPPORTED and build(interp=0x200) == UNSUPPORTED and build(interp=0x102, lens=None) == UNSUPPORTED
    assert build(xy_rs=30) == BAD_ARG and build(dst_h=(1 << 20) + 1) == TOO_LARGE and build(frac=ctypes.c_void_p((1 << 24) + 64)) == OVERLAP
    assert build(lens=None) == BAD_ARG and build(lens=None, interp=0x100, frac=None) == BAD_ARG
    assert build(lens=nan_lens, theta_max=NAN) == NOT_FINITE and build(lens=zero_fx) == BAD_ARG and all(build(lens=r) == BAD_ARG for r in reserved)
    assert build(theta_max=NAN) == BAD_ARG and build(theta_max=-1.0) == BAD_ARG

    a, b, r = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21), ctypes.c_void_p(1 << 22)
    H = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    H_nan = (ctypes.c_double * 9)(1, 0, 0, 0, NAN, 0, 0, 0, 1)

    def points(src=a, dst=b, res=None, n=0, H=H, lens=good, theta_max=1.5, direction=0x101, iters=10, tol_px=1e-3, dtype=_lib.F64):
        return lib.bevwarp_project_points_lens(src, dst, res, n, H, lens, theta_max, direction, iters, tol_px, dtype, None)

    assert points() == OK and points(direction=0x100) == OK and points(res=r) == OK  # n == 0: nothing to do, no launch
    assert points(direction=0x102) == BAD_ARG and points(direction=0x200) == BAD_ARG and points(direction=0x300) == BAD_ARG and points(direction=0x100, res=r) == BAD_ARG
    assert points(src=None) == BAD_ARG and points(iters=0) == BAD_ARG and points(iters=101) == BAD_ARG and points(tol_px=NAN) == BAD_ARG
    assert points(dtype=_lib.U8, lens=None) == UNSUPPORTED and points(H=H_nan, lens=None) == NOT_FINITE
    assert points(lens=None) == BAD_ARG and points(lens=nan_lens, theta_max=-1.0) == NOT_FINITE and points(lens=zero_fx) == BAD_ARG
    assert all(points(lens=x) == BAD_ARG for x in reserved) and points(theta_max=NAN) == BAD_ARG and points(theta_max=-1.0) == BAD_ARG and points(theta_max=INF) == OK
    assert points(n=1000, res=a) == OVERLAP and points(n=1000, lens=None, res=a) == BAD_ARG
    assert points(n=1000, src=ctypes.c_void_p((1 << 20) + 8)) == BAD_ARG


# ---- the Python entries: argument errors before any device is asked for ----

def test_python_entries_validate_before_the_device():
    import torch

    import bev
    from bev_amd import points, warp
    img = torch.zeros((24, 40, 3), dtype=torch.uint8)  # host tensors: the last thing the entries look at
    pts = torch.zeros((4, 2), dtype=torch.float64)
    M = np.eye(3)
    for call in (lambda **kw: warp.warp_perspective_lens(img, M, (36, 20), K, kw.pop("dist", FR.K_TEST), **kw),
                 lambda **kw: warp.build_warp_map(M, (36, 20), K=K, dist_coeff=kw.pop("dist", FR.K_TEST), device="cpu", **kw),
                 lambda **kw: points.distort_points(pts, K, kw.pop("dist", FR.K_TEST), **kw),
                 lambda **kw: points.undistort_points(pts, K, kw.pop("dist", FR.K_TEST), **kw)):
        with pytest.raises(ValueError, match="4 values"):
            call(dist=[0.1, 0.2, 0.0, 0.0, 0.3], lens_model="fisheye")
        with pytest.raises(ValueError, match="theta_max"):
            call(r2_max=1.0, lens_model="fisheye")
        with pytest.raises(ValueError, match="r2_max"):
            call(theta_max=1.0, dist=LR.LENS_A)
        with pytest.raises(ValueError, match="lens_model"):
            call(lens_model="equisolid")
        with pytest.raises(ValueError, match="CUDA"):
            call(lens_model="fisheye")  # every argument is in order: the device is asked for last
        with pytest.raises(ValueError, match="CUDA"):
            call(lens_model="fisheye", dist=None, theta_max=2.0)  # no coefficients: still a fisheye lens, nothing is handed to the pinhole path
    with pytest.raises(ValueError, match="needs the camera matrix"):
        warp.build_warp_map(M, (36, 20), lens_model="fisheye", device="cpu")
    for fn in (points.distort_points, points.undistort_points):
        with pytest.raises(ValueError, match="theta_max"):
            fn(pts, K, FR.K_TEST, lens_model="fisheye", theta_max=-1.0)
        with pytest.raises(ValueError, match="theta_max"):
            fn(pts, K, FR.K_TEST, lens_model="fisheye", theta_max=NAN)
        with pytest.raises(ValueError, match="finite"):
            fn(pts, K, [NAN, 0, 0, 0], lens_model="fisheye")
    with pytest.raises(ValueError, match="iters"):
        points.undistort_points(pts, K, FR.K_TEST, lens_model="fisheye", iters=0)
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = 10.0
    calib = bev.Calib(fx=200.0, fy=200.0, cx=319.5, cy=179.5, T=T, dist_coeff=list(FR.K_TEST))
    with pytest.raises(ValueError, match="CUDA"):
        points.world_to_raw(calib, pts, lens_model="fisheye")
    with pytest.raises(ValueError, match="theta_max"):
        points.raw_to_world(calib, pts, lens_model="fisheye", r2_max=2.0)


# ---- the code objects: no scratch, no LDS, at most 128 VGPRs ----

def test_fisheye_kernels_code_objects(tmp_path):
    found = codeobj.kernels("warp_fisheye.hip", tmp_path, "fisheye_pixel.h")
    assert len(found) == 2 * 4 * 2 * 2 and all("warp_fisheye_kernel" in n for n in found), sorted(found)  # dtype x channels x interpolation x border
    codeobj.assert_lean(found)
    found = codeobj.kernels("warp_map_fisheye.hip", tmp_path, "fisheye_pixel.h")
    assert len(found) == 2 and all("build_map_fisheye_kernel" in n for n in found), sorted(found)  # interpolation
    codeobj.assert_lean(found)
    found = codeobj.kernels("points_fisheye.hip", tmp_path, "fisheye_pixel.h")
    assert len(found) == 2 * 2 and all("points_fisheye_kernel" in n for n in found), sorted(found)  # dtype x direction
    codeobj.assert_lean(found)
    for unit, header in (("warp_fisheye.hip", "lens_sample.h"), ("warp_fisheye.hip", "lens_lane.inc"), ("warp_lens.hip", "lens_lane.inc"),
                         ("warp_map_fisheye.hip", "map_build.inc"), ("warp_map.hip", "map_build.inc"), ("points_fisheye.hip", "points_stream.inc"),
                         ("points_lens.hip", "points_stream.h")):
        codeobj.makefile_flags(unit, header)


def test_the_units_call_no_library_trigonometry():
    """The definition brings its own arctangent: no atan, atan2, sin, cos or tan in the new units and the headers they add."""
    for name in ("fisheye_pixel.h", "warp_fisheye.hip", "warp_map_fisheye.hip", "points_fisheye.hip"):
        with open(os.path.join(ROOT, "bev_amd", "csrc", name)) as f:
            code = "\n".join(line.split("//")[0] for line in f)
        assert not re.search(r"\b(atan2?|sin|cos|tan|sincos)f?\s*\(", code), name
